// msa_alignapi.inc -- the build's own host-pointer entries (included by msa_capi.hip after msa_devcall.inc): an
// alignment with its CIGAR, one pair (msa_*_align) or a batch (msa_*_align_batch), through align_pairs below
//     msa_sw_align, msa_sw_align_batch                  Smith-Waterman
//     msa_sw_align_scored, ..._batch_scored, *32        ... under a substitution matrix, 7 or 31 symbols
//     msa_nw_align, msa_nw_align_batch                  banded global alignment, +1 / 0
//     msa_nw_align_scored, ..._batch_scored, *32        ... under match / mismatch scores or a matrix, 8 or 32 symbols
//     msa_fit_align, msa_fit_align_batch, *32           all of A in a substring of B
//     msa_overlap_align, msa_overlap_align_batch, *32   a suffix of one sequence against a prefix of the other
//     msa_extend_align, msa_extend_align_batch, *32     the best pair of prefixes (anchored start, free end)
//     msa_extend_align_banded, ..._batch_banded, *32    ... inside a band, each pair clipped to it
//     (msa_extend_align_xdrop, ..._batch_xdrop, *32     ... stopped by X-drop: msa_xdropapi.inc, through align_pairs)
//     msa_profile_align, msa_profile_align_batch        a position-specific profile: local, global, fit
// The host encodes the inputs, runs plans (the flow / band kernels behind msa_plan_run) and the device walks
// (traceback_kernel, msa_plan_traceback_batch), and turns a walk's O(m + n) ops into a CIGAR.
namespace {

// Device footprint of one global alignment (msa_devcall.inc's footprint_dir / footprint_planes are a local one's):
// the plan's cells (1 B per cell of the skewed band layout -- the stripes' own phase counts, as lay_out_pairs sizes
// them -- or none for a score-only call), its granule slots (two per item of 4 stripes, n + margins granules each; a
// chunked band plan has up to (warm-up + chunk) / 4 + 1 items per chunk), the 16 code copies, the ops and the pooled size classes' slack.  A banded pair therefore reserves
// ~(2 band + 64) B per row, not the full matrix.
size_t footprint_nw(int64_t m, int64_t n, int band, bool dir) {
  const int S = stripes_of(m);
  int pmax = 0;
  for (int k = 0; k < S; ++k) {
    StripeGeom g;
    stripe_geom(k, (int)m, (int)n, band, g, 16);
    pmax = std::max(pmax, g.P);
  }
  const size_t cells = dir ? (size_t)S * pmax * MSA_K * 64 : 0;
  size_t items = (size_t)(S + BK_W - 1) / BK_W;
  if (band >= 0) {
    const size_t nch = (size_t)(S + band_chunk() - 1) / band_chunk();
    items = std::max(items, nch * (size_t)((band_warm() + band_chunk()) / BK_W + 1));
  }
  return cells + 2 * items * (size_t)(n + 2 * MSA_GOFF + 32) * sizeof(unsigned long long) + 16 * (size_t)(n + 512) +
         3 * (size_t)(m + n) + (size_t(24) << 20);
}

// What a kind of alignment is, as data: everything in which the entries below differ.
enum GapRule { GAPS_LOCAL, GAPS_GLOBAL };  // gap costs >= 0 and scores in int8 | 0 <= gap_extend <= gap_open
enum Footprint { FOOT_MATRIX, FOOT_BAND };  // footprint_dir / footprint_planes | footprint_nw
struct AlignSpec {
  int status;               // MSA_ERR_ARG: the caller's alphabet or matrix is no scoring
  int alg_walk, alg_score;  // the plan with direction bytes, and the value plan of the same recurrence without
  int match, mismatch, start_type, track_end;  // the plan description's
  bool scored;              // tab is msa_plan_create_scored's 8 x 8 table (else match / mismatch score)
  int8_t tab[1024];         // (wide: msa_plan_create_scored32's 32 x 32 table)
  SymbolMap symbols;        // first-seen with the kind's code limit, or the caller's alphabet as a fixed map
  GapRule gaps;
  bool banded;              // a band is accepted
  Footprint footprint;
  // the walk of a single-pair plan: msa_plan_traceback or msa_plan_traceback_nw
  int (*walk)(msa_plan*, int64_t, const uint8_t*, uint8_t*, int64_t, int64_t*, void*);
  Border border;            // how the walk's ops become the whole alignment
  bool walk_for_beg;        // the walk is wanted for the start cell too, not only for a CIGAR
  bool wide = false;        // more than 8 symbols: 5-bit codes, tab is 32 x 32
  bool stop_is_beg = false; // the walk's stop cell (i, j) is the alignment's 0-based start, reported through
                            // AlignOut::beg where a walk ran (-1, -1 where none did); never a reason to walk
  bool clip_to_band = false;  // a band >= 0 is required, and a pair with |m - n| > band is shortened to its in-band
                              // prefixes (extend_band_clip) where a global kind answers MSA_ERR_ARG
  const int8_t* prof = nullptr;  // the rows are positions of this profile, a_len rows of 32 scores, not symbols of A
                                 // (msa_plan_create_profile; A is unused, tab too)
};

// Smith-Waterman: code 7 is the kernels' out-of-matrix sentinel, so 7 codes
AlignSpec spec_sw(int match, int mismatch, const char* preset) {
  return AlignSpec{MSA_OK, MSA_SW_AFFINE, MSA_SW_AFFINE, match, mismatch, 0, 1, false, {}, SymbolMap(7, preset),
                   GAPS_LOCAL, false, FOOT_MATRIX, msa_plan_traceback, BORDER_NONE, true};
}
// A spec scored by the caller's alphabet -- a symbol's code is its index -- and its n_sym x n_sym matrix, under plan
// kind alg.  reserved: the codes at the top that the kernels keep for themselves, so 8 - reserved symbols fit 3-bit
// codes and up to 32 - reserved make a wide spec.  status MSA_ERR_ARG for a NULL alphabet or matrix, n_sym outside
// 1..max_sym or a duplicate symbol
AlignSpec with_matrix(AlignSpec s, int alg, const char* alphabet, size_t n_sym, const int8_t* sub, size_t max_sym,
                      size_t reserved) {
  s.alg_walk = s.alg_score = alg;
  s.scored = true;
  if (!alphabet || !sub || n_sym < 1 || n_sym > max_sym) s.status = MSA_ERR_ARG;
  s.wide = s.status == MSA_OK && n_sym > 8 - reserved;
  if (s.wide) s.symbols = SymbolMap((int)(32 - reserved));
  const size_t stride = s.wide ? 32 : 8;
  for (size_t a = 0; s.status == MSA_OK && a < n_sym; ++a) {
    if (!s.symbols.add(alphabet[a])) s.status = MSA_ERR_ARG;
    for (size_t b = 0; b < n_sym; ++b) s.tab[stride * a + b] = sub[n_sym * a + b];
  }
  s.symbols.fix();
  return s;
}
// Smith-Waterman under the caller's matrix (MSA_SW_SCORED).  The highest code is the sentinel's, so max_sym is 7, or
// 31 (the *32 entries); up to 7 symbols make the same spec under either, 8..31 a wide one
AlignSpec spec_sw_scored(const char* alphabet, size_t n_sym, const int8_t* sub, size_t max_sym) {
  return with_matrix(spec_sw(0, 0, ""), MSA_SW_SCORED, alphabet, n_sym, sub, max_sym, 1);
}
// global, +1 / 0 over the call's own symbols
AlignSpec spec_nw(const char* preset) {
  return AlignSpec{MSA_OK, MSA_NW_ALIGN, MSA_NW_BANDED, 1, 0, -1, 0, false, {}, SymbolMap(8, preset),
                   GAPS_GLOBAL, true, FOOT_BAND, msa_plan_traceback_nw, BORDER_GLOBAL, false};
}
// global under the caller's matrix.  max_sym: 8, or 32 (the *32 entries); up to 8 symbols make the same spec under
// either, 9..32 a wide one
AlignSpec spec_scored(const char* alphabet, size_t n_sym, const int8_t* sub, size_t max_sym = 8) {
  return with_matrix(spec_nw(""), MSA_NW_SCORED, alphabet, n_sym, sub, max_sym, 0);
}
// ... and with free ends on B: all of A in a substring of B
AlignSpec spec_fit(const char* alphabet, size_t n_sym, const int8_t* sub, size_t max_sym = 8) {
  AlignSpec s = spec_scored(alphabet, n_sym, sub, max_sym);
  s.alg_walk = s.alg_score = MSA_NW_FIT;
  s.banded = false;
  s.border = BORDER_FIT;
  return s;
}
// ... and on A too: a suffix of one sequence against a prefix of the other, or one inside the other.  The walk's ops are
// the whole alignment (both prefixes are free: nothing is appended) and its stop cell is where the alignment begins
AlignSpec spec_overlap(const char* alphabet, size_t n_sym, const int8_t* sub, size_t max_sym = 8) {
  AlignSpec s = spec_fit(alphabet, n_sym, sub, max_sym);
  s.alg_walk = s.alg_score = MSA_NW_OVERLAP;
  s.border = BORDER_NONE;
  s.stop_is_beg = true;
  return s;
}
// The global alignment's borders and walk with a free END instead: the best pair of prefixes.  The start is anchored
// at (0, 0), so the walk's ops are completed along the border exactly as a global alignment's are
AlignSpec spec_extend(const char* alphabet, size_t n_sym, const int8_t* sub, size_t max_sym = 8) {
  AlignSpec s = spec_fit(alphabet, n_sym, sub, max_sym);
  s.alg_walk = s.alg_score = MSA_NW_EXTEND;
  s.border = BORDER_GLOBAL;
  return s;
}
// ... inside a band: the banded global alignment's cells, footprint and border gap (a walk never leaves the band, so
// the gap it stops at is inside it); the band's rule for the sizes is the clip
AlignSpec spec_extend_band(const char* alphabet, size_t n_sym, const int8_t* sub, size_t max_sym = 8) {
  AlignSpec s = spec_extend(alphabet, n_sym, sub, max_sym);
  s.alg_walk = s.alg_score = MSA_NW_EXTEND_BAND;
  s.banded = true;
  s.footprint = FOOT_BAND;
  s.clip_to_band = true;
  return s;
}

// A profile's positions against the caller's alphabet -- a symbol's code is its index --, local (the highest code is
// the sentinel's: 31 symbols), global or fit (32).  prof32: the caller's m x n_sym scores padded to 32 columns (the
// entry owns it).  status MSA_ERR_ARG for a NULL alphabet, n_sym out of range or a duplicate symbol
AlignSpec spec_profile(int mode, const int8_t* prof32, const char* alphabet, size_t n_sym) {
  AlignSpec s = mode == MSA_PROFILE_LOCAL ? spec_sw(0, 0, "") : spec_nw("");
  s.alg_walk = s.alg_score = mode == MSA_PROFILE_LOCAL ? MSA_SW_SCORED
                             : mode == MSA_PROFILE_FIT ? MSA_NW_FIT
                                                       : MSA_NW_SCORED;
  const size_t max_sym = mode == MSA_PROFILE_LOCAL ? 31 : 32;
  s.match = s.mismatch = 0;
  s.banded = false;
  if (mode == MSA_PROFILE_FIT) s.border = BORDER_FIT;
  s.wide = true;
  s.prof = prof32;
  s.symbols = SymbolMap((int)max_sym);
  if (!alphabet || !prof32 || n_sym < 1 || n_sym > max_sym) s.status = MSA_ERR_ARG;
  for (size_t a = 0; s.status == MSA_OK && a < n_sym; ++a)
    if (!s.symbols.add(alphabet[a])) s.status = MSA_ERR_ARG;
  s.symbols.fix();
  return s;
}

// The pairs of a call: pair p is A[a_off[p] .. + m[p]) against B[b_off[p] .. + n[p]).
struct AlignIn {
  const char *A, *B;
  size_t a_len, b_len;
  int64_t np;
  const int64_t *a_off, *m, *b_off, *n;
};
// ... of a single entry: one pair, the whole of A0 against the whole of B0 (owns what `in` points to)
struct OnePairIn {
  int64_t m, n, zero = 0;
  AlignIn in;
  OnePairIn(const char* A0, size_t m_, const char* B0, size_t n_)
      : m((int64_t)m_), n((int64_t)n_), in{A0, B0, m_, n_, 1, &zero, &m, &zero, &n} {}
  OnePairIn(const OnePairIn&) = delete;
};
// Where a pair's two coordinates go: [2 p] and [2 p + 1] of a batch entry's array, a single entry's two pointers
// (p = 0), or nowhere.
struct PairOut {
  int64_t *i = nullptr, *j = nullptr;
  PairOut() = default;
  PairOut(int64_t* i_, int64_t* j_) : i(i_), j(j_) {}
  explicit PairOut(int64_t* ij) : i(ij), j(ij ? ij + 1 : nullptr) {}
  void put(int64_t p, int64_t vi, int64_t vj) const {
    if (i) i[2 * p] = vi;
    if (j) j[2 * p] = vj;
  }
};
struct AlignOut {
  int32_t* score;
  PairOut end, beg;  // local: the end cell, the start cell; overlap: {a_end, b_end}, {a_beg, b_beg}; extension:
                     // {a_end, b_end}, nothing
  PairOut span;      // fit: {beg_j, end_j}, beg_j = -1 without a walk
  char* cigars;      // the CIGARs back to back, each with its NUL; cigar_off[np + 1]
  size_t cigar_cap;
  int64_t* cigar_off;
  int32_t* fin_h = nullptr;  // extension: H(m, n) of every pair, the global alignment's score (fin[0] of its result);
                             // MSA_SCORE_NONE for a pair a banded extension clipped
};
struct GapBand {
  int32_t gap_open, gap_extend;
  int band;
};

// Pairs [p0, p1) of a call as one plan on one stream: admit `bytes`, upload the range's code spans (pairs' offsets
// relative to them: coinciding ranges are sent once), create the plan, run it, walk it, fetch the results, each
// walk's info and ops, complete the ops along the border and append the CIGARs to `all`.  single = 1: a plan for
// one pair spread over many workgroups (the flow / band kernels where they apply), walked by the single walker;
// 0: a batch plan, one workgroup per pair, every pair walked in one msa_plan_traceback_batch launch.
int align_range(const AlignSpec& spec, int single, const GapBand& gb, bool want_tb, const uint8_t* ca,
                const uint8_t* cb, const AlignIn& in, int64_t p0, int64_t p1, size_t bytes, const AlignOut& out,
                std::string& all) {
  const int64_t K = p1 - p0;
  int64_t a_lo = INT64_MAX, a_hi = 0, b_lo = INT64_MAX, b_hi = 0;
  for (int64_t p = p0; p < p1; ++p) {
    a_lo = std::min(a_lo, in.a_off[p]);
    a_hi = std::max(a_hi, in.a_off[p] + in.m[p]);
    b_lo = std::min(b_lo, in.b_off[p]);
    b_hi = std::max(b_hi, in.b_off[p] + in.n[p]);
  }
  std::vector<int64_t> ao((size_t)K), bo((size_t)K);
  for (int64_t k = 0; k < K; ++k) {
    ao[(size_t)k] = in.a_off[p0 + k] - a_lo;
    bo[(size_t)k] = in.b_off[p0 + k] - b_lo;
  }
  const std::vector<int64_t> off = ops_offsets(in.m + p0, in.n + p0, K);
  const int64_t ops_cap = single ? in.m[p0] + in.n[p0] + 2 : off[(size_t)K];
  int rc;
  DeviceCall dc(bytes);
  if ((rc = dc.status()) != MSA_OK) return rc;
  // (a profile call has no row codes: the plan takes its rows [a_lo, a_hi) of the profile and owns their device copy)
  void *dA = spec.prof ? nullptr : dc.alloc((size_t)(a_hi - a_lo)), *dB = dc.alloc((size_t)(b_hi - b_lo));
  if ((!dA && !spec.prof) || !dB) return MSA_ERR_NOMEM;
  if ((dA && (rc = dc.upload(dA, ca + a_lo, (size_t)(a_hi - a_lo)))) ||
      (rc = dc.upload(dB, cb + b_lo, (size_t)(b_hi - b_lo))))
    return rc;
  msa_plan_desc d;
  std::memset(&d, 0, sizeof(d));
  d.alg = want_tb ? spec.alg_walk : spec.alg_score;
  d.cells = want_tb ? MSA_CELLS_DIR : MSA_CELLS_NONE;
  d.match = spec.match;
  d.mismatch = spec.mismatch;
  d.gap_open = gb.gap_open;
  d.gap_extend = gb.gap_extend;
  d.start_type = spec.start_type;
  d.band = gb.band;
  d.track_end = spec.track_end;
  d.single = single;
  d.n_pairs = K;
  d.m = in.m + p0;
  d.n = in.n + p0;
  d.a_off = ao.data();
  d.b_off = bo.data();
  msa_plan* P = nullptr;
  rc = spec.prof ? dc.create_profile_plan(d, spec.prof + 32 * a_lo, a_hi - a_lo, &P)
                 : dc.create_plan(d, spec.scored ? spec.tab : nullptr, &P, spec.wide);
  if (rc != MSA_OK) return rc;
  void *dDir = nullptr, *dOps = nullptr, *dOff = nullptr, *dInfo = nullptr;
  const hipStream_t st = dc.stream();
  if (want_tb) {
    int64_t elems = 0;
    msa_plan_cells_size(P, &elems);
    if (!(dDir = dc.alloc((size_t)elems)) || !(dOps = dc.alloc((size_t)ops_cap)) ||
        (!single && !(dOff = dc.alloc(sizeof(int64_t) * (size_t)(K + 1)))) || !(dInfo = dc.alloc(64 * (size_t)K)))
      return MSA_ERR_NOMEM;
    if (!single && (rc = dc.upload(dOff, off.data(), sizeof(int64_t) * (size_t)(K + 1)))) return rc;
  }
  if ((rc = msa_plan_run(P, (const uint8_t*)dA, (const uint8_t*)dB, dDir, nullptr, nullptr, st))) return rc;
  // the walks on the device: only the ops come back, not the direction bytes
  if (want_tb) {
    if (!single)
      rc = msa_plan_traceback_batch(P, (const uint8_t*)dDir, (uint8_t*)dOps, (const int64_t*)dOff, (int64_t*)dInfo, st);
    else
      rc = spec.walk(P, 0, (const uint8_t*)dDir, (uint8_t*)dOps, ops_cap, (int64_t*)dInfo, st);
    if (rc != MSA_OK) return rc;
  }
  std::vector<msa_pair_result> res((size_t)K);
  if ((rc = msa_plan_results(P, res.data(), st)) != MSA_OK) return rc;
  // (the scores, end cells and span ends are the caller's whatever becomes of the walks)
  for (int64_t k = 0; k < K; ++k) {
    if (out.score) out.score[p0 + k] = res[(size_t)k].score;
    if (out.fin_h) out.fin_h[p0 + k] = res[(size_t)k].fin[0];
    out.end.put(p0 + k, res[(size_t)k].end_i, res[(size_t)k].end_j);
    out.span.put(p0 + k, -1, res[(size_t)k].end_j);
    if (spec.stop_is_beg) out.beg.put(p0 + k, -1, -1);
  }
  if (!want_tb) return MSA_OK;
  std::vector<int64_t> info(8 * (size_t)K);
  std::vector<char> ops;
  if (single) {  // four info words, then as many ops as the walk made
    if ((rc = dc.download(info.data(), dInfo, 4 * sizeof(int64_t))) || (rc = dc.sync()) ||
        (rc = dc.fetch_ops(info.data(), dOps, ops)))
      return rc;
  } else {
    ops.resize((size_t)off[(size_t)K]);
    if ((rc = dc.download(info.data(), dInfo, 64 * (size_t)K)) || (rc = dc.download(ops.data(), dOps, ops.size())) ||
        (rc = dc.sync()))
      return rc;
  }
  for (int64_t k = 0; k < K; ++k) {
    const int64_t* inf = &info[8 * (size_t)k];
    if (inf[3] != 0) return (int)inf[3];  // (a batch: the first failing pair's walk status)
    std::string o(ops.data() + off[(size_t)k], (size_t)inf[0]);
    const int64_t beg_j = complete_border(o, inf[1] - 1, inf[2] - 1, spec.border);
    if (spec.border == BORDER_FIT) out.span.put(p0 + k, beg_j, res[(size_t)k].end_j);
    if (spec.walk_for_beg) out.beg.put(p0 + k, inf[1], inf[2]);
    if (spec.stop_is_beg) out.beg.put(p0 + k, inf[1] - 1, inf[2] - 1);
    if (out.cigars) {
      out.cigar_off[p0 + k] = (int64_t)all.size();
      all += cigar_of(o.data(), o.size());
      all.push_back('\0');
    }
  }
  return MSA_OK;
}

const int64_t kPairLimit = int64_t(1) << 26;  // rows / columns of a pair (msa_sw_align has no limit of its own)

// A banded extension with X-drop termination (msa_xdropapi.inc): its ranges of pairs run the one-wave-per-pair fill and
// walk of msa_xdrop.hip, not a plan, admitted with the compact band form's bytes
struct XDrop {
  int32_t xdrop;
  int64_t* diagonals;  // n_pairs, or nullptr
};
size_t footprint_xdrop(int64_t m, int64_t n, int band, bool dir);
int xdrop_range(const AlignSpec& spec, const GapBand& gb, const XDrop& xd, bool want_tb, const uint8_t* ca,
                const uint8_t* cb, const AlignIn& in, int64_t p0, int64_t p1, size_t bytes, const AlignOut& out,
                std::string& all);

// Every alignment entry: check the arguments (MSA_ERR_ARG; size_lim bounds m and n), the gap rule
// (MSA_ERR_UNSUPPORTED), the band against the lengths (MSA_ERR_ARG; a banded extension clips instead), encode with
// one symbol map for the call, A then B (MSA_ERR_ALPHABET), and only then ask for the device; then align_range chunk by chunk -- consecutive pairs
// whose summed single-pair footprints fit a quarter of the device budget, at most 2^20 of them -- and hand out the
// CIGARs.  xd: a banded extension with X-drop termination -- the same checks in the same order, a band above
// MSA_XDROP_BAND_MAX (after the band of the longest sequence stood in for a wider one) answered with the gap rule's
// MSA_ERR_UNSUPPORTED, and every range through xdrop_range.
int align_pairs(AlignSpec spec, int single, const AlignIn& in0, int64_t size_lim, int32_t gap_open,
                int32_t gap_extend, int64_t band_in, const AlignOut& out, const XDrop* xd = nullptr) {
  if (spec.status != MSA_OK) return spec.status;
  if ((!in0.A && !spec.prof) || !in0.B || !in0.a_off || !in0.m || !in0.b_off || !in0.n || in0.np < 1 ||
      (out.cigars && !out.cigar_off) || band_in < (spec.clip_to_band ? 0 : -1))
    return MSA_ERR_ARG;
  AlignIn in = in0;  // (a banded extension: with the clipped sizes, below)
  int64_t span_max = 0;
  for (int64_t p = 0; p < in.np; ++p) {
    const int64_t m = in.m[p], n = in.n[p], ao = in.a_off[p], bo = in.b_off[p];
    if (m < 1 || n < 1 || m > size_lim || n > size_lim || ao < 0 || bo < 0 ||
        (uint64_t)ao + (uint64_t)m > in.a_len || (uint64_t)bo + (uint64_t)n > in.b_len)
      return MSA_ERR_ARG;
    span_max = std::max(span_max, std::max(m, n));
  }
  if (spec.gaps == GAPS_LOCAL ? (spec.match < -128 || spec.match > 127 || spec.mismatch < -128 || spec.mismatch > 127 ||
                                 gap_open < 0 || gap_extend < 0)
                              : (gap_extend < 0 || gap_open < gap_extend))
    return MSA_ERR_UNSUPPORTED;
  if (xd && std::min(band_in, span_max) > MSA_XDROP_BAND_MAX) return MSA_ERR_UNSUPPORTED;
  if (!spec.banded) band_in = -1;
  std::vector<int64_t> cm, cn;  // a banded extension's sizes: every pair's in-band prefixes (offsets stay)
  if (spec.clip_to_band) {
    cm.assign(in.m, in.m + in.np);
    cn.assign(in.n, in.n + in.np);
    for (int64_t p = 0; p < in.np; ++p) extend_band_clip(in.m[p], in.n[p], band_in, cm[(size_t)p], cn[(size_t)p]);
    in.m = cm.data();
    in.n = cn.data();
  } else if (band_in >= 0) {
    for (int64_t p = 0; p < in.np; ++p)
      if (std::llabs(in.m[p] - in.n[p]) > band_in) return MSA_ERR_ARG;
  }
  // (a band that holds every cell of every pair is no band -- but for a banded extension, whose plan kind needs one:
  // there it is the band of the longest sequence, which holds every cell just as well)
  const GapBand gb{gap_open, gap_extend,
                   spec.clip_to_band ? (int)std::min(band_in, span_max)
                                     : ((band_in < 0 || band_in >= span_max) ? -1 : (int)band_in)};
  std::vector<uint8_t> ca(spec.prof ? 0 : in.a_len), cb(in.b_len);
  int rc = spec.prof ? MSA_OK : spec.symbols.encode(in.A, in.a_len, ca.data());
  if (rc == MSA_OK) rc = spec.symbols.encode(in.B, in.b_len, cb.data());
  if (rc != MSA_OK) return rc;
  if ((rc = ensure_device()) != MSA_OK) return rc;
  const bool want_tb = out.cigars || (spec.walk_for_beg && (out.beg.i || out.beg.j));
  // (a profile call: every plan of it holds its pairs' rows of the profile, 32 B each)
  auto fp = [&](int64_t p) -> size_t {
    const size_t rows = spec.prof ? 32 * (size_t)in.m[p] : 0;
    if (xd) return footprint_xdrop(in.m[p], in.n[p], gb.band, want_tb);
    if (spec.footprint == FOOT_BAND) return rows + footprint_nw(in.m[p], in.n[p], gb.band, want_tb);
    return rows + (want_tb ? footprint_dir(in.m[p], in.n[p]) : footprint_planes(in.m[p], in.n[p], 0, 1));
  };
  int64_t binfo[5];
  admission().info(current_device(), binfo);
  const size_t quarter = (size_t)binfo[0] / 4;
  std::string all;  // the CIGARs, back to back
  for (int64_t p0 = 0, p1; p0 < in.np; p0 = p1) {
    size_t bytes = fp(p0);
    p1 = p0 + 1;
    while (p1 < in.np && p1 - p0 < (int64_t(1) << 20) && bytes + fp(p1) <= quarter) bytes += fp(p1++);
    rc = xd ? xdrop_range(spec, gb, *xd, want_tb, ca.data(), cb.data(), in, p0, p1, bytes, out, all)
            : align_range(spec, single, gb, want_tb, ca.data(), cb.data(), in, p0, p1, bytes, out, all);
    if (rc != MSA_OK) return rc;
  }
  // (a clipped pair has no H(m, n): its fill ended at (m', n'))
  for (int64_t p = 0; spec.clip_to_band && out.fin_h && p < in.np; ++p)
    if (in.m[p] != in0.m[p] || in.n[p] != in0.n[p]) out.fin_h[p] = MSA_SCORE_NONE;
  if (out.cigars) {
    out.cigar_off[in.np] = (int64_t)all.size();
    if (all.size() > out.cigar_cap) return MSA_ERR_CAPACITY;
    std::memcpy(out.cigars, all.data(), all.size());
  }
  return MSA_OK;
}

}  // namespace

extern "C" {

int msa_sw_align(const char* A0, size_t m, const char* B0, size_t n, int32_t match, int32_t mismatch,
                 int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* end_i, int64_t* end_j,
                 int64_t* beg_i, int64_t* beg_j, char* cigar, size_t cigar_cap) {
  const OnePairIn one(A0, m, B0, n);
  int64_t coff[2];
  const AlignOut out{score, PairOut(end_i, end_j), PairOut(beg_i, beg_j), PairOut(), cigar, cigar_cap, coff};
  return align_pairs(spec_sw(match, mismatch, "ACGT"), 1, one.in, INT64_MAX, gap_open, gap_extend, -1, out);
}

int msa_nw_align(const char* A0, size_t m, const char* B0, size_t n, int32_t gap_open, int32_t gap_extend,
                 int64_t band, int32_t* score, char* cigar, size_t cigar_cap) {
  const OnePairIn one(A0, m, B0, n);
  int64_t coff[2];
  const AlignOut out{score, PairOut(), PairOut(), PairOut(), cigar, cigar_cap, coff};
  return align_pairs(spec_nw("ACGT"), 1, one.in, kPairLimit, gap_open, gap_extend, band, out);
}

int msa_nw_align_scored(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                        const int8_t* sub, int32_t gap_open, int32_t gap_extend, int64_t band, int32_t* score,
                        char* cigar, size_t cigar_cap) {
  const OnePairIn one(A0, m, B0, n);
  int64_t coff[2];
  const AlignOut out{score, PairOut(), PairOut(), PairOut(), cigar, cigar_cap, coff};
  return align_pairs(spec_scored(alphabet, n_sym, sub), 1, one.in, kPairLimit, gap_open, gap_extend, band, out);
}

int msa_fit_align(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                  const int8_t* sub, int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* beg_j,
                  int64_t* end_j, char* cigar, size_t cigar_cap) {
  const OnePairIn one(A0, m, B0, n);
  int64_t coff[2], be[2] = {-1, -1};
  const AlignOut out{score, PairOut(), PairOut(), PairOut(be), cigar, cigar_cap, coff};
  const int rc = align_pairs(spec_fit(alphabet, n_sym, sub), 1, one.in, kPairLimit, gap_open, gap_extend, -1, out);
  // (a cigar too small still has its score and span)
  if (rc == MSA_OK || rc == MSA_ERR_CAPACITY) {
    if (beg_j) *beg_j = be[0];
    if (end_j) *end_j = be[1];
  }
  return rc;
}

int msa_nw_align_scored32(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                          const int8_t* sub, int32_t gap_open, int32_t gap_extend, int64_t band, int32_t* score,
                          char* cigar, size_t cigar_cap) {
  const OnePairIn one(A0, m, B0, n);
  int64_t coff[2];
  const AlignOut out{score, PairOut(), PairOut(), PairOut(), cigar, cigar_cap, coff};
  return align_pairs(spec_scored(alphabet, n_sym, sub, 32), 1, one.in, kPairLimit, gap_open, gap_extend, band, out);
}

int msa_fit_align32(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                    const int8_t* sub, int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* beg_j,
                    int64_t* end_j, char* cigar, size_t cigar_cap) {
  const OnePairIn one(A0, m, B0, n);
  int64_t coff[2], be[2] = {-1, -1};
  const AlignOut out{score, PairOut(), PairOut(), PairOut(be), cigar, cigar_cap, coff};
  const int rc = align_pairs(spec_fit(alphabet, n_sym, sub, 32), 1, one.in, kPairLimit, gap_open, gap_extend, -1, out);
  if (rc == MSA_OK || rc == MSA_ERR_CAPACITY) {
    if (beg_j) *beg_j = be[0];
    if (end_j) *end_j = be[1];
  }
  return rc;
}

int msa_sw_align_batch(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                       const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n, int32_t match,
                       int32_t mismatch, int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* end_ij,
                       int64_t* beg_ij, char* cigars, size_t cigar_cap, int64_t* cigar_off) {
  const AlignIn in{A, B, a_len, b_len, n_pairs, a_off, m, b_off, n};
  const AlignOut out{score, PairOut(end_ij), PairOut(beg_ij), PairOut(), cigars, cigar_cap, cigar_off};
  return align_pairs(spec_sw(match, mismatch, ""), 0, in, kPairLimit, gap_open, gap_extend, -1, out);
}

int msa_nw_align_batch(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                       const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                       int32_t gap_open, int32_t gap_extend, int64_t band, int32_t* score, char* cigars,
                       size_t cigar_cap, int64_t* cigar_off) {
  const AlignIn in{A, B, a_len, b_len, n_pairs, a_off, m, b_off, n};
  const AlignOut out{score, PairOut(), PairOut(), PairOut(), cigars, cigar_cap, cigar_off};
  return align_pairs(spec_nw(""), 0, in, kPairLimit, gap_open, gap_extend, band, out);
}

int msa_nw_align_batch_scored(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                              const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                              const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                              int32_t gap_extend, int64_t band, int32_t* score, char* cigars, size_t cigar_cap,
                              int64_t* cigar_off) {
  const AlignIn in{A, B, a_len, b_len, n_pairs, a_off, m, b_off, n};
  const AlignOut out{score, PairOut(), PairOut(), PairOut(), cigars, cigar_cap, cigar_off};
  return align_pairs(spec_scored(alphabet, n_sym, sub), 0, in, kPairLimit, gap_open, gap_extend, band, out);
}

int msa_fit_align_batch(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                        const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                        const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                        int32_t gap_extend, int32_t* score, int64_t* beg_end, char* cigars, size_t cigar_cap,
                        int64_t* cigar_off) {
  if (!beg_end) return MSA_ERR_ARG;
  const AlignIn in{A, B, a_len, b_len, n_pairs, a_off, m, b_off, n};
  const AlignOut out{score, PairOut(), PairOut(), PairOut(beg_end), cigars, cigar_cap, cigar_off};
  return align_pairs(spec_fit(alphabet, n_sym, sub), 0, in, kPairLimit, gap_open, gap_extend, -1, out);
}

int msa_nw_align_batch_scored32(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                                const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                                const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                                int32_t gap_extend, int64_t band, int32_t* score, char* cigars, size_t cigar_cap,
                                int64_t* cigar_off) {
  const AlignIn in{A, B, a_len, b_len, n_pairs, a_off, m, b_off, n};
  const AlignOut out{score, PairOut(), PairOut(), PairOut(), cigars, cigar_cap, cigar_off};
  return align_pairs(spec_scored(alphabet, n_sym, sub, 32), 0, in, kPairLimit, gap_open, gap_extend, band, out);
}

int msa_fit_align_batch32(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                          const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                          const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                          int32_t gap_extend, int32_t* score, int64_t* beg_end, char* cigars, size_t cigar_cap,
                          int64_t* cigar_off) {
  if (!beg_end) return MSA_ERR_ARG;
  const AlignIn in{A, B, a_len, b_len, n_pairs, a_off, m, b_off, n};
  const AlignOut out{score, PairOut(), PairOut(), PairOut(beg_end), cigars, cigar_cap, cigar_off};
  return align_pairs(spec_fit(alphabet, n_sym, sub, 32), 0, in, kPairLimit, gap_open, gap_extend, -1, out);
}

// ---- overlap alignment (MSA_NW_OVERLAP): the fit entries with both of A's ends free as well; 8 symbols, or 32 for
// the *32 entries
static int overlap_align(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                         const int8_t* sub, size_t max_sym, int32_t gap_open, int32_t gap_extend, int32_t* score,
                         int64_t* beg_ij, int64_t* end_ij, char* cigar, size_t cigar_cap) {
  const OnePairIn one(A0, m, B0, n);
  int64_t coff[2];
  const AlignOut out{score, PairOut(end_ij), PairOut(beg_ij), PairOut(), cigar, cigar_cap, coff};
  return align_pairs(spec_overlap(alphabet, n_sym, sub, max_sym), 1, one.in, kPairLimit, gap_open, gap_extend, -1, out);
}
static int overlap_align_batch(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                               const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                               const char* alphabet, size_t n_sym, const int8_t* sub, size_t max_sym,
                               int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* beg_ij,
                               int64_t* end_ij, char* cigars, size_t cigar_cap, int64_t* cigar_off) {
  if (!beg_ij || !end_ij) return MSA_ERR_ARG;
  const AlignIn in{A, B, a_len, b_len, n_pairs, a_off, m, b_off, n};
  const AlignOut out{score, PairOut(end_ij), PairOut(beg_ij), PairOut(), cigars, cigar_cap, cigar_off};
  return align_pairs(spec_overlap(alphabet, n_sym, sub, max_sym), 0, in, kPairLimit, gap_open, gap_extend, -1, out);
}

int msa_overlap_align(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                      const int8_t* sub, int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* beg_ij,
                      int64_t* end_ij, char* cigar, size_t cigar_cap) {
  return overlap_align(A0, m, B0, n, alphabet, n_sym, sub, 8, gap_open, gap_extend, score, beg_ij, end_ij, cigar,
                       cigar_cap);
}

int msa_overlap_align32(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                        const int8_t* sub, int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* beg_ij,
                        int64_t* end_ij, char* cigar, size_t cigar_cap) {
  return overlap_align(A0, m, B0, n, alphabet, n_sym, sub, 32, gap_open, gap_extend, score, beg_ij, end_ij, cigar,
                       cigar_cap);
}

int msa_overlap_align_batch(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                            const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                            const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                            int32_t gap_extend, int32_t* score, int64_t* beg_ij, int64_t* end_ij, char* cigars,
                            size_t cigar_cap, int64_t* cigar_off) {
  return overlap_align_batch(A, a_len, B, b_len, n_pairs, a_off, m, b_off, n, alphabet, n_sym, sub, 8, gap_open,
                             gap_extend, score, beg_ij, end_ij, cigars, cigar_cap, cigar_off);
}

int msa_overlap_align_batch32(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                              const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                              const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                              int32_t gap_extend, int32_t* score, int64_t* beg_ij, int64_t* end_ij, char* cigars,
                              size_t cigar_cap, int64_t* cigar_off) {
  return overlap_align_batch(A, a_len, B, b_len, n_pairs, a_off, m, b_off, n, alphabet, n_sym, sub, 32, gap_open,
                             gap_extend, score, beg_ij, end_ij, cigars, cigar_cap, cigar_off);
}

// ---- extension alignment (MSA_NW_EXTEND): the overlap entries with {a_end, b_end} and H(m, n) for their two cells;
// 8 symbols, or 32 for the *32 entries.  banded (MSA_NW_EXTEND_BAND, the *_banded entries): inside `band`, clipped
static int extend_align(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                        const int8_t* sub, size_t max_sym, int32_t gap_open, int32_t gap_extend, int32_t* score,
                        int64_t* end_ij, int32_t* global_score, char* cigar, size_t cigar_cap, bool banded = false,
                        int64_t band = -1) {
  const OnePairIn one(A0, m, B0, n);
  int64_t coff[2];
  const AlignOut out{score, PairOut(end_ij), PairOut(), PairOut(), cigar, cigar_cap, coff, global_score};
  const AlignSpec spec = banded ? spec_extend_band(alphabet, n_sym, sub, max_sym)
                                : spec_extend(alphabet, n_sym, sub, max_sym);
  return align_pairs(spec, 1, one.in, kPairLimit, gap_open, gap_extend, band, out);
}
static int extend_align_batch(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                              const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                              const char* alphabet, size_t n_sym, const int8_t* sub, size_t max_sym,
                              int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* end_ij,
                              int32_t* global_score, char* cigars, size_t cigar_cap, int64_t* cigar_off,
                              bool banded = false, int64_t band = -1) {
  if (!end_ij) return MSA_ERR_ARG;
  const AlignIn in{A, B, a_len, b_len, n_pairs, a_off, m, b_off, n};
  const AlignOut out{score, PairOut(end_ij), PairOut(), PairOut(), cigars, cigar_cap, cigar_off, global_score};
  const AlignSpec spec = banded ? spec_extend_band(alphabet, n_sym, sub, max_sym)
                                : spec_extend(alphabet, n_sym, sub, max_sym);
  return align_pairs(spec, 0, in, kPairLimit, gap_open, gap_extend, band, out);
}

int msa_extend_align(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                     const int8_t* sub, int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* end_ij,
                     int32_t* global_score, char* cigar, size_t cigar_cap) {
  return extend_align(A0, m, B0, n, alphabet, n_sym, sub, 8, gap_open, gap_extend, score, end_ij, global_score, cigar,
                      cigar_cap);
}

int msa_extend_align32(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                       const int8_t* sub, int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* end_ij,
                       int32_t* global_score, char* cigar, size_t cigar_cap) {
  return extend_align(A0, m, B0, n, alphabet, n_sym, sub, 32, gap_open, gap_extend, score, end_ij, global_score, cigar,
                      cigar_cap);
}

int msa_extend_align_batch(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                           const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                           const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                           int32_t gap_extend, int32_t* score, int64_t* end_ij, int32_t* global_score, char* cigars,
                           size_t cigar_cap, int64_t* cigar_off) {
  return extend_align_batch(A, a_len, B, b_len, n_pairs, a_off, m, b_off, n, alphabet, n_sym, sub, 8, gap_open,
                            gap_extend, score, end_ij, global_score, cigars, cigar_cap, cigar_off);
}

int msa_extend_align_batch32(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                             const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                             const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                             int32_t gap_extend, int32_t* score, int64_t* end_ij, int32_t* global_score,
                             char* cigars, size_t cigar_cap, int64_t* cigar_off) {
  return extend_align_batch(A, a_len, B, b_len, n_pairs, a_off, m, b_off, n, alphabet, n_sym, sub, 32, gap_open,
                            gap_extend, score, end_ij, global_score, cigars, cigar_cap, cigar_off);
}

int msa_extend_band_clip(int64_t m, int64_t n, int64_t band, int64_t* m_eff, int64_t* n_eff) {
  int64_t me, ne;
  if (!extend_band_clip(m, n, band, me, ne)) return MSA_ERR_ARG;
  if (m_eff) *m_eff = me;
  if (n_eff) *n_eff = ne;
  return MSA_OK;
}

int msa_extend_align_banded(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                            const int8_t* sub, int32_t gap_open, int32_t gap_extend, int64_t band, int32_t* score,
                            int64_t* end_ij, int32_t* global_score, char* cigar, size_t cigar_cap) {
  return extend_align(A0, m, B0, n, alphabet, n_sym, sub, 8, gap_open, gap_extend, score, end_ij, global_score, cigar,
                      cigar_cap, true, band);
}

int msa_extend_align_banded32(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                              const int8_t* sub, int32_t gap_open, int32_t gap_extend, int64_t band, int32_t* score,
                              int64_t* end_ij, int32_t* global_score, char* cigar, size_t cigar_cap) {
  return extend_align(A0, m, B0, n, alphabet, n_sym, sub, 32, gap_open, gap_extend, score, end_ij, global_score, cigar,
                      cigar_cap, true, band);
}

int msa_extend_align_batch_banded(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                                  const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                                  const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                                  int32_t gap_extend, int64_t band, int32_t* score, int64_t* end_ij,
                                  int32_t* global_score, char* cigars, size_t cigar_cap, int64_t* cigar_off) {
  return extend_align_batch(A, a_len, B, b_len, n_pairs, a_off, m, b_off, n, alphabet, n_sym, sub, 8, gap_open,
                            gap_extend, score, end_ij, global_score, cigars, cigar_cap, cigar_off, true, band);
}

int msa_extend_align_batch_banded32(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                                    const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                                    const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                                    int32_t gap_extend, int64_t band, int32_t* score, int64_t* end_ij,
                                    int32_t* global_score, char* cigars, size_t cigar_cap, int64_t* cigar_off) {
  return extend_align_batch(A, a_len, B, b_len, n_pairs, a_off, m, b_off, n, alphabet, n_sym, sub, 32, gap_open,
                            gap_extend, score, end_ij, global_score, cigars, cigar_cap, cigar_off, true, band);
}

// ---- local alignment under a substitution matrix (MSA_SW_SCORED): msa_sw_align / msa_sw_align_batch with the
// caller's alphabet and matrix in place of match / mismatch; 7 symbols, or 31 for the *32 entries
static int sw_align_scored(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                           const int8_t* sub, size_t max_sym, int32_t gap_open, int32_t gap_extend, int32_t* score,
                           int64_t* end_i, int64_t* end_j, int64_t* beg_i, int64_t* beg_j, char* cigar,
                           size_t cigar_cap) {
  const OnePairIn one(A0, m, B0, n);
  int64_t coff[2];
  const AlignOut out{score, PairOut(end_i, end_j), PairOut(beg_i, beg_j), PairOut(), cigar, cigar_cap, coff};
  return align_pairs(spec_sw_scored(alphabet, n_sym, sub, max_sym), 1, one.in, INT64_MAX, gap_open, gap_extend, -1,
                     out);
}
static int sw_align_batch_scored(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                                 const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                                 const char* alphabet, size_t n_sym, const int8_t* sub, size_t max_sym,
                                 int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* end_ij,
                                 int64_t* beg_ij, char* cigars, size_t cigar_cap, int64_t* cigar_off) {
  const AlignIn in{A, B, a_len, b_len, n_pairs, a_off, m, b_off, n};
  const AlignOut out{score, PairOut(end_ij), PairOut(beg_ij), PairOut(), cigars, cigar_cap, cigar_off};
  return align_pairs(spec_sw_scored(alphabet, n_sym, sub, max_sym), 0, in, kPairLimit, gap_open, gap_extend, -1, out);
}

int msa_sw_align_scored(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                        const int8_t* sub, int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* end_i,
                        int64_t* end_j, int64_t* beg_i, int64_t* beg_j, char* cigar, size_t cigar_cap) {
  return sw_align_scored(A0, m, B0, n, alphabet, n_sym, sub, 7, gap_open, gap_extend, score, end_i, end_j, beg_i,
                         beg_j, cigar, cigar_cap);
}

int msa_sw_align_scored32(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                          const int8_t* sub, int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* end_i,
                          int64_t* end_j, int64_t* beg_i, int64_t* beg_j, char* cigar, size_t cigar_cap) {
  return sw_align_scored(A0, m, B0, n, alphabet, n_sym, sub, 31, gap_open, gap_extend, score, end_i, end_j, beg_i,
                         beg_j, cigar, cigar_cap);
}

int msa_sw_align_batch_scored(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                              const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                              const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                              int32_t gap_extend, int32_t* score, int64_t* end_ij, int64_t* beg_ij, char* cigars,
                              size_t cigar_cap, int64_t* cigar_off) {
  return sw_align_batch_scored(A, a_len, B, b_len, n_pairs, a_off, m, b_off, n, alphabet, n_sym, sub, 7, gap_open,
                               gap_extend, score, end_ij, beg_ij, cigars, cigar_cap, cigar_off);
}

int msa_sw_align_batch_scored32(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                                const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                                const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                                int32_t gap_extend, int32_t* score, int64_t* end_ij, int64_t* beg_ij, char* cigars,
                                size_t cigar_cap, int64_t* cigar_off) {
  return sw_align_batch_scored(A, a_len, B, b_len, n_pairs, a_off, m, b_off, n, alphabet, n_sym, sub, 31, gap_open,
                               gap_extend, score, end_ij, beg_ij, cigars, cigar_cap, cigar_off);
}

// ---- profile alignment: the rows are the m positions of a position-specific profile (msa_plan_create_profile), every
// pair all of them against one sequence of B; the three modes are MSA_SW_SCORED, MSA_NW_SCORED and MSA_NW_FIT plans
// and their entries' walks, with one result shape: a start and an end cell
static int profile_align(int mode, int single, const int8_t* prof, size_t m, const char* B, size_t b_len,
                         int64_t n_pairs, const int64_t* b_off, const int64_t* n, const char* alphabet, size_t n_sym,
                         int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* beg_ij, int64_t* end_ij,
                         char* cigars, size_t cigar_cap, int64_t* cigar_off) {
  if (mode != MSA_PROFILE_LOCAL && mode != MSA_PROFILE_GLOBAL && mode != MSA_PROFILE_FIT) return MSA_ERR_ARG;
  // the caller's m x n_sym rows padded to the plan's 32 columns (codes no symbol has score 0; a local plan puts
  // its sentinel's score into column 31 itself)
  const bool sized = prof && n_sym >= 1 && n_sym <= 32 && m >= 1 && m <= (size_t)kPairLimit;
  std::vector<int8_t> prof32(sized ? 32 * m : 0);
  for (size_t r = 0; sized && r < m; ++r) std::copy(prof + n_sym * r, prof + n_sym * (r + 1), &prof32[32 * r]);
  const AlignSpec spec = spec_profile(mode, sized ? prof32.data() : nullptr, alphabet, n_sym);
  if (spec.status != MSA_OK || !sized || n_pairs < 1 || n_pairs > kPairLimit) return MSA_ERR_ARG;
  const std::vector<int64_t> zero((size_t)n_pairs, 0), ms((size_t)n_pairs, (int64_t)m);
  std::vector<int64_t> span(mode == MSA_PROFILE_FIT ? 2 * (size_t)n_pairs : 0, -1);
  const AlignIn in{nullptr, B, m, b_len, n_pairs, zero.data(), ms.data(), b_off, n};
  const bool local = mode == MSA_PROFILE_LOCAL;
  const AlignOut out{score, local ? PairOut(end_ij) : PairOut(), local ? PairOut(beg_ij) : PairOut(),
                     mode == MSA_PROFILE_FIT ? PairOut(span.data()) : PairOut(), cigars, cigar_cap, cigar_off};
  const int rc = align_pairs(spec, single, in, kPairLimit, gap_open, gap_extend, -1, out);
  // (a cigar buffer too small still has its scores and cells)
  if (!local && (rc == MSA_OK || rc == MSA_ERR_CAPACITY))
    for (int64_t p = 0; p < n_pairs; ++p) {
      const bool fit = mode == MSA_PROFILE_FIT;
      PairOut(beg_ij).put(p, 0, fit ? span[2 * (size_t)p] : 0);
      PairOut(end_ij).put(p, (int64_t)m, fit ? span[2 * (size_t)p + 1] : n[p]);
    }
  return rc;
}

int msa_profile_align(int mode, const int8_t* prof, size_t m, const char* B0, size_t n, const char* alphabet,
                      size_t n_sym, int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* beg_ij,
                      int64_t* end_ij, char* cigar, size_t cigar_cap) {
  const int64_t zero = 0, n1 = (int64_t)n;
  int64_t coff[2];
  return profile_align(mode, 1, prof, m, B0, n, 1, &zero, &n1, alphabet, n_sym, gap_open, gap_extend, score, beg_ij,
                       end_ij, cigar, cigar_cap, coff);
}

int msa_profile_align_batch(int mode, const int8_t* prof, size_t m, const char* B, size_t b_len, int64_t n_pairs,
                            const int64_t* b_off, const int64_t* n, const char* alphabet, size_t n_sym,
                            int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* beg_ij, int64_t* end_ij,
                            char* cigars, size_t cigar_cap, int64_t* cigar_off) {
  return profile_align(mode, 0, prof, m, B, b_len, n_pairs, b_off, n, alphabet, n_sym, gap_open, gap_extend, score,
                       beg_ij, end_ij, cigars, cigar_cap, cigar_off);
}

}  // extern "C"

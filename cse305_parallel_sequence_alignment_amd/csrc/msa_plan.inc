// msa_plan.inc -- plan creation (included by msa_capi.hip): msa_plan_create decides from the description which kernel
// family a plan launches, lays the pairs out, and lets that family's shape function fill the plan's launch records.
#ifndef MSA_CHUNK_WARM
// C3's pair converges within ~900 rows, its synthetic mutated copy within ~1,024; 20 stripes = 1,280 rows
#define MSA_CHUNK_WARM 20  // warm-up stripes of a chunk (both chunked paths' default)
#endif
#ifndef MSA_CHUNK_MIN
#define MSA_CHUNK_MIN 10   // stripes per chunk of the chunked stripe launch, at least
#endif

namespace {

// the kernel family a plan launches (choose_mode); the numbers are what msa_plan_launch_info reports
enum PlanMode {
  PM_STRIPE = 0,        // stripe_kernel: a batch, or one pair in items of W stripes
  PM_FLOW = 1,          // flow_kernel (+ pass-2 blocks in the launch, or flow_fill_kernel behind it)
  PM_CHUNKED = 2,       // stripe_kernel over chunks of one banded pair, the exact launch behind it
  PM_SPLIT = 3,         // stripe_kernel, a small batch split into items (kp.single == 3)
  PM_BAND = 4,          // band_kernel, the exact launch alone
  PM_BAND_CHUNKED = 5,  // band_kernel over chunks, the exact launch behind it
  PM_CFLOW = 6,         // cflow_kernel: packed score-only couples
};

// one kernel launch of a plan (fn == nullptr: the plan has no such launch)
struct Launch {
  kfn_t fn = nullptr;
  int grid = 1, threads = 64;
  size_t lds = 0;
  msa_kparams kp{};
};

// queues a launch with the run's arguments, under the launch's own kernel parameters and the given epoch
int enqueue(const Launch& l, KArgs a, uint32_t epoch, hipStream_t st) {
  a.kp = l.kp;
  a.kp.epoch = epoch;
  hipLaunchKernelGGL(l.fn, dim3(l.grid), dim3(l.threads), l.lds, st, a);
  HIPCHK(hipGetLastError());
  return MSA_OK;
}

// diagnostic environment variables: an integer (dflt when unset), a string value
long env_int(const char* name, long dflt) {
  const char* e = std::getenv(name);
  return e ? std::strtol(e, nullptr, 10) : dflt;
}
bool env_is(const char* name, const char* value) {
  const char* e = std::getenv(name);
  return e && std::strcmp(e, value) == 0;
}

inline int stripes_of(int64_t m, int R = 1) { return (int)((m + 64 * R - 1) / (64 * R)); }

// epochs are process-wide, so granules left in a pooled block by an earlier plan
// can never carry the epoch a new run polls for (0 is never handed out)
uint32_t next_epoch() {
  uint32_t ep = g_epoch.fetch_add(1) + 1;
  if (ep == 0) ep = g_epoch.fetch_add(1) + 1;
  return ep;
}

}  // namespace

struct msa_plan {
  msa_plan_desc d;
  PlanMode mode = PM_STRIPE;
  Launch main;   // the DP launch (chunked modes: the chunks)
  Launch exact;  // chunked modes: the exact single-mode launch, queued behind the chunks; it exits at
                 // once unless a chunk failed to converge (rank convergence, msa_kernels.hip)
  Launch fill;   // flow, long pairs: pass 2 as a launch of its own behind pass 1 (flow_fill_kernel)
  int nc = 1;
  int tp = 0;  // end-cell tracking (choose_algorithm): 0 none, 1 compare-select, 2 packed (value, step) key
  int KS = MSA_KS_BATCH;    // DP steps per phase
  std::vector<msa_pair_desc> pairs;
  int64_t total_stripes = 0, cells_elems = 0;
  bool flow2 = false;  // flow: + pass-2 blocks (O_H, direction bytes), inside the launch or as `fill`
  bool fused_reduce = false;  // the pass-2 blocks write the pair result (fl_block_done): no reduce launch
  unsigned long long *d_br = nullptr, *d_snap = nullptr;
  int4* d_blk = nullptr;
  int* d_order = nullptr;
  bool timing = true;  // record HIP events around the DP kernel (msa_plan_last_kernel_ms)
  bool timed = false;  // events of the last run exist
  int R = 1;      // flow kernel rows per lane
  int nflow = 0;  // two-pass: pass-1 workgroups (the rest of the grid runs pass-2 blocks)
  int brw = 0, nseg = 0, nblk = 0;
  int ps = FL_PS;  // phases per pass-2 segment (FL_PS_FILL when pass 2 is a launch of its own)
  int gslots = 0;  // granule slots the family's items publish into (0: no granule buffer)
  int gbuf_stride = 0;
  // device
  msa_pair_desc* d_pairs = nullptr;
  msa_stripe_meta* d_meta = nullptr;
  // [0] ticket, [4..11] per-XCD item chunks; flow kernels: [32] arrival, [64] pass-2 blocks, each
  // in a 128-byte line of its own (thousands of pass-2 waves claim blocks while pass-1 workgroups
  // claim their items: on one line the item claims queued ~16 us behind them).  Reset every run.
  int* d_ticket = nullptr;
  int* d_err = nullptr;     // sticky error word: set by a kernel wait that hit its spin limit; cleared
                            // only at plan creation and by msa_plan_clear_error
  unsigned long long* d_gbuf = nullptr;
  uint8_t* d_cod = nullptr;                // MSA_NCOPY byte-shifted padded column-code copies
  msa_pair_desc* d_segs = nullptr;         // distinct column sequences (b_off, n, cod_off)
  std::vector<msa_pair_desc> segs;
  int64_t cod_copy = 0;                    // bytes per copy
  PairResult* d_res = nullptr;
  unsigned long long* d_sum = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  uint32_t epoch = 0;
  unsigned long long* stamps = nullptr;  // diagnostic build
  std::vector<hipStream_t> streams;      // every stream work of this plan was queued on
                                         // (msa_plan_destroy waits on all of them)
  std::vector<std::pair<void*, size_t>> blocks;  // pooled device blocks owned by the plan
  // chunked banded single pair (main.kp.single == 2)
  int n_chunks = 0;
  int* d_ck = nullptr;  // [chunk][2][2][ckw] band states (msa_kernels.hip)
  int ckw = 0;
  int* d_dk = nullptr;    // per-chunk constant d_k
  int* d_okk = nullptr;   // per-chunk converged flag
  int* d_skip = nullptr;  // 1: every chunk converged (the exact launch exits)
  bool h16 = false;       // band_kernel chunks >= 1 write int16 cells to d_h16 (chunk_add_kernel widens)
  int16_t* d_h16 = nullptr;
  // algorithms that score from a table: the substitution scores S[8 a + b] (row code a, column code b; 1 / 0 for
  // MSA_NW_BANDED and MSA_NW_ALIGN) and their device table, one 8-byte profile per row code in the launch's space
  // (alloc_buffers); 5-bit codes (msa_plan_create_scored32): S[32 a + b], uploaded as it is (1,024 bytes)
  // MSA_SW_SCORED: either layout, MSA_VIRT_SCORE in the virtual code's row and column
  int8_t sub[1024] = {};
  uint2* d_sub = nullptr;
  // a profile plan (msa_plan_create_profile) scores from this instead: prof_rows rows of 32 int8, row r = the scores of
  // profile position r by column code, the plan's own device copy (16-byte aligned: a pooled block; a lane loads its
  // row as two dwordx4).  MSA_SW_SCORED: MSA_VIRT_SCORE in column 31 of every row.  The host copy lives until the
  // upload (alloc_buffers)
  std::vector<int8_t> prof;
  int64_t prof_rows = 0;
  uint4* d_prof = nullptr;

  bool chunked() const { return mode == PM_CHUNKED || mode == PM_BAND_CHUNKED; }
  void note_stream(hipStream_t s) {
    if (std::find(streams.begin(), streams.end(), s) == streams.end()) streams.push_back(s);
  }
  // a pooled device block of `bytes`, owned by the plan
  template <class T>
  bool alloc(T** p, size_t bytes) {
    void* q = dev_pool().get(bytes);
    if (!q) return false;
    blocks.emplace_back(q, bytes);
    *p = (T*)q;
    return true;
  }
  // ... zero-filled (fill: the byte)
  template <class T>
  bool alloc_set(T** p, size_t bytes, int fill = 0) {
    return alloc(p, bytes) && hipMemset(*p, fill, bytes) == hipSuccess;
  }
};

namespace {

struct Extents { int S = 0, P = 0; };  // most stripes / most 16-step layout blocks of any pair

// what walks the plan's direction bytes: its algorithm's walker if the plan wrote bytes -- and, for the walk that
// starts at the fill's end cell, tracked one (an MSA_SW_SCORED plan always does) -- else TB_NONE
msa_walk walker_of(const msa_plan* P) {
  const msa_walk w = msa_alg_info_of(P->main.kp.alg).walker;
  return (P->d.cells != MSA_CELLS_DIR || (w == TB_SW && !P->d.track_end)) ? TB_NONE : w;
}
// the algorithms that score as MSA_NW_SCORED does (table or match / mismatch) under free ends, on the stripe kernel alone
bool free_ends(int alg) {
  return alg == MSA_NW_FIT || alg == MSA_NW_OVERLAP || alg == MSA_NW_EXTEND || alg == MSA_NW_EXTEND_BAND;
}

// ---- step 1: kernel algorithm and end-cell tracking mode --------------------------------------------
// wide32: a 32 x 32 table over 5-bit codes (msa_plan_create_scored32: MSA_NW_SCORED, MSA_NW_FIT, MSA_NW_OVERLAP,
// MSA_NW_EXTEND, MSA_NW_EXTEND_BAND only)
// sw_smax: max(0, the largest table entry over real codes) of an MSA_SW_SCORED plan (unused by every other plan)
// profile: the 32-code id's profile twin (msa_plan_create_profile: MSA_SW_SCORED, MSA_NW_SCORED, MSA_NW_FIT only)
int choose_algorithm(const msa_plan_desc* desc, bool wide32, bool profile, int sw_smax, int& kalg, int& tp) {
  const int out_mode = desc->cells;
  switch (desc->alg) {
    case MSA_SW_LINEAR:
      kalg = (desc->match >= 0 && desc->mismatch >= 0) ? MSA_ALG_SWL0 : MSA_ALG_SWL;
      if (kalg == MSA_ALG_SWL0 && !desc->single && out_mode == MSA_OUT_NONE && !desc->track_end &&
          desc->n_pairs >= 2) {
        // score-only batch: two pairs per lane as packed int16 (MSA_ALG_SWLP) when every pair
        // couple (2c, 2c+1) shares its row / column counts and column sequence (one stripe
        // geometry, one code stream) and G = H + g(i+j) stays inside int16
        bool pk = true;
        const int64_t g = desc->gap_extend, smax = std::max({0, desc->match, desc->mismatch});
        for (int64_t p = 0; p < desc->n_pairs && pk; ++p) {
          const int64_t q = (p & 1) ? p - 1 : p;
          pk = desc->m[p] == desc->m[q] && desc->n[p] == desc->n[q] && desc->b_off[p] == desc->b_off[q] &&
               g * (desc->m[p] + desc->n[p] + 2) + smax * std::min(desc->m[p], desc->n[p]) + 2 * g + 127 < 32000 &&
               desc->match + 2 * g <= 127;
        }
        if (pk) kalg = MSA_ALG_SWLP;
      }
      break;
    case MSA_SW_AFFINE: kalg = MSA_ALG_SWA; break;
    case MSA_SW_SCORED:
      // MSA_SW_AFFINE with f = S[row code][column code] (the plan's table: plan_create): a kernel algorithm of its
      // own (new stripe_kernel instantiations).  The gap costs' and the table's sizes are check_ranges'
      kalg = MSA_ALG_SWS;
      break;
    case MSA_NW_BANDED: kalg = MSA_ALG_NWA; break;
    case MSA_NW_ALIGN:
      // MSA_NW_BANDED's recurrence with one direction byte per cell, walked by msa_plan_traceback_nw: direction
      // bytes only, the reference's scores (f = 1 / 0; any other scoring is MSA_NW_SCORED's) and gaps with g, h >= 0
      kalg = MSA_ALG_NWA;
      if (out_mode != MSA_OUT_DIR || desc->match != 1 || desc->mismatch != 0 || desc->gap_extend < 0 ||
          desc->gap_open < desc->gap_extend)
        return MSA_ERR_UNSUPPORTED;
      break;
    case MSA_NW_SCORED:
      // MSA_NW_ALIGN with f = S[row code][column code] (the plan's table: plan_create); the table's and the gaps'
      // sizes are check_ranges'
      kalg = MSA_ALG_NWA;
      break;
    // the free-end kinds: kernel algorithms of their own (msa_alg.h), none with a band -- |i - j| <= band means nothing
    // when an end is free; which ends are free is not selectable
    case MSA_NW_FIT: kalg = MSA_ALG_FIT; break;
    case MSA_NW_OVERLAP: kalg = MSA_ALG_OVL; break;
    case MSA_NW_EXTEND: kalg = MSA_ALG_EXT; break;
    // ... but for the extension inside a band, a plan kind of its own with a rule of its own for the sizes (msa.h at
    // msa_extend_align_banded: the caller clips, so |m - n| <= band holds here as for a global plan).  It needs a
    // band; MSA_NW_EXTEND keeps rejecting one
    case MSA_NW_EXTEND_BAND:
      kalg = MSA_ALG_EXTB;
      if (desc->band < 0) return MSA_ERR_UNSUPPORTED;
      break;
    case MSA_REF_GOTOH: {
      // start type -1 (main_alignment_function's single subproblem) with direction bytes or no
      // cells: the tagged-max form (every interior value is finite; values carried x4)
      int64_t span = 0;
      for (int64_t p = 0; p < desc->n_pairs; ++p) span = std::max(span, desc->m[p] + desc->n[p] + 2);
      const bool ref1 = desc->start_type == -1 && (out_mode == MSA_OUT_DIR || out_mode == MSA_OUT_NONE) &&
                        desc->gap_extend >= 0 && desc->gap_open >= desc->gap_extend &&
                        (int64_t)4 * (desc->gap_open + 1) * span < (int64_t(1) << 28);
      kalg = ref1 ? MSA_ALG_REF1 : MSA_ALG_REF;
      break;
    }
    case MSA_PARTIAL: kalg = MSA_ALG_PART; break;
    default: return MSA_ERR_ARG;
  }
  if (wide32 && (kalg = msa_alg_info_of(kalg).twin32) == MSA_ALG_NONE) return MSA_ERR_UNSUPPORTED;
  if (profile) {
    // (no band under a profile: MSA_ALG_NWP accepts none, so any band but -1 is unsupported below)
    if (kalg != MSA_ALG_SWS && kalg != MSA_ALG_NWA && kalg != MSA_ALG_FIT) return MSA_ERR_UNSUPPORTED;
    kalg = kalg == MSA_ALG_SWS ? MSA_ALG_SWP : kalg == MSA_ALG_NWA ? MSA_ALG_NWP : MSA_ALG_FITP;
  }
  const msa_alg_info t = msa_alg_info_of(kalg);
  if (desc->alg == MSA_SW_SCORED || desc->alg == MSA_NW_SCORED || free_ends(desc->alg)) {
    // the kinds that score from a table: direction bytes or the score alone, a band only where the algorithm accepts
    // one, and under the Gotoh cell gaps with g, h >= 0
    if ((out_mode != MSA_OUT_DIR && out_mode != MSA_OUT_NONE) || (!t.band && desc->band != -1) ||
        (t.cell == CELL_GOTOH && (desc->gap_extend < 0 || desc->gap_open < desc->gap_extend)))
      return MSA_ERR_UNSUPPORTED;
  }
  // the best cell under the zero floor: its position on request (packed couples: score only; an MSA_SW_SCORED plan
  // always tracks its end cell)
  tp = (t.result == RES_BEST && !t.packed() && (desc->track_end || t.table)) ? 1 : 0;
  if (tp) {
    // the first-maximum position packs with the value into one int (TRACKPOS 2) when every local score is below 2^16
    // and a stripe has < 2^15 steps.  A local score gains at most max(0, match, mismatch) per diagonal step (gaps
    // only subtract), and a path has at most min(m, n) diagonal steps.  (MSA_SW_SCORED: the table's largest entry
    // over real codes in their place.)
    const int64_t smax = t.table ? sw_smax : std::max({0, desc->match, desc->mismatch});
    bool pack = true;
    for (int64_t p = 0; p < desc->n_pairs && pack; ++p)
      pack = smax * std::min(desc->m[p], desc->n[p]) < 65536 && desc->n[p] + 512 < 32768;
    if (pack) tp = 2;
  }
  // (an MSA_NW_EXTEND plan always tracks its end cell, by compare-select: its values may be negative, which the
  // packed key cannot hold)
  if (t.result == RES_BEST_ANY) tp = 1;
  return MSA_OK;
}

// the kernel parameters every family starts from (its shape function sets the launch's own)
msa_kparams base_kparams(const msa_plan_desc* desc, int kalg) {
  msa_kparams kp{};
  kp.alg = kalg;
  kp.out = desc->cells;
  kp.match = desc->match;
  kp.mismatch = desc->mismatch;
  kp.gap_open = desc->gap_open;
  kp.gap_ext = desc->gap_extend;
  if (msa_alg_info_of(kalg).linear()) kp.gap_open = kp.gap_ext = desc->gap_extend;
  kp.h = desc->gap_open - desc->gap_extend;
  kp.start_type = desc->start_type;
  kp.band = msa_alg_info_of(kalg).band ? desc->band : -1;
  kp.single = desc->single ? 1 : 0;
  kp.n_pairs = (int)desc->n_pairs;
  return kp;
}

// ---- step 2: every pair's sizes and scores are inside what the kernels' number formats hold ---------
// the largest |score| of a substitution table
int sub_abs_max(const int8_t* sub, int count) {
  int s = 0;
  for (int k = 0; k < count; ++k) s = std::max(s, std::abs((int)sub[k]));
  return s;
}
// `scored`: the table of an MSA_NW_SCORED or MSA_NW_FIT plan (nullptr for every other plan), 64 scores or, for the
// 32-code kernels, 1,024
// sw_smax: as for choose_algorithm
// prof_abs: the largest |entry| of a profile plan's profile (-1: no profile plan), in the table's place
int check_ranges(const msa_plan_desc* desc, const msa_kparams& kp, const int8_t* scored, int sw_smax, int prof_abs) {
  const msa_alg_info t = msa_alg_info_of(kp.alg);
  for (int64_t p = 0; p < desc->n_pairs; ++p) {
    const int64_t m = desc->m[p], n = desc->n[p];
    if (m <= 0 || n <= 0 || m > (1 << 26) || n > (1 << 26)) return MSA_ERR_ARG;
    if (scored || (prof_abs >= 0 && t.cell == CELL_GOTOH)) {
      // MSA_NW_SCORED (MSA_ALG_NWA in band_kernel or stripe_kernel).  With s = the largest |S|, g, h >= 0, G = g + h:
      //   K = (s + 2 G + 2 g) T + h < 2^28,   T = m + n + 256.
      // Every value either kernel forms -- in or out of a row's band, E / F / H, stripe_kernel's H or band_kernel's
      // shifted H~ = H + g (i + j), Z = H~ - h -- is a SOURCE plus one STEP change per cell of a dependency path.
      // A step moves left, up or diagonally, so it moves to a later anti-diagonal, and a lane touches rows 1..m and
      // columns 1 - 79 .. n + 78 (stripe_geom: a stripe starts <= 16 + 63 columns before its band and ends within
      // 63 + 15 after it): a path has fewer than T steps, and |i + j| < T everywhere.
      //   steps, unshifted: the diagonal adds S (|.| <= s), E and F subtract g or G: at most max(s, G) a step;
      //   steps, shifted:   the diagonal adds the profile byte S + 2g + h and Z takes h off, E~ and F~ add 0 or take
      //                     h off: at most s + 2g + h a step (the byte itself is sign-extended from int8: choose_mode
      //                     keeps it <= 127, and it is >= -128 since S >= -128);
      //   sources: 0; the borders and the guessed rows -h - g k, k <= max(m, n), shifted by at most g T + h more:
      //            within 2h + 2g T; and -inf = MSA_NEG = -2^30 (U, E, F at a stripe's start, U + sc included; the
      //            masked inputs; band_fix's and the head / tail phases' edge values; the left border past the band).
      // So a finite value stays within 2h + 2g T + (s + 2g + h) T <= K of 0, shifted or not, and so does what the
      // kernels form from it: the unshifted final state and checkpoint rows (a shifted value less g (i + j), h added).
      // A -inf drifts by at most (s + 2g + h) T while shifted and by g T + h more where it is unshifted (the
      // checkpoint rows; the out-of-band lanes between the edge fix-ups drift like any other path): within K of -2^30.
      // K < 2^28 therefore keeps every finite value above -2^28 > MSA_NEG / 2, the threshold chunk_check_kernel and
      // chunk_add_kernel take for -inf (the walk reads bytes only), every drifted -inf in [-2^30 - 2^28, -2^30 + 2^28],
      // below that threshold, and everything inside int32.  (The chunk warm-up compares rows up to a constant and
      // falls back to the exact launch: negative scores change how often it converges, not what it computes.)
      // MSA_NW_FIT (MSA_ALG_FIT, stripe_kernel only, unshifted) adds one source, its top border H(0, j) = 0: within
      // the bound like the corner's 0.  Its paths, steps, left border and -inf are the unbanded MSA_ALG_NWA's, and
      // what it forms beside the cells is a copy of one of them (the row-m maximum): the same inequality holds.
      // MSA_NW_OVERLAP (MSA_ALG_OVL) replaces the left border's -h - g i by one more zero source, H(i, 0) = 0 with
      // E = F = -inf: inside the bound that the replaced border needed.  Paths, steps and -inf are unchanged, and the
      // last-column maxima are copies of cells again: the same inequality holds.
      // MSA_NW_EXTEND (MSA_ALG_EXT) is the unbanded MSA_ALG_NWA itself in the stripe kernel, unshifted: same sources,
      // steps and -inf, and the tracked maximum is a copy of a cell: the same inequality holds.
      // MSA_NW_EXTEND_BAND (MSA_ALG_EXTB) is the BANDED MSA_ALG_NWA in the stripe kernel, unshifted: the banded global
      // plan's sources (the borders up to the band, -inf past it), steps and drifting out-of-band lanes between the
      // edge fix-ups -- all counted above --, and the tracked maximum is a copy of an in-band cell: the same inequality.
      // The 32-code kernels (MSA_ALG_NWA32, MSA_ALG_FIT32, MSA_ALG_OVL32, MSA_ALG_EXT32, MSA_ALG_EXTB32: stripe_kernel, unshifted, raw S) differ in where a step's
      // S comes from, not in what a step is: the same inequality with s over the 1,024 scores.
      // The profile kernels (MSA_ALG_NWP, MSA_ALG_FITP) are those kernels again with a row's 32 bytes taken from the
      // profile: the same inequality with s over the whole profile (a row past m scores 0: within s).
      const int64_t s = prof_abs >= 0 ? prof_abs : sub_abs_max(scored, t.wide ? 1024 : 64);
      const int64_t g = kp.gap_ext, h = kp.h, G = kp.gap_open;
      if ((s + 2 * G + 2 * g) * (m + n + 256) + h >= (int64_t(1) << 28)) return MSA_ERR_UNSUPPORTED;
    }
    if (t.linear()) {
      // shifted recurrence G = H + g*(i+j): G must stay far from the -2^30 sentinel
      // and from int32 overflow; the profile byte holds score + 2g
      const int64_t g = kp.gap_open;
      const int64_t top = g * (m + n + 2) + (int64_t)std::max({0, kp.match, kp.mismatch}) * std::min(m, n);
      const int64_t sm = kp.match + 2 * g, sx = kp.mismatch + 2 * g;  // profile bytes (int8)
      if (g < 0 || top >= (int64_t(1) << 29) || sm > 127 || sm < -128 || sx > 127 || sx < -128)
        return MSA_ERR_UNSUPPORTED;
    }
    if (t.cell == CELL_SWAFF && !t.table) {
      // int8 profile bytes; H stays far from the -2^30 sentinel and from int32 overflow
      const int64_t top = (int64_t)std::max({0, kp.match, kp.mismatch}) * std::min(m, n);
      if (kp.match < -128 || kp.match > 127 || kp.mismatch < -128 || kp.mismatch > 127 || kp.gap_open < 0 ||
          kp.gap_ext < 0 || top >= (int64_t(1) << 29))
        return MSA_ERR_UNSUPPORTED;
    }
    if (t.cell == CELL_SWAFF && t.table) {
      // MSA_SW_SCORED: MSA_ALG_SWA's bound with smax = max(0, the largest S over real codes) for max(0, match,
      // mismatch).  One inequality on the top suffices, unlike the global plans' two-sided K above, because the zero
      // floor stops every drift downwards: H >= 0 in every cell, virtual ones included, and E (F) is a max that
      // contains the left (upper) cell's H - gap_open, so E, F >= -gap_open however long the row or column: no value
      // drifts with m + n, and no negative S, real (>= -128) or virtual (MSA_VIRT_SCORE), outlives its own cell --
      // d = H_diag + S enters a max with 0.  Upwards, an H is a sum of at most min(m, n) diagonal scores <= smax less
      // gap costs >= 0 (a virtual cell adds none), so H <= smax min(m, n) < 2^29 and H + S stays inside int32.  A -inf
      // (MSA_NEG: E, F and the diagonal at a stripe's start, the masked inputs) meets one subtraction of a gap cost or
      // one addition of an S before a max with a finite value, exactly as in MSA_ALG_SWA.
      if (kp.gap_open < 0 || kp.gap_ext < 0 || (int64_t)sw_smax * std::min(m, n) >= (int64_t(1) << 29))
        return MSA_ERR_UNSUPPORTED;
    }
    if (kp.band >= 0 && std::llabs(m - n) > kp.band) return MSA_ERR_ARG;
  }
  return MSA_OK;
}

// ---- step 3: the kernel family, from the description alone ------------------------------------------
// LDS of a flow workgroup without its pass-2 area: flags, link rings and the code copies -- whole rows
// when they fit (*whole: kp.code_whole, no ring bookkeeping), else fixed-size rings, so any n fits
// aff: the flow kernels' two-value algorithms (nc == 2: SW affine, the reference's Gotoh in tagged form)
size_t flow_lds_bytes(const msa_plan_desc* desc, bool aff, bool* whole) {
  const size_t lds0 = (size_t)(FL_FLAGS + (FL_W + 1) * 256 * (aff ? 2 : 1)) * 4;
  const size_t all = lds0 + (size_t)(aff ? 4 : FL_NCOPY) * (fl_code_bytes((int)desc->n[0]) + 16);
  *whole = all <= 96 * 1024;
  return *whole ? all : lds0 + (size_t)(aff ? 4 : FL_NCOPY) * FL_CSTR;
}
// LDS of a cflow workgroup whose code rows hold nmax columns
size_t cflow_lds_bytes(int64_t nmax) {
  return (size_t)(FL_FLAGS + (CF_W + 1) * 256) * 4 + (size_t)FL_NCOPY * (fl_code_bytes((int)nmax) + 16);
}
int64_t max_n(const msa_plan_desc* desc) { return *std::max_element(desc->n, desc->n + desc->n_pairs); }
// work items of a batch launch: pairs, or packed couples
int batch_items(const msa_plan_desc* desc, int kalg) {
  return (kalg == MSA_ALG_SWLP) ? (int)((desc->n_pairs + 1) / 2) : (int)desc->n_pairs;
}

// band_kernel's diagnostic knobs, read once per process: warm-up and output stripes of a chunk (multiples
// of BK_W).  A warm-up shorter than one item (BK_W stripes) gives chunk_check nothing to compare
// (checkpoint slot 2c is never written): chunking is then off
int band_warm() {
  static const int v = std::max(0, (int)env_int("MSA_BAND_WARM", MSA_CHUNK_WARM) / BK_W * BK_W);
  return v;
}
int band_chunk() {
  static const int v = std::max(BK_W, (int)env_int("MSA_BAND_CHUNK", 12) / BK_W * BK_W);
  return v;
}

// smax: the largest score of an MSA_NW_SCORED plan's table (unused by every other plan)
PlanMode choose_mode(const msa_plan_desc* desc, int kalg, int tp, int smax) {
  const int out_mode = desc->cells;
  const msa_alg_info t = msa_alg_info_of(kalg);
  // 5-bit codes: stripe_kernel alone has the 32-code lookup -- a single pair (any band: the exact masked launch), a batch
  if (t.wide) return PM_STRIPE;
  // MSA_SW_SCORED: stripe_kernel alone scores the SW-affine cell from a table (the flow kernels build their profile
  // from match / mismatch, and the split launch is not instantiated for it) -- one pair or a batch
  if (t.cell == CELL_SWAFF && t.table) return PM_STRIPE;
  const int band = t.band ? desc->band : -1;
  if (desc->single) {
    // flow kernels: one SW-linear pair (8 byte-shifted LDS code rings), or one SW-affine / reference-Gotoh (start
    // type -1, tagged) pair with direction bytes (two values per link column, 4 code rings); the column codes stream
    // through fixed-size LDS rings, so any n fits affine: profile bytes score + 2e + (o - e) must be int8
    const bool aff_ok = kalg == MSA_ALG_SWA && out_mode == MSA_OUT_DIR && desc->gap_extend >= 0 &&
                        desc->gap_open >= desc->gap_extend &&
                        std::max(desc->match, desc->mismatch) + desc->gap_open + desc->gap_extend <= 127 &&
                        std::min(desc->match, desc->mismatch) + desc->gap_open + desc->gap_extend >= -128 &&
                        (int64_t)desc->gap_extend * (desc->m[0] + desc->n[0] + 2) < (int64_t(1) << 28);
    // Gotoh: profile bytes 4 (f + 2g) <= 127; the shifted tagged values 4 (T + g(i+j)) stay far
    // inside int32 (REF1's own bound covers the shift: |T| + g(i+j) <= (g+h+1) span)
    const bool got_ok = kalg == MSA_ALG_REF1 && out_mode == MSA_OUT_DIR && 4 * (1 + 2 * desc->gap_extend) <= 127;
    // SW linear with a negative score (MSA_ALG_SWL) runs the flow kernels in X-space (X = H - g under the zero floor,
    // msa_flow.hip): fl_profile's bytes are score + g there, not the score + 2g of G-space that check_ranges admits
    // down to -128.  The top is covered (score + g <= score + 2g <= 127, g >= 0); the bottom needs min(match,
    // mismatch) + g >= -128 of its own.  One below it the byte wraps: mismatch -130 with g = 1 (-129) ran as +127 and
    // an all-mismatch 65 x 70 pair scored 8,190 instead of 0.  Such a pair runs the stripe kernel, whose G-space byte
    // (-128) fits.  Scores >= 0 (MSA_ALG_SWL0) run in G-space in both kernels.
    const bool lin_ok = kalg == MSA_ALG_SWL0 ||
                        (kalg == MSA_ALG_SWL && std::min(desc->match, desc->mismatch) + desc->gap_extend >= -128);
    bool whole;
    if ((lin_ok ? (out_mode == MSA_OUT_H || (out_mode == MSA_OUT_NONE && !tp)) : (aff_ok || got_ok)) &&
        flow_lds_bytes(desc, t.nc == 2, &whole) <= device_lds_max())
      return PM_FLOW;
    // A banded pair has only ~(2*band+64)/(64*lag) stripes in flight at once: band_kernel's chains of
    // 4-stripe items, as long as its code rows fit LDS; chunked from 4 chunks up, when cells are written
    // (direction bytes: MSA_NW_ALIGN, chunked like H -- a chunk's bytes do not depend on its constant)
    // (MSA_ALG_NWA alone: a banded extension, MSA_ALG_EXTB, has a band too and stays on the exact stripe launch below,
    // as every free-end plan does -- band_kernel and the chunks keep no best cell)
    if (kalg == MSA_ALG_NWA && band >= 0) {
      const int S = stripes_of(desc->m[0]);
      // MSA_NW_SCORED: band_kernel works on values shifted by g (i + j), so its profile bytes are S + 2g + h; a
      // table whose largest does not fit int8 runs the exact stripe launch, whose bytes are the raw S (lin_ok's
      // precedent above; the low side cannot fail: S >= -128 and g, h >= 0)
      if (desc->alg == MSA_NW_SCORED && (int64_t)smax + desc->gap_extend + desc->gap_open > 127) return PM_STRIPE;
      if (bk_lds_bytes(bk_code_bytes((int)desc->m[0], (int)desc->n[0], band)) <= device_lds_max()) {
        const bool chunks = (S + band_chunk() - 1) / band_chunk() >= 4 && out_mode != MSA_OUT_NONE && band_warm() >= BK_W;
        return chunks ? PM_BAND_CHUNKED : PM_BAND;
      }
      // direction bytes never take the chunked stripe launch (its chunks write int32 cells): the exact stripe launch
      if (out_mode == MSA_OUT_DIR) return PM_STRIPE;
      // else the stripe kernel: one workgroup per chunk of >= MSA_CHUNK_MIN stripes, from 4 chunks up
      const int cc = std::max(MSA_CHUNK_MIN, (S + device_cus() - 1) / device_cus());
      return (S + cc - 1) / cc >= 4 ? PM_CHUNKED : PM_STRIPE;
    }
    return PM_STRIPE;
  }
  // Packed score-only batches (C4): cflow_kernel (msa_cflow.hip) -- items of CF_W stripes of one couple, chained
  // through granules, claimed item-major -- for batches of fewer couples than two per CU whose code rows fit LDS.
  // MSA_C4_KERNEL=lockstep / =cflow (diagnostics) force either kernel (read per plan, not cached: a test forces
  // either kernel in one process). A batch with at least two couples per CU keeps the lock-step kernel's SIMDs busy
  // (its 8 waves per workgroup hide each other's step latency): measured on C4's shape, 1,024 pairs 2.39 ms lock-step
  // vs 2.73 cflow; 512 pairs 2.07 vs 1.58, 128 pairs 0.72 vs 0.55 (profiles/r05_c4_*_bench.json)
  const int slots = 2 * device_cus();
  if (kalg == MSA_ALG_SWLP && !env_is("MSA_C4_KERNEL", "lockstep") && cflow_lds_bytes(max_n(desc)) <= 96 * 1024 &&
      (env_is("MSA_C4_KERNEL", "cflow") || batch_items(desc, kalg) < slots))
    return PM_CFLOW;
  // A batch with fewer pairs (couples) than two workgroups per CU leaves CUs idle while each workgroup walks its
  // pair's whole stripe chain (C4 at 8 GPUs: 128 pairs per rank).  Then every pair is split into items of W stripes,
  // chained through granules (kp.single == 3): a pair's stripes run on several CUs at once.  Measured (C4 shape, 4k x
  // 4k, packed couples, ms): 64 couples 1.72 -> 0.80, 128: 1.39, 256: 2.38.
  bool eq_m = true;
  for (int64_t p = 1; p < desc->n_pairs; ++p) eq_m = eq_m && desc->m[p] == desc->m[0];
  if (eq_m && batch_items(desc, kalg) < slots && stripes_of(desc->m[0]) >= 2 * MSA_WAVES_BATCH && band < 0 &&
      desc->alg != MSA_NW_ALIGN && desc->alg != MSA_NW_SCORED &&  // (a batch of global alignments with direction
      !free_ends(desc->alg))                  // bytes, scored, fit, overlap or extension: whole pairs per workgroup)
    return PM_SPLIT;
  return PM_STRIPE;
}

// what the pair layout depends on: steps per phase, and for flow plans rows per lane and the passes
void set_layout_mode(msa_plan& P, const msa_plan_desc* desc) {
  const int kalg = P.main.kp.alg;
  if (P.mode != PM_FLOW) {
    P.KS = desc->single ? ks_single(kalg) : ks_batch(kalg);
    return;
  }
  P.KS = 16;
  P.flow2 = desc->cells == MSA_OUT_H || P.nc == 2;
  // SW two-pass plans reduce their pair result inside the launch when the cell index fits 32 bits
  // (MSA_FUSED_REDUCE=0: the reduce_blocks_kernel launch, for A/B; read per plan)
  const char* fr = std::getenv("MSA_FUSED_REDUCE");
  const int64_t cells1 = (desc->m[0] + 1) * (desc->n[0] + 1);
  P.fused_reduce = P.flow2 && kalg != MSA_ALG_REF1 && cells1 < (int64_t(1) << 32) && !(fr && fr[0] == '0');
  // rows per lane of the flow kernel: 2 in every two-pass plan (SW linear with H; the reference's Gotoh and
  // SW affine with direction bytes), which halves the inter-wave hand-offs per row; 1 in score-only plans
  P.R = P.flow2 ? 2 : 1;
}

// ---- step 4: where every pair's stripes, cells and column codes go ----------------------------------
Extents lay_out_pairs(msa_plan& P, const msa_plan_desc* desc) {
  const int band = P.main.kp.band;
  int64_t stripe0 = 0, off = 0, cod_bytes = 0;
  std::map<std::pair<int64_t, int64_t>, int64_t> seg_of;
  Extents ex;
  P.pairs.resize(desc->n_pairs);
  for (int64_t p = 0; p < desc->n_pairs; ++p) {
    const int64_t m = desc->m[p], n = desc->n[p];
    const int S = stripes_of(m);
    int pmax = 0;
    for (int k = 0; k < S; ++k) {
      StripeGeom g;
      stripe_geom(k, (int)m, (int)n, band, g, P.KS);
      pmax = std::max(pmax, g.P * (P.KS / MSA_K));  // in 16-step layout blocks
    }
    if (P.mode == PM_FLOW)  // the flow kernels' own geometry (R rows per lane)
      for (int k = 0; k < stripes_of(m, P.R); ++k) pmax = std::max(pmax, fl_P(k, (int)m, (int)n, P.R));
    msa_pair_desc& pd = P.pairs[p];
    pd.a_off = desc->a_off[p];
    pd.b_off = desc->b_off[p];
    pd.m = (int)m;
    pd.n = (int)n;
    pd.stripe0 = (int)stripe0;
    pd.pmax = pmax;
    pd.out_off = off;
    // padded column-code segment, shared by pairs with the same column sequence
    const auto key = std::make_pair(pd.b_off, (int64_t)n);
    auto it = seg_of.find(key);
    if (it == seg_of.end()) {
      it = seg_of.emplace(key, cod_bytes).first;
      msa_pair_desc sd{};
      sd.b_off = pd.b_off;
      sd.n = (int)n;
      sd.cod_off = cod_bytes;
      P.segs.push_back(sd);
      cod_bytes += ((n + 2 * MSA_CPAD) + 63) & ~int64_t(63);
    }
    pd.cod_off = it->second;
    // R = 2 layout: (m+127)/128 stripes of pmax * 2048 cells
    const int64_t cells = std::max((int64_t)S * pmax * MSA_K * 64,
                                   (int64_t)stripes_of(m, P.R) * pmax * MSA_K * 64 * P.R);
    off += (cells + 63) & ~int64_t(63);
    stripe0 += S;
    ex.S = std::max(ex.S, S);
    ex.P = std::max(ex.P, pmax);
  }
  P.total_stripes = stripe0;
  P.cells_elems = off;
  P.cod_copy = cod_bytes;
  return ex;
}

// ---- step 5: one shape function per family: each fills the plan's launch records from the description, the pair
// layout and the device facts (CUs, the LDS limit, occupancy through kernel_shape), and counts its granule slots
// the launch's grid: its items, at most per_cu workgroups a CU (and what the occupancy allows)
int size_grid(Launch& l, int per_cu) {
  if (l.lds > device_lds_max()) {
    std::fprintf(stderr, "msa: problem needs %zu B of LDS per workgroup (> %zu B, the device's limit)\n", l.lds,
                 device_lds_max());
    return MSA_ERR_UNSUPPORTED;
  }
  const int occ = kernel_shape(l.fn, l.threads, l.lds);
  if (occ < 0) return MSA_ERR_HIP;
  l.grid = std::max(1, std::min(l.kp.n_items, device_cus() * std::min(occ, per_cu)));
  return MSA_OK;
}

// stripe_kernel's wrap row buffer entries per carried value (batch mode)
int row_words(const Extents& ex) { return ((ex.P * MSA_K + MSA_ROWOFF + 32) + 15) & ~15; }
// stripe_kernel's LDS: schedule, link rings, row buffer, for a single pair the code ring, and for 5-bit codes the
// 32 x 32 table (a profile plan has none)
size_t stripe_lds_bytes(const msa_kparams& kp, int W, int nc) {
  return 4 * (16 + (size_t)kp.sched_cap * 8 + (size_t)(2 * W + 1) * nc * MSA_RING + (size_t)nc * kp.lds_row_words +
              (kp.single == 1 ? (size_t)4 * (MSA_CRING / 4 + 16) : 0) +
              (msa_alg_info_of(kp.alg).wide && !msa_alg_info_of(kp.alg).profile ? 256 : 0));
}

// PM_STRIPE, PM_SPLIT: stripe_kernel over a batch's pairs (one workgroup walks a pair's whole stripe chain,
// the wrap link through the LDS row buffer), over a small batch's items, or over one pair's items
int shape_stripe(msa_plan& P, const msa_plan_desc* desc, int tp, const Extents& ex) {
  Launch& l = P.main;
  msa_kparams& kp = l.kp;
  const bool single = kp.single == 1;
  const int W = single ? MSA_WAVES_SINGLE : MSA_WAVES_BATCH;
  l.fn = pick_kernel(kp.alg, kp.out, tp, single);
  if (!l.fn) return MSA_ERR_UNSUPPORTED;
  l.threads = (W + 1 + (single ? 1 : 0)) * 64;
  kp.lds_code_bytes = 0;  // column codes come from the staged global copies (stage_codes_kernel)
  if (single) {
    kp.sched_cap = W;
    kp.n_items = (stripes_of(desc->m[0]) + W - 1) / W;
    P.gslots = (kp.n_items - 1) * P.nc;
  } else if (P.mode == PM_SPLIT) {
    // Items of C > W stripes (fewer items, the waves cycling inside one) were slower at every count --
    // 128 couples with C = 16: 1.81, 256 with C = 32: 2.46 -- since an item's second round of stripes waits
    // for its first to finish, so a pair's chain grows to ~(S / W) stripe lengths; kp.chunk_c
    // stays general (the kernel runs any multiple of W) but the plan uses C = W.  Items of
    // four stripes (a 4-wave instantiation) were slower too: 128 pairs 0.81 -> 1.01 ms.
    const int C = W;
    kp.single = 3;
    kp.chunk_c = C;
    kp.groups = (stripes_of(desc->m[0]) + C - 1) / C;
    kp.n_items = batch_items(desc, kp.alg) * kp.groups;
    kp.sched_cap = C;
    // the wave W-1 -> wave 0 wrap link inside an item goes through the LDS row buffer
    if (C > W) kp.lds_row_words = row_words(ex);
    P.gslots = kp.n_items > 1 ? kp.n_items * P.nc : 0;  // item k publishes into slot k
  } else {
    kp.sched_cap = ex.S;
    kp.lds_row_words = row_words(ex);
    kp.n_items = batch_items(desc, kp.alg);
  }
  l.lds = stripe_lds_bytes(kp, W, P.nc);
  return size_grid(l, 2);
}

// PM_CHUNKED: the chunked stripe launch of a banded pair whose band_kernel code rows do not fit LDS. The band has
// only ~9 stripes in flight, so the exact launch is one long chain of ~S x 8 phases. Chunked mode runs it as n_chunks
// independent chains of chunk_c (+ warm-up) stripes at once (rank convergence, msa_kernels.hip header), with the
// exact launch kept behind it as the fallback. Measured on MI355X for C3 (profiles/r03_c3_*), when this was C3's
// path: (warm, chunk) = (24, 24) 0.925 ms, (24, 12) 0.768, (16, 16) 0.733, (20, 10) 0.678 -- and (16, 8) did not
// converge in every chunk (the exact fallback ran: 18.3 ms).  Chunk workgroups of 4 or 12 waves instead of 8: 0.90
// and 0.72 ms (8: 0.67).  (20, 6) = 254 chunks, one per CU: not every chunk converged (17.4 ms with the fallback) --
// more start rows, and the slowest needs more than 1,280 rows.
int shape_chunked_stripe(msa_plan& P, const msa_plan_desc* desc, int tp, const Extents& ex) {
  const int rc = shape_stripe(P, desc, tp, ex);  // the exact single-mode launch
  if (rc != MSA_OK) return rc;
  P.exact = P.main;
  Launch& l = P.main;
  msa_kparams& kp = l.kp;
  const int S = stripes_of(desc->m[0]), ncu = device_cus();
  kp.single = 2;
  kp.chunk_c = std::max(MSA_CHUNK_MIN, (S + ncu - 1) / ncu);
  kp.chunk_warm = MSA_CHUNK_WARM;
  kp.n_items = P.n_chunks = (S + kp.chunk_c - 1) / kp.chunk_c;
  kp.sched_cap = kp.chunk_c + MSA_CHUNK_WARM;
  kp.lds_row_words = row_words(ex);
  l.fn = pick_kernel(kp.alg, kp.out, 0, false);
  l.threads = (MSA_WAVES_BATCH + 1) * 64;
  l.lds = stripe_lds_bytes(kp, MSA_WAVES_BATCH, P.nc);
  P.ckw = (2 * kp.band + 1 + 3) & ~3;
  // every chunk at once (one workgroup each); more chunks than slots just queue
  return size_grid(l, 2) == MSA_OK ? MSA_OK : MSA_ERR_UNSUPPORTED;
}

// PM_CFLOW: cflow_kernel over items of CF_W stripes of one couple; item t publishes the last link of its
// stripes into slot t (read by item t + couples)
int shape_cflow(msa_plan& P, const msa_plan_desc* desc) {
  Launch& l = P.main;
  msa_kparams& kp = l.kp;
  const int64_t mmax = *std::max_element(desc->m, desc->m + desc->n_pairs);
  l.fn = cflow_kernel<CF_W>;
  l.threads = (CF_W + 1) * 64;
  l.lds = cflow_lds_bytes(max_n(desc));
  kp.lds_code_bytes = fl_code_bytes((int)max_n(desc));
  kp.code_whole = 1;
  kp.n_items = batch_items(desc, kp.alg) * ((stripes_of(mmax) + CF_W - 1) / CF_W);
  P.gslots = kp.n_items;
  return size_grid(l, INT_MAX);
}

// PM_FLOW: flow_kernel over one pair's items of FL_W stripes, with pass 2 (two-pass plans) inside the
// launch or behind it
int shape_flow(msa_plan& P, const msa_plan_desc* desc, int tp) {
  Launch& l = P.main;
  msa_kparams& kp = l.kp;
  const bool nneg = desc->match >= 0 && desc->mismatch >= 0;
  bool whole;
  const size_t flow_lds = flow_lds_bytes(desc, P.nc == 2, &whole);
  l.fn = pick_flow(kp.alg, kp.out == MSA_OUT_NONE, P.flow2, tp, P.R, nneg);
  if (!l.fn) return MSA_ERR_UNSUPPORTED;
  l.threads = (FL_W + 2) * 64;
  kp.code_whole = whole ? 1 : 0;
  kp.lds_code_bytes = fl_code_bytes((int)desc->n[0]);
  kp.n_items = (stripes_of(desc->m[0], P.R) + FL_W - 1) / FL_W;
  P.gslots = (kp.n_items - 1) * P.nc;
  // pass-2 blocks: FL_P2INTS ints per wave (inputs + column codes staged in LDS); either fits (choose_mode)
  l.lds = P.flow2 ? std::max(flow_lds, (size_t)(FL_W + 2) * fl_p2ints(FL_PS) * 4) : flow_lds;
  // Items go to the 8 XCDs in runs of G consecutive items, round-robin (workgroup b takes tickets of XCD b % 8 first,
  // round-robin placement puts it there): a run hands off inside one L2.  When an XCD's share fits its workgroups
  // (chunk <= CUs per XCD) the runs are 8 contiguous chunks (7 seams).  A longer pair keeps more items in flight than
  // an XCD has workgroups (97k: ~240 of 381 items at once, 32 CUs per XCD): contiguous chunks would then serialize --
  // chunk c + 1 waits for chunk c's last items, which wait for a free workgroup of XCD c (measured 28 ms for 97k x
  // 97k) -- so the runs shrink to G = CUs per XCD / 8 and every XCD holds its share of the items in flight.  Speed
  // only: an item only waits on an earlier one and every workgroup is resident (one per CU, grid <= CUs), whatever
  // the placement.
  const int ncu = device_cus();
  const int per_xcd = std::max(1, ncu / 8);
  const int chunk = (kp.n_items + 7) / 8;
  kp.sched_cap = chunk <= per_xcd ? chunk : std::max(1, per_xcd / 8);  // G
  l.grid = P.nflow = 8 * std::max(1, std::min(chunk, per_xcd));
  if (P.flow2) {
    // two-pass: the remaining CUs run pass-2 blocks inside the same launch, one flow workgroup per CU (the LDS
    // floor): a pass-2 workgroup sharing a CU with a pass-1 one takes issue slots from its chain waves.  A long pair
    // keeps ~n / (W lag) items in flight (97k: ~240), so pass 1 may hold most CUs; then every CU also gets a pass-2
    // workgroup (two per CU), whose waves issue at the lowest priority, behind the pass-1 waves (s_setprio,
    // msa_flow.hip).  MSA_FLOW_LDS_MIN (bytes, diagnostic, read once per process) overrides the one-per-CU floor.
    static const long lds_min = env_int("MSA_FLOW_LDS_MIN", 80 * 1024 + 1024);
    l.lds = std::max(l.lds, (size_t)std::max(0L, lds_min));
    if (P.nflow > ncu / 2) {
      // pass 1 holds most CUs: pass 2 runs as a launch of its own behind it (flow_fill_kernel), whose
      // register budget is the pass-2 code's alone (97k x 97k: 23 -> ~16 ms)
      Launch& f = P.fill;
      f.fn = pick_fill(kp.alg, tp, P.R, nneg);
      if (!f.fn) return MSA_ERR_UNSUPPORTED;
      f.threads = FL_FILLW * 64;
      f.lds = (size_t)FL_FILLW * fl_p2ints(FL_PS_FILL) * 4;
      P.ps = FL_PS_FILL;  // its blocks are segments of FL_PS_FILL phases (pass 1 saves state that often)
      const int focc = kernel_shape(f.fn, f.threads, f.lds);
      if (focc < 0) return MSA_ERR_HIP;
      f.grid = ncu * std::max(1, std::min(focc, 8));
    } else {
      l.grid = std::max(l.grid + 8, 8 * per_xcd);
    }
  }
  if (kernel_shape(l.fn, l.threads, l.lds) < 0) return MSA_ERR_HIP;
  P.fill.kp = kp;  // (the fill launch takes pass 1's arguments)
  return MSA_OK;
}

// PM_BAND, PM_BAND_CHUNKED: band_kernel (msa_band.hip), flag-synchronised chains of 4-stripe items.  The
// exact launch chains all of the pair's items; chunked (rank convergence, >= 4 chunks) runs chunks of C
// output stripes, each started W stripes early from a guessed row, with the exact launch queued behind as
// the fallback.  MSA_BAND_WARM / MSA_BAND_CHUNK (diagnostic) override the warm-up and chunk stripes
// (multiples of 4).  Item t publishes (Z, F~) of its last row into slot t (chunked and exact launches).
int shape_band(msa_plan& P, const msa_plan_desc* desc) {
  Launch& l = P.main;
  msa_kparams& kp = l.kp;
  const int m0 = (int)desc->m[0], n0 = (int)desc->n[0], band = kp.band;
  const int S = stripes_of(m0), ncu = device_cus();
  // (direction bytes, MSA_NW_ALIGN: an instantiation of its own -- the value plans' code is unchanged)
  l.fn = desc->cells == MSA_CELLS_DIR ? band_kernel<true> : band_kernel<false>;
  l.threads = (BK_W + 1) * 64;
  kp.lds_code_bytes = bk_code_bytes(m0, n0, band);
  l.lds = bk_lds_bytes(kp.lds_code_bytes);
  const int bocc = kernel_shape(l.fn, l.threads, l.lds);
  if (bocc < 0) return MSA_ERR_HIP;
  kp.groups = kp.n_items = (S + BK_W - 1) / BK_W;  // the exact launch
  kp.chunk_c = S;
  l.grid = std::max(1, std::min(kp.n_items, ncu * bocc));
  int items = kp.n_items;
  if (P.mode == PM_BAND_CHUNKED) {
    const int warm = band_warm(), cc = band_chunk();
    P.exact = l;
    P.n_chunks = (S + cc - 1) / cc;
    kp.single = 2;
    kp.chunk_c = cc;
    kp.chunk_warm = warm;
    // item slots per chunk: its warm-up + output stripes in items of BK_W (a chunk whose warm-up
    // would reach the matrix border starts at row 0 instead -- band_kernel -- and so has more)
    int ipc = 1;
    for (int c2 = 0; c2 < P.n_chunks; ++c2) {
      const int ks0 = c2 * cc, ke = std::min(S, ks0 + cc);
      int kb = ks0 - warm;
      if (kb < 0 || kb * 64 <= band + 64) kb = 0;
      ipc = std::max(ipc, (ke - kb + BK_W - 1) / BK_W);
    }
    kp.groups = ipc;
    kp.n_items = P.n_chunks * kp.groups;
    l.grid = std::max(1, std::min(kp.n_items, ncu * bocc));
    items = std::max(items, kp.n_items);
    P.ckw = (2 * band + 1 + 3) & ~3;
    // int16 chunk cells: a chunk >= 1 starts from its guessed row (H <= -h, inside the band >= -h - g band) at row r0
    // > band + 64, so an in-band cell (i, j) is reached from (r0, j - i + r0), in the band, along its diagonal: -h -
    // g band <= H <= i - r0 - h.  Both bounds fit int16 with room when rows + h + g band stays under 30,000 (C3:
    // 2,112 + 2 + 512); the cells are then written as 2 B, and chunk_add_kernel reads 2 B and writes 4 B per cell
    // instead of reading and re-writing 4 B.  MSA_BAND_H16=0 (diagnostic, read once per process) keeps int32 cells.
    static const bool h16_on = env_int("MSA_BAND_H16", 1) != 0;
    const long long rows = (long long)(warm + cc) * 64 + 64;
    P.h16 = h16_on && desc->cells == MSA_CELLS_H && kp.h >= 0 && kp.gap_ext >= 0 &&
            rows + kp.h + (long long)kp.gap_ext * band <= 30000;
  }
  P.gslots = items > 1 ? 2 * items : 0;
  return MSA_OK;
}

// ---- step 6: device buffers -------------------------------------------------------------------------
int alloc_buffers(msa_plan& P) {
  const int np = (int)P.pairs.size();
  if (!P.alloc(&P.d_pairs, sizeof(msa_pair_desc) * np)) return MSA_ERR_HIP;
  HIPCHK(hipMemcpy(P.d_pairs, P.pairs.data(), sizeof(msa_pair_desc) * np, hipMemcpyHostToDevice));
  if (!P.alloc_set(&P.d_meta, sizeof(msa_stripe_meta) * std::max<int64_t>(1, P.total_stripes))) return MSA_ERR_HIP;
  if (!P.alloc(&P.d_ticket, 4 * MSA_NTICKET) || !P.alloc_set(&P.d_err, 64)) return MSA_ERR_HIP;
  if (!P.alloc(&P.d_cod, (size_t)MSA_NCOPY * P.cod_copy + 64)) return MSA_ERR_HIP;
  if (!P.alloc(&P.d_segs, sizeof(msa_pair_desc) * P.segs.size())) return MSA_ERR_HIP;
  HIPCHK(hipMemcpy(P.d_segs, P.segs.data(), sizeof(msa_pair_desc) * P.segs.size(), hipMemcpyHostToDevice));
  if (!P.alloc(&P.d_res, sizeof(PairResult) * np) || !P.alloc(&P.d_sum, 64)) return MSA_ERR_HIP;
  // (the walks of a fit, overlap or extension plan start at the run's end cell: until a run has written one it is
  // (-1, -1), outside the matrix, which both walkers answer with MSA_ERR_ARG whatever the pooled block held before)
  if (free_ends(P.d.alg)) HIPCHK(hipMemset(P.d_res, 0xff, sizeof(PairResult) * np));
  const msa_alg_info t = msa_alg_info_of(P.main.kp.alg);
  if (t.profile) {
    // the profile as plan_create made it: stripe_kernel's bytes are the raw scores, loaded by the lanes themselves
    if (!P.alloc(&P.d_prof, P.prof.size())) return MSA_ERR_HIP;
    HIPCHK(hipMemcpy(P.d_prof, P.prof.data(), P.prof.size(), hipMemcpyHostToDevice));
    std::vector<int8_t>().swap(P.prof);
  } else if (t.wide) {
    // the 32 x 32 table as it is: stripe_kernel's bytes are the raw S (each workgroup copies it to LDS)
    if (!P.alloc(&P.d_sub, sizeof(P.sub))) return MSA_ERR_HIP;
    HIPCHK(hipMemcpy(P.d_sub, P.sub, sizeof(P.sub), hipMemcpyHostToDevice));
  } else if (t.table) {
    // (Smith-Waterman: stripe_kernel, so the raw S -- with plan_create's MSA_VIRT_SCORE in column 7)
    // the substitution table, one 8-byte profile per row code: band_kernel's bytes are S + 2g + h (its values are
    // shifted by g (i + j); wrapped to a byte as the kernel's own arithmetic did for the 1 / 0 plans), stripe_kernel's S
    const bool bandk = P.mode == PM_BAND || P.mode == PM_BAND_CHUNKED;
    const int add = bandk ? 2 * P.main.kp.gap_ext + P.main.kp.h : 0;
    uint8_t tab[64];
    for (int k = 0; k < 64; ++k) tab[k] = (uint8_t)((P.sub[k] + add) & 0xff);
    if (!P.alloc(&P.d_sub, sizeof(tab))) return MSA_ERR_HIP;
    HIPCHK(hipMemcpy(P.d_sub, tab, sizeof(tab), hipMemcpyHostToDevice));
  }
  if (P.gslots > 0) {  // granules: one slot of the longest column count (+ margins) per publishing item
    int nmax = 0;
    for (const msa_pair_desc& pd : P.pairs) nmax = std::max(nmax, pd.n);
    P.gbuf_stride = ((nmax + 2 * MSA_GOFF + 16) + 15) & ~15;
    if (!P.alloc_set(&P.d_gbuf, (size_t)P.gslots * P.gbuf_stride * sizeof(unsigned long long))) return MSA_ERR_HIP;
  }
  if (P.flow2) {
    const int S = stripes_of(P.pairs[0].m, P.R);
    P.brw = 16 * P.pairs[0].pmax + 16;
    P.nseg = (P.pairs[0].pmax + P.ps - 1) / P.ps;
    P.nblk = S * P.nseg;
    // pass-2 blocks in expected readiness order: stripe s starts ~6.5 phases after
    // stripe s-1, and segment seg is complete ps (seg + 1) phases after its start
    std::vector<int> order(P.nblk);
    std::vector<double> key(P.nblk);
    for (int b = 0; b < P.nblk; ++b) {
      order[b] = b;
      key[b] = (P.R == 2 ? 7.5 : 6.5) * (b / P.nseg) + (double)P.ps * (b % P.nseg + 1);
    }
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return key[x] < key[y]; });
    // (affine: the F~ bottom rows follow the Z rows; a snapshot is 4 values per lane)
    const bool two = P.nc == 2;
    const size_t brb = sizeof(unsigned long long) * (size_t)S * P.brw * (two ? 2 : 1);
    const size_t snb = sizeof(unsigned long long) * (size_t)P.nblk * (two ? 128 * (P.R + 1) : 128 * P.R);
    if (!P.alloc_set(&P.d_br, brb) || !P.alloc_set(&P.d_snap, snb)) return MSA_ERR_HIP;
    if (!P.alloc(&P.d_blk, sizeof(int4) * (size_t)P.nblk)) return MSA_ERR_HIP;
    if (!P.alloc(&P.d_order, sizeof(int) * (size_t)P.nblk)) return MSA_ERR_HIP;
    HIPCHK(hipMemcpy(P.d_order, order.data(), sizeof(int) * (size_t)P.nblk, hipMemcpyHostToDevice));
  }
  if (P.chunked()) {
    // entries a chunk never writes (outside the band row / matrix) read as -inf
    if (!P.alloc_set(&P.d_ck, sizeof(int) * (size_t)P.n_chunks * 4 * P.ckw, 0xC0)) return MSA_ERR_HIP;
    if (!P.alloc(&P.d_dk, sizeof(int) * P.n_chunks) || !P.alloc(&P.d_okk, sizeof(int) * P.n_chunks) ||
        !P.alloc(&P.d_skip, 64))
      return MSA_ERR_HIP;
    if (P.h16 && P.d.cells == MSA_CELLS_H) {
      const msa_pair_desc& pd = P.pairs[0];
      const int S = stripes_of(pd.m);
      const size_t per = (size_t)pd.pmax * MSA_K * 64;
      if (S > P.main.kp.chunk_c && !P.alloc(&P.d_h16, sizeof(int16_t) * per * (size_t)(S - P.main.kp.chunk_c)))
        return MSA_ERR_HIP;
    }
    if (!P.d_h16) P.h16 = false;
  }
  HIPCHK(hipEventCreate(&P.ev0));
  HIPCHK(hipEventCreate(&P.ev1));
  // the memsets above went to the null stream, which does not order the non-blocking
  // streams runs are launched on: finish them before the plan can run anywhere
  HIPCHK(hipStreamSynchronize(nullptr));
  return MSA_OK;
}

}  // namespace

// ---- the C entry points (C linkage by their declarations in msa.h; msa_plan_destroy: msa_capi.hip) ------
static int plan_create(const msa_plan_desc* desc, const int8_t* sub, bool wide32, const int8_t* prof,
                       int64_t prof_rows, msa_plan** out);

int msa_plan_create(const msa_plan_desc* desc, msa_plan** out) {
  return plan_create(desc, nullptr, false, nullptr, 0, out);
}

int msa_plan_create_scored(const msa_plan_desc* desc, const int8_t* sub, msa_plan** out) {
  return plan_create(desc, sub, false, nullptr, 0, out);
}

int msa_plan_create_scored32(const msa_plan_desc* desc, const int8_t* sub32, msa_plan** out) {
  if (!sub32) return MSA_ERR_ARG;
  return plan_create(desc, sub32, true, nullptr, 0, out);
}

int msa_plan_create_profile(const msa_plan_desc* desc, const int8_t* prof, int64_t prof_rows, msa_plan** out) {
  if (!prof || prof_rows < 1) return MSA_ERR_ARG;
  return plan_create(desc, nullptr, false, prof, prof_rows, out);
}

// sub: 64 scores S[8 a + b] or nullptr, or with wide32 1,024 scores S[32 a + b]
// prof: nullptr, or (without sub) prof_rows x 32 scores, row r = profile position r by column code
static int plan_create(const msa_plan_desc* desc, const int8_t* sub, bool wide32, const int8_t* prof,
                       int64_t prof_rows, msa_plan** out) {
  if (!desc || !out || desc->n_pairs <= 0 || !desc->m || !desc->n || !desc->a_off || !desc->b_off) return MSA_ERR_ARG;
  const bool sw_scored = desc->alg == MSA_SW_SCORED;
  if (sub && desc->alg != MSA_NW_SCORED && !free_ends(desc->alg) && !sw_scored) return MSA_ERR_UNSUPPORTED;
  if (prof) {
    if (!sw_scored && desc->alg != MSA_NW_SCORED && desc->alg != MSA_NW_FIT) return MSA_ERR_UNSUPPORTED;
    // every pair's rows lie inside the profile (many pairs may name the same rows)
    for (int64_t p = 0; p < desc->n_pairs; ++p)
      if (desc->a_off[p] < 0 || desc->a_off[p] > prof_rows || desc->m[p] > prof_rows - desc->a_off[p])
        return MSA_ERR_ARG;
  }
  int rc = ensure_device();
  if (rc != MSA_OK) return rc;
  // (a plan without device buffers yet destroys cleanly: no streams, no blocks, null events)
  std::unique_ptr<msa_plan, void (*)(msa_plan*)> P(new (std::nothrow) msa_plan(), msa_plan_destroy);
  if (!P) return MSA_ERR_NOMEM;
  P->d = *desc;
  P->d.m = P->d.n = P->d.a_off = P->d.b_off = nullptr;
  P->d.single = desc->single ? 1 : 0;
  // MSA_SW_SCORED: the launch's own table.  The highest code (7, or 31 over 5-bit codes) is the virtual column's, so
  // the caller's entries with either index equal to it are ignored: that column carries MSA_VIRT_SCORE in every row
  // (and so does its row, which no input selects); smax is taken over the real codes alone
  int sw_smax = 0, prof_abs = -1;
  if (prof) {
    // the launch's own profile.  MSA_SW_SCORED: column 31 is the virtual column's in every row, as in a table (the
    // caller's entries there are ignored), and smax is taken over the real codes; s is the largest |entry| of all
    P->prof.assign(prof, prof + 32 * prof_rows);
    P->prof_rows = prof_rows;
    prof_abs = 0;
    for (int64_t r = 0; r < prof_rows; ++r)
      for (int b = 0; b < 32; ++b) {
        int8_t& v = P->prof[(size_t)(32 * r + b)];
        if (sw_scored && b == 31) { v = (int8_t)MSA_VIRT_SCORE; continue; }
        prof_abs = std::max(prof_abs, std::abs((int)v));
        sw_smax = std::max(sw_smax, (int)v);
      }
    if (sw_scored) P->d.track_end = 1;  // (always tracked, as under a table)
  } else if (sw_scored) {
    if (!sub && (desc->match < -128 || desc->match > 127 || desc->mismatch < -128 || desc->mismatch > 127))
      return MSA_ERR_UNSUPPORTED;
    const int nc = wide32 ? 32 : 8;
    for (int a = 0; a < nc; ++a)
      for (int b = 0; b < nc; ++b) {
        const bool virt = a == nc - 1 || b == nc - 1;
        const int v = virt ? MSA_VIRT_SCORE : (sub ? (int)sub[nc * a + b] : (a == b ? desc->match : desc->mismatch));
        P->sub[nc * a + b] = (int8_t)v;
        if (!virt) sw_smax = std::max(sw_smax, v);
      }
    P->d.track_end = 1;  // (always tracked: the walkers' check)
  }
  int kalg, tp;
  if ((rc = choose_algorithm(desc, wide32, prof != nullptr, sw_smax, kalg, tp)) != MSA_OK) return rc;
  P->tp = tp;
  if (desc->single && desc->n_pairs != 1) return MSA_ERR_ARG;
  // (alg, cells, tracking) combinations no kernel computes: every family takes a subset of the stripe kernel's
  if (!pick_kernel(kalg, desc->cells, tp, desc->single != 0)) return MSA_ERR_UNSUPPORTED;
  // (direction bytes of the banded recurrence are MSA_NW_ALIGN's: their stripe kernel instantiation exists for it alone)
  if (desc->alg == MSA_NW_BANDED && desc->cells == MSA_CELLS_DIR) return MSA_ERR_UNSUPPORTED;
  P->main.kp = base_kparams(desc, kalg);
  P->nc = msa_alg_info_of(kalg).nc;
  if (msa_alg_info_of(kalg).band && P->main.kp.h < 0) return MSA_ERR_UNSUPPORTED;
  // the substitution scores of the banded recurrence: MSA_NW_SCORED's table, or its match / mismatch; 1 / 0 for
  // MSA_NW_BANDED and MSA_NW_ALIGN, whatever their description says; MSA_NW_FIT, MSA_NW_OVERLAP, MSA_NW_EXTEND and
  // MSA_NW_EXTEND_BAND score as MSA_NW_SCORED does
  const bool scored = desc->alg == MSA_NW_SCORED || free_ends(desc->alg);
  int smax = 0;
  if (scored && !sub && !prof &&
      (desc->match < -128 || desc->match > 127 || desc->mismatch < -128 || desc->mismatch > 127))
    return MSA_ERR_UNSUPPORTED;
  if (wide32 && !sw_scored) std::memcpy(P->sub, sub, sizeof(P->sub));
  for (int k = 0; k < 64 && !wide32 && !sw_scored && !prof; ++k) {
    const bool diag = k / 8 == k % 8;
    P->sub[k] = sub ? sub[k] : (int8_t)(scored ? (diag ? desc->match : desc->mismatch) : (diag ? 1 : 0));
    smax = k ? std::max(smax, (int)P->sub[k]) : (int)P->sub[k];
  }
  if ((rc = check_ranges(desc, P->main.kp, scored && !prof ? P->sub : nullptr, sw_smax, prof_abs)) != MSA_OK)
    return rc;
  P->mode = choose_mode(desc, kalg, tp, smax);
  set_layout_mode(*P, desc);
  const Extents ex = lay_out_pairs(*P, desc);
  switch (P->mode) {
    case PM_STRIPE: case PM_SPLIT: rc = shape_stripe(*P, desc, tp, ex); break;
    case PM_CHUNKED: rc = shape_chunked_stripe(*P, desc, tp, ex); break;
    case PM_FLOW: rc = shape_flow(*P, desc, tp); break;
    case PM_BAND: case PM_BAND_CHUNKED: rc = shape_band(*P, desc); break;
    case PM_CFLOW: rc = shape_cflow(*P, desc); break;
  }
  if (rc != MSA_OK) return rc;
  if ((rc = alloc_buffers(*P)) != MSA_OK) return rc;
  *out = P.release();
  return MSA_OK;
}

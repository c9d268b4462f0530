// msa_seedapi.inc -- seed extension (included by msa_capi.hip after msa_xdropapi.inc): both flanks of a seed in one
// call, the alignment through the seed with its CIGAR (the contract is include/msa.h's at msa_seed_align)
//     msa_seed_align, msa_seed_align_batch, *32
// A seed's flanks are two tasks of xdrop_tasks: the right one A[seed_a + seed_len ..) against B[seed_b + seed_len ..)
// read forwards, the left one A[.. seed_a) against B[.. seed_b) read backwards in place from the bytes next to the
// seed (msa_xdrop_flank_run's step -1) -- no reversed copy is made or uploaded.
namespace {

struct SeedIn {
  const int64_t *a, *b, *len;  // per pair, relative to the pair
};
struct SeedOut {
  int32_t* score;
  int64_t *beg_ij, *end_ij;  // 2 per pair
  int32_t* flank_score;      // {left, right} per pair, or nullptr
  int64_t* diagonals;        // {left, right} per pair, or nullptr
  char* cigars;
  size_t cigar_cap;
  int64_t* cigar_off;
};

// Seeds [p0, p1) of a call: their launched flanks as one range of tasks -- 2 p (left) and 2 p + 1 (right) next to each
// other, so both flanks of a seed share a workgroup; empty flanks are left out --, then the stitching.  fl[4 p ..] =
// the clipped {m', n'} of seed p's left and right flank, 0 for a flank that is not launched
int seed_range(const AlignSpec& spec, const GapBand& gb, int32_t xdrop, bool want_tb, const uint8_t* ca,
               const uint8_t* cb, const AlignIn& in, const SeedIn& sd, const int64_t* fl, int64_t p0, int64_t p1,
               size_t bytes, const SeedOut& out, std::string& all) {
  std::vector<XTask> tasks;
  for (int64_t p = p0; p < p1; ++p) {
    const int64_t sa = in.a_off[p] + sd.a[p], sb = in.b_off[p] + sd.b[p], *f = fl + 4 * p;
    if (f[0]) tasks.push_back(XTask{f[0], f[1], sa - 1, sb - 1, -1});
    if (f[2]) tasks.push_back(XTask{f[2], f[3], sa + sd.len[p], sb + sd.len[p], 1});
  }
  std::vector<XTaskOut> res;
  if (!tasks.empty()) {
    const int rc = xdrop_tasks(spec, gb, xdrop, want_tb, ca, cb, tasks, bytes, res);
    if (rc != MSA_OK) return rc;
  }
  const XTaskOut none{0, 0, 0, 0, 0, std::string()};  // the empty extension
  const int stride = spec.wide ? 32 : 8;
  size_t t = 0;
  for (int64_t p = p0; p < p1; ++p) {
    const int64_t sa = sd.a[p], sb = sd.b[p], len = sd.len[p], *f = fl + 4 * p;
    const XTaskOut& L = f[0] ? res[t++] : none;
    const XTaskOut& R = f[2] ? res[t++] : none;
    int64_t seed = 0;
    for (int64_t k = 0; k < len; ++k)
      seed += spec.tab[stride * ca[in.a_off[p] + sa + k] + cb[in.b_off[p] + sb + k]];
    out.score[p] = (int32_t)(L.score + seed + R.score);
    out.beg_ij[2 * p] = sa - L.end_i;
    out.beg_ij[2 * p + 1] = sb - L.end_j;
    out.end_ij[2 * p] = sa + len + R.end_i;
    out.end_ij[2 * p + 1] = sb + len + R.end_j;
    if (out.flank_score) out.flank_score[2 * p] = (int32_t)L.score, out.flank_score[2 * p + 1] = (int32_t)R.score;
    if (out.diagonals) out.diagonals[2 * p] = L.D, out.diagonals[2 * p + 1] = R.D;
    if (!out.cigars) continue;
    // end -> start: the right flank's ops as walked, the seed, and the left flank's -- walked from its far end to the
    // seed, which is start -> end already -- turned round
    std::string o = R.ops;
    o.append((size_t)len, 'M');
    o.append(L.ops.rbegin(), L.ops.rend());
    out.cigar_off[p] = (int64_t)all.size();
    all += cigar_of(o.data(), o.size());
    all.push_back('\0');
  }
  return MSA_OK;
}

int seed_pairs(AlignSpec spec, const AlignIn& in, const SeedIn& sd, int32_t gap_open, int32_t gap_extend,
               int64_t band_in, int32_t xdrop, const SeedOut& out) {
  if (spec.status != MSA_OK) return spec.status;
  if (!in.A || !in.B || !in.a_off || !in.m || !in.b_off || !in.n || !sd.a || !sd.b || !sd.len || !out.score ||
      !out.beg_ij || !out.end_ij || (out.cigars && !out.cigar_off) || in.np < 1)
    return MSA_ERR_ARG;
  int64_t span_max = 0;
  for (int64_t p = 0; p < in.np; ++p) {
    const int64_t m = in.m[p], n = in.n[p], ao = in.a_off[p], bo = in.b_off[p];
    if (m < 1 || n < 1 || m > kPairLimit || n > kPairLimit || ao < 0 || bo < 0 ||
        (uint64_t)ao + (uint64_t)m > in.a_len || (uint64_t)bo + (uint64_t)n > in.b_len)
      return MSA_ERR_ARG;
    if (sd.len[p] < 0 || sd.a[p] < 0 || sd.b[p] < 0 || sd.len[p] > m - sd.a[p] || sd.len[p] > n - sd.b[p])
      return MSA_ERR_ARG;
    span_max = std::max(span_max, std::max(m, n));
  }
  if (band_in < 0) return MSA_ERR_ARG;
  if (std::min(band_in, span_max) > MSA_XDROP_BAND_MAX || gap_extend < 0 || gap_open < gap_extend)
    return MSA_ERR_UNSUPPORTED;
  // (the band of the longest sequence holds every cell of every flank: it stands in for a wider one)
  const GapBand gb{gap_open, gap_extend, (int)std::min(band_in, span_max)};
  const int smax = table_smax(spec);
  for (int64_t p = 0; p < in.np; ++p)
    if (!value_range_ok(smax, gb, in.m[p] + in.n[p])) return MSA_ERR_UNSUPPORTED;
  std::vector<uint8_t> ca(in.a_len), cb(in.b_len);
  int rc = spec.symbols.encode(in.A, in.a_len, ca.data());
  if (rc == MSA_OK) rc = spec.symbols.encode(in.B, in.b_len, cb.data());
  if (rc != MSA_OK) return rc;
  // every flank clipped to the band on its own, as msa_extend_align_xdrop clips the pair it is given
  std::vector<int64_t> fl(4 * (size_t)in.np, 0);
  int64_t launched = 0;
  for (int64_t p = 0; p < in.np; ++p) {
    const int64_t ra = in.m[p] - sd.a[p] - sd.len[p], rb = in.n[p] - sd.b[p] - sd.len[p];
    int64_t* f = &fl[4 * (size_t)p];  // (a flank with an empty side is no flank: extend_band_clip leaves its 0, 0)
    if (extend_band_clip(sd.a[p], sd.b[p], band_in, f[0], f[1])) ++launched;
    if (extend_band_clip(ra, rb, band_in, f[2], f[3])) ++launched;
  }
  if (launched && (rc = ensure_device()) != MSA_OK) return rc;
  const bool want_tb = out.cigars != nullptr;
  auto fp = [&](int64_t p) -> size_t {
    const int64_t* f = &fl[4 * (size_t)p];
    return (f[0] ? footprint_xdrop(f[0], f[1], gb.band, want_tb) : 0) +
           (f[2] ? footprint_xdrop(f[2], f[3], gb.band, want_tb) : 0);
  };
  size_t quarter = SIZE_MAX;
  if (launched) {
    int64_t binfo[5];
    admission().info(current_device(), binfo);
    quarter = (size_t)binfo[0] / 4;
  }
  std::string all;  // the CIGARs, back to back
  for (int64_t p0 = 0, p1; p0 < in.np; p0 = p1) {
    size_t bytes = fp(p0);
    p1 = p0 + 1;
    while (p1 < in.np && p1 - p0 < (int64_t(1) << 20) && bytes + fp(p1) <= quarter) bytes += fp(p1++);
    rc = seed_range(spec, gb, xdrop, want_tb, ca.data(), cb.data(), in, sd, fl.data(), p0, p1, bytes, out, all);
    if (rc != MSA_OK) return rc;
  }
  if (out.cigars) {
    out.cigar_off[in.np] = (int64_t)all.size();
    if (all.size() > out.cigar_cap) return MSA_ERR_CAPACITY;
    std::memcpy(out.cigars, all.data(), all.size());
  }
  return MSA_OK;
}

int seed_align(const char* A0, size_t m, const char* B0, size_t n, int64_t seed_a, int64_t seed_b, int64_t seed_len,
               const char* alphabet, size_t n_sym, const int8_t* sub, size_t max_sym, int32_t gap_open,
               int32_t gap_extend, int64_t band, int32_t xdrop, int32_t* score, int64_t* beg_ij, int64_t* end_ij,
               int32_t* flank_score, int64_t* diagonals, char* cigar, size_t cigar_cap) {
  const OnePairIn one(A0, m, B0, n);
  int64_t coff[2];
  return seed_pairs(spec_extend_band(alphabet, n_sym, sub, max_sym), one.in, SeedIn{&seed_a, &seed_b, &seed_len},
                    gap_open, gap_extend, band, xdrop,
                    SeedOut{score, beg_ij, end_ij, flank_score, diagonals, cigar, cigar_cap, coff});
}
int seed_align_batch(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs, const int64_t* a_off,
                     const int64_t* m, const int64_t* b_off, const int64_t* n, const int64_t* seed_a,
                     const int64_t* seed_b, const int64_t* seed_len, const char* alphabet, size_t n_sym,
                     const int8_t* sub, size_t max_sym, int32_t gap_open, int32_t gap_extend, int64_t band,
                     int32_t xdrop, int32_t* score, int64_t* beg_ij, int64_t* end_ij, int32_t* flank_score,
                     int64_t* diagonals, char* cigars, size_t cigar_cap, int64_t* cigar_off) {
  return seed_pairs(spec_extend_band(alphabet, n_sym, sub, max_sym), AlignIn{A, B, a_len, b_len, n_pairs, a_off, m, b_off, n},
                    SeedIn{seed_a, seed_b, seed_len}, gap_open, gap_extend, band, xdrop,
                    SeedOut{score, beg_ij, end_ij, flank_score, diagonals, cigars, cigar_cap, cigar_off});
}

}  // namespace

extern "C" {

int msa_seed_align(const char* A0, size_t m, const char* B0, size_t n, int64_t seed_a, int64_t seed_b,
                   int64_t seed_len, const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                   int32_t gap_extend, int64_t band, int32_t xdrop, int32_t* score, int64_t* beg_ij, int64_t* end_ij,
                   int32_t* flank_score, int64_t* diagonals, char* cigar, size_t cigar_cap) {
  return seed_align(A0, m, B0, n, seed_a, seed_b, seed_len, alphabet, n_sym, sub, 8, gap_open, gap_extend, band, xdrop,
                    score, beg_ij, end_ij, flank_score, diagonals, cigar, cigar_cap);
}

int msa_seed_align32(const char* A0, size_t m, const char* B0, size_t n, int64_t seed_a, int64_t seed_b,
                     int64_t seed_len, const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                     int32_t gap_extend, int64_t band, int32_t xdrop, int32_t* score, int64_t* beg_ij,
                     int64_t* end_ij, int32_t* flank_score, int64_t* diagonals, char* cigar, size_t cigar_cap) {
  return seed_align(A0, m, B0, n, seed_a, seed_b, seed_len, alphabet, n_sym, sub, 32, gap_open, gap_extend, band,
                    xdrop, score, beg_ij, end_ij, flank_score, diagonals, cigar, cigar_cap);
}

int msa_seed_align_batch(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                         const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                         const int64_t* seed_a, const int64_t* seed_b, const int64_t* seed_len, const char* alphabet,
                         size_t n_sym, const int8_t* sub, int32_t gap_open, int32_t gap_extend, int64_t band,
                         int32_t xdrop, int32_t* score, int64_t* beg_ij, int64_t* end_ij, int32_t* flank_score,
                         int64_t* diagonals, char* cigars, size_t cigar_cap, int64_t* cigar_off) {
  return seed_align_batch(A, a_len, B, b_len, n_pairs, a_off, m, b_off, n, seed_a, seed_b, seed_len, alphabet, n_sym,
                          sub, 8, gap_open, gap_extend, band, xdrop, score, beg_ij, end_ij, flank_score, diagonals,
                          cigars, cigar_cap, cigar_off);
}

int msa_seed_align_batch32(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                           const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                           const int64_t* seed_a, const int64_t* seed_b, const int64_t* seed_len, const char* alphabet,
                           size_t n_sym, const int8_t* sub, int32_t gap_open, int32_t gap_extend, int64_t band,
                           int32_t xdrop, int32_t* score, int64_t* beg_ij, int64_t* end_ij, int32_t* flank_score,
                           int64_t* diagonals, char* cigars, size_t cigar_cap, int64_t* cigar_off) {
  return seed_align_batch(A, a_len, B, b_len, n_pairs, a_off, m, b_off, n, seed_a, seed_b, seed_len, alphabet, n_sym,
                          sub, 32, gap_open, gap_extend, band, xdrop, score, beg_ij, end_ij, flank_score, diagonals,
                          cigars, cigar_cap, cigar_off);
}

}  // extern "C"

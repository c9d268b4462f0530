// msa_xdropapi.inc -- banded extension alignment with X-drop termination (included by msa_capi.hip after
// msa_alignapi.inc): the device-resident entries over msa_xdrop.hip's two kernels
//     msa_xdrop_flank_run (msa_xdrop_extend_run is it with every pair read forwards), msa_xdrop_extend_walk
// and the host-pointer entries built on them through align_pairs (every check and its order are the *_banded twins')
//     msa_extend_align_xdrop, msa_extend_align_batch_xdrop, *32
extern "C" {

int msa_xdrop_flank_run(const uint8_t* dA, const uint8_t* dB, int64_t n_pairs, const int64_t* d_m,
                        const int64_t* d_n, const int64_t* d_a_off, const int64_t* d_b_off, const int8_t* d_step,
                        const int8_t* d_sub32, int32_t match, int32_t mismatch, int32_t gap_open, int32_t gap_extend,
                        int32_t band, int32_t xdrop, uint8_t* d_dir, const int64_t* d_dir_off, int64_t* d_res,
                        void* stream) {
  if (!dA || !dB || !d_m || !d_n || !d_a_off || !d_b_off || !d_res || (d_dir && !d_dir_off) || n_pairs < 1 ||
      n_pairs > (int64_t(1) << 26) || band < 0)
    return MSA_ERR_ARG;
  if (gap_extend < 0 || gap_open < gap_extend || band > MSA_XDROP_BAND_MAX ||
      (!d_sub32 && (match < -128 || match > 127 || mismatch < -128 || mismatch > 127)))
    return MSA_ERR_UNSUPPORTED;
  const int rc = ensure_device();
  if (rc != MSA_OK) return rc;
  const int np = (int)n_pairs;
  // (without steps: the instantiation that has none, the forward fill as it was)
  hipLaunchKernelGGL(d_step ? xdrop_fill_kernel<true> : xdrop_fill_kernel<false>,
                     dim3((unsigned)((np + XD_WPB - 1) / XD_WPB)), dim3(64 * XD_WPB),
                     xd_lds_bytes(band), (hipStream_t)stream, dA, dB, np, (const long long*)d_m,
                     (const long long*)d_n, (const long long*)d_a_off, (const long long*)d_b_off, d_step, d_sub32,
                     (int)match, (int)mismatch, (int)gap_extend, (int)gap_open, (int)band, (int)xdrop, d_dir,
                     (const long long*)d_dir_off, (long long*)d_res);
  HIPCHK(hipGetLastError());
  return MSA_OK;
}

int msa_xdrop_extend_run(const uint8_t* dA, const uint8_t* dB, int64_t n_pairs, const int64_t* d_m,
                         const int64_t* d_n, const int64_t* d_a_off, const int64_t* d_b_off, const int8_t* d_sub32,
                         int32_t match, int32_t mismatch, int32_t gap_open, int32_t gap_extend, int32_t band,
                         int32_t xdrop, uint8_t* d_dir, const int64_t* d_dir_off, int64_t* d_res, void* stream) {
  return msa_xdrop_flank_run(dA, dB, n_pairs, d_m, d_n, d_a_off, d_b_off, nullptr, d_sub32, match, mismatch, gap_open,
                             gap_extend, band, xdrop, d_dir, d_dir_off, d_res, stream);
}

int msa_xdrop_extend_walk(int64_t n_pairs, int32_t band, const uint8_t* d_dir, const int64_t* d_dir_off,
                          const int64_t* d_res, uint8_t* d_ops, const int64_t* d_ops_off, int64_t* d_info,
                          void* stream) {
  if (!d_dir || !d_dir_off || !d_res || !d_ops || !d_ops_off || !d_info || n_pairs < 1 ||
      n_pairs > (int64_t(1) << 26) || band < 0)
    return MSA_ERR_ARG;
  if (band > MSA_XDROP_BAND_MAX) return MSA_ERR_UNSUPPORTED;
  const int rc = ensure_device();
  if (rc != MSA_OK) return rc;
  const int np = (int)n_pairs;
  hipLaunchKernelGGL(xdrop_walk_kernel, dim3((unsigned)((np + XD_WPB - 1) / XD_WPB)), dim3(64 * XD_WPB), 0,
                     (hipStream_t)stream, d_dir, (const long long*)d_dir_off, (const long long*)d_res, np, (int)band,
                     d_ops, (const long long*)d_ops_off, (long long*)d_info);
  HIPCHK(hipGetLastError());
  return MSA_OK;
}

}  // extern "C"

namespace {

static_assert(MSA_XDROP_BAND_MAX == XD_BAND_MAX, "msa.h states the kernel's cap");

// Device footprint of one pair: the compact band form's (2 band + 1)(m + 1) bytes (none for a score-only call), the
// codes, the ops, the per-pair words, and the pooled size classes' slack
size_t footprint_xdrop(int64_t m, int64_t n, int band, bool dir) {
  return (dir ? (size_t)(2 * band + 1) * (size_t)(m + 1) + 2 * (size_t)(m + n) + 64 : 0) + (size_t)(m + n) + 256 +
         (size_t(8) << 20);
}

// the largest |score| of a spec's table, and the value-range inequality of msa_plan_create_scored over `span` = m + n
int table_smax(const AlignSpec& spec) {
  const int k = spec.wide ? 32 : 8;
  int smax = 0;
  for (int a = 0; a < k; ++a)
    for (int b = 0; b < k; ++b) smax = std::max(smax, std::abs((int)spec.tab[k * a + b]));
  return smax;
}
bool value_range_ok(int smax, const GapBand& gb, int64_t span) {
  return ((int64_t)smax + 2 * (int64_t)gb.gap_open + 2 * (int64_t)gb.gap_extend) * (span + 256) +
             ((int64_t)gb.gap_open - gb.gap_extend) <
         (int64_t(1) << 28);
}

// One fill of msa_xdrop.hip with its walk: m x n (clipped already, |m - n| <= the band) from the call's codes at
// ca[a_off] and cb[b_off], read forwards (step +1) or backwards in place (step -1: a_off and b_off name the LAST bytes
// of the two sequences, a seed's left flank).  What comes back: the result words and, for a walk, its ops (end -> start)
// completed along the border
struct XTask {
  int64_t m, n, a_off, b_off;
  int step;
};
struct XTaskOut {
  int64_t score, end_i, end_j, D, fin;
  std::string ops;
};

// align_range's sibling: the tasks of one range through msa_xdrop_flank_run and, for CIGARs, msa_xdrop_extend_walk on
// one stream; the same uploads (the window of the codes that the tasks read, coinciding ranges sent once, a reversed
// task's [a_off - m + 1, a_off] included) and the same border completion.  res holds every task's result once every
// fill has status 0 (whatever becomes of the walks)
int xdrop_tasks(const AlignSpec& spec, const GapBand& gb, int32_t xdrop, bool want_tb, const uint8_t* ca,
                const uint8_t* cb, const std::vector<XTask>& tasks, size_t bytes, std::vector<XTaskOut>& res_out) {
  const int64_t K = (int64_t)tasks.size();
  int64_t a_lo = INT64_MAX, a_hi = 0, b_lo = INT64_MAX, b_hi = 0;
  bool reversed = false;
  for (const XTask& t : tasks) {
    const bool back = t.step < 0;
    a_lo = std::min(a_lo, back ? t.a_off - t.m + 1 : t.a_off);
    a_hi = std::max(a_hi, back ? t.a_off + 1 : t.a_off + t.m);
    b_lo = std::min(b_lo, back ? t.b_off - t.n + 1 : t.b_off);
    b_hi = std::max(b_hi, back ? t.b_off + 1 : t.b_off + t.n);
    reversed = reversed || back;
  }
  // one block of per-task words: m, n, a_off, b_off (K each), dir_off, ops_off (K + 1 each), the table, and the steps
  // (one int8 each) where a task reads backwards
  std::vector<int64_t> meta(6 * (size_t)K + 2 + 128 + (reversed ? ((size_t)K + 7) / 8 : 0));
  int64_t *hm = meta.data(), *hn = hm + K, *hao = hn + K, *hbo = hao + K, *hdo = hbo + K, *hoo = hdo + K + 1;
  int8_t* htab = (int8_t*)(hoo + K + 1);
  int8_t* hstep = htab + 1024;
  hdo[0] = 0;
  for (int64_t k = 0; k < K; ++k) {
    const XTask& t = tasks[(size_t)k];
    hm[k] = t.m;
    hn[k] = t.n;
    hao[k] = t.a_off - a_lo;
    hbo[k] = t.b_off - b_lo;
    hdo[k + 1] = hdo[k] + (want_tb ? (int64_t)(2 * gb.band + 1) * (hm[k] + 1) : 0);
    if (reversed) hstep[k] = (int8_t)t.step;
  }
  const std::vector<int64_t> ooff = ops_offsets(hm, hn, K);
  std::copy(ooff.begin(), ooff.end(), hoo);
  std::memset(htab, 0, 1024);
  for (int a = 0; a < (spec.wide ? 32 : 8); ++a)
    for (int b = 0; b < (spec.wide ? 32 : 8); ++b) htab[32 * a + b] = spec.tab[(spec.wide ? 32 : 8) * a + b];
  int rc;
  DeviceCall dc(bytes);
  if ((rc = dc.status()) != MSA_OK) return rc;
  void *dA = dc.alloc((size_t)(a_hi - a_lo)), *dB = dc.alloc((size_t)(b_hi - b_lo));
  int64_t* dMeta = (int64_t*)dc.alloc(meta.size() * sizeof(int64_t));
  int64_t* dRes = (int64_t*)dc.alloc(64 * (size_t)K);
  if (!dA || !dB || !dMeta || !dRes) return MSA_ERR_NOMEM;
  if ((rc = dc.upload(dA, ca + a_lo, (size_t)(a_hi - a_lo))) || (rc = dc.upload(dB, cb + b_lo, (size_t)(b_hi - b_lo))) ||
      (rc = dc.upload(dMeta, meta.data(), meta.size() * sizeof(int64_t))))
    return rc;
  void *dDir = nullptr, *dOps = nullptr, *dInfo = nullptr;
  if (want_tb && (!(dDir = dc.alloc((size_t)hdo[K])) || !(dOps = dc.alloc((size_t)ooff[(size_t)K])) ||
                  !(dInfo = dc.alloc(64 * (size_t)K))))
    return MSA_ERR_NOMEM;
  const hipStream_t st = dc.stream();
  int64_t *dm = dMeta, *dn = dm + K, *dao = dn + K, *dbo = dao + K, *ddo = dbo + K, *doo = ddo + K + 1;
  const int8_t* dtab = (const int8_t*)(doo + K + 1);
  if ((rc = msa_xdrop_flank_run((const uint8_t*)dA, (const uint8_t*)dB, K, dm, dn, dao, dbo,
                                reversed ? dtab + 1024 : nullptr, dtab, 0, 0, gb.gap_open, gb.gap_extend, gb.band,
                                xdrop, (uint8_t*)dDir, ddo, dRes, st)))
    return rc;
  if (want_tb && (rc = msa_xdrop_extend_walk(K, gb.band, (const uint8_t*)dDir, ddo, dRes, (uint8_t*)dOps, doo,
                                             (int64_t*)dInfo, st)))
    return rc;
  std::vector<int64_t> res(8 * (size_t)K), info(want_tb ? 8 * (size_t)K : 0);
  std::vector<char> ops(want_tb ? (size_t)ooff[(size_t)K] : 0);
  if ((rc = dc.download(res.data(), dRes, 64 * (size_t)K)) ||
      (want_tb && ((rc = dc.download(info.data(), dInfo, 64 * (size_t)K)) ||
                   (rc = dc.download(ops.data(), dOps, ops.size())))) ||
      (rc = dc.sync()))
    return rc;
  for (int64_t k = 0; k < K; ++k)
    if (res[8 * (size_t)k + 5] != 0) return (int)res[8 * (size_t)k + 5];  // (the first failing task's status)
  res_out.resize((size_t)K);
  for (int64_t k = 0; k < K; ++k) {
    const int64_t* r = &res[8 * (size_t)k];
    res_out[(size_t)k] = XTaskOut{r[0], r[1], r[2], r[3], r[4], std::string()};
  }
  for (int64_t k = 0; want_tb && k < K; ++k) {
    const int64_t* inf = &info[8 * (size_t)k];
    if (inf[3] != 0) return (int)inf[3];
    std::string& o = res_out[(size_t)k].ops;
    o.assign(ops.data() + ooff[(size_t)k], (size_t)inf[0]);
    complete_border(o, inf[1] - 1, inf[2] - 1, spec.border);
  }
  return MSA_OK;
}

// pairs [p0, p1) of a call (clipped already, |m - n| <= gb.band), each one forward task; the results and CIGARs
int xdrop_range(const AlignSpec& spec, const GapBand& gb, const XDrop& xd, bool want_tb, const uint8_t* ca,
                const uint8_t* cb, const AlignIn& in, int64_t p0, int64_t p1, size_t bytes, const AlignOut& out,
                std::string& all) {
  // the value-range inequality of msa_plan_create_scored, where a plan's creation would decide it
  const int smax = table_smax(spec);
  std::vector<XTask> tasks;
  for (int64_t p = p0; p < p1; ++p) {
    if (!value_range_ok(smax, gb, in.m[p] + in.n[p])) return MSA_ERR_UNSUPPORTED;
    tasks.push_back(XTask{in.m[p], in.n[p], in.a_off[p], in.b_off[p], 1});
  }
  std::vector<XTaskOut> res;
  const int rc = xdrop_tasks(spec, gb, xd.xdrop, want_tb, ca, cb, tasks, bytes, res);
  for (size_t k = 0; k < res.size(); ++k) {
    const int64_t p = p0 + (int64_t)k;
    if (out.score) out.score[p] = (int32_t)res[k].score;
    if (out.fin_h) out.fin_h[p] = (int32_t)res[k].fin;
    if (xd.diagonals) xd.diagonals[p] = res[k].D;
    out.end.put(p, res[k].end_i, res[k].end_j);
  }
  if (rc != MSA_OK || !want_tb) return rc;
  for (size_t k = 0; out.cigars && k < res.size(); ++k) {
    out.cigar_off[p0 + (int64_t)k] = (int64_t)all.size();
    all += cigar_of(res[k].ops.data(), res[k].ops.size());
    all.push_back('\0');
  }
  return MSA_OK;
}

int extend_align_xdrop(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                       const int8_t* sub, size_t max_sym, int32_t gap_open, int32_t gap_extend, int64_t band,
                       int32_t xdrop, int32_t* score, int64_t* end_ij, int32_t* global_score, int64_t* diagonals,
                       char* cigar, size_t cigar_cap) {
  const OnePairIn one(A0, m, B0, n);
  int64_t coff[2];
  const AlignOut out{score, PairOut(end_ij), PairOut(), PairOut(), cigar, cigar_cap, coff, global_score};
  const XDrop xd{xdrop, diagonals};
  return align_pairs(spec_extend_band(alphabet, n_sym, sub, max_sym), 1, one.in, kPairLimit, gap_open, gap_extend,
                     band, out, &xd);
}
int extend_align_batch_xdrop(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                             const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                             const char* alphabet, size_t n_sym, const int8_t* sub, size_t max_sym, int32_t gap_open,
                             int32_t gap_extend, int64_t band, int32_t xdrop, int32_t* score, int64_t* end_ij,
                             int32_t* global_score, int64_t* diagonals, char* cigars, size_t cigar_cap,
                             int64_t* cigar_off) {
  if (!end_ij) return MSA_ERR_ARG;
  const AlignIn in{A, B, a_len, b_len, n_pairs, a_off, m, b_off, n};
  const AlignOut out{score, PairOut(end_ij), PairOut(), PairOut(), cigars, cigar_cap, cigar_off, global_score};
  const XDrop xd{xdrop, diagonals};
  return align_pairs(spec_extend_band(alphabet, n_sym, sub, max_sym), 0, in, kPairLimit, gap_open, gap_extend, band,
                     out, &xd);
}

}  // namespace

extern "C" {

int msa_extend_align_xdrop(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                           const int8_t* sub, int32_t gap_open, int32_t gap_extend, int64_t band, int32_t xdrop,
                           int32_t* score, int64_t* end_ij, int32_t* global_score, int64_t* diagonals, char* cigar,
                           size_t cigar_cap) {
  return extend_align_xdrop(A0, m, B0, n, alphabet, n_sym, sub, 8, gap_open, gap_extend, band, xdrop, score, end_ij,
                            global_score, diagonals, cigar, cigar_cap);
}

int msa_extend_align_xdrop32(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                             const int8_t* sub, int32_t gap_open, int32_t gap_extend, int64_t band, int32_t xdrop,
                             int32_t* score, int64_t* end_ij, int32_t* global_score, int64_t* diagonals, char* cigar,
                             size_t cigar_cap) {
  return extend_align_xdrop(A0, m, B0, n, alphabet, n_sym, sub, 32, gap_open, gap_extend, band, xdrop, score, end_ij,
                            global_score, diagonals, cigar, cigar_cap);
}

int msa_extend_align_batch_xdrop(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                                 const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                                 const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                                 int32_t gap_extend, int64_t band, int32_t xdrop, int32_t* score, int64_t* end_ij,
                                 int32_t* global_score, int64_t* diagonals, char* cigars, size_t cigar_cap,
                                 int64_t* cigar_off) {
  return extend_align_batch_xdrop(A, a_len, B, b_len, n_pairs, a_off, m, b_off, n, alphabet, n_sym, sub, 8, gap_open,
                                  gap_extend, band, xdrop, score, end_ij, global_score, diagonals, cigars, cigar_cap,
                                  cigar_off);
}

int msa_extend_align_batch_xdrop32(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                                   const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                                   const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                                   int32_t gap_extend, int64_t band, int32_t xdrop, int32_t* score, int64_t* end_ij,
                                   int32_t* global_score, int64_t* diagonals, char* cigars, size_t cigar_cap,
                                   int64_t* cigar_off) {
  return extend_align_batch_xdrop(A, a_len, B, b_len, n_pairs, a_off, m, b_off, n, alphabet, n_sym, sub, 32, gap_open,
                                  gap_extend, band, xdrop, score, end_ij, global_score, diagonals, cigars, cigar_cap,
                                  cigar_off);
}

}  // extern "C"

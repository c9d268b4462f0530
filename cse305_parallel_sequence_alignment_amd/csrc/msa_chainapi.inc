// msa_chainapi.inc -- seed chaining (included by msa_capi.hip after msa_seedapi.inc): the device-resident entry over
// msa_chain.hip's kernel
//     msa_chain_run
// and the host-pointer entries built on it -- the anchors' checks, ranges of problems through DeviceCall, and the chain
// extraction, which is host work (the contract is include/msa.h's at msa_chain_seeds)
//     msa_chain_seeds, msa_chain_seeds_batch
namespace {

static_assert(MSA_CHAIN_LOOKBACK_MAX == CH_LOOKBACK_MAX, "msa.h states the kernel's cap");
static_assert(kPairLimit == CH_LIMIT, "the kernel's coordinate bound is the library's");

struct ChainParams {
  int32_t match, gap_open, gap_extend;
  int64_t band, max_dist;
  int32_t lookback;
};

// the parameter bounds (MSA_ERR_UNSUPPORTED): with them every value of the recurrence fits an int32
bool chain_params_ok(const ChainParams& c) {
  if (c.match < 1 || c.gap_extend < 0 || c.gap_open < c.gap_extend || c.band < 0 || c.max_dist < 1 ||
      c.lookback < 1 || c.lookback > MSA_CHAIN_LOOKBACK_MAX)
    return false;
  if ((int64_t)c.match * kPairLimit >= (int64_t(1) << 30)) return false;
  const int64_t L = std::min(c.band, kPairLimit);
  const int64_t gc = L ? ((int64_t)c.gap_open - c.gap_extend) + (int64_t)c.gap_extend * L : 0;
  return gc < (int64_t(1) << 30);
}

}  // namespace

extern "C" {

int msa_chain_run(const int64_t* d_a, const int64_t* d_b, const int64_t* d_len, int64_t n_problems,
                  const int64_t* d_off, int32_t match, int32_t gap_open, int32_t gap_extend, int64_t band,
                  int64_t max_dist, int32_t lookback, int32_t* d_f, int32_t* d_pred, int32_t* d_status, void* stream) {
  if (!d_a || !d_b || !d_len || !d_off || !d_f || !d_pred || !d_status || n_problems < 1 ||
      n_problems > (int64_t(1) << 26))
    return MSA_ERR_ARG;
  if (!chain_params_ok(ChainParams{match, gap_open, gap_extend, band, max_dist, lookback})) return MSA_ERR_UNSUPPORTED;
  const int rc = ensure_device();
  if (rc != MSA_OK) return rc;
  const int np = (int)n_problems;
  hipLaunchKernelGGL(chain_kernel, dim3((unsigned)((np + CH_WPB - 1) / CH_WPB)), dim3(64 * CH_WPB),
                     ch_lds_bytes(lookback), (hipStream_t)stream, (const long long*)d_a, (const long long*)d_b,
                     (const long long*)d_len, np, (const long long*)d_off, (int)match, (int)(gap_open - gap_extend),
                     (int)gap_extend, (int)std::min(band, kPairLimit), (int)std::min(max_dist, kPairLimit),
                     (int)lookback, d_f, d_pred, d_status);
  HIPCHK(hipGetLastError());
  return MSA_OK;
}

}  // extern "C"

namespace {

// Device footprint of a range of problems holding `anchors` anchors: three int64 inputs and two int32 outputs per
// anchor, the offsets and a status per problem, and the pooled size classes' slack
size_t footprint_chain(int64_t anchors, int64_t problems) {
  return 32 * (size_t)anchors + 12 * (size_t)problems + 64 + (size_t(8) << 20);
}

// problems [p0, p1) of a call through msa_chain_run: f and pred of their anchors (indexed as the call's)
int chain_range(const ChainParams& c, const int64_t* a, const int64_t* b, const int64_t* len, const int64_t* off,
                int64_t p0, int64_t p1, int32_t* f, int32_t* pred) {
  const int64_t K = p1 - p0, lo = off[p0], T = off[p1] - lo;
  std::vector<int64_t> roff((size_t)K + 1);
  for (int64_t k = 0; k <= K; ++k) roff[(size_t)k] = off[p0 + k] - lo;
  int rc;
  DeviceCall dc(footprint_chain(T, K));
  if ((rc = dc.status()) != MSA_OK) return rc;
  const size_t in = (size_t)T * sizeof(int64_t), out = (size_t)T * sizeof(int32_t);
  int64_t* dIn = (int64_t*)dc.alloc(3 * in);
  int64_t* dOff = (int64_t*)dc.alloc(roff.size() * sizeof(int64_t));
  int32_t* dOut = (int32_t*)dc.alloc(2 * out);
  int32_t* dSt = (int32_t*)dc.alloc((size_t)K * sizeof(int32_t));
  if (!dIn || !dOff || !dOut || !dSt) return MSA_ERR_NOMEM;
  if ((rc = dc.upload(dIn, a + lo, in)) || (rc = dc.upload(dIn + T, b + lo, in)) ||
      (rc = dc.upload(dIn + 2 * T, len + lo, in)) || (rc = dc.upload(dOff, roff.data(), roff.size() * sizeof(int64_t))))
    return rc;
  if ((rc = msa_chain_run(dIn, dIn + T, dIn + 2 * T, K, dOff, c.match, c.gap_open, c.gap_extend, c.band, c.max_dist,
                          c.lookback, dOut, dOut + T, dSt, dc.stream())))
    return rc;
  std::vector<int32_t> st((size_t)K);
  if ((rc = dc.download(f + lo, dOut, out)) || (rc = dc.download(pred + lo, dOut + T, out)) ||
      (rc = dc.download(st.data(), dSt, st.size() * sizeof(int32_t))) || (rc = dc.sync()))
    return rc;
  for (int32_t s : st)
    if (s != 0) return s;  // (the first failing problem's status; the host checked the same rules before)
  return MSA_OK;
}

// The chains of one problem of n anchors from its f and pred: chain_of per anchor, the kept chains' scores by rank
// (score may be nullptr) -> their number, or MSA_ERR_NOMATCH for a pred that is no earlier anchor
int chain_extract(const int32_t* f, const int32_t* pred, int64_t n, int32_t min_score, int32_t* chain_of,
                  int32_t* score) {
  std::vector<int32_t> order((size_t)n);
  for (int64_t t = 0; t < n; ++t) {
    order[(size_t)t] = (int32_t)t;
    chain_of[t] = -1;
    if (pred[t] < -1 || pred[t] >= t) return MSA_ERR_NOMATCH;
  }
  std::sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return f[x] != f[y] ? f[x] > f[y] : x < y; });
  std::vector<char> taken((size_t)n, 0);
  std::vector<int32_t> members;
  int32_t rank = 0;
  for (int32_t end : order) {
    if (taken[(size_t)end]) continue;
    members.clear();
    int32_t u = end;
    for (; u >= 0 && !taken[(size_t)u]; u = pred[u]) {
      taken[(size_t)u] = 1;
      members.push_back(u);
    }
    const int32_t sc = f[end] - (u >= 0 ? f[u] : 0);
    if (sc < min_score) continue;
    for (int32_t t : members) chain_of[t] = rank;
    if (score) score[rank] = sc;
    ++rank;
  }
  return rank;
}

int chain_problems(const int64_t* a, const int64_t* b, const int64_t* len, int64_t np, const int64_t* off,
                   const ChainParams& c, int32_t min_score, int32_t* f_out, int32_t* pred_out, int32_t* chain_of,
                   int32_t* n_chains, int32_t* chain_score) {
  if (!off || !chain_of || !n_chains || np < 1 || np > (int64_t(1) << 26) || off[0] < 0) return MSA_ERR_ARG;
  int64_t n_max = 0;
  for (int64_t p = 0; p < np; ++p) {
    const int64_t n = off[p + 1] - off[p];
    if (n < 0 || n > kPairLimit) return MSA_ERR_ARG;
    n_max = std::max(n_max, n);
  }
  const int64_t lo = off[0], hi = off[np];
  if (hi > lo && (!a || !b || !len)) return MSA_ERR_ARG;
  for (int64_t p = 0; p < np; ++p)
    for (int64_t t = off[p]; t < off[p + 1]; ++t) {
      if (a[t] < 0 || b[t] < 0 || len[t] < 1 || a[t] > kPairLimit || b[t] > kPairLimit || len[t] > kPairLimit ||
          a[t] + len[t] > kPairLimit || b[t] + len[t] > kPairLimit)
        return MSA_ERR_ARG;
      if (t == off[p]) continue;
      const int64_t be = b[t] + len[t], be0 = b[t - 1] + len[t - 1];
      if (be < be0 || (be == be0 && a[t] + len[t] < a[t - 1] + len[t - 1])) return MSA_ERR_ARG;
    }
  if (!chain_params_ok(c)) return MSA_ERR_UNSUPPORTED;
  // (indexed as the call's arrays, from 0: the anchors below off[0] are not touched)
  std::vector<int32_t> f_own(f_out ? 0 : (size_t)hi), pred_own(pred_out ? 0 : (size_t)hi);
  int32_t* f = f_out ? f_out : f_own.data();
  int32_t* pred = pred_out ? pred_out : pred_own.data();
  int rc;
  if (n_max <= 1) {  // nothing to chain: no device call
    for (int64_t t = lo; t < hi; ++t) f[t] = (int32_t)(c.match * len[t]), pred[t] = -1;
  } else {
    if ((rc = ensure_device()) != MSA_OK) return rc;
    int64_t binfo[5];
    admission().info(current_device(), binfo);
    const size_t quarter = (size_t)binfo[0] / 4;
    for (int64_t p0 = 0, p1; p0 < np; p0 = p1) {
      p1 = p0 + 1;
      while (p1 < np && p1 - p0 < (int64_t(1) << 20) && footprint_chain(off[p1 + 1] - off[p0], p1 + 1 - p0) <= quarter)
        ++p1;
      if ((rc = chain_range(c, a, b, len, off, p0, p1, f, pred)) != MSA_OK) return rc;
    }
  }
  for (int64_t p = 0; p < np; ++p) {
    rc = chain_extract(f + off[p], pred + off[p], off[p + 1] - off[p], min_score, chain_of + off[p],
                       chain_score ? chain_score + off[p] : nullptr);
    if (rc < 0) return rc;
    n_chains[p] = rc;
  }
  return MSA_OK;
}

}  // namespace

extern "C" {

int msa_chain_seeds_batch(const int64_t* a, const int64_t* b, const int64_t* len, int64_t n_problems,
                          const int64_t* off, int32_t match, int32_t gap_open, int32_t gap_extend, int64_t band,
                          int64_t max_dist, int32_t lookback, int32_t min_score, int32_t* f, int32_t* pred,
                          int32_t* chain_of, int32_t* n_chains, int32_t* chain_score) {
  return chain_problems(a, b, len, n_problems, off, ChainParams{match, gap_open, gap_extend, band, max_dist, lookback},
                        min_score, f, pred, chain_of, n_chains, chain_score);
}

int msa_chain_seeds(const int64_t* a, const int64_t* b, const int64_t* len, int64_t n, int32_t match,
                    int32_t gap_open, int32_t gap_extend, int64_t band, int64_t max_dist, int32_t lookback,
                    int32_t min_score, int32_t* f, int32_t* pred, int32_t* chain_of, int32_t* n_chains,
                    int32_t* chain_score) {
  if (n < 0) return MSA_ERR_ARG;
  const int64_t off[2] = {0, n};
  // (no anchors: chain_of has nothing to hold and may be NULL)
  int32_t none = 0;
  return chain_problems(a, b, len, 1, off, ChainParams{match, gap_open, gap_extend, band, max_dist, lookback},
                        min_score, f, pred, n == 0 && !chain_of ? &none : chain_of, n_chains, chain_score);
}

}  // extern "C"

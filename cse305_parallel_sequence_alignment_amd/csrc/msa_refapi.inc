// msa_refapi.inc -- the reference's API as host-pointer entries of the C-ABI (included by msa_capi.hip after
// msa_devcall.inc): host arrays in, host arrays out, every DP cell on the GPU (line numbers: the reference's sources)
//     msa_subproblem                  subproblem_alignment.h:36-74, .cpp:329-355, :105-172
//     msa_main_alignment              main_alignment.cpp:353-410 (+ :11-22, :32-55)
//     msa_optimal_alignment           main_alignment.cpp:158-351
//     msa_main_alignment_partitioned  main_alignment.cpp:365,372 (the partition step it leaves commented out)
//     msa_non_parallel_tables         subproblem_alignment.cpp:401-421
//     msa_partial_tables              partial.cpp:13-79
//     msa_partial_partition           partial.cpp:81-163
//     msa_partition_tables            partial.cpp:128-145 over the caller's tables
//   (msa_rowapi.inc: msa_subproblem_f64, msa_subproblem_row)
// The host encodes the inputs, runs plans (stripe_kernel and the flow kernels behind msa_plan_run) and the device
// walk (traceback_kernel); the reference's own rules for what comes back -- find_alignment's nodes from a walk's
// O(m + n) ops or from tables, the stitching, the printed text, the partition's sort -- are msa_refwalk.h's.

namespace {

// Result of one single-pair fill.
struct OnePair {
  msa_pair_result res;
  std::vector<int32_t> meta;  // 12 per stripe
  int pmax = 0;
  int64_t S = 0;
  std::vector<int32_t> planes[3];
};

// Fill one pair of code arrays on the GPU and copy its cells back.  cells: NONE/H/TAB.
int run_one(int alg, int cells, const uint8_t* ca, int64_t m, const uint8_t* cb, int64_t n, int match, int mismatch,
            int gap_open, int gap_ext, int start_type, int band, int track_end, OnePair& out) {
  int rc = ensure_device();
  if (rc != MSA_OK) return rc;
  const int nplanes = (cells == MSA_CELLS_TAB) ? 3 : (cells == MSA_CELLS_NONE ? 0 : 1);
  const size_t esz = (cells == MSA_CELLS_DIR) ? 1 : 4;
  DeviceCall dc(footprint_planes(m, n, nplanes, (int)esz));
  if ((rc = dc.status()) != MSA_OK) return rc;
  void *dA = dc.alloc(m), *dB = dc.alloc(n), *c[3] = {nullptr, nullptr, nullptr};
  if (!dA || !dB) return MSA_ERR_NOMEM;
  if ((rc = dc.upload(dA, ca, m)) != MSA_OK || (rc = dc.upload(dB, cb, n)) != MSA_OK) return rc;
  SinglePairDesc sd(alg, cells, m, n);
  sd.d.match = match;
  sd.d.mismatch = mismatch;
  sd.d.gap_open = gap_open;
  sd.d.gap_extend = gap_ext;
  sd.d.start_type = start_type;
  sd.d.band = band;
  sd.d.track_end = track_end;
  msa_plan* P = nullptr;
  if ((rc = dc.create_plan(sd.d, nullptr, &P)) != MSA_OK) return rc;
  int64_t elems = 0;
  msa_plan_cells_size(P, &elems);
  for (int k = 0; k < nplanes; ++k)
    if (!(c[k] = dc.alloc((size_t)elems * esz))) return MSA_ERR_NOMEM;
  if ((rc = msa_plan_run(P, (const uint8_t*)dA, (const uint8_t*)dB, c[0], c[1], c[2], dc.stream())) != MSA_OK)
    return rc;
  if ((rc = msa_plan_results(P, &out.res, dc.stream())) != MSA_OK) return rc;
  out.S = msa_plan_stripes(P);
  out.meta.resize((size_t)out.S * 12);
  if ((rc = msa_plan_stripe_meta(P, out.meta.data(), out.S, dc.stream())) != MSA_OK) return rc;
  out.pmax = P->pairs[0].pmax;
  for (int k = 0; k < nplanes; ++k) {
    out.planes[k].resize((size_t)elems);
    if ((rc = dc.download(out.planes[k].data(), c[k], (size_t)elems * esz)) != MSA_OK) return rc;
  }
  return dc.sync();
}

// One reference-Gotoh fill (subproblem_alignment.cpp:329-355) and its
// find_alignment walk (:105-172), both on the GPU, one stream: direction bytes
// stay in HBM; only the walk's ops (<= m+n bytes) and the final state come back.
struct RefWalk {
  msa_pair_result res;
  std::vector<char> ops;  // end -> start: the table each step leaves ('M' T1, 'D' T2, 'I' T3)
  // (T1, T2, T3)(m, n) as the reference's doubles
  double fin(int v) const { return dinf(res.fin[v]); }
  // find_alignment's result: the end node by the reference's rule over the final state, the nodes from the ops
  int nodes(int64_t m, int64_t n, uint64_t idA, uint64_t idB, int end_type, double h, std::vector<msa_node>& path,
            msa_node& endn) const {
    const double f[3] = {fin(0), fin(1), fin(2)};
    endn = end_node_of(end_type, h, f, m, n, idA, idB);
    return nodes_from_ops(ops.data(), ops.size(), m, n, idA, idB, endn, path);
  }
};
int run_ref_walk(const uint8_t* ca, int64_t m, const uint8_t* cb, int64_t n, int gap_open, int gap_ext,
                 int start_type, int end_type, RefWalk& out) {
  int rc = ensure_device();
  if (rc != MSA_OK) return rc;
  DeviceCall dc(footprint_dir(m, n));
  if ((rc = dc.status()) != MSA_OK) return rc;
  void *dA = dc.alloc(m), *dB = dc.alloc(n);
  if (!dA || !dB) return MSA_ERR_NOMEM;
  if ((rc = dc.upload(dA, ca, m)) != MSA_OK || (rc = dc.upload(dB, cb, n)) != MSA_OK) return rc;
  SinglePairDesc sd(MSA_REF_GOTOH, MSA_CELLS_DIR, m, n);
  sd.d.match = 1;
  sd.d.mismatch = 0;
  sd.d.gap_open = gap_open;
  sd.d.gap_extend = gap_ext;
  sd.d.start_type = start_type;
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  msa_plan* P = nullptr;
  if ((rc = dc.cached_plan(PlanKey{dev, m, n, gap_open, gap_ext, start_type}, sd.d, &P)) != MSA_OK) return rc;
  int64_t elems = 0;
  msa_plan_cells_size(P, &elems);
  const int64_t cap = m + n + 2;
  void *dDir, *dOps, *dInfo;
  if (!(dDir = dc.alloc((size_t)elems)) || !(dOps = dc.alloc((size_t)cap)) || !(dInfo = dc.alloc(64)))
    return MSA_ERR_NOMEM;
  if ((rc = msa_plan_run(P, (const uint8_t*)dA, (const uint8_t*)dB, dDir, nullptr, nullptr, dc.stream()))) return rc;
  if ((rc = msa_plan_traceback_gotoh(P, 0, end_type, (const uint8_t*)dDir, (uint8_t*)dOps, cap, (int64_t*)dInfo,
                                     dc.stream())))
    return rc;
  int64_t info[8];
  if ((rc = dc.download(info, dInfo, sizeof(info))) != MSA_OK) return rc;
  if ((rc = msa_plan_results(P, &out.res, dc.stream())) != MSA_OK) return rc;  // (synchronizes the stream)
  if ((rc = dc.fetch_ops(info, dOps, out.ops)) != MSA_OK) return rc;
  dc.succeeded();
  return MSA_OK;
}

// Skewed-layout accessors (see msa_kernels.hip header).
inline size_t skew_idx(const OnePair& P, int64_t i, int64_t j) {
  const int64_t s = (i - 1) >> 6, r = (i - 1) & 63;
  const int64_t t = j - P.meta[(size_t)s * 12] + r;
  return (size_t)((((s * P.pmax * 4) + (t >> 2)) * 64 + r) * 4 + (t & 3));
}

// Rows 1..m of a fill's planes, from the stripe layout to row-major (m + 1) x (n + 1) tables (row 0 is the
// caller's border); a NULL table is skipped.
void deskew_rows(const OnePair& P, int64_t m, int64_t n, int32_t* const outs[3]) {
  for (int64_t i = 1; i <= m; ++i)
    for (int64_t j = 0; j <= n; ++j) {
      const size_t e = skew_idx(P, i, j);
      for (int v = 0; v < 3; ++v)
        if (outs[v]) outs[v][i * (n + 1) + j] = P.planes[v][e];
    }
}

// What an entry hands out: nodes (*n_out always, the nodes if asked for and they fit) and text (NUL-terminated;
// *text_len its length; text may be NULL to size it).
int hand_out_nodes(const std::vector<msa_node>& v, msa_node* out, size_t cap, size_t* n_out) {
  if (n_out) *n_out = v.size();
  if (!out) return MSA_OK;
  if (v.size() > cap) return MSA_ERR_CAPACITY;
  std::memcpy(out, v.data(), sizeof(msa_node) * v.size());
  return MSA_OK;
}
int hand_out_text(const std::string& s, char* text, size_t text_cap, size_t* text_len) {
  if (text_len) *text_len = s.size();
  if (!text) return MSA_OK;
  if (s.size() + 1 > text_cap) return MSA_ERR_CAPACITY;
  std::memcpy(text, s.c_str(), s.size() + 1);
  return MSA_OK;
}

// The double path: Subproblem tables by the GPU row sweep, then find_alignment.
// *fin receives (T1,T2,T3)(m',n').
int subproblem_path_f64(const char* A1, const char* B1, size_t m_in, size_t n_in, size_t idA_in, size_t idB_in,
                        int start_type, int end_type, double g, double h, std::vector<msa_node>& path, msa_node& endn,
                        double fin[3]) {
  const bool inv = m_in > n_in;
  const size_t m = inv ? n_in : m_in, n = inv ? m_in : n_in;
  std::vector<double> T[3];
  for (auto& t : T) t.resize((m + 1) * (n + 1));
  int invf = 0;
  int rc = msa_subproblem_f64(A1, B1, m_in, n_in, idA_in, idB_in, start_type, g, h, MSA_F64_COMPUTE_TABLES,
                              T[0].data(), T[1].data(), T[2].data(), &invf);
  if (rc != MSA_OK) return rc;
  for (int v = 0; v < 3; ++v) fin[v] = T[v][m * (n + 1) + n];
  // A, B, idA, idB as the Subproblem holds them after its swap; f (subproblem_alignment.h:83-88) on the characters
  const char *A = inv ? B1 : A1, *B = inv ? A1 : B1;
  const size_t idA = inv ? idB_in : idA_in, idB = inv ? idA_in : idB_in;
  return find_alignment(T[0].data(), T[1].data(), T[2].data(), (int64_t)m, (int64_t)n, idA, idB, end_type, g, h,
                        [&](int64_t i, int64_t j) { return A[idA + i] == B[idB + j]; }, path, endn);
}

}  // namespace

extern "C" {

int msa_subproblem(const char* A1, const char* B1, size_t m_in, size_t n_in, size_t idA_in, size_t idB_in,
                   int start_type, int end_type, double g, double h, int32_t* T1, int32_t* T2, int32_t* T3,
                   msa_node* nodes, size_t nodes_cap, size_t* n_nodes, msa_node* end_node, int* invert) {
  // m = n = 0 crashes the reference (compute_row: workers(n-1), subproblem_alignment.cpp:258)
  if (!A1 || !B1 || (m_in == 0 && n_in == 0)) return MSA_ERR_ARG;
  if (!exact_gh(g, h)) {
    // non-integral (or negative) g, h: int32 tables cannot hold them; the path comes
    // from the double row sweep (msa_subproblem_f64 gives the tables themselves)
    if (T1 || T2 || T3) return MSA_ERR_UNSUPPORTED;
    if (invert) *invert = m_in > n_in ? 1 : 0;
    if (!(nodes || n_nodes || end_node)) return MSA_OK;
    std::vector<msa_node> path;
    msa_node endn;
    double fin[3];
    const int r = subproblem_path_f64(A1, B1, m_in, n_in, idA_in, idB_in, start_type, end_type, g, h, path, endn,
                                      fin);
    if (r != MSA_OK) return r;
    if (end_node) *end_node = endn;
    return hand_out_nodes(path, nodes, nodes_cap, n_nodes);
  }
  int rc = MSA_OK;
  // constructor swap (subproblem_alignment.h:37-54)
  const bool inv = m_in > n_in;
  const char* A = inv ? B1 : A1;
  const char* B = inv ? A1 : B1;
  const int64_t m = inv ? n_in : m_in, n = inv ? m_in : n_in;
  const uint64_t idA = inv ? idB_in : idA_in, idB = inv ? idA_in : idB_in;
  if (invert) *invert = inv ? 1 : 0;
  if (m == 0) {
    // a one-row subproblem (partitions put points on the matrix edge): compute_tables
    // writes only the row-0 borders, find_alignment's loop never runs and
    // alignment_begin = NULL (subproblem_alignment.cpp:147-170): no path nodes.
    const int gi = (int)g, hi = (int)h;
    int32_t* outs[3] = {T1, T2, T3};
    double fin[3] = {0, 0, 0};
    for (int64_t c = 0; c <= n; ++c) {
      int32_t r0[3];
      ref_row0(start_type, gi, hi, c, r0);
      for (int v = 0; v < 3; ++v) {
        if (outs[v]) outs[v][c] = r0[v] == MSA_NEG ? INT32_MIN : r0[v];
        if (c == n) fin[v] = dinf(r0[v]);
      }
    }
    if (n_nodes) *n_nodes = 0;
    if (end_node) *end_node = end_node_of(end_type, h, fin, 0, n, idA, idB);
    return MSA_OK;
  }
  std::vector<uint8_t> ca(m), cb(n);
  if ((rc = msa_encode_pair(A + idA + 1, m, B + idB + 1, n, ca.data(), cb.data())) != MSA_OK) return rc;
  const int gi = (int)g, hi = (int)h;
  const bool want_tabs = T1 || T2 || T3;
  const bool want_path = nodes || n_nodes || end_node;
  OnePair P;
  RefWalk RW;
  if (want_tabs) {
    if ((rc = run_one(MSA_REF_GOTOH, MSA_CELLS_TAB, ca.data(), m, cb.data(), n, 1, 0, gi + hi, gi, start_type, -1, 0,
                      P)) != MSA_OK)
      return rc;
  } else if (want_path) {  // fill + walk on the device
    if ((rc = run_ref_walk(ca.data(), m, cb.data(), n, gi + hi, gi, start_type, end_type, RW)) != MSA_OK) return rc;
  } else {  // compute_tables alone: nothing comes back
    if ((rc = run_one(MSA_REF_GOTOH, MSA_CELLS_NONE, ca.data(), m, cb.data(), n, 1, 0, gi + hi, gi, start_type, -1, 0,
                      P)) != MSA_OK)
      return rc;
  }
  std::vector<int32_t> tabs[3];
  if (want_tabs) {
    const int64_t W = n + 1;
    for (int v = 0; v < 3; ++v) tabs[v].assign((size_t)((m + 1) * W), MSA_NEG);
    for (int64_t c = 0; c <= n; ++c) {
      int32_t r0[3];
      ref_row0(start_type, gi, hi, c, r0);
      for (int v = 0; v < 3; ++v) tabs[v][(size_t)c] = r0[v];
    }
    int32_t* const rows[3] = {tabs[0].data(), tabs[1].data(), tabs[2].data()};
    deskew_rows(P, m, n, rows);
    int32_t* outs[3] = {T1, T2, T3};
    for (int v = 0; v < 3; ++v)
      if (outs[v])
        for (size_t e = 0; e < tabs[v].size(); ++e) outs[v][e] = tabs[v][e] == MSA_NEG ? INT32_MIN : tabs[v][e];
  }
  if (want_path) {
    std::vector<msa_node> path;
    msa_node endn;
    if (want_tabs) {  // the caller asked for the tables anyway: walk them
      rc = find_alignment(tabs[0].data(), tabs[1].data(), tabs[2].data(), m, n, idA, idB, end_type, g, h,
                          [&](int64_t i, int64_t j) { return ca[i - 1] == cb[j - 1]; }, path, endn);
    } else {
      rc = RW.nodes(m, n, idA, idB, end_type, h, path, endn);
    }
    if (rc != MSA_OK) return rc;
    if (end_node) *end_node = endn;
    return hand_out_nodes(path, nodes, nodes_cap, n_nodes);
  }
  return MSA_OK;
}

int msa_main_alignment(const char* A1, const char* B1, size_t m, size_t n, size_t p, double g, double h, char* text,
                       size_t text_cap, size_t* text_len, double* score) {
  (void)p;  // only the reference's thread count (bit-identical results)
  if (!A1 || !B1 || m == 0 || n == 0) return MSA_ERR_ARG;
  int rc = MSA_OK;
  std::vector<msa_node> path;
  msa_node endn;
  // single subproblem [(0,0,-1),(m,n,1)]: start -1, end -1 (main_alignment.cpp:250-251)
  if (!exact_gh(g, h)) {
    double fin[3];
    if ((rc = subproblem_path_f64(A1, B1, m, n, 0, 0, -1, -1, g, h, path, endn, fin)) != MSA_OK) return rc;
    if (score) *score = std::max(std::max(fin[0], fin[1]), fin[2]);
  } else {
    const bool inv = m > n;
    const char* A = inv ? B1 : A1;
    const char* B = inv ? A1 : B1;
    const int64_t mm = inv ? n : m, nn = inv ? m : n;
    std::vector<uint8_t> ca(mm), cb(nn);
    if ((rc = msa_encode_pair(A + 1, mm, B + 1, nn, ca.data(), cb.data())) != MSA_OK) return rc;
    RefWalk RW;
    const int gi = (int)g, hi = (int)h;
    // fill + find_alignment's walk on the device; only the walk's ops come back
    if ((rc = run_ref_walk(ca.data(), mm, cb.data(), nn, gi + hi, gi, -1, -1, RW)) != MSA_OK) return rc;
    if ((rc = RW.nodes(mm, nn, 0, 0, -1, h, path, endn)) != MSA_OK) return rc;
    if (score) *score = std::max(std::max(RW.fin(0), RW.fin(1)), RW.fin(2));
  }
  return hand_out_text(alignment_text(1, path, A1, m, B1, n), text, text_cap, text_len);
}

// ---- optimal_alignment over a partition (main_alignment.cpp:158-351) -------

int msa_optimal_alignment(const char* A1, const char* B1, size_t m, size_t n, size_t p, double g, double h,
                          const msa_node* bp, size_t n_bp, int flags, char* text, size_t text_cap, size_t* text_len,
                          msa_node* path, size_t path_cap, size_t* n_path) {
  (void)p;  // the reference's processor budget (omega, ParallelPrefix, assign_processors :158-200)
            // only sizes its thread counts; results do not depend on it
  if (!A1 || !B1 || !bp || n_bp < 2) return MSA_ERR_ARG;  // workers(num-1) with num = 0 throws (:232)
  if (flags & ~MSA_OPT_FIX_ALL) return MSA_ERR_ARG;
  const size_t num = n_bp - 1;
  for (size_t k = 0; k < num; ++k) {
    // size_t lengths: a decreasing coordinate would wrap to ~2^64 in the reference
    if (bp[k + 1].i < bp[k].i || bp[k + 1].j < bp[k].j) return MSA_ERR_ARG;
    if (bp[k + 1].i > m || bp[k + 1].j > n) return MSA_ERR_ARG;
    if (bp[k + 1].i == bp[k].i && bp[k + 1].j == bp[k].j) return MSA_ERR_ARG;  // 0 x 0: crashes (:258)
  }
  const bool fix = (flags & MSA_OPT_FIX_ALL) != 0;
  const std::vector<size_t> order = solve_order(num, fix);
  std::vector<SubResult> sub(num);
  // independent subproblems run concurrently, each on its own pooled stream
  std::atomic<size_t> next{0};
  std::atomic<int> err{MSA_OK};
  auto worker = [&]() {
    for (;;) {
      const size_t q = next.fetch_add(1);
      if (q >= order.size() || err.load() != MSA_OK) return;
      const size_t k = order[q];
      const size_t lenA = bp[k + 1].i - bp[k].i, lenB = bp[k + 1].j - bp[k].j;
      SubResult& S = sub[k];
      S.nodes.resize(lenA + lenB + 2);
      size_t cnt = 0;
      int inv = 0;
      // OptimalAlignmentMapThread (:11-22): Subproblem(A, B, lenA, lenB, ida, idb, p', start, end, g, h)
      const int r = msa_subproblem(A1, B1, lenA, lenB, bp[k].i, bp[k].j, bp[k].t, -bp[k + 1].t, g, h, nullptr,
                                   nullptr, nullptr, S.nodes.data(), S.nodes.size(), &cnt, &S.endn, &inv);
      if (r != MSA_OK) {
        int expect = MSA_OK;
        err.compare_exchange_strong(expect, r);
        return;
      }
      S.nodes.resize(cnt);
      S.solved = true;
    }
  };
  const size_t nthreads = std::min<size_t>(8, order.size());
  std::vector<std::thread> pool;
  for (size_t t = 1; t < nthreads; ++t) pool.emplace_back(worker);
  worker();
  for (auto& t : pool) t.join();
  if (err.load() != MSA_OK) return err.load();
  const std::vector<msa_node> out = stitch(sub, fix);
  const int rc = hand_out_nodes(out, path, path_cap, n_path);
  if (rc != MSA_OK) return rc;
  return hand_out_text(alignment_text(order.size(), out, A1, m, B1, n), text, text_cap, text_len);
}

int msa_main_alignment_partitioned(const char* A1, const char* B1, size_t m, size_t n, size_t p, double g,
                                   double h, int flags, char* text, size_t text_cap, size_t* text_len) {
  if (!A1 || !B1 || m == 0 || n == 0 || p == 0) return MSA_ERR_ARG;
  std::vector<msa_node> part(p + 2);
  size_t np = 0;
  // findPartialBalancedPartitionParallel(A, B, m, n, p, g, h, -1, -1, pbp), the call the
  // reference leaves commented out (main_alignment.cpp:365,372); partial.cpp reads
  // A[i-1], so it gets the 0-based view A1+1 of the caller's 1-based buffers
  int rc = msa_partial_partition(A1 + 1, B1 + 1, m, n, p, g, h, -1, -1, part.data(), part.size(), &np);
  if (rc != MSA_OK) return rc;
  return msa_optimal_alignment(A1, B1, m, n, p, g, h, part.data(), np, flags, text, text_cap, text_len, nullptr, 0,
                               nullptr);
}

int msa_non_parallel_tables(const char* A1, const char* B1, size_t m, size_t n, size_t idA, size_t idB,
                            int start_type, int end_type, double g, double h, char* text, size_t text_cap,
                            size_t* text_len) {
  if (!A1 || !B1 || (m == 0 && n == 0)) return MSA_ERR_ARG;
  const size_t mm = std::min(m, n), nn = std::max(m, n);
  const size_t cells = (mm + 1) * (nn + 1);
  std::vector<double> T[3];
  for (auto& t : T) t.resize(cells);
  int rc;
  if (exact_gh(g, h)) {  // the int32 stripe kernel; INT32_MIN = -inf
    std::vector<int32_t> Ti[3];
    for (auto& t : Ti) t.resize(cells);
    rc = msa_subproblem(A1, B1, m, n, idA, idB, start_type, end_type, g, h, Ti[0].data(), Ti[1].data(),
                        Ti[2].data(), nullptr, 0, nullptr, nullptr, nullptr);
    if (rc != MSA_OK) return rc;
    for (int v = 0; v < 3; ++v)
      for (size_t e = 0; e < cells; ++e) T[v][e] = Ti[v][e] == INT32_MIN ? -INFINITY : (double)Ti[v][e];
  } else {  // any g, h: the double row sweep
    rc = msa_subproblem_f64(A1, B1, m, n, idA, idB, start_type, g, h, MSA_F64_NON_PARALLEL, T[0].data(),
                            T[1].data(), T[2].data(), nullptr);
    if (rc != MSA_OK) return rc;
  }
  // subproblem_alignment.cpp:401-421: "T1:" then each row as "%lf " per cell, newline
  std::string s;
  s.reserve(cells * 3 * 10 + 64);
  char num[400];  // "%lf" of any finite double fits (<= 317 chars)
  static const char* names[3] = {"T1:\n", "T2:\n", "T3:\n"};
  for (int v = 0; v < 3; ++v) {
    s += names[v];
    for (size_t i = 0; i <= mm; ++i) {
      for (size_t j = 0; j <= nn; ++j) {
        const int k = std::snprintf(num, sizeof(num), "%lf ", T[v][i * (nn + 1) + j]);
        s.append(num, (size_t)std::min(k, (int)sizeof(num) - 1));
      }
      s += '\n';
    }
  }
  return hand_out_text(s, text, text_cap, text_len);
}

int msa_partial_tables(const char* A0, const char* B0, size_t m_in, size_t n_in, double g, double h, int start_type,
                       int end_type, int32_t* T1, int32_t* T2, int32_t* T3, int32_t* R1, int32_t* R2, int32_t* R3) {
  if (!A0 || !B0 || m_in == 0 || n_in == 0) return MSA_ERR_ARG;
  const int64_t m = (int64_t)m_in, n = (int64_t)n_in;
  const int GH = (int)(g + h), G = (int)g;  // partial.cpp's (int) truncations
  std::vector<uint8_t> ca(m), cb(n), ra(m), rb(n);
  int rc = msa_encode_pair(A0, m, B0, n, ca.data(), cb.data());
  if (rc != MSA_OK) return rc;
  for (int64_t k = 0; k < m; ++k) ra[k] = ca[m - 1 - k];
  for (int64_t k = 0; k < n; ++k) rb[k] = cb[n - 1 - k];
  const int64_t WR = n + 2;
  if (T1 || T2 || T3) {
    OnePair F;
    if ((rc = run_one(MSA_PARTIAL, MSA_CELLS_TAB, ca.data(), m, cb.data(), n, 0, 1, GH, G, start_type, -1, 0, F)) !=
        MSA_OK)
      return rc;
    int32_t* outs[3] = {T1, T2, T3};
    for (int64_t c = 0; c <= n; ++c) {
      int32_t r0[3];
      part_row0(start_type, GH, c, r0);
      for (int v = 0; v < 3; ++v)
        if (outs[v]) outs[v][c] = r0[v];
    }
    deskew_rows(F, m, n, outs);
  }
  if (R1 || R2 || R3) {
    OnePair R;
    if ((rc = run_one(MSA_PARTIAL, MSA_CELLS_TAB, ra.data(), m, rb.data(), n, 0, 1, GH, G, end_type, -1, 0, R)) !=
        MSA_OK)
      return rc;
    int32_t* outs[3] = {R1, R2, R3};
    for (int v = 0; v < 3; ++v)
      if (outs[v])
        for (int64_t e = 0; e < (m + 2) * WR; ++e) outs[v][e] = INT32_MIN;
    // R[i][j] = R'[m+1-i][n+1-j]: R' row 0 = border, rows 1..m from the layout
    for (int64_t ip = 0; ip <= m; ++ip)
      for (int64_t jp = 0; jp <= n; ++jp) {
        int32_t val[3];
        if (ip == 0) {
          part_row0(end_type, GH, jp, val);
        } else {
          const size_t e = skew_idx(R, ip, jp);
          for (int v = 0; v < 3; ++v) val[v] = R.planes[v][e];
        }
        for (int v = 0; v < 3; ++v)
          if (outs[v]) outs[v][(m + 1 - ip) * WR + (n + 1 - jp)] = val[v];
      }
  }
  return MSA_OK;
}

int msa_partial_partition(const char* A0, const char* B0, size_t m_in, size_t n_in, size_t p, double g, double h,
                          int start_type, int end_type, msa_node* out, size_t cap, size_t* n_out) {
  if (!A0 || !B0 || m_in == 0 || n_in == 0 || p == 0) return MSA_ERR_ARG;
  int rc = ensure_device();
  if (rc != MSA_OK) return rc;
  const int64_t m = (int64_t)m_in, n = (int64_t)n_in;
  const int GH = (int)(g + h), G = (int)g, HH = (int)h;
  std::vector<uint8_t> ca(m), cb(n), ra(m), rb(n);
  if ((rc = msa_encode_pair(A0, m, B0, n, ca.data(), cb.data())) != MSA_OK) return rc;
  for (int64_t k = 0; k < m; ++k) ra[k] = ca[m - 1 - k];
  for (int64_t k = 0; k < n; ++k) rb[k] = cb[n - 1 - k];
  DeviceCall dc(2 * footprint_planes(m, n, 3, 4));  // forward + reverse tables
  if ((rc = dc.status()) != MSA_OK) return rc;
  void *dA, *dB, *dRA, *dRB, *F[3], *R[3];
  if (!(dA = dc.alloc(m)) || !(dB = dc.alloc(n)) || !(dRA = dc.alloc(m)) || !(dRB = dc.alloc(n)))
    return MSA_ERR_NOMEM;
  if ((rc = dc.upload(dA, ca.data(), m)) || (rc = dc.upload(dB, cb.data(), n)) ||
      (rc = dc.upload(dRA, ra.data(), m)) || (rc = dc.upload(dRB, rb.data(), n)))
    return rc;
  SinglePairDesc sd(MSA_PARTIAL, MSA_CELLS_TAB, m, n);
  sd.d.match = 0;
  sd.d.mismatch = 1;
  sd.d.gap_open = GH;
  sd.d.gap_extend = G;
  msa_plan *pf = nullptr, *pr = nullptr;
  sd.d.start_type = start_type;
  if ((rc = dc.create_plan(sd.d, nullptr, &pf)) != MSA_OK) return rc;
  sd.d.start_type = end_type;
  if ((rc = dc.create_plan(sd.d, nullptr, &pr)) != MSA_OK) return rc;
  int64_t elems = 0;
  msa_plan_cells_size(pf, &elems);
  for (int v = 0; v < 3; ++v)
    if (!(F[v] = dc.alloc((size_t)elems * 4)) || !(R[v] = dc.alloc((size_t)elems * 4))) return MSA_ERR_NOMEM;
  std::vector<unsigned long long> hk(2 * (p + 1));
  const size_t key_bytes = sizeof(unsigned long long) * hk.size();
  void* keys = dc.alloc(key_bytes);
  if (!keys) return MSA_ERR_NOMEM;
  if ((rc = dc.clear(keys, key_bytes)) != MSA_OK) return rc;
  if ((rc = msa_plan_run(pf, (const uint8_t*)dA, (const uint8_t*)dB, F[0], F[1], F[2], dc.stream()))) return rc;
  if ((rc = msa_plan_run(pr, (const uint8_t*)dRA, (const uint8_t*)dRB, R[0], R[1], R[2], dc.stream()))) return rc;
  if (p > 1) {
    const PartSkew tabs{(const int32_t*)F[0], (const int32_t*)F[1], (const int32_t*)F[2],
                        (const int32_t*)R[0], (const int32_t*)R[1], (const int32_t*)R[2],
                        pf->d_pairs, pr->d_pairs, pf->d_meta, pr->d_meta};
    hipLaunchKernelGGL(partition_kernel<PartSkew>, dim3(2048), dim3(256), 0, dc.stream(), tabs, (int)m, (int)n, (int)p,
                       HH, (unsigned long long*)keys);
    HIPCHK(hipGetLastError());
  }
  if ((rc = dc.download(hk.data(), keys, key_bytes)) != MSA_OK || (rc = dc.sync()) != MSA_OK) return rc;
  {
    int e1 = 0, e2 = 0;
    HIPCHK(hipMemcpy(&e1, pf->d_err, sizeof(e1), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&e2, pr->d_err, sizeof(e2), hipMemcpyDeviceToHost));
    if (e1 || e2) return MSA_ERR_TIMEOUT;
  }
  return hand_out_nodes(partition_from_keys(hk, m, n, p), out, cap, n_out);
}

int msa_partition_tables(const int32_t* T1, const int32_t* T2, const int32_t* T3, const int32_t* R1,
                         const int32_t* R2, const int32_t* R3, size_t m_in, size_t n_in, size_t p, double h,
                         msa_node* out, size_t cap, size_t* n_out) {
  if (!T1 || !T2 || !T3 || !R1 || !R2 || !R3 || p == 0) return MSA_ERR_ARG;
  if (m_in >= (1u << 30) || n_in >= (1u << 30)) return MSA_ERR_UNSUPPORTED;
  int rc = ensure_device();
  if (rc != MSA_OK) return rc;
  const int64_t m = (int64_t)m_in, n = (int64_t)n_in;
  const int HH = (int)h;
  std::vector<unsigned long long> hk(2 * (p + 1), 0ull);
  if (p > 1 && m > 0 && n > 0) {
    const size_t ef = (size_t)(m + 1) * (n + 1), er = (size_t)(m + 2) * (n + 2);
    DeviceCall dc(3 * 4 * (ef + er));
    if ((rc = dc.status()) != MSA_OK) return rc;
    void *F[3], *R[3];
    const int32_t* hf[3] = {T1, T2, T3};
    const int32_t* hr[3] = {R1, R2, R3};
    for (int v = 0; v < 3; ++v) {
      if (!(F[v] = dc.alloc(4 * ef)) || !(R[v] = dc.alloc(4 * er))) return MSA_ERR_NOMEM;
      if ((rc = dc.upload(F[v], hf[v], 4 * ef)) || (rc = dc.upload(R[v], hr[v], 4 * er))) return rc;
    }
    const size_t key_bytes = sizeof(unsigned long long) * hk.size();
    void* keys = dc.alloc(key_bytes);
    if (!keys) return MSA_ERR_NOMEM;
    if ((rc = dc.clear(keys, key_bytes)) != MSA_OK) return rc;
    const PartRowMajor tabs{(const int32_t*)F[0], (const int32_t*)F[1], (const int32_t*)F[2],
                            (const int32_t*)R[0], (const int32_t*)R[1], (const int32_t*)R[2]};
    hipLaunchKernelGGL(partition_kernel<PartRowMajor>, dim3(2048), dim3(256), 0, dc.stream(), tabs, (int)m, (int)n,
                       (int)p, HH, (unsigned long long*)keys);
    HIPCHK(hipGetLastError());
    if ((rc = dc.download(hk.data(), keys, key_bytes)) != MSA_OK || (rc = dc.sync()) != MSA_OK) return rc;
  }
  return hand_out_nodes(partition_from_keys(hk, m, n, p), out, cap, n_out);
}

}  // extern "C"

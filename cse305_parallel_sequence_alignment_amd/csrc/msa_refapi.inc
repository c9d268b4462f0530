// msa_refapi.inc -- the host-pointer entry points of the C-ABI (included by msa_capi.hip after the plan
// machinery): host arrays in, host arrays out, every DP cell and every walk on the GPU.
//
//   the reference's API (line numbers: the reference's sources)
//     msa_subproblem                  subproblem_alignment.h:36-74, .cpp:329-355, :105-172
//     msa_main_alignment              main_alignment.cpp:353-410 (+ :11-22, :32-55)
//     msa_optimal_alignment           main_alignment.cpp:158-351
//     msa_main_alignment_partitioned  main_alignment.cpp:365,372 (the partition step it leaves commented out)
//     msa_non_parallel_tables         subproblem_alignment.cpp:401-421
//     msa_partial_tables              partial.cpp:13-79
//     msa_partial_partition           partial.cpp:81-163
//     msa_partition_tables            partial.cpp:128-145 over the caller's tables
//   build extensions: an alignment with its CIGAR, one pair or a batch (align_pairs below)
//     msa_sw_align, msa_sw_align_batch                  Smith-Waterman
//     msa_nw_align, msa_nw_align_batch                  banded global alignment, +1 / 0
//     msa_nw_align_scored, msa_nw_align_batch_scored    ... under match / mismatch scores or an 8 x 8 matrix
//     msa_fit_align, msa_fit_align_batch                all of A in a substring of B
//   (msa_rowapi.inc: msa_subproblem_f64, msa_subproblem_row)
//
// The host encodes the inputs, runs plans (stripe_kernel and the flow / band kernels behind msa_plan_run) and the
// device walks (traceback_kernel, msa_plan_traceback_batch), and turns a walk's O(m + n) ops into the reference's
// align nodes or a CIGAR.

namespace {

using namespace msa_host;  // msa_hostutil.h: SymbolMap, cigar_of, complete_border, SinglePairDesc, ops_offsets


// Device footprint of one call, for admission control (Admit, msa_capi.hip), estimated from m and n
// before anything is allocated.  A two-pass flow plan with direction bytes holds the 1 B/cell plane
// ((m + 128)(n + 160) at R = 2), the pass-2 inputs BR (2 x 8 B per column of every 128-row stripe:
// ~m n / 8) and SNAP (3 x 128 x 8 B per 128-row x 128-column block: ~0.19 m n), and small buffers
// (16 code copies, pooled size classes round up by < 2 MiB each).  Stripe-kernel fills with int32
// planes: planes x 4 B per cell of the skewed layout plus ~0.1 B/cell of granules.
size_t footprint_dir(int64_t m, int64_t n) {
  return (size_t)(1.35 * (double)(m + 128) * (double)(n + 288)) + 16 * (size_t)(n + 512) + 2 * (size_t)(m + n) +
         (size_t(24) << 20);
}
size_t footprint_planes(int64_t m, int64_t n, int planes, int esz) {
  return (size_t)((planes * esz + 0.1) * (double)(m + 64) * (double)(n + 96)) + 16 * (size_t)(n + 512) +
         (size_t(16) << 20);
}

// Idle plans of the reference walk (run_ref_walk), by shape.  Creating a plan (pooled
// buffers, the host-side pass-2 block order, descriptor copies) measured 0.52 ms of a 1.94 ms
// main_alignment_function call at 10k.  A call takes a plan out of the cache (one caller per
// plan) and returns it after a successful run, once its stream has synchronized; at most
// kIdlePlans stay cached (the least recently returned is destroyed).
struct PlanKey {
  int dev;
  int64_t m, n;
  int go, ge, st;
  bool operator==(const PlanKey& o) const {
    return dev == o.dev && m == o.m && n == o.n && go == o.go && ge == o.ge && st == o.st;
  }
};
constexpr size_t kIdlePlans = 8;
std::mutex& plan_cache_mu() {
  static std::mutex mu;
  return mu;
}
std::deque<std::pair<PlanKey, msa_plan*>>& plan_cache() {
  static auto* q = new std::deque<std::pair<PlanKey, msa_plan*>>();  // never destroyed: no exit-order issue
  return *q;
}
struct CachedPlan {
  msa_plan* p = nullptr;
  PlanKey key{};
  bool ok = false;  // set on the success path only: a plan whose run failed is destroyed
  int acquire(const PlanKey& k, const msa_plan_desc& d) {
    key = k;
    {
      std::lock_guard<std::mutex> lk(plan_cache_mu());
      auto& q = plan_cache();
      for (auto it = q.begin(); it != q.end(); ++it)
        if (it->first == k) {
          p = it->second;
          q.erase(it);
          return MSA_OK;
        }
    }
    return msa_plan_create(&d, &p);
  }
  ~CachedPlan() {
    if (!p) return;
    if (!ok) {
      msa_plan_destroy(p);
      return;
    }
    // the caller's stream has synchronized (~DeviceCall's body runs first): nothing of this plan is in
    // flight, so an eviction must not wait on streams other callers may be using by then
    p->streams.clear();
    msa_plan* evict = nullptr;
    {
      std::lock_guard<std::mutex> lk(plan_cache_mu());
      auto& q = plan_cache();
      q.emplace_front(key, p);
      if (q.size() > kIdlePlans) {
        evict = q.back().second;
        q.pop_back();
      }
    }
    msa_plan_destroy(evict);
  }
};

// The device resources of one host-pointer call, constructed after ensure_device() succeeded: its reservation
// against the device budget (Admit; a footprint of 0 reserves nothing), a pooled non-blocking stream, pooled
// blocks, plans.  The one rule all of them are under: a block, or a plan with its blocks, goes back to its pool
// only after the stream that used it has been waited on, on every exit path, errors included -- or another thread
// is handed memory the stream still writes to.  The member order below is that rule.  The destructor's body
// waits for the stream; then the members go in reverse order: the cached plan returns to the plan cache (when the
// call marked success; it is destroyed otherwise), the plans are destroyed, the blocks and then the stream return
// to their pools, and the reservation, which covered all of them, is released last.
class DeviceCall {
 public:
  explicit DeviceCall(size_t footprint) {
    if (footprint) adm_.emplace(footprint);  // waits until the call fits the device budget
    stream_.s = stream_pool().get();
  }
  ~DeviceCall() {
    if (stream_.s) (void)hipStreamSynchronize(stream_.s);
  }
  DeviceCall(const DeviceCall&) = delete;
  DeviceCall& operator=(const DeviceCall&) = delete;

  int status() const { return stream_.s ? MSA_OK : MSA_ERR_HIP; }
  hipStream_t stream() const { return stream_.s; }
  // a pooled block; nullptr: MSA_ERR_NOMEM
  void* alloc(size_t bytes) {
    if (blocks_.n == kMaxBlocks) return nullptr;
    bytes = bytes ? bytes : 16;
    void* p = dev_pool().get(bytes);
    if (p) blocks_.v[blocks_.n++] = {p, bytes};
    return p;
  }
  // (stream-ordered: the host side of a download holds its bytes after the next sync())
  int upload(void* dst, const void* src, size_t bytes) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream_.s));
    return MSA_OK;
  }
  int download(void* dst, const void* src, size_t bytes) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream_.s));
    return MSA_OK;
  }
  int clear(void* dst, size_t bytes) {
    HIPCHK(hipMemsetAsync(dst, 0, bytes, stream_.s));
    return MSA_OK;
  }
  int sync() {
    HIPCHK(hipStreamSynchronize(stream_.s));
    return MSA_OK;
  }
  // a plan of this call's own (sub: msa_plan_create_scored's table, or nullptr), destroyed with the call
  // wide32: sub is a 32 x 32 table (msa_plan_create_scored32)
  int create_plan(const msa_plan_desc& d, const int8_t* sub, msa_plan** out, bool wide32 = false) {
    if (plans_.n == kMaxPlans) return MSA_ERR_NOMEM;
    const int rc = wide32 ? msa_plan_create_scored32(&d, sub, out) : msa_plan_create_scored(&d, sub, out);
    if (rc == MSA_OK) plans_.v[plans_.n++] = *out;
    return rc;
  }
  // the idle plan of this shape from the plan cache, or a new one; it goes (back) to the cache if succeeded()
  int cached_plan(const PlanKey& k, const msa_plan_desc& d, msa_plan** out) {
    const int rc = cached_.acquire(k, d);
    *out = cached_.p;
    return rc;
  }
  void succeeded() { cached_.ok = true; }
  // A device walk's ops (end -> start), once its info words {n_ops, i + 1, j + 1, status, ...} are on the host:
  // the walk's status if it failed, else info[0] bytes of d_ops (waits for them).
  int fetch_ops(const int64_t* info, const void* d_ops, std::vector<char>& ops) {
    if (info[3] != 0) return (int)info[3];
    ops.resize((size_t)info[0]);
    if (info[0] == 0) return MSA_OK;
    const int rc = download(ops.data(), d_ops, ops.size());
    return rc != MSA_OK ? rc : sync();
  }

 private:
  static constexpr int kMaxBlocks = 16, kMaxPlans = 2;
  struct Stream {
    hipStream_t s = nullptr;
    ~Stream() { stream_pool().put(s); }
  };
  struct Blocks {
    std::pair<void*, size_t> v[kMaxBlocks];
    int n = 0;
    ~Blocks() {
      for (int k = n; k-- > 0;) dev_pool().put(v[k].first, v[k].second);
    }
  };
  struct Plans {
    msa_plan* v[kMaxPlans];
    int n = 0;
    ~Plans() {
      for (int k = n; k-- > 0;) msa_plan_destroy(v[k]);
    }
  };
  std::optional<Admit> adm_;
  Stream stream_;
  Blocks blocks_;
  Plans plans_;
  CachedPlan cached_;
};

// DevPool's out-of-memory path: destroy the current device's idle cached plans (their blocks return to
// the pool, which then frees that device's cached blocks and retries the allocation; other devices'
// plans stay cached).
void drain_plan_cache() {
  std::vector<msa_plan*> victims;
  const int dev = current_device();
  {
    std::lock_guard<std::mutex> lk(plan_cache_mu());
    auto& q = plan_cache();
    for (auto it = q.begin(); it != q.end();) {
      if (it->first.dev == dev) {
        victims.push_back(it->second);
        it = q.erase(it);
      } else {
        ++it;
      }
    }
  }
  for (msa_plan* v : victims) msa_plan_destroy(v);
}

// Admission control's view of the memory held outside admitted calls (msa_capi.hip, Admission):
// the idle cached plans of device dev (their footprint estimate) and the pool's free blocks.
size_t idle_plan_bytes(int dev) {
  std::lock_guard<std::mutex> lk(plan_cache_mu());
  size_t b = 0;
  for (const auto& e : plan_cache())
    if (e.first.dev == dev) b += footprint_dir(e.first.m, e.first.n);
  return b;
}
size_t idle_device_bytes(int dev) { return idle_plan_bytes(dev) + dev_pool().cached(dev); }
void reclaim_idle_device_bytes(int dev) {
  int cur = 0;
  (void)hipGetDevice(&cur);
  if (cur != dev) (void)hipSetDevice(dev);
  drain_plan_cache();      // idle plans of this device -> their blocks back to the pool
  dev_pool().release(dev);  // -> freed
  if (cur != dev) (void)hipSetDevice(cur);
}
const bool g_reclaim_installed = (g_pool_reclaim = &drain_plan_cache, true);

bool integral_small(double x) { return std::isfinite(x) && std::floor(x) == x && std::fabs(x) < (double)(1 << 20); }

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

// Row 0 of the reference Gotoh tables (ComputeFirstRowMapThread, :212-227).
void ref_row0(int st, int g, int h, int64_t c, int32_t v[3]) {
  const int32_t NEG = MSA_NEG;
  if (c == 0) {
    v[0] = (st == 1 || st == -1) ? 0 : NEG;
    v[1] = (st == -2) ? 0 : NEG;
    v[2] = (st == -3) ? 0 : NEG;
  } else {
    v[0] = NEG;
    v[2] = NEG;
    v[1] = (st == -2) ? (int32_t)(-g * c) : ((st == 1 || st == 3) ? NEG : (int32_t)(-h - g * c));
  }
}

// Row 0 of partial.cpp's int tables (initializeTables, :13-31).
void part_row0(int st, int GH, int64_t c, int32_t v[3]) {
  v[0] = (c == 0 && st == 1) ? 0 : INT32_MIN;
  v[1] = (c >= 1 && st == 2) ? (int32_t)((uint32_t)(-GH) * (uint32_t)c) : INT32_MIN;
  v[2] = INT32_MIN;
}

inline double dinf(int32_t x) { return x == MSA_NEG ? -INFINITY : (double)x; }

// find_alignment's end node (subproblem_alignment.cpp:112-146) from the state
// fin = (T1,T2,T3)(m,n), MSA_NEG = -inf.
msa_node end_node_of(int end_type, double h, const int32_t fin[3], int64_t i, int64_t j, uint64_t idA,
                     uint64_t idB) {
  msa_node cur;
  cur.pad = 0;
  auto hprime = [&](int k) { return (k == end_type && end_type <= -2) ? h : 0.0; };
  if (end_type > 0) {
    cur.t = end_type;
    if (end_type == 1) { cur.i = i + idA; cur.j = j + idB; }
    else if (end_type == 2) { cur.i = 0; cur.j = j + idB; }
    else { cur.i = i + idA; cur.j = 0; }
  } else {
    const double t1 = dinf(fin[0]), t2 = dinf(fin[1]) + hprime(-2), t3 = dinf(fin[2]) + hprime(-3);
    if (t1 >= t2 && t1 >= t3) { cur.t = 1; cur.i = i + idA; cur.j = j + idB; }
    else if (t2 >= t1 && t2 >= t3) { cur.t = 2; cur.i = 0; cur.j = j + idB; }
    else { cur.t = 3; cur.i = i + idA; cur.j = 0; }
  }
  return cur;
}

// Subproblem::find_alignment (subproblem_alignment.cpp:105-172) from the device
// walk's ops (end -> start; op k = the table step k leaves from: 'M' T1, 'D' T2,
// 'I' T3) and the final state fin = (T1,T2,T3)(m,n).  The end node is rebuilt by
// the reference's end rule (:112-146) and must be the walk's first table; node k
// is created by step k-1 with t = the table step k leaves from, at the
// reference's coordinates (Q2 typo :151 kept); the node the last step would
// create is dropped (alignment_begin = curr_point->next, Q1 :170).
int nodes_from_ops(const std::vector<char>& ops, int64_t m, int64_t n, uint64_t idA, uint64_t idB, int end_type,
                   double h, const int32_t fin[3], std::vector<msa_node>& nodes, msa_node& endn) {
  msa_node cur = end_node_of(end_type, h, fin, m, n, idA, idB);
  endn = cur;
  auto tab = [](char c) { return c == 'M' ? 1 : (c == 'D' ? 2 : (c == 'I' ? 3 : 0)); };
  const size_t L = ops.size();
  if (L == 0 || tab(ops[0]) != cur.t) return MSA_ERR_NOMATCH;
  std::vector<msa_node> rev;
  rev.reserve(L);
  rev.push_back(cur);
  int64_t i = m, j = n;
  for (size_t k = 0; k < L; ++k) {
    if (i <= 0 || j <= 0) return MSA_ERR_NOMATCH;  // the walk went past find_alignment's stop
    const int ct = tab(ops[k]);
    if (!ct) return MSA_ERR_NOMATCH;
    const int nt = (k + 1 < L) ? tab(ops[k + 1]) : 0;  // 0: the dropped last node
    if (k + 1 < L && !nt) return MSA_ERR_NOMATCH;
    msa_node nw;
    nw.pad = 0;
    nw.t = nt;
    if (ct == 1) {
      if (nt == 1) { nw.i = i - 1 + idA; nw.j = j - 1 + idA; }  // Q2 (subproblem_alignment.cpp:151)
      else if (nt == 2) { nw.i = 0; nw.j = j - 1 + idB; }
      else { nw.i = i - 1 + idA; nw.j = 0; }
      i--; j--;
    } else if (ct == 2) {
      if (nt == 1) { nw.i = i + idA; nw.j = j - 1 + idB; }
      else if (nt == 2) { nw.i = 0; nw.j = j - 1 + idB; }
      else { nw.i = i + idA; nw.j = 0; }
      j--;
    } else {
      if (nt == 1) { nw.i = i - 1 + idA; nw.j = j + idB; }
      else if (nt == 2) { nw.i = 0; nw.j = j + idB; }
      else { nw.i = i - 1 + idA; nw.j = 0; }
      i--;
    }
    if (k + 1 < L) rev.push_back(nw);
  }
  if (i != 0 && j != 0) return MSA_ERR_NOMATCH;  // the walk stopped before the border
  nodes.assign(rev.rbegin(), rev.rend());
  return MSA_OK;
}

// Exact find_alignment over int32 tables (MSA_NEG = -inf) -- used when the
// caller asked for the tables anyway.
int walk_tables(const int32_t* T1, const int32_t* T2, const int32_t* T3, int64_t m, int64_t n, const uint8_t* ca,
                const uint8_t* cb, uint64_t idA, uint64_t idB, int end_type, int g, int h,
                std::vector<msa_node>& nodes, msa_node& endn) {
  const int64_t W = n + 1;
  auto at = [&](const int32_t* T, int64_t i, int64_t j) { return T[i * W + j]; };
  // x == c + y with -inf absorbing (double semantics of the reference)
  auto eqp = [](int32_t x, int64_t c, int32_t y) {
    if (y == MSA_NEG) return x == MSA_NEG;
    return x != MSA_NEG && (int64_t)x == c + y;
  };
  int32_t fin[3] = {at(T1, m, n), at(T2, m, n), at(T3, m, n)};
  int64_t i = m, j = n;
  msa_node cur = end_node_of(end_type, (double)h, fin, i, j, idA, idB);
  endn = cur;
  std::vector<msa_node> rev;
  rev.push_back(cur);
  int ct = cur.t;
  const int64_t GH = (int64_t)g + h;
  while (i > 0 && j > 0) {
    msa_node nw;
    nw.pad = 0;
    int nt = 0;
    if (ct == 1) {
      const int64_t f = (ca[i - 1] == cb[j - 1]) ? 1 : 0;
      const int32_t v = at(T1, i, j);
      if (eqp(v, f, at(T1, i - 1, j - 1))) { nt = 1; nw.i = i - 1 + idA; nw.j = j - 1 + idA; }
      else if (eqp(v, f, at(T2, i - 1, j - 1))) { nt = 2; nw.i = 0; nw.j = j - 1 + idB; }
      else if (eqp(v, f, at(T3, i - 1, j - 1))) { nt = 3; nw.i = i - 1 + idA; nw.j = 0; }
      i--; j--;
    } else if (ct == 2) {
      const int32_t v = at(T2, i, j);
      if (eqp(v, -GH, at(T1, i, j - 1))) { nt = 1; nw.i = i + idA; nw.j = j - 1 + idB; }
      else if (eqp(v, -(int64_t)g, at(T2, i, j - 1))) { nt = 2; nw.i = 0; nw.j = j - 1 + idB; }
      else if (eqp(v, -GH, at(T3, i, j - 1))) { nt = 3; nw.i = i + idA; nw.j = 0; }
      j--;
    } else {
      const int32_t v = at(T3, i, j);
      if (eqp(v, -GH, at(T1, i - 1, j))) { nt = 1; nw.i = i - 1 + idA; nw.j = j + idB; }
      else if (eqp(v, -GH, at(T2, i - 1, j))) { nt = 2; nw.i = 0; nw.j = j + idB; }
      else if (eqp(v, -(int64_t)g, at(T3, i - 1, j))) { nt = 3; nw.i = i - 1 + idA; nw.j = 0; }
      i--;
    }
    if (!nt) return MSA_ERR_NOMATCH;
    nw.t = nt;
    ct = nt;
    rev.push_back(nw);
  }
  nodes.clear();
  for (size_t k = rev.size() - 1; k-- > 0;) nodes.push_back(rev[k]);
  return MSA_OK;
}

// find_alignment (subproblem_alignment.cpp:105-172) over the reference's double
// tables, with its exact double expressions (f + T, -g - h + T, -g + T) -- the
// traceback of the double row sweep (msa_subproblem_f64) for non-integral g, h.
// A, B, idA, idB as the Subproblem holds them after its swap.
int walk_f64(const double* T1, const double* T2, const double* T3, int64_t m, int64_t n, const char* A, const char* B,
             uint64_t idA, uint64_t idB, int end_type, double g, double h, std::vector<msa_node>& nodes,
             msa_node& endn) {
  const int64_t W = n + 1;
  auto at = [&](const double* T, int64_t i, int64_t j) { return T[i * W + j]; };
  auto hprime = [&](int k) { return (k == end_type && end_type <= -2) ? h : 0.0; };
  int64_t i = m, j = n;
  msa_node cur;
  cur.pad = 0;
  if (end_type > 0) {
    cur.t = end_type;
    if (end_type == 1) { cur.i = i + idA; cur.j = j + idB; }
    else if (end_type == 2) { cur.i = 0; cur.j = j + idB; }
    else { cur.i = i + idA; cur.j = 0; }
  } else {
    const double t1 = at(T1, m, n), t2 = at(T2, m, n) + hprime(-2), t3 = at(T3, m, n) + hprime(-3);
    if (t1 >= t2 && t1 >= t3) { cur.t = 1; cur.i = i + idA; cur.j = j + idB; }
    else if (t2 >= t1 && t2 >= t3) { cur.t = 2; cur.i = 0; cur.j = j + idB; }
    else { cur.t = 3; cur.i = i + idA; cur.j = 0; }
  }
  endn = cur;
  std::vector<msa_node> rev;
  rev.push_back(cur);
  int ct = cur.t;
  while (i > 0 && j > 0) {
    msa_node nw;
    nw.pad = 0;
    int nt = 0;
    if (ct == 1) {
      const double f = (A[idA + i] == B[idB + j]) ? 1.0 : 0.0;
      const double v = at(T1, i, j);
      if (v == f + at(T1, i - 1, j - 1)) { nt = 1; nw.i = i - 1 + idA; nw.j = j - 1 + idA; }  // Q2 (:151)
      else if (v == f + at(T2, i - 1, j - 1)) { nt = 2; nw.i = 0; nw.j = j - 1 + idB; }
      else if (v == f + at(T3, i - 1, j - 1)) { nt = 3; nw.i = i - 1 + idA; nw.j = 0; }
      i--; j--;
    } else if (ct == 2) {
      const double v = at(T2, i, j);
      if (v == -g - h + at(T1, i, j - 1)) { nt = 1; nw.i = i + idA; nw.j = j - 1 + idB; }
      else if (v == -g + at(T2, i, j - 1)) { nt = 2; nw.i = 0; nw.j = j - 1 + idB; }
      else if (v == -g - h + at(T3, i, j - 1)) { nt = 3; nw.i = i + idA; nw.j = 0; }
      j--;
    } else {
      const double v = at(T3, i, j);
      if (v == -g - h + at(T1, i - 1, j)) { nt = 1; nw.i = i - 1 + idA; nw.j = j + idB; }
      else if (v == -g - h + at(T2, i - 1, j)) { nt = 2; nw.i = 0; nw.j = j + idB; }
      else if (v == -g + at(T3, i - 1, j)) { nt = 3; nw.i = i - 1 + idA; nw.j = 0; }
      i--;
    }
    // the reference would loop forever on an uninitialised node here (:147-169)
    if (!nt) return MSA_ERR_NOMATCH;
    nw.t = nt;
    ct = nt;
    rev.push_back(nw);
  }
  nodes.clear();
  for (size_t k = rev.size() - 1; k-- > 0;) nodes.push_back(rev[k]);
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
  return walk_f64(T[0].data(), T[1].data(), T[2].data(), (int64_t)m, (int64_t)n, inv ? B1 : A1, inv ? A1 : B1,
                  inv ? idB_in : idA_in, inv ? idA_in : idB_in, end_type, g, h, path, endn);
}

bool exact_gh(double g, double h) {
  return integral_small(g) && integral_small(h) && g >= 0 && g + h >= 0;
}

int check_gh(double g, double h) {
  if (!integral_small(g) || !integral_small(h)) return MSA_ERR_UNSUPPORTED;
  if (g < 0 || g + h < 0) return MSA_ERR_UNSUPPORTED;
  return MSA_OK;
}

}  // namespace

namespace {

// One solved subproblem: its node list (alignment_begin .. alignment_end,
// possibly empty: alignment_begin = NULL) and its alignment_end node.
struct SubResult {
  bool solved = false;
  std::vector<msa_node> nodes;
  msa_node endn{};
};

// Which subproblems optimal_alignment solves, in its order (main_alignment.cpp:232-341):
// round r = 0, 1, 2 takes r, r+3, ... while i < num-3 (threads) and then one more
// at the first i past that, if i < num.  Rounds 1 and 2 run only when num > 3, so
// with 2 or 3 subproblems only subproblem 0 is solved.  fix: every subproblem.
std::vector<size_t> solve_order(size_t num, bool fix) {
  std::vector<size_t> order;
  if (fix) {
    for (size_t k = 0; k < num; ++k) order.push_back(k);
    return order;
  }
  const bool num_sub_3 = num > 3;
  for (size_t r = 0; r < 3; ++r) {
    if (r > 0 && !num_sub_3) break;
    size_t i = r;
    while (num_sub_3 && i < num - 3) {
      order.push_back(i);
      i += 3;
    }
    if (i < num) order.push_back(i);
  }
  return order;
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
    if (n_nodes) *n_nodes = path.size();
    if (end_node) *end_node = endn;
    if (nodes) {
      if (path.size() > nodes_cap) return MSA_ERR_CAPACITY;
      std::memcpy(nodes, path.data(), sizeof(msa_node) * path.size());
    }
    return MSA_OK;
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
    int32_t fin[3] = {0, 0, 0};
    for (int64_t c = 0; c <= n; ++c) {
      int32_t r0[3];
      ref_row0(start_type, gi, hi, c, r0);
      for (int v = 0; v < 3; ++v) {
        if (outs[v]) outs[v][c] = r0[v] == MSA_NEG ? INT32_MIN : r0[v];
        if (c == n) fin[v] = r0[v];
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
    for (int64_t i = 1; i <= m; ++i)
      for (int64_t j = 0; j <= n; ++j) {
        const size_t e = skew_idx(P, i, j);
        for (int v = 0; v < 3; ++v) tabs[v][(size_t)(i * W + j)] = P.planes[v][e];
      }
    int32_t* outs[3] = {T1, T2, T3};
    for (int v = 0; v < 3; ++v)
      if (outs[v])
        for (size_t e = 0; e < tabs[v].size(); ++e) outs[v][e] = tabs[v][e] == MSA_NEG ? INT32_MIN : tabs[v][e];
  }
  if (want_path) {
    std::vector<msa_node> path;
    msa_node endn;
    if (want_tabs) {
      rc = walk_tables(tabs[0].data(), tabs[1].data(), tabs[2].data(), m, n, ca.data(), cb.data(), idA, idB,
                       end_type, gi, hi, path, endn);
    } else {
      rc = nodes_from_ops(RW.ops, m, n, idA, idB, end_type, h, RW.res.fin, path, endn);
    }
    if (rc != MSA_OK) return rc;
    if (n_nodes) *n_nodes = path.size();
    if (end_node) *end_node = endn;
    if (nodes) {
      if (path.size() > nodes_cap) return MSA_ERR_CAPACITY;
      std::memcpy(nodes, path.data(), sizeof(msa_node) * path.size());
    }
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
    if ((rc = nodes_from_ops(RW.ops, mm, nn, 0, 0, -1, h, RW.res.fin, path, endn)) != MSA_OK) return rc;
    if (score) *score = std::max(std::max(dinf(RW.res.fin[0]), dinf(RW.res.fin[1])), dinf(RW.res.fin[2]));
  }
  static const char hdr[] = "bp1\nbp1.2\nbp2\nbp3\nbp4\n";
  const size_t L = path.size();
  const size_t need = sizeof(hdr) - 1 + 2 * (L + 1) + 1;
  if (text_len) *text_len = need - 1;
  if (!text) return MSA_OK;
  if (need > text_cap) return MSA_ERR_CAPACITY;
  size_t o = 0;
  std::memcpy(text, hdr, sizeof(hdr) - 1);
  o += sizeof(hdr) - 1;
  // print_seq (main_alignment.cpp:32-55) on the UNSWAPPED arrays (quirk Q3);
  // indices past the caller's buffers print '?' (the reference reads out of bounds)
  for (size_t k = 0; k < L; ++k)
    text[o++] = (path[k].t == 1 || path[k].t == 3) ? (path[k].i <= m ? A1[path[k].i] : '?') : '-';
  text[o++] = '\n';
  for (size_t k = 0; k < L; ++k)
    text[o++] = (path[k].t == 1 || path[k].t == 2) ? (path[k].j <= n ? B1[path[k].j] : '?') : '-';
  text[o++] = '\n';
  text[o] = 0;
  return MSA_OK;
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
  // concatenate (:344-348): end of subproblem i-1 -> begin of subproblem i for
  // i = 1 .. num-2; the link into the last subproblem is never made (fix: made)
  std::vector<msa_node> out;
  const size_t last_link = fix ? num - 1 : (num >= 2 ? num - 2 : 0);
  for (size_t k = 0; k < num; ++k) {
    if (!sub[k].solved || sub[k].nodes.empty()) break;  // alignment_begin == NULL ends the walk
    out.insert(out.end(), sub[k].nodes.begin(), sub[k].nodes.end());
    if (k + 1 > last_link || k + 1 >= num) break;  // the end node's next stays NULL
  }
  if (n_path) *n_path = out.size();
  if (path) {
    if (out.size() > path_cap) return MSA_ERR_CAPACITY;
    std::memcpy(path, out.data(), sizeof(msa_node) * out.size());
  }
  // stdout: bp1..bp4 per solved subproblem (in solve order; the reference's threads
  // interleave these lines), then print_seq (:32-55) of the stitched list
  static const char hdr[] = "bp1\nbp1.2\nbp2\nbp3\nbp4\n";
  const size_t L = out.size();
  const size_t need = (sizeof(hdr) - 1) * order.size() + 2 * (L + 1) + 1;
  if (text_len) *text_len = need - 1;
  if (!text) return MSA_OK;
  if (need > text_cap) return MSA_ERR_CAPACITY;
  size_t o = 0;
  for (size_t k = 0; k < order.size(); ++k) {
    std::memcpy(text + o, hdr, sizeof(hdr) - 1);
    o += sizeof(hdr) - 1;
  }
  for (size_t k = 0; k < L; ++k)
    text[o++] = (out[k].t == 1 || out[k].t == 3) ? (out[k].i <= m ? A1[out[k].i] : '?') : '-';
  text[o++] = '\n';
  for (size_t k = 0; k < L; ++k)
    text[o++] = (out[k].t == 1 || out[k].t == 2) ? (out[k].j <= n ? B1[out[k].j] : '?') : '-';
  text[o++] = '\n';
  text[o] = 0;
  return MSA_OK;
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
  if (text_len) *text_len = s.size();
  if (!text) return MSA_OK;
  if (s.size() + 1 > text_cap) return MSA_ERR_CAPACITY;
  std::memcpy(text, s.c_str(), s.size() + 1);
  return MSA_OK;
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
  const int64_t W = n + 1, WR = n + 2;
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
    for (int64_t i = 1; i <= m; ++i)
      for (int64_t j = 0; j <= n; ++j) {
        const size_t e = skew_idx(F, i, j);
        for (int v = 0; v < 3; ++v)
          if (outs[v]) outs[v][i * W + j] = F.planes[v][e];
      }
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

// findPartitionParallel's tail (partial.cpp:128-145) from the band winners partition_kernel
// reduced: per k the row band's or the column band's best cell, then (0,0,-1), (m,n,1) and
// the reference's std::sort.
static int partition_from_keys(const std::vector<unsigned long long>& hk, int64_t m, int64_t n, size_t p, msa_node* out,
                               size_t cap, size_t* n_out) {
  const int64_t bm = m / (int64_t)p, bn = n / (int64_t)p;
  std::vector<msa_node> part;
  part.push_back(msa_node{0, 0, -1, 0});
  for (size_t k = 1; k < p; ++k) {
    // decode a band winner; key 0 = no cell beat INT_MIN -> {0,0,0}
    auto decode = [&](unsigned long long key, bool row, int32_t& val, msa_node& nd) {
      nd = msa_node{0, 0, 0, 0};
      val = INT32_MIN;
      if (!key) return;
      val = (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u);
      const int64_t idx = (int64_t)((~(uint32_t)((key >> 2) & 0x3fffffffu)) & 0x3fffffffu);
      nd.t = (int32_t)(key & 3u);
      if (row) { nd.i = (uint64_t)(k * bm + idx / n); nd.j = (uint64_t)(1 + idx % n); }
      else { nd.j = (uint64_t)(k * bn + idx / m); nd.i = (uint64_t)(1 + idx % m); }
    };
    int32_t vr, vc;
    msa_node br, bc;
    decode(hk[2 * k], true, vr, br);
    decode(hk[2 * k + 1], false, vc, bc);
    part.push_back(vr > vc ? br : bc);  // partial.cpp:131-135: ties go to the column
  }
  part.push_back(msa_node{(uint64_t)m, (uint64_t)n, 1, 0});
  // partial.cpp:141-143: std::sort with the reference's comparator.  Past 16 elements
  // std::sort (introsort) is not stable, so points that tie on (i, j) -- the (0,0,0) of a
  // band with no cell above INT_MIN when p > m or p > n -- land where libstdc++'s introsort
  // puts them; the same header algorithm on the same sequence of comparisons reproduces the
  // reference's order (tests/golden/partial_ties.json, made by the reference's build).
  std::sort(part.begin(), part.end(), [](const msa_node& a, const msa_node& b) {
    return (a.i < b.i) || (a.i == b.i && a.j < b.j);
  });
  if (n_out) *n_out = part.size();
  if (out) {
    if (part.size() > cap) return MSA_ERR_CAPACITY;
    std::memcpy(out, part.data(), sizeof(msa_node) * part.size());
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
  return partition_from_keys(hk, m, n, p, out, cap, n_out);
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
  return partition_from_keys(hk, m, n, p, out, cap, n_out);
}

}  // extern "C"

// ---- alignments with their CIGARs: one pair (msa_*_align) or a batch (msa_*_align_batch) ----------------------
namespace {

// Device footprint of one global alignment (footprint_dir / footprint_planes above are a local one's): the plan's
// cells (1 B per cell of the skewed band layout -- the stripes' own phase counts, as lay_out_pairs sizes them -- or
// none for a score-only call), its granule slots (two
// per item of 4 stripes, n + margins granules each; a chunked band plan has up to (warm-up + chunk) / 4 + 1 items
// per chunk), the 16 code copies, the ops and the pooled size classes' slack.  A banded pair therefore reserves
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
};

// Smith-Waterman: code 7 is the kernels' out-of-matrix sentinel, so 7 codes
AlignSpec spec_sw(int match, int mismatch, const char* preset) {
  return AlignSpec{MSA_OK, MSA_SW_AFFINE, MSA_SW_AFFINE, match, mismatch, 0, 1, false, {}, SymbolMap(7, preset),
                   GAPS_LOCAL, false, FOOT_MATRIX, msa_plan_traceback, BORDER_NONE, true};
}
// Smith-Waterman under the caller's alphabet -- a symbol's code is its index -- and its n_sym x n_sym matrix
// (MSA_SW_SCORED).  The highest code is the sentinel's, so max_sym is 7, or 31 (the *32 entries); up to 7 symbols make
// the same spec under either, 8..31 a wide one.  status MSA_ERR_ARG as for spec_scored
AlignSpec spec_sw_scored(const char* alphabet, size_t n_sym, const int8_t* sub, size_t max_sym) {
  AlignSpec s = spec_sw(0, 0, "");
  s.alg_walk = s.alg_score = MSA_SW_SCORED;
  s.scored = true;
  if (!alphabet || !sub || n_sym < 1 || n_sym > max_sym) s.status = MSA_ERR_ARG;
  s.wide = s.status == MSA_OK && n_sym > 7;
  if (s.wide) s.symbols = SymbolMap(31);
  const size_t stride = s.wide ? 32 : 8;
  for (size_t a = 0; s.status == MSA_OK && a < n_sym; ++a) {
    if (!s.symbols.add(alphabet[a])) s.status = MSA_ERR_ARG;
    for (size_t b = 0; b < n_sym; ++b) s.tab[stride * a + b] = sub[n_sym * a + b];
  }
  s.symbols.fix();
  return s;
}
// global, +1 / 0 over the call's own symbols
AlignSpec spec_nw(const char* preset) {
  return AlignSpec{MSA_OK, MSA_NW_ALIGN, MSA_NW_BANDED, 1, 0, -1, 0, false, {}, SymbolMap(8, preset),
                   GAPS_GLOBAL, true, FOOT_BAND, msa_plan_traceback_nw, BORDER_GLOBAL, false};
}
// global under the caller's alphabet -- a symbol's code is its index -- and its n_sym x n_sym matrix;
// status MSA_ERR_ARG for a NULL alphabet or matrix, n_sym outside 1..max_sym or a duplicate symbol.  max_sym: 8, or 32
// (the *32 entries); up to 8 symbols make the same spec under either, 9..32 a wide one
AlignSpec spec_scored(const char* alphabet, size_t n_sym, const int8_t* sub, size_t max_sym = 8) {
  AlignSpec s = spec_nw("");
  s.alg_walk = s.alg_score = MSA_NW_SCORED;
  s.scored = true;
  if (!alphabet || !sub || n_sym < 1 || n_sym > max_sym) s.status = MSA_ERR_ARG;
  s.wide = s.status == MSA_OK && n_sym > 8;
  if (s.wide) s.symbols = SymbolMap(32);
  const size_t stride = s.wide ? 32 : 8;
  for (size_t a = 0; s.status == MSA_OK && a < n_sym; ++a) {
    if (!s.symbols.add(alphabet[a])) s.status = MSA_ERR_ARG;
    for (size_t b = 0; b < n_sym; ++b) s.tab[stride * a + b] = sub[n_sym * a + b];
  }
  s.symbols.fix();
  return s;
}
// ... and with free ends on B: all of A in a substring of B
AlignSpec spec_fit(const char* alphabet, size_t n_sym, const int8_t* sub, size_t max_sym = 8) {
  AlignSpec s = spec_scored(alphabet, n_sym, sub, max_sym);
  s.alg_walk = s.alg_score = MSA_NW_FIT;
  s.banded = false;
  s.border = BORDER_FIT;
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
  PairOut end, beg;  // local: the end cell, the start cell
  PairOut span;      // fit: {beg_j, end_j}, beg_j = -1 without a walk
  char* cigars;      // the CIGARs back to back, each with its NUL; cigar_off[np + 1]
  size_t cigar_cap;
  int64_t* cigar_off;
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
  void *dA = dc.alloc((size_t)(a_hi - a_lo)), *dB = dc.alloc((size_t)(b_hi - b_lo));
  if (!dA || !dB) return MSA_ERR_NOMEM;
  if ((rc = dc.upload(dA, ca + a_lo, (size_t)(a_hi - a_lo))) || (rc = dc.upload(dB, cb + b_lo, (size_t)(b_hi - b_lo))))
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
  if ((rc = dc.create_plan(d, spec.scored ? spec.tab : nullptr, &P, spec.wide)) != MSA_OK) return rc;
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
    out.end.put(p0 + k, res[(size_t)k].end_i, res[(size_t)k].end_j);
    out.span.put(p0 + k, -1, res[(size_t)k].end_j);
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
    if (out.cigars) {
      out.cigar_off[p0 + k] = (int64_t)all.size();
      all += cigar_of(o.data(), o.size());
      all.push_back('\0');
    }
  }
  return MSA_OK;
}

const int64_t kPairLimit = int64_t(1) << 26;  // rows / columns of a pair (msa_sw_align has no limit of its own)

// Every alignment entry: check the arguments (MSA_ERR_ARG; size_lim bounds m and n), the gap rule
// (MSA_ERR_UNSUPPORTED), the band against the lengths (MSA_ERR_ARG), encode with one symbol map for the call, A
// then B (MSA_ERR_ALPHABET), and only then ask for the device; then align_range chunk by chunk -- consecutive pairs
// whose summed single-pair footprints fit a quarter of the device budget, at most 2^20 of them -- and hand out the
// CIGARs.
int align_pairs(AlignSpec spec, int single, const AlignIn& in, int64_t size_lim, int32_t gap_open,
                int32_t gap_extend, int64_t band_in, const AlignOut& out) {
  if (spec.status != MSA_OK) return spec.status;
  if (!in.A || !in.B || !in.a_off || !in.m || !in.b_off || !in.n || in.np < 1 || (out.cigars && !out.cigar_off) ||
      band_in < -1)
    return MSA_ERR_ARG;
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
  if (!spec.banded) band_in = -1;
  if (band_in >= 0)
    for (int64_t p = 0; p < in.np; ++p)
      if (std::llabs(in.m[p] - in.n[p]) > band_in) return MSA_ERR_ARG;
  // (a band that holds every cell of every pair is no band)
  const GapBand gb{gap_open, gap_extend, (band_in < 0 || band_in >= span_max) ? -1 : (int)band_in};
  std::vector<uint8_t> ca(in.a_len), cb(in.b_len);
  int rc = spec.symbols.encode(in.A, in.a_len, ca.data());
  if (rc == MSA_OK) rc = spec.symbols.encode(in.B, in.b_len, cb.data());
  if (rc != MSA_OK) return rc;
  if ((rc = ensure_device()) != MSA_OK) return rc;
  const bool want_tb = out.cigars || (spec.walk_for_beg && (out.beg.i || out.beg.j));
  auto fp = [&](int64_t p) -> size_t {
    if (spec.footprint == FOOT_BAND) return footprint_nw(in.m[p], in.n[p], gb.band, want_tb);
    return want_tb ? footprint_dir(in.m[p], in.n[p]) : footprint_planes(in.m[p], in.n[p], 0, 1);
  };
  int64_t binfo[5];
  admission().info(current_device(), binfo);
  const size_t quarter = (size_t)binfo[0] / 4;
  std::string all;  // the CIGARs, back to back
  for (int64_t p0 = 0, p1; p0 < in.np; p0 = p1) {
    size_t bytes = fp(p0);
    p1 = p0 + 1;
    while (p1 < in.np && p1 - p0 < (int64_t(1) << 20) && bytes + fp(p1) <= quarter) bytes += fp(p1++);
    if ((rc = align_range(spec, single, gb, want_tb, ca.data(), cb.data(), in, p0, p1, bytes, out, all)) != MSA_OK)
      return rc;
  }
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

}  // extern "C"

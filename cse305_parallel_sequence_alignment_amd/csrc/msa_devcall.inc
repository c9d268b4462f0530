// msa_devcall.inc -- what every host-pointer entry of the C-ABI runs its device work through (included by
// msa_capi.hip after the plan machinery, before msa_refapi.inc, msa_rowapi.inc and msa_alignapi.inc): the device
// footprint estimates for admission control, the cache of idle reference-walk plans, DeviceCall, and the hooks
// that give idle device memory back.

namespace {

using namespace msa_host;  // msa_hostutil.h, msa_refwalk.h: the entries' pure host-side steps

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
  // ... scored by prof_rows rows of a profile (msa_plan_create_profile)
  int create_profile_plan(const msa_plan_desc& d, const int8_t* prof, int64_t prof_rows, msa_plan** out) {
    if (plans_.n == kMaxPlans) return MSA_ERR_NOMEM;
    const int rc = msa_plan_create_profile(&d, prof, prof_rows, out);
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

}  // namespace

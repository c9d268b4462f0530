// msa_capi.hip -- host side of the C-ABI (include/msa.h): plans, launches,
// and the reference-compatible entry points.  All DP cells are computed by the
// kernels in msa_kernels.hip; the host only encodes inputs, de-skews outputs
// and walks traceback bits (O(m+n), like the reference's find_alignment).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <condition_variable>
#include <mutex>
#include <new>
#include <optional>
#include <string>
#include <thread>
#include <deque>
#include <climits>
#include <map>
#include <memory>
#include <tuple>
#include <vector>

#include "../../include/msa.h"
#include "msa_hostutil.h"
#include "msa_refwalk.h"
#include "msa_kernels.hip"
#include "msa_flow.hip"
#include "msa_cflow.hip"
#include "msa_band.hip"
#include "msa_rowsweep.hip"
#include "msa_traceback.hip"
#include "msa_tbatch.hip"
#include "msa_xdrop.hip"
#include "msa_chain.hip"

using namespace msa;

namespace {

#define HIPCHK(x)                                         \
  do {                                                    \
    hipError_t e_ = (x);                                  \
    if (e_ != hipSuccess) {                               \
      std::fprintf(stderr, "msa: %s failed: %s\n", #x, hipGetErrorString(e_)); \
      return MSA_ERR_HIP;                                 \
    }                                                     \
  } while (0)

int g_dev_checked = 0;
int g_dev_ok = 0;
std::mutex g_dev_mu;

int ensure_device() {
  std::lock_guard<std::mutex> lk(g_dev_mu);
  if (!g_dev_checked) {
    g_dev_checked = 1;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
      g_dev_ok = 0;
    } else {
      hipDeviceProp_t prop;
      int dev = 0;
      (void)hipGetDevice(&dev);
      g_dev_ok = (hipGetDeviceProperties(&prop, dev) == hipSuccess) &&
                 (std::strncmp(prop.gcnArchName, "gfx950", 6) == 0);
      if (!g_dev_ok) std::fprintf(stderr, "msa: device 0 is %s, need gfx950\n", prop.gcnArchName);
    }
  }
  return g_dev_ok ? MSA_OK : MSA_ERR_NODEV;
}

int current_device() {
  int dev = 0;
  (void)hipGetDevice(&dev);
  return dev;
}

// Frees pooled blocks held by idle cached plans (msa_devcall.inc) when the device runs out.
void (*g_pool_reclaim)() = nullptr;

// Device memory pool.  The reference's harness calls main_alignment_function
// from hardware_concurrency threads at once (testing.cpp:145-158, 269-280,
// 352-358); with plain hipMalloc/hipFree every call would serialize on
// hipFree's implicit device synchronization.  Blocks are cached per (device,
// size class) (powers of two up to 1 MiB, then 2 MiB multiples) in one
// mutex-protected free list, so a block allocated while device d was current
// is only handed to a caller for which d is current.  A block is only returned
// by its owner after the stream work that used it has completed (run_one syncs
// its stream, msa_plan_destroy syncs every stream the plan queued work on), so
// a block never changes hands while a kernel uses it.
class DevPool {
 public:
  static size_t size_class(size_t b) {
    if (b < 256) b = 256;
    if (b <= (size_t(1) << 20)) {
      size_t c = 256;
      while (c < b) c <<= 1;
      return c;
    }
    const size_t mb2 = size_t(2) << 20;
    return (b + mb2 - 1) / mb2 * mb2;
  }
  void* get(size_t bytes) {
    const size_t c = size_class(bytes);
    const int dev = current_device();
    {
      std::lock_guard<std::mutex> lk(mu_);
      auto it = free_.find(std::make_pair(dev, c));
      if (it != free_.end()) {
        void* p = it->second;
        free_.erase(it);
        cached_ -= c;
        return p;
      }
    }
    void* p = nullptr;
    if (hipMalloc(&p, c) != hipSuccess) {
      // cached blocks of other sizes (and those idle cached plans hold) may be what fills the
      // device: release them, retry once
      (void)hipGetLastError();
      if (g_pool_reclaim) g_pool_reclaim();
      release(dev);
      p = nullptr;
      if (hipMalloc(&p, c) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
      }
    }
    std::lock_guard<std::mutex> lk(mu_);
    owner_[p] = dev;
    return p;
  }
  void put(void* p, size_t bytes) {
    if (!p) return;
    const size_t c = size_class(bytes);
    {
      std::lock_guard<std::mutex> lk(mu_);
      auto o = owner_.find(p);
      const int dev = (o != owner_.end()) ? o->second : current_device();
      if (cached_ + c <= kCap) {
        free_.emplace(std::make_pair(dev, c), p);
        cached_ += c;
        return;
      }
      owner_.erase(p);
    }
    (void)hipFree(p);
  }
  // free every cached block of device dev
  void release(int dev) {
    std::vector<void*> victims;
    {
      std::lock_guard<std::mutex> lk(mu_);
      for (auto it = free_.begin(); it != free_.end();) {
        if (it->first.first == dev) {
          victims.push_back(it->second);
          cached_ -= it->first.second;
          owner_.erase(it->second);
          it = free_.erase(it);
        } else {
          ++it;
        }
      }
    }
    for (void* v : victims) (void)hipFree(v);
  }
  size_t cached() {
    std::lock_guard<std::mutex> lk(mu_);
    return cached_;
  }
  size_t cached(int dev) {  // free blocks of device dev
    std::lock_guard<std::mutex> lk(mu_);
    size_t b = 0;
    for (const auto& e : free_)
      if (e.first.first == dev) b += e.first.second;
    return b;
  }

 private:
  static constexpr size_t kCap = size_t(8) << 30;  // bytes kept cached (HBM is 288 GB)
  std::mutex mu_;
  std::multimap<std::pair<int, size_t>, void*> free_;  // (device, size class) -> block
  std::map<void*, int> owner_;                         // block -> device it was allocated on
  size_t cached_ = 0;
};

DevPool& dev_pool() {
  static DevPool* p = new DevPool();  // never destroyed: no HIP calls during static teardown
  return *p;
}

// Admission control at the drop-in boundary.  The reference's callers run main_alignment_function
// from hardware_concurrency threads at once, each on whole sequences (testing.cpp:209-287, call at
// :261; :295-369, call at :345): on a 256-thread host, a 97k pair's ~13 GB footprint (1 B/cell
// direction bytes + pass-2 inputs) times the callers in flight exceeds any device.  Every host-pointer
// entry point therefore reserves its call's device footprint (estimated from m, n before anything
// is allocated: a call never holds part of its memory while it waits) against a per-device budget and
// waits -- FIFO, so no caller is overtaken -- until it fits.  A call larger than the whole budget
// runs alone (it waits until nothing else is admitted).  Budget: MSA_DEVICE_BUDGET_MB, else 90% of
// the device's memory; msa_set_device_budget overrides it at run time.
// Memory the library holds on a device outside the admitted calls: idle cached plans of the reference
// walk and free blocks of the device pool (msa_devcall.inc).  An admission that would put admitted +
// idle bytes over the budget first releases the idle ones, so cached memory never pushes admitted calls
// into the allocator's out-of-memory path.
size_t idle_device_bytes(int dev);
size_t idle_plan_bytes(int dev);
void reclaim_idle_device_bytes(int dev);

class Admission {
 public:
  void acquire(int dev, size_t bytes) {
    std::unique_lock<std::mutex> lk(mu_);
    Dev& d = get(dev);
    const uint64_t t = d.next++;
    bool waited = false;
    cv_.wait(lk, [&] {
      const bool ok = d.serving == t && (d.inuse == 0 || d.inuse + bytes <= d.budget);
      waited = waited || !ok;
      return ok;
    });
    d.inuse += bytes;
    d.peak = std::max(d.peak, d.inuse);
    d.admitted++;
    if (waited) d.waits++;
    d.serving++;
    const size_t inuse = d.inuse, budget = d.budget;
    cv_.notify_all();  // the next ticket may fit too
    lk.unlock();
    if (inuse + idle_device_bytes(dev) > budget) {
      reclaim_idle_device_bytes(dev);
      std::lock_guard<std::mutex> lk2(mu_);
      get(dev).reclaims++;
    }
  }
  void release(int dev, size_t bytes) {
    std::lock_guard<std::mutex> lk(mu_);
    Dev& d = get(dev);
    d.inuse -= std::min(bytes, d.inuse);
    cv_.notify_all();
  }
  void set_budget(int dev, size_t bytes) {
    std::lock_guard<std::mutex> lk(mu_);
    Dev& d = get(dev);
    d.budget = bytes ? bytes : default_budget(dev);
    d.peak = d.inuse;
    d.waits = d.admitted = d.reclaims = 0;
    cv_.notify_all();
  }
  void info(int dev, int64_t* out, int n = 5) {
    std::lock_guard<std::mutex> lk(mu_);
    Dev& d = get(dev);
    out[0] = (int64_t)d.budget;
    out[1] = (int64_t)d.inuse;
    out[2] = (int64_t)d.peak;
    out[3] = (int64_t)d.waits;
    out[4] = (int64_t)d.admitted;
    if (n > 5) out[5] = (int64_t)d.reclaims;
  }

 private:
  struct Dev {
    bool init = false;
    size_t budget = 0, inuse = 0, peak = 0;
    uint64_t next = 0, serving = 0, waits = 0, admitted = 0, reclaims = 0;
  };
  static size_t default_budget(int dev) {
    const char* e = std::getenv("MSA_DEVICE_BUDGET_MB");
    if (e && std::atoll(e) > 0) return (size_t)std::atoll(e) << 20;
    size_t fr = 0, tot = 0;
    int cur = 0;
    (void)hipGetDevice(&cur);
    if (cur != dev) (void)hipSetDevice(dev);
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); tot = size_t(16) << 30; }
    if (cur != dev) (void)hipSetDevice(cur);
    return tot / 10 * 9;
  }
  Dev& get(int dev) {  // (mu_ held)
    Dev& d = dev_[dev];
    if (!d.init) {
      d.init = true;
      d.budget = default_budget(dev);
    }
    return d;
  }
  std::mutex mu_;
  std::condition_variable cv_;
  std::map<int, Dev> dev_;
};

Admission& admission() {
  static Admission* a = new Admission();
  return *a;
}

// RAII reservation of one call's device footprint (declare it before the call's streams and blocks:
// destroyed last, after they have been synchronized and returned)
struct Admit {
  int dev = 0;
  size_t bytes = 0;
  explicit Admit(size_t b) : bytes(b) {
    (void)hipGetDevice(&dev);
    admission().acquire(dev, bytes);
  }
  ~Admit() { admission().release(dev, bytes); }
  Admit(const Admit&) = delete;
  Admit& operator=(const Admit&) = delete;
};

// Non-blocking streams reused across calls (creating one costs ~10s of us), one
// free list per device: a stream is only handed to a caller whose current device
// created it.
class StreamPool {
 public:
  hipStream_t get() {
    const int dev = current_device();
    {
      std::lock_guard<std::mutex> lk(mu_);
      auto& fl = free_[dev];
      if (!fl.empty()) {
        hipStream_t s = fl.back();
        fl.pop_back();
        return s;
      }
    }
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(mu_);
    owner_[s] = dev;
    return s;
  }
  void put(hipStream_t s) {
    if (!s) return;
    std::lock_guard<std::mutex> lk(mu_);
    auto o = owner_.find(s);
    free_[o != owner_.end() ? o->second : current_device()].push_back(s);
  }

 private:
  std::mutex mu_;
  std::map<int, std::vector<hipStream_t>> free_;
  std::map<hipStream_t, int> owner_;
};

std::atomic<uint32_t> g_epoch{0};  // granule epoch of the next run (msa_plan_run)

StreamPool& stream_pool() {
  static StreamPool* p = new StreamPool();
  return *p;
}

typedef void (*kfn_t)(KArgs);

// Per-process caches of what plan creation asks the runtime: compute units per device
// (hipGetDeviceProperties is slow, and main_alignment_function creates a plan per call)
// and, per (device, kernel, block, LDS), the dynamic-LDS attribute and the occupancy.
std::mutex g_shape_mu;
int device_cus() {
  static std::map<int, int> cus;
  const int dev = current_device();
  std::lock_guard<std::mutex> lk(g_shape_mu);
  auto it = cus.find(dev);
  if (it != cus.end()) return it->second;
  hipDeviceProp_t prop;
  const int n = (hipGetDeviceProperties(&prop, dev) == hipSuccess) ? prop.multiProcessorCount : 1;
  cus[dev] = n;
  return n;
}
// LDS a workgroup may allocate on the current device: min(sharedMemPerBlockOptin, 160 KiB), read once
// per device (plans reject larger requests instead of failing the attribute call on a smaller part)
size_t device_lds_max() {
  static std::map<int, size_t> lds;
  const int dev = current_device();
  std::lock_guard<std::mutex> lk(g_shape_mu);
  auto it = lds.find(dev);
  if (it != lds.end()) return it->second;
  hipDeviceProp_t prop;
  size_t v = 64 * 1024;
  if (hipGetDeviceProperties(&prop, dev) == hipSuccess)
    v = std::max<size_t>(prop.sharedMemPerBlockOptin, prop.sharedMemPerBlock);
  v = std::min<size_t>(v, 160 * 1024);
  lds[dev] = v;
  return v;
}
// raises the kernel's dynamic-LDS limit to the CU's whole LDS (once per device and kernel: plans of
// one kernel with different LDS sizes then never lower it under each other) and returns its
// occupancy at `lds` bytes (blocks per CU, >= 1), or -1
int kernel_shape(kfn_t fn, int threads, size_t lds) {
  static std::map<std::tuple<int, kfn_t, int, size_t>, int> occ_of;
  static std::map<std::pair<int, kfn_t>, bool> attr_set;
  const size_t lds_max = device_lds_max();
  const auto key = std::make_tuple(current_device(), fn, threads, lds);
  std::lock_guard<std::mutex> lk(g_shape_mu);
  auto it = occ_of.find(key);
  if (it != occ_of.end()) return it->second;
  if (lds > lds_max) return -1;
  const auto ak = std::make_pair(current_device(), fn);
  if (!attr_set[ak]) {
    if (hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max) != hipSuccess)
      return -1;
    attr_set[ak] = true;
  }
  int occ = 1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)fn, threads, lds) != hipSuccess || occ < 1)
    occ = 1;
  occ_of[key] = occ;
  return occ;
}

// single-pair phase length: 32 steps for one carried value (SW linear); 16 when
// two or three values per cell are carried (register pressure: no spills)
constexpr int ks_single(int alg) {
  const msa_alg_info t = msa_alg_info_of(alg);
  return (t.linear() && !t.packed()) ? MSA_KS_SINGLE : 16;
}
constexpr int ks_batch(int alg) { return msa_alg_info_of(alg).packed() ? MSA_KS_BATCH_SWLP : MSA_KS_BATCH; }

template <int ALG, int OUT, int TP>
kfn_t kf(bool sgl) {
  // single pair: (MSA_WAVES_SINGLE waves, MSA_KS_SINGLE steps/phase); batch: (MSA_WAVES_BATCH, MSA_KS_BATCH)
  return sgl ? stripe_kernel<ALG, OUT, TP, MSA_WAVES_SINGLE, ks_single(ALG), true>
                               : stripe_kernel<ALG, OUT, TP, MSA_WAVES_BATCH, ks_batch(ALG), false>;
}

// the score-only and the direction-byte instantiation of one algorithm under one tracking mode
template <int ALG, int TP>
kfn_t kf_nd(int out, bool sgl) {
  if (out == MSA_OUT_NONE) return kf<ALG, MSA_OUT_NONE, TP>(sgl);
  if (out == MSA_OUT_DIR) return kf<ALG, MSA_OUT_DIR, TP>(sgl);
  return nullptr;
}

// names every stripe_kernel instantiation the library holds (what each algorithm is: msa_alg.h)
kfn_t pick_kernel(int alg, int out, int tp, bool sgl) {
#define K3(A, O) return tp == 2 ? kf<A, O, 2>(sgl) : (tp ? kf<A, O, 1>(sgl) : kf<A, O, 0>(sgl))
  switch (alg) {
    case MSA_ALG_SWL:
      if (out == MSA_OUT_NONE) K3(MSA_ALG_SWL, MSA_OUT_NONE);
      if (out == MSA_OUT_H) K3(MSA_ALG_SWL, MSA_OUT_H);
      break;
    case MSA_ALG_SWLP:
      if (out == MSA_OUT_NONE && !sgl && tp == 0) return kf<MSA_ALG_SWLP, MSA_OUT_NONE, 0>(false);
      break;
    case MSA_ALG_SWL0:
      if (out == MSA_OUT_NONE) K3(MSA_ALG_SWL0, MSA_OUT_NONE);
      if (out == MSA_OUT_H) K3(MSA_ALG_SWL0, MSA_OUT_H);
      break;
    case MSA_ALG_SWA:
      if (out == MSA_OUT_NONE) K3(MSA_ALG_SWA, MSA_OUT_NONE);
      if (out == MSA_OUT_H) K3(MSA_ALG_SWA, MSA_OUT_H);
      if (out == MSA_OUT_DIR) K3(MSA_ALG_SWA, MSA_OUT_DIR);
      break;
    case MSA_ALG_NWA:
      if (out == MSA_OUT_H) return kf<MSA_ALG_NWA, MSA_OUT_H, 0>(sgl);
      // (direction bytes: MSA_NW_ALIGN plans only -- msa_plan_create keeps (MSA_NW_BANDED, DIR) unsupported)
      return kf_nd<MSA_ALG_NWA, 0>(out, sgl);
    case MSA_ALG_REF:
      if (out == MSA_OUT_TAB) return kf<MSA_ALG_REF, MSA_OUT_TAB, 0>(sgl);
      if (out == MSA_OUT_H) return kf<MSA_ALG_REF, MSA_OUT_H, 0>(sgl);
      return kf_nd<MSA_ALG_REF, 0>(out, sgl);
    case MSA_ALG_REF1: return kf_nd<MSA_ALG_REF1, 0>(out, sgl);
    case MSA_ALG_PART:
      if (out == MSA_OUT_TAB) return kf<MSA_ALG_PART, MSA_OUT_TAB, 0>(sgl);
      break;
    // instantiations of their own each: the MSA_ALG_NWA kernels' code is unchanged by them
    case MSA_ALG_FIT: return kf_nd<MSA_ALG_FIT, 0>(out, sgl);
    case MSA_ALG_NWA32: return kf_nd<MSA_ALG_NWA32, 0>(out, sgl);
    case MSA_ALG_FIT32: return kf_nd<MSA_ALG_FIT32, 0>(out, sgl);
    case MSA_ALG_OVL: return kf_nd<MSA_ALG_OVL, 0>(out, sgl);
    case MSA_ALG_OVL32: return kf_nd<MSA_ALG_OVL32, 0>(out, sgl);
    // the first maximum over all interior cells is tracked by compare-select (1; never the packed key, whose values
    // must be non-negative)
    case MSA_ALG_EXT: return tp == 1 ? kf_nd<MSA_ALG_EXT, 1>(out, sgl) : nullptr;
    case MSA_ALG_EXT32: return tp == 1 ? kf_nd<MSA_ALG_EXT32, 1>(out, sgl) : nullptr;
    // ... inside a band (MSA_NW_EXTEND_BAND): the banded global kernels' edge phases with that tracker in them --
    // instantiations of their own again, the MSA_ALG_EXT and MSA_ALG_NWA kernels' code is unchanged
    case MSA_ALG_EXTB: return tp == 1 ? kf_nd<MSA_ALG_EXTB, 1>(out, sgl) : nullptr;
    case MSA_ALG_EXTB32: return tp == 1 ? kf_nd<MSA_ALG_EXTB32, 1>(out, sgl) : nullptr;
    // an MSA_SW_SCORED plan always tracks its end cell: compare-select (1) or the packed key (2) only
    case MSA_ALG_SWS: return tp == 2 ? kf_nd<MSA_ALG_SWS, 2>(out, sgl) : tp == 1 ? kf_nd<MSA_ALG_SWS, 1>(out, sgl) : nullptr;
    case MSA_ALG_SWS32:
      return tp == 2 ? kf_nd<MSA_ALG_SWS32, 2>(out, sgl) : tp == 1 ? kf_nd<MSA_ALG_SWS32, 1>(out, sgl) : nullptr;
    // the profile plans: their 32-code twins' instantiations under the other score source
    case MSA_ALG_NWP: return kf_nd<MSA_ALG_NWP, 0>(out, sgl);
    case MSA_ALG_FITP: return kf_nd<MSA_ALG_FITP, 0>(out, sgl);
    case MSA_ALG_SWP:
      return tp == 2 ? kf_nd<MSA_ALG_SWP, 2>(out, sgl) : tp == 1 ? kf_nd<MSA_ALG_SWP, 1>(out, sgl) : nullptr;
  }
#undef K3
  return nullptr;
}

// single-pair SW linear (msa_flow.hip): pass 1 (chain), pass 2 (fill + H)
kfn_t pick_flow(int alg, bool best, bool save, int tp, int R, bool nneg) {
  // SW affine / the reference's Gotoh (direction bytes): pass 1 + in-launch pass 2, two rows per lane;
  // SW affine with scores >= 0: pass 1 applies the zero floor in its head phases only
  if (alg == MSA_ALG_SWA) {
    if (!save || R != 2) return nullptr;
    return nneg ? flow_kernel<false, false, true, true, 2, 1> : flow_kernel<true, false, true, true, 2, 1>;
  }
  if (alg == MSA_ALG_REF1) return save && R == 2 ? flow_kernel<true, false, true, true, 2, 2> : nullptr;
  // score-only plans: pass 1 alone, one row per lane, best cell tracked in the chain;
  // H plans: pass 1 + in-launch pass 2, two rows per lane
  const bool fl = (alg == MSA_ALG_SWL);
  if (best) return fl ? flow_kernel<true, true, false, false> : flow_kernel<false, true, false, false>;
  if (save && R == 2) {
    if (fl) return tp ? flow_kernel<true, false, true, true, 2> : flow_kernel<true, false, true, false, 2>;
    return tp ? flow_kernel<false, false, true, true, 2> : flow_kernel<false, false, true, false, 2>;
  }
  return nullptr;
}

// the separate pass-2 launch of a long pair (flow_fill_kernel), same instantiation parameters
kfn_t pick_fill(int alg, int tp, int R, bool nneg) {
  if (R != 2) return nullptr;
  if (alg == MSA_ALG_SWA) return nneg ? flow_fill_kernel<false, false, 2, 1> : flow_fill_kernel<true, false, 2, 1>;
  if (alg == MSA_ALG_REF1) return flow_fill_kernel<true, false, 2, 2>;
  if (alg == MSA_ALG_SWL) return tp ? flow_fill_kernel<true, true, 2, 0> : flow_fill_kernel<true, false, 2, 0>;
  return tp ? flow_fill_kernel<false, true, 2, 0> : flow_fill_kernel<false, false, 2, 0>;
}

}  // namespace

#include "msa_plan.inc"

extern "C" {

const char* msa_status_string(int s) {
  switch (s) {
    case MSA_OK: return "ok";
    case MSA_ERR_ARG: return "invalid argument";
    case MSA_ERR_ALPHABET: return "more than 8 distinct symbols";
    case MSA_ERR_HIP: return "HIP runtime error";
    case MSA_ERR_NODEV: return "no gfx950 device";
    case MSA_ERR_UNSUPPORTED: return "unsupported parameters (GPU path needs integral g,h)";
    case MSA_ERR_TIMEOUT: return "cross-workgroup wait timed out";
    case MSA_ERR_NOMEM: return "out of memory";
    case MSA_ERR_CAPACITY: return "output buffer too small";
    case MSA_ERR_NOMATCH: return "traceback found no predecessor";
  }
  return "unknown status";
}

int msa_version(void) { return 1; }

int msa_set_device_budget(int64_t bytes) {
  if (bytes < 0) return MSA_ERR_ARG;
  int rc = ensure_device();
  if (rc != MSA_OK) return rc;
  admission().set_budget(current_device(), (size_t)bytes);
  return MSA_OK;
}

int msa_device_budget_info(int64_t* out5) {
  if (!out5) return MSA_ERR_ARG;
  int rc = ensure_device();
  if (rc != MSA_OK) return rc;
  admission().info(current_device(), out5);
  return MSA_OK;
}

int msa_device_memory_info(int64_t* out4) {
  if (!out4) return MSA_ERR_ARG;
  int rc = ensure_device();
  if (rc != MSA_OK) return rc;
  const int dev = current_device();
  int64_t b[6];
  admission().info(dev, b, 6);
  out4[0] = b[1];
  out4[1] = (int64_t)idle_plan_bytes(dev);
  out4[2] = (int64_t)dev_pool().cached(dev);
  out4[3] = b[5];
  return MSA_OK;
}

int msa_device_count(int* count) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  if (count) *count = n;
  return n > 0 ? MSA_OK : MSA_ERR_NODEV;
}

int msa_encode_pair(const char* A0, size_t m, const char* B0, size_t n, uint8_t* ca, uint8_t* cb) {
  // DNA fast path: fixed codes so batches share one code map
  msa_host::SymbolMap map(8, "ACGT");
  const int rc = map.encode(A0, m, ca);
  return rc != MSA_OK ? rc : map.encode(B0, n, cb);
}

void msa_plan_destroy(msa_plan* P) {
  if (!P) return;
  // the plan's blocks go back to the pool: every run, traceback and score copy it
  // queued (on whichever streams) must be complete
  for (hipStream_t s : P->streams) (void)hipStreamSynchronize(s);
  for (auto& b : P->blocks) dev_pool().put(b.first, b.second);
  if (P->ev0) (void)hipEventDestroy(P->ev0);
  if (P->ev1) (void)hipEventDestroy(P->ev1);
  delete P;
}

int msa_plan_cells_size(const msa_plan* P, int64_t* elems) {
  if (!P || !elems) return MSA_ERR_ARG;
  *elems = (P->d.cells == MSA_CELLS_NONE) ? 0 : P->cells_elems;
  return MSA_OK;
}

int64_t msa_plan_stripes(const msa_plan* P) { return P ? P->total_stripes : 0; }

int msa_plan_pair_layout(const msa_plan* P, int64_t pair, int64_t* out4) {
  if (!P || !out4 || pair < 0 || pair >= (int64_t)P->pairs.size()) return MSA_ERR_ARG;
  const msa_pair_desc& pd = P->pairs[(size_t)pair];
  out4[0] = pd.stripe0;
  out4[1] = pd.pmax;
  out4[2] = pd.out_off;
  out4[3] = P->KS | ((int64_t)P->R << 16);  // bits 16+: rows per lane of the layout (0 = 1)
  return MSA_OK;
}

int msa_plan_run(msa_plan* P, const uint8_t* dA, const uint8_t* dB, void* c0, void* c1, void* c2, void* stream) {
  // (a profile plan's rows are its own: it reads no row codes)
  if (!P || !dB || (!dA && !P->d_prof)) return MSA_ERR_ARG;
  if (P->d.cells != MSA_CELLS_NONE && !c0) return MSA_ERR_ARG;
  if (P->d.cells == MSA_CELLS_TAB && (!c1 || !c2)) return MSA_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  P->note_stream(st);
  KArgs a;
  std::memset(&a, 0, sizeof(a));
  P->epoch = next_epoch();
  a.A = dA;
  a.B = dB;
  a.pairs = P->d_pairs;
  a.meta = P->d_meta;
  a.ticket = P->d_ticket;
  a.err = P->d_err;
  a.gbuf = P->d_gbuf;
  a.gbuf_stride = P->gbuf_stride;
  if (P->d.cells == MSA_CELLS_DIR) a.outDir = (uint8_t*)c0;
  else a.outH = (int32_t*)c0;
  a.outT2 = (int32_t*)c1;
  a.outT3 = (int32_t*)c2;
  a.stamps = P->stamps;
  a.cod = P->d_cod;
  a.cod_copy = P->cod_copy;
  a.sub = P->d_sub;
  a.prof = P->d_prof;
  a.br = P->d_br;
  a.snap = P->d_snap;
  a.blk = P->d_blk;
  a.border = P->d_order;
  a.nflow = P->nflow;
  a.best_key = P->fused_reduce ? reinterpret_cast<unsigned long long*>(P->d_ticket + MSA_TK_BEST) : nullptr;
  a.brw = P->brw;
  a.nseg = P->nseg;
  a.ps_shift = __builtin_ctz((unsigned)P->ps);
  a.nblk = P->nblk;
  {
    // (the SW kernels' virtual code: 7, or 31 over 5-bit codes)
    const msa_alg_info t = msa_alg_info_of(P->main.kp.alg);
    const unsigned virt = t.local() ? (t.wide ? MSA_VIRT_CODE32 : MSA_VIRT_CODE) : 0u;
    // about two output words per thread for one long pair (64 x 256 threads took 22 us for
    // C3's 97k columns, 24 dependent rounds each), at least 64 workgroups per segment
    const int64_t words = MSA_NCOPY * (P->cod_copy / 4) / std::max<int64_t>(1, (int64_t)P->segs.size());
    const unsigned gx = (unsigned)std::min<int64_t>(1024, std::max<int64_t>(64, words / 512));
    hipLaunchKernelGGL(stage_codes_kernel, dim3(gx, (unsigned)P->segs.size()), dim3(256), 0, st, dB, P->d_segs,
                       (int)P->segs.size(), P->d_cod, (long long)P->cod_copy, virt, t.wide ? 31u : 7u,
                       P->d_ticket);
    HIPCHK(hipGetLastError());
  }
  const bool ev = P->timing;  // timing events are instrumentation: msa_plan_set_timing
  if (ev) HIPCHK(hipEventRecord(P->ev0, st));
  P->timed = ev;
  if (P->chunked()) {
    a.ck = P->d_ck;
    a.ckw = P->ckw;
    if (P->h16 && P->d.cells == MSA_CELLS_H) a.outH16 = P->d_h16;
  }
  int rc = enqueue(P->main, a, P->epoch, st);
  if (rc != MSA_OK) return rc;
  if (P->chunked()) {
    // verify every chunk's constant, add the prefix of the constants to its cells; then the
    // exact single-mode launch, which returns at once when *skip == 1
    // (a fused check + add launch, roles by arrival ticket, the adders' first loads in flight
    // across the checks, measured slower: C3 0.94 vs 0.67 ms)
    hipLaunchKernelGGL(chunk_check_kernel, dim3(P->n_chunks), dim3(256), 0, st, (const int*)P->d_ck, P->ckw, P->d_dk,
                       P->d_okk);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(chunk_add_kernel, dim3(32, P->n_chunks), dim3(256), 0, st,
                       P->d.cells == MSA_CELLS_H ? a.outH : (int32_t*)nullptr, (const int16_t*)a.outH16,
                       (const msa_pair_desc*)P->d_pairs,
                       P->d_meta, (const int*)P->d_dk, (const int*)P->d_okk, P->n_chunks, P->main.kp.chunk_c, P->d_skip,
                       P->d_ticket);
    HIPCHK(hipGetLastError());
    KArgs b = a;
    b.ck = nullptr;
    b.outH16 = nullptr;  // the exact launch writes every cell as int32
    b.skip = P->d_skip;
    // its own epoch: the band kernel's chunked launch leaves granules of this run's epoch in the
    // slots the exact launch reads
    if ((rc = enqueue(P->exact, b, next_epoch(), st)) != MSA_OK) return rc;
  }
  // long pair: pass 2 behind pass 1
  if (P->fill.fn && (rc = enqueue(P->fill, a, P->epoch, st)) != MSA_OK) return rc;
  if (ev) HIPCHK(hipEventRecord(P->ev1, st));
  if (P->flow2 && P->main.kp.alg != MSA_ALG_REF1) {  // (Gotoh: the final state is in the last stripe's meta)
    if (!P->fused_reduce) {  // (fused: the pass-2 blocks folded the result into the best-cell key)
      hipLaunchKernelGGL(reduce_blocks_kernel, dim3(1), dim3(1024), 0, st, (const int4*)P->d_blk, P->nblk, P->d_res);
      HIPCHK(hipGetLastError());
    }
    return MSA_OK;
  }
  const int np = (int)P->d.n_pairs;
  hipLaunchKernelGGL(reduce_pairs_kernel, dim3(np), dim3(64), 0, st, P->d_pairs, P->d_meta, np,
                     (int)msa_alg_info_of(P->main.kp.alg).result, P->d_res);
  HIPCHK(hipGetLastError());
  return MSA_OK;
}

#ifdef MSA_STAMPS
extern "C" int msa_debug_stamps(msa_plan* P, unsigned long long* d) { P->stamps = d; return 0; }
#endif

int msa_plan_set_timing(msa_plan* P, int on) {
  if (!P) return MSA_ERR_ARG;
  P->timing = on != 0;
  return MSA_OK;
}

int msa_plan_last_kernel_ms(msa_plan* P, float* ms) {
  if (!P || !ms) return MSA_ERR_ARG;
  if (!P->timed) return MSA_ERR_ARG;  // no run with timing on yet
  HIPCHK(hipEventSynchronize(P->ev1));
  HIPCHK(hipEventElapsedTime(ms, P->ev0, P->ev1));
  return MSA_OK;
}

int msa_plan_results(msa_plan* P, msa_pair_result* out, void* stream) {
  if (!P || !out) return MSA_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  int err = 0;
  HIPCHK(hipMemcpyAsync(&err, P->d_err, sizeof(err), hipMemcpyDeviceToHost, st));
  unsigned long long key = 0;
  if (P->fused_reduce)  // one pair: its result is the pass-2 blocks' best-cell key
    HIPCHK(hipMemcpyAsync(&key, P->d_ticket + MSA_TK_BEST, sizeof(key), hipMemcpyDeviceToHost, st));
  else
    HIPCHK(hipMemcpyAsync(out, P->d_res, sizeof(PairResult) * P->d.n_pairs, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  static_assert(sizeof(PairResult) == sizeof(msa_pair_result), "result layout");
  if (P->fused_reduce) {
    const PairResult r = best_key_decode(key, P->pairs[0].n);
    std::memcpy(out, &r, sizeof(r));
  }
  if (err) {
    std::fprintf(stderr, "msa: a kernel wait hit its spin limit (site %d) in a run since the plan was created "
                 "or last cleared\n", err);
    return MSA_ERR_TIMEOUT;
  }
  return MSA_OK;
}

int msa_plan_run_info(msa_plan* P, int32_t* out4, void* stream) {
  if (!P || !out4) return MSA_ERR_ARG;
  out4[0] = P->chunked() ? 2 : (P->mode == PM_FLOW ? 1 : 0);
  out4[1] = P->n_chunks;
  out4[2] = -1;
  out4[3] = P->chunked() ? (P->main.kp.chunk_warm | (P->h16 ? (1 << 16) : 0)) : 0;  // bit 16: int16 chunk cells
  if (P->chunked()) {
    int v = 0;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(&v, P->d_skip, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    out4[2] = v;
  }
  return MSA_OK;
}

int msa_plan_launch_info(const msa_plan* P, int32_t* out8) {
  if (!P || !out8) return MSA_ERR_ARG;
  const int32_t v[8] = {P->mode, P->main.grid, P->main.threads, (int32_t)P->main.lds, P->nflow,
                        P->fill.fn ? P->fill.grid : 0, P->R, P->main.kp.n_items};
  std::copy(v, v + 8, out8);
  return MSA_OK;
}

int msa_plan_format_info(const msa_plan* P, int32_t* out4) {
  if (!P || !out4) return MSA_ERR_ARG;
  const int alg = P->main.kp.alg;
  out4[0] = alg == MSA_ALG_SWLP ? 1 : (alg == MSA_ALG_REF1 ? 2 : 0);
  out4[1] = P->tp;
  out4[2] = P->h16 ? 1 : 0;
  out4[3] = (msa_alg_info_of(alg).wide ? 1 : 0) | (msa_alg_info_of(alg).profile ? 2 : 0);
  return MSA_OK;
}

int msa_plan_error(msa_plan* P, int* code, void* stream) {
  if (!P || !code) return MSA_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemcpyAsync(code, P->d_err, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return MSA_OK;
}

int msa_plan_clear_error(msa_plan* P, void* stream) {
  if (!P) return MSA_ERR_ARG;
  HIPCHK(hipMemsetAsync(P->d_err, 0, sizeof(int), (hipStream_t)stream));
  return MSA_OK;
}

int msa_plan_scores(msa_plan* P, int32_t* dst, void* stream) {
  if (!P || !dst) return MSA_ERR_ARG;
  // the score field of every PairResult, device to device (no host sync)
  P->note_stream((hipStream_t)stream);
  if (P->fused_reduce) {  // the pair result from the best-cell key first
    hipLaunchKernelGGL(best_key_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned long long*>(P->d_ticket + MSA_TK_BEST), (long long)P->pairs[0].n,
                       P->d_res);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemcpy2DAsync(dst, sizeof(int32_t), P->d_res, sizeof(PairResult), sizeof(int32_t), (size_t)P->d.n_pairs,
                          hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MSA_OK;
}

int msa_plan_stripe_meta(msa_plan* P, int32_t* out, int64_t cap, void* stream) {
  if (!P || !out || cap < P->total_stripes) return MSA_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  static_assert(sizeof(msa_stripe_meta) == 12 * 4, "meta layout");
  HIPCHK(hipMemcpyAsync(out, P->d_meta, sizeof(msa_stripe_meta) * P->total_stripes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return MSA_OK;
}

int msa_plan_traceback(msa_plan* P, int64_t pair, const uint8_t* dDir, uint8_t* d_ops, int64_t ops_cap,
                       int64_t* d_info, void* stream) {
  if (!P || !dDir || !d_ops || !d_info || ops_cap < 0 || pair < 0 || pair >= P->d.n_pairs) return MSA_ERR_ARG;
  // the walk starts at the fill's end cell: plans without track_end have none
  // (an MSA_SW_SCORED plan always has one: plan_create sets its track_end)
  if (walker_of(P) != TB_SW) return MSA_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  P->note_stream(st);
  hipLaunchKernelGGL((P->R == 2 ? traceback_kernel<TB_SW, 2> : traceback_kernel<TB_SW>), dim3(1), dim3(384), 0, st, dDir, P->d_pairs, P->d_meta,
                     (const PairResult*)P->d_res, (int)pair, 0, 0, d_ops, (long long)ops_cap, (long long*)d_info,
                     P->mode == PM_FLOW ? 1 : 0,
                     P->fused_reduce ? reinterpret_cast<const unsigned long long*>(P->d_ticket + MSA_TK_BEST) : nullptr);
  HIPCHK(hipGetLastError());
  return MSA_OK;
}

int msa_plan_traceback_gotoh(msa_plan* P, int64_t pair, int end_type, const uint8_t* dDir, uint8_t* d_ops,
                             int64_t ops_cap, int64_t* d_info, void* stream) {
  if (!P || !dDir || !d_ops || !d_info || ops_cap < 0 || pair < 0 || pair >= P->d.n_pairs) return MSA_ERR_ARG;
  if (end_type < -3 || end_type > 3 || end_type == 0) return MSA_ERR_ARG;
  const msa_walk kind = walker_of(P);
  if (kind != TB_REF && kind != TB_REF_TAG) return MSA_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  P->note_stream(st);
  // REF1 bytes hold tags (3 / 2 / 1 = T1 / T2 / T3), REF bytes the table numbers
  hipLaunchKernelGGL(kind == TB_REF_TAG ? (P->R == 2 ? traceback_kernel<TB_REF_TAG, 2> : traceback_kernel<TB_REF_TAG>)
                                        : traceback_kernel<TB_REF>, dim3(1),
                     dim3(384), 0, st, dDir, P->d_pairs, P->d_meta, (const PairResult*)P->d_res, (int)pair, end_type,
                     (int)P->main.kp.h, d_ops, (long long)ops_cap, (long long*)d_info, P->mode == PM_FLOW ? 1 : 0,
                     (const unsigned long long*)nullptr);
  HIPCHK(hipGetLastError());
  return MSA_OK;
}

int msa_plan_traceback_nw(msa_plan* P, int64_t pair, const uint8_t* dDir, uint8_t* d_ops, int64_t ops_cap,
                          int64_t* d_info, void* stream) {
  if (!P || !dDir || !d_ops || !d_info || ops_cap < 0 || pair < 0 || pair >= P->d.n_pairs) return MSA_ERR_ARG;
  const msa_walk kind = walker_of(P);
  if (kind != TB_NW && kind != TB_FIT) return MSA_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  P->note_stream(st);
  // stripe starts from the stripe meta (band geometry); the walk needs no end type and no PairResult (a fit plan's
  // walk, TB_FIT: the same walk from the run's end cell (m, end_j) in its PairResult; an overlap plan's end cell
  // may lie on the last column instead, (end_i, n), or be the empty overlap's (m, 0), which ends the walk at once;
  // an extension plan's is any interior cell, or the empty extension's (0, 0), no walk either)
  hipLaunchKernelGGL((kind == TB_FIT ? traceback_kernel<TB_FIT> : traceback_kernel<TB_NW>), dim3(1), dim3(384), 0, st, dDir, P->d_pairs, P->d_meta,
                     (const PairResult*)P->d_res, (int)pair, 0, 0, d_ops, (long long)ops_cap, (long long*)d_info, 0,
                     (const unsigned long long*)nullptr);
  HIPCHK(hipGetLastError());
  return MSA_OK;
}

int msa_plan_traceback_batch(msa_plan* P, const uint8_t* dDir, uint8_t* d_ops, const int64_t* d_ops_off,
                             int64_t* d_info, void* stream) {
  if (!P || !dDir || !d_ops || !d_ops_off || !d_info) return MSA_ERR_ARG;
  // one row per lane, stripe starts in the stripe meta, a PairResult per pair: the flow kernels' plans (two rows
  // per lane, computed stripe starts, the fused best-cell key) stay with the single walker
  if (P->mode == PM_FLOW || P->R == 2 || P->fused_reduce) return MSA_ERR_UNSUPPORTED;
  // (TB_FIT: the global walk from each pair's end cell: fit (m, end_j); overlap (end_i, end_j), one of them on the last
  // row or column -- or (m, 0), the empty overlap, whose walk the kernel's own `j > 0` ends before its first step;
  // extension (end_i, end_j) anywhere inside -- or (0, 0), the empty extension, ended by `i > 0` likewise)
  const msa_walk kind = walker_of(P);
  if (kind != TB_NW && kind != TB_SW && kind != TB_FIT) return MSA_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  P->note_stream(st);
  const int np = (int)P->d.n_pairs;
  hipLaunchKernelGGL((kind == TB_FIT  ? traceback_batch_kernel<TB_FIT>
                      : kind == TB_NW ? traceback_batch_kernel<TB_NW>
                                      : traceback_batch_kernel<TB_SW>),
                     dim3((unsigned)((np + TBB_WPB - 1) / TBB_WPB)), dim3(64 * TBB_WPB), 0, st, dDir, P->d_pairs,
                     P->d_meta, (const PairResult*)P->d_res, np, d_ops, (const long long*)d_ops_off,
                     (long long*)d_info);
  HIPCHK(hipGetLastError());
  return MSA_OK;
}

int msa_plan_checksum(msa_plan* P, const int32_t* dH, int64_t pair, uint64_t* digest, void* stream) {
  if (!P || !dH || !digest || pair < 0 || pair >= P->d.n_pairs) return MSA_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(P->d_sum, 0, 8, st));
  hipLaunchKernelGGL(checksum_kernel, dim3(1024), dim3(256), 0, st, dH, P->d_pairs, P->d_meta, (int)pair,
                     P->main.kp.band, P->R, P->d_sum);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(digest, P->d_sum, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return MSA_OK;
}

}  // extern "C"
// the host-pointer entries: the device-call scaffold, then the reference's API and the alignment entries over it
#include "msa_devcall.inc"
#include "msa_refapi.inc"
#include "msa_rowapi.inc"
#include "msa_alignapi.inc"
#include "msa_xdropapi.inc"
#include "msa_seedapi.inc"
#include "msa_chainapi.inc"

// rt.hip -- the runtime under the extern "C" surface of libmlhip.so (include/mlhip.h): the thread's error text, the
// process's device list and the sharding threads, the leased streams and scratch arenas of the host-buffer calls, the host
// worker pool, and the table of per-curve operations every api_*.hip unit dispatches through.  No kernels here.
// There is no CPU fallback: every compute entry point needs a HIP device (MLHIP_ENODEVICE otherwise).
#include <pthread.h>
#include <sched.h>

#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>
#include <string>

#include "ec.h"
#include "mlhip_rt.h"

using namespace mlhip;
using namespace mlhip_rt;

namespace {
thread_local std::string g_err;
thread_local int g_device_sel = -1;  // mlhip_set_device on this thread; -1: follow the process's device list
thread_local int g_device = 0;       // device of the call in progress on this thread (set by ensure_device)

// ---- the process's device list (mlhip_init / MLHIP_DEVICES) ---------------------------------------------------------
// one process, one host thread per device, the C ABI takes a device list.  A host-buffer MSM / pairing
// batch issued by a thread that has not pinned itself to one device (mlhip_set_device) is cut into contiguous shards,
// one per listed device, when it is large enough to pay (MLHIP_MULTI_MIN pairs, MLHIP_MULTI_MIN_PAIRINGS pairings).
std::mutex g_devs_mu;
std::vector<int> g_devs;
bool g_devs_set = false;
std::atomic<bool> g_devs_bad{false};  // (read without the lock by ensure_device / mlhip_get_devices) MLHIP_DEVICES did not parse: every compute call fails until mlhip_init / mlhip_shutdown
size_t g_multi_min_msm = (size_t)1 << 21, g_multi_min_pairing = (size_t)1 << 17;

bool parse_device_list(const char* e, std::vector<int>& out) {
  out.clear();
  if (!e || !*e) return true;
  if (!strcmp(e, "all")) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    for (int i = 0; i < n && i < MLHIP_MAX_DEVICES; i++) out.push_back(i);
    return true;
  }
  const char* q = e;
  while (*q) {
    char* end = nullptr;
    long v = strtol(q, &end, 10);
    if (end == q || v < 0 || v >= MLHIP_MAX_DEVICES || out.size() >= 64) return false;
    out.push_back((int)v);
    q = end;
    if (*q == ',') q++;
    else if (*q) return false;
  }
  return true;
}

std::vector<int> device_list() {
  std::lock_guard<std::mutex> lk(g_devs_mu);
  if (!g_devs_set) {
    g_devs_set = true;
    g_devs_bad = !parse_device_list(getenv("MLHIP_DEVICES"), g_devs);
    if (g_devs_bad) g_devs.clear();
    if (const char* e = getenv("MLHIP_MULTI_MIN")) g_multi_min_msm = strtoull(e, nullptr, 10);
    if (const char* e = getenv("MLHIP_MULTI_MIN_PAIRINGS")) g_multi_min_pairing = strtoull(e, nullptr, 10);
  }
  return g_devs;
}

template <class F>
int host_sum(const void* pts, size_t n, void* out) {
  const Affine<F>* p = (const Affine<F>*)pts;
  XYZZ<F> acc;
  xyzz_set_inf<F>(acc);
  for (size_t i = 0; i < n; i++) xyzz_madd<F>(acc, p[i], false);
  Affine<F> r;
  xyzz_to_affine<F>(r, acc);
  memcpy(out, &r, sizeof(r));
  return 0;
}

// The rows of the curve table, by curve id.  MLHIP_CURVE_OPS(C) is every member of CurveOps but the last, which only
// BLS12-377 has.
#define MLHIP_CURVE_OPS(C)                                                                                    \
  sizeof(Fp<C>), sizeof(Affine<FpField<C>>), sizeof(Affine<Fp2Field<C>>), 12 * sizeof(Fp<C>), C::FR_BITS,     \
      MLHIP_TU_OPS(MLHIP_OP_ROW, C) host_sum<FpField<C>>, host_sum<Fp2Field<C>>
const CurveOps g_curves[] = {
    {MLHIP_CURVE_OPS(Bn254)},
    {MLHIP_CURVE_OPS(Bls381)},
    {MLHIP_CURVE_OPS(Bls377), mlhip_tu_g1_count_outside_subgroup_Bls377},
};
static_assert(MLHIP_CURVE_BN254 == 0 && MLHIP_CURVE_BLS12_381 == 1 && MLHIP_CURVE_BLS12_377 == 2, "g_curves is indexed by curve id");

std::mutex g_leases_mu;
std::vector<Lease> g_leases[MLHIP_MAX_DEVICES];  // idle leases per device

}  // namespace

namespace mlhip_rt {
const CurveOps* curve_ops(int curve) {
  return curve >= 0 && curve < (int)(sizeof(g_curves) / sizeof(g_curves[0])) ? &g_curves[curve] : nullptr;
}

int& call_device() { return g_device; }

int ensure_device() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return mlhip_rt::fail(MLHIP_ENODEVICE,
                          std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "count is 0"));
  int d = g_device_sel;
  const std::vector<int> l = device_list();
  if (g_devs_bad)
    return mlhip_rt::fail(MLHIP_EINVAL, "MLHIP_DEVICES is malformed (want \"all\" or a comma-separated list of device indices 0 .. 63)");
  if (d < 0) d = l.empty() ? 0 : l[0];
  if (d < 0 || d >= n || d >= MLHIP_MAX_DEVICES) return mlhip_rt::fail(MLHIP_EINVAL, "device index out of range");
  g_device = d;
  HIPCHK(hipSetDevice(d));
  return 0;
}

std::vector<int> spread_devices(size_t units, bool pairing) {
  if (g_device_sel >= 0) return {};
  std::vector<int> l = device_list();
  if (l.size() < 2 || units < (pairing ? g_multi_min_pairing : g_multi_min_msm)) return {};
  if (l.size() > units) l.resize(units);
  return l;
}

int run_on_devices(const std::vector<int>& devs, size_t n, const std::function<int(size_t, size_t, size_t)>& fn) {
  const size_t D = devs.size();
  std::vector<int> rcs(D, 0);
  std::vector<std::string> errs(D);
  auto body = [&](size_t r) {
    const int saved = g_device_sel;
    g_device_sel = devs[r];
    rcs[r] = fn(r, n * r / D, n * (r + 1) / D);
    if (rcs[r]) errs[r] = g_err;
    g_device_sel = saved;
  };
  std::vector<std::thread> th;
  th.reserve(D);
  for (size_t r = 1; r < D; r++) th.emplace_back(body, r);
  body(0);
  for (std::thread& t : th) t.join();
  for (size_t r = 0; r < D; r++)
    if (rcs[r]) return mlhip_rt::fail(rcs[r], "device " + std::to_string(devs[r]) + " (shard " + std::to_string(r) + "): " + errs[r]);
  return 0;
}

// ---- HostCall: the leased stream and scratch arena of one host-buffer call (mlhip_rt.h) ----------------------------------
HostCall::HostCall() : device(g_device) {
  {
    std::lock_guard<std::mutex> lk(g_leases_mu);
    std::vector<Lease>& idle = g_leases[device];
    if (!idle.empty()) {
      l = idle.back();
      idle.pop_back();
    }
  }
  if (!l.st && hipStreamCreateWithFlags(&l.st, hipStreamNonBlocking) != hipSuccess) {
    l.st = nullptr;
    rc = mlhip_rt::fail(MLHIP_EHIP, "hipStreamCreate failed");
  }
}
HostCall::~HostCall() {
  if (!l.st) return;
  (void)hipStreamSynchronize(l.st);  // nothing of this call is left in flight when the caller gets its buffers back
  std::lock_guard<std::mutex> lk(g_leases_mu);
  g_leases[device].push_back(l);
}
void HostCall::reserve(size_t bytes) {
  if (rc) return;
  bytes += 8 * 256;  // alignment slack for up to 8 buffers
  if (bytes <= l.cap) return;
  if (l.arena) (void)hipFree(l.arena);  // idle lease: nothing of ours is in flight
  l.arena = nullptr;
  l.cap = 0;
  const size_t want = bytes + bytes / 4;
  if (hipMalloc((void**)&l.arena, want) != hipSuccess) {
    (void)hipGetLastError();
    l.arena = nullptr;
    rc = mlhip_rt::fail(MLHIP_ENOMEM, "hipMalloc of the call's scratch failed");
    return;
  }
  l.cap = want;
}
void* HostCall::dev(size_t bytes) {
  if (rc) return nullptr;
  const size_t start = (used + 255) & ~(size_t)255;
  if (start + bytes > l.cap) {
    rc = mlhip_rt::fail(MLHIP_EINVAL, "internal: scratch arena overrun");
    return nullptr;
  }
  used = start + bytes;
  return l.arena + start;
}
void* HostCall::up(const void* src, size_t bytes) {
  void* p = dev(bytes);
  if (p && bytes && hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, l.st) != hipSuccess)
    rc = mlhip_rt::fail(MLHIP_EHIP, "hipMemcpy H2D failed");
  return rc ? nullptr : p;
}
int HostCall::down(void* dst, const void* dsrc, size_t bytes) {
  if (rc) return rc;
  hipError_t e = hipMemcpyAsync(dst, dsrc, bytes, hipMemcpyDeviceToHost, l.st);
  if (e == hipSuccess) e = hipStreamSynchronize(l.st);
  if (e != hipSuccess) rc = mlhip_rt::fail(MLHIP_EHIP, std::string("hipMemcpy D2H: ") + hipGetErrorString(e));
  return rc;
}

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// ---- host worker threads (the per-window half of an MSM's host tail) ----------------------------------------------------
// One small pool per process, started on first use and never joined (a Go process loads the library for its lifetime;
// the workers sleep on a condition variable between calls, after a short spin so that back-to-back MSMs do not pay a
// futex wake-up each).  One call at a time owns the pool; a second caller arriving meanwhile does its own jobs.
// A call never waits for a worker longer than the job would take the caller itself: jobs are pure functions of a blob
// the call COPIES into the (reference-counted) job record, so the caller can run a job a worker has claimed but not
// finished a second time and take whichever result is there first -- a worker that the scheduler parked behind a
// spinning thread for a timeslice (seen: 6 ms, once in 200 MSMs) costs nothing, and a worker that wakes up late only
// ever touches the record, never the caller's memory.
namespace {
struct HostJob {
  void (*fn)(const void*, int, void*);
  int njobs = 0;
  size_t out_stride = 0;
  std::vector<unsigned char> in, out_worker, out_caller;
  std::atomic<int> next{0};
  std::atomic<int> state[64];  // 0 not started, 1 claimed by a worker, 2 worker's result valid, 3 caller's result valid
};
struct HostPool {
  std::mutex owner;  // held by the call that is using the workers
  std::mutex mu;
  std::condition_variable cv;
  std::atomic<unsigned long> gen{0};
  std::shared_ptr<HostJob> job;  // guarded by mu
  int workers = 0;
  int spin = 2000;  // pause iterations a worker spins for the next job before it sleeps (host_pool_start)
};
HostPool* g_host_pool = nullptr;
std::once_flag g_host_pool_once;

void host_worker(HostPool* pool) {
  unsigned long seen = 0;
  for (;;) {
    // spin for a few tens of microseconds (a job is often followed by another one at once), then sleep
    bool fresh = false;
    for (int i = 0; i < pool->spin && !fresh; i++) {
      fresh = pool->gen.load(std::memory_order_acquire) != seen;
      if (!fresh) __builtin_ia32_pause();
    }
    std::shared_ptr<HostJob> j;
    {
      std::unique_lock<std::mutex> lk(pool->mu);
      pool->cv.wait(lk, [&] { return pool->gen.load(std::memory_order_relaxed) != seen; });
      seen = pool->gen.load(std::memory_order_relaxed);
      j = pool->job;
    }
    if (!j) continue;
    for (;;) {
      const int k = j->next.fetch_add(1, std::memory_order_relaxed);
      if (k >= j->njobs) break;
      int expect = 0;
      if (!j->state[k].compare_exchange_strong(expect, 1, std::memory_order_acq_rel)) continue;
      j->fn(j->in.data(), k, j->out_worker.data() + (size_t)k * j->out_stride);
      expect = 1;
      (void)j->state[k].compare_exchange_strong(expect, 2, std::memory_order_acq_rel);  // lost: the caller redid it
    }
  }
}

// Pool size: MLHIP_HOST_THREADS (threads per call incl. the caller) or, by default, what this PROCESS may use -- the
// affinity mask, not the machine's core count -- divided among the ranks that share the host (LOCAL_WORLD_SIZE, set by
// torch.distributed.run: `bench.py --gpus 8` is 8 processes on one host, each with its own pool, beside torch's threads):
// min(8, share) for a lone process, min(8, share / 2) when several ranks share the host, and the workers then spin a
// tenth as long before they sleep (a spinning worker of one rank is a core another rank's tail cannot have).
void host_pool_start() {
  int total = 0;
  if (const char* e = getenv("MLHIP_HOST_THREADS")) total = atoi(e);
  int local_world = 1;
  if (const char* e = getenv("LOCAL_WORLD_SIZE")) local_world = atoi(e) > 1 ? atoi(e) : 1;
  if (total <= 0) {
    int cores = 0;
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof(set), &set) == 0) cores = CPU_COUNT(&set);
    if (cores <= 0) cores = (int)std::thread::hardware_concurrency();
    if (cores <= 0) cores = 1;
    int share = cores / local_world;
    if (local_world > 1) share /= 2;
    total = share >= 8 ? 8 : (share > 0 ? share : 1);
  }
  if (total > 64) total = 64;
  HostPool* pool = new HostPool;  // never freed: the workers outlive every static destructor
  pool->workers = total - 1;
  pool->spin = local_world > 1 ? 200 : 2000;
  for (int i = 0; i < pool->workers; i++) {
    std::thread t(host_worker, pool);
    (void)pthread_setname_np(t.native_handle(), "mlhip-host");  // tests count them (tests/test_dist_gpu.py)
    t.detach();
  }
  g_host_pool = pool;
}
}  // namespace

void host_parallel(int njobs, void (*fn)(const void*, int, void*), const void* in, size_t in_bytes, void* out, size_t out_stride) {
  std::call_once(g_host_pool_once, host_pool_start);
  HostPool* pool = g_host_pool;
  std::unique_lock<std::mutex> own(pool->owner, std::try_to_lock);
  if (njobs < 2 || njobs > 64 || pool->workers == 0 || !own.owns_lock()) {
    for (int k = 0; k < njobs; k++) fn(in, k, (unsigned char*)out + (size_t)k * out_stride);
    return;
  }
  auto j = std::make_shared<HostJob>();
  j->fn = fn;
  j->njobs = njobs;
  j->out_stride = out_stride;
  j->in.assign((const unsigned char*)in, (const unsigned char*)in + in_bytes);
  j->out_worker.resize((size_t)njobs * out_stride);
  j->out_caller.resize((size_t)njobs * out_stride);
  for (int k = 0; k < njobs; k++) j->state[k].store(0, std::memory_order_relaxed);
  {
    std::lock_guard<std::mutex> lk(pool->mu);
    pool->job = j;
    pool->gen.fetch_add(1, std::memory_order_release);
  }
  pool->cv.notify_all();
  // the caller takes jobs from the top end, the workers from the bottom
  for (int k = njobs - 1; k >= 0; k--) {
    int st = j->state[k].load(std::memory_order_acquire);
    if (st == 0) {
      int expect = 0;
      if (j->state[k].compare_exchange_strong(expect, 3, std::memory_order_acq_rel)) {
        // claimed and (below) computed by the caller; nobody else looks at out_caller before the call returns
        fn(j->in.data(), k, j->out_caller.data() + (size_t)k * out_stride);
        continue;
      }
      st = expect;
    }
    if (st == 1) {
      // a worker is on it: give it about the time of one job, then do the job here as well
      for (int spin = 0; spin < 400 && j->state[k].load(std::memory_order_acquire) == 1; spin++) __builtin_ia32_pause();
      if (j->state[k].load(std::memory_order_acquire) == 1) {
        fn(j->in.data(), k, j->out_caller.data() + (size_t)k * out_stride);
        int expect = 1;
        (void)j->state[k].compare_exchange_strong(expect, 3, std::memory_order_acq_rel);  // lost: the worker's is there
      }
    }
  }
  for (int k = 0; k < njobs; k++) {
    const int st = j->state[k].load(std::memory_order_acquire);
    const unsigned char* src = (st == 2 ? j->out_worker.data() : j->out_caller.data()) + (size_t)k * out_stride;
    memcpy((unsigned char*)out + (size_t)k * out_stride, src, out_stride);
  }
}
}  // namespace mlhip_rt

extern "C" {

// 104 = round 4; bit 16 set in the test build (MLHIP_BUILD_ALT=1: the second implementations are compiled in)
int mlhip_version(void) { return 105 | (kBuildAlt ? 0x10000 : 0); }

const char* mlhip_last_error(void) { return g_err.c_str(); }

int mlhip_device_count(int* count) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) n = 0;
  if (count) *count = n;
  return 0;
}

int mlhip_set_device(int device) {
  if (device < -1 || device >= MLHIP_MAX_DEVICES) return mlhip_rt::fail(MLHIP_EINVAL, "device index: -1 (unpin) or 0 .. 63");
  g_device_sel = device;
  return 0;
}

int mlhip_init(const int* devices, int n_devices) {
  if (n_devices < 0 || n_devices > 64 || (n_devices > 0 && !devices))
    return mlhip_rt::fail(MLHIP_EINVAL, "device list: 0 .. 64 entries");
  std::vector<int> l;
  if (n_devices == 0) {
    parse_device_list("all", l);
  } else {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) count = 0;  // no device here: the first compute call reports it
    for (int i = 0; i < n_devices; i++) {
      if (devices[i] < 0 || devices[i] >= MLHIP_MAX_DEVICES || (count > 0 && devices[i] >= count))
        return mlhip_rt::fail(MLHIP_EINVAL, "device list: index out of range (0 .. min(63, device count - 1))");
      l.push_back(devices[i]);
    }
  }
  (void)device_list();  // the environment's thresholds are read once, before the list is replaced
  std::lock_guard<std::mutex> lk(g_devs_mu);
  g_devs = l;
  g_devs_bad = false;
  return 0;
}

int mlhip_get_devices(int* devices, int cap) {
  const std::vector<int> l = device_list();
  if (g_devs_bad) return mlhip_rt::fail(MLHIP_EINVAL, "MLHIP_DEVICES is malformed");
  for (size_t i = 0; i < l.size() && (int)i < cap; i++)
    if (devices) devices[i] = l[i];
  return (int)l.size();
}

int mlhip_shutdown(void) {
  mlhip_release_cache();
  std::lock_guard<std::mutex> lk(g_devs_mu);
  g_devs.clear();
  g_devs_set = false;  // the next call reads MLHIP_DEVICES again
  g_devs_bad = false;
  return 0;
}

int mlhip_sizes(int curve, size_t* fp, size_t* g1, size_t* g2, size_t* gt) {
  const CurveOps* ops = curve_ops(curve);
  if (!ops) return mlhip_rt::fail(MLHIP_EINVAL, "unknown curve id");
  if (fp) *fp = ops->fp;
  if (g1) *g1 = ops->g1;
  if (g2) *g2 = ops->g2;
  if (gt) *gt = ops->gt;
  return 0;
}

int mlhip_release_cache(void) {
  // the fixed-base tables of the batched scalar multiplication (one per curve and device; msm_scalar_mul.h)
  for (const CurveOps& c : g_curves) {
    c.release_cache();
    (void)c.miller_products(nullptr, -1, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr);  // the long products' scratch
  }
  release_plan_pool();
  // the idle leases (stream + scratch arena) of the other host-buffer entry points go too
  std::vector<Lease> leases;
  {
    std::lock_guard<std::mutex> lk(g_leases_mu);
    for (std::vector<Lease>& v : g_leases) {
      leases.insert(leases.end(), v.begin(), v.end());
      v.clear();
    }
  }
  for (Lease& l : leases) {
    if (l.arena) (void)hipFree(l.arena);
    if (l.st) (void)hipStreamDestroy(l.st);
  }
  return 0;
}

}  // extern "C"

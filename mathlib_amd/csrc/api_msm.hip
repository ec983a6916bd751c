// api_msm.hip -- the MSM entry points of include/mlhip.h: the pooled plans behind the host-buffer calls, the plan API, the
// batched MSMs and scalar multiplications, and the host sums.  Argument checking and dispatch; no kernels here.
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "ec.h"
#include "mlhip_rt.h"
#include "msm_body.h"

using namespace mlhip;
using namespace mlhip_rt;

namespace {
int ilog2(size_t v) {
  int l = 0;
  while (v > 1) {
    v >>= 1;
    l++;
  }
  return l;
}

// ---- a small pool of plans + device input buffers for the host-buffer entry points ---------------------------
// The reference's MultiScalarMul takes fresh host slices per call; creating and, above all, destroying a plan
// (a dozen hipFree's, ~2.5 ms) and the input buffers per call cost as much as the kernels of a 2^20-point MSM.
// Entries are reused across calls and threads when curve / group / window / device match and the size fits
// (capacity between n and 4 n).  At most POOL_MAX entries and POOL_MAX_BYTES of device memory stay allocated (an entry
// is ~0.6 GB at n = 2^20, ~10 GB at 2^24; many goroutines with small MSMs each find their own entry);
// MLHIP_NO_PLAN_CACHE=1 disables the pool, mlhip_release_cache() empties it.
struct PoolEntry {
  mlhip_msm_plan* plan = nullptr;
  void *d_pts = nullptr, *d_sc = nullptr;
  hipStream_t stream = nullptr;  // the entry's own non-blocking stream: concurrent callers do not meet on the null stream
  int curve = 0, group = 0, c = 0, device = 0;
  int bits = 0;  // the plan's scalar width (fr_bits: full width) -- a full-width plan never serves a short call, nor the reverse
  size_t cap = 0;
  bool busy = false, pooled = false;
  unsigned long stamp = 0;
  size_t bytes = 0;  // device memory the entry took (free memory before - after its creation)
};
constexpr size_t POOL_MAX = 16;  // per device
constexpr size_t POOL_MAX_BYTES = (size_t)32 << 30;  // per device
std::mutex g_pool_mu;
std::vector<PoolEntry*> g_pool;
unsigned long g_pool_clock = 0;

void pool_free_entry(PoolEntry* e) {
  (void)hipSetDevice(e->device);
  if (e->d_pts) (void)hipFree(e->d_pts);
  if (e->d_sc) (void)hipFree(e->d_sc);
  if (e->plan) mlhip_msm_plan_destroy(e->plan);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

PoolEntry* pool_acquire(int curve, int group, int c, int bits, size_t n, size_t ptsz, int& rc) {
  const char* off = getenv("MLHIP_NO_PLAN_CACHE");
  const bool use_pool = !(off && off[0] == '1');
  std::vector<PoolEntry*> victims;
  if (use_pool) {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (PoolEntry* e : g_pool)
      if (!e->busy && e->curve == curve && e->group == group && e->c == c && e->bits == bits && e->device == call_device() && e->cap >= n &&
          e->cap <= 4 * n) {
        e->busy = true;
        e->stamp = ++g_pool_clock;
        return e;
      }
    // evict this device's least recently used idle entries while its share of the pool is full or over budget
    for (;;) {
      size_t total = 0, count = 0;
      for (PoolEntry* e : g_pool)
        if (e->device == call_device()) {
          total += e->bytes;
          count++;
        }
      if (count < POOL_MAX && total <= POOL_MAX_BYTES) break;
      size_t vi = g_pool.size();
      for (size_t i = 0; i < g_pool.size(); i++)
        if (g_pool[i]->device == call_device() && !g_pool[i]->busy && (vi == g_pool.size() || g_pool[i]->stamp < g_pool[vi]->stamp)) vi = i;
      if (vi == g_pool.size()) break;  // everything is in use
      victims.push_back(g_pool[vi]);
      g_pool.erase(g_pool.begin() + vi);
    }
  }
  for (PoolEntry* v : victims) pool_free_entry(v);
  size_t free_before = 0, free_after = 0, total_mem = 0;
  (void)hipMemGetInfo(&free_before, &total_mem);
  PoolEntry* e = new PoolEntry();
  e->curve = curve;
  e->group = group;
  e->c = c;
  e->bits = bits;
  e->device = call_device();
  e->cap = n;
  e->busy = true;
  for (int attempt = 0;; attempt++) {
    rc = plan_create_ex(curve, group, n, c, 0, &e->plan, bits);
    if (!rc && (hipMalloc(&e->d_pts, n * ptsz) != hipSuccess || hipMalloc(&e->d_sc, n * 32) != hipSuccess))
      rc = mlhip_rt::fail(MLHIP_ENOMEM, "hipMalloc of MSM inputs failed");
    if (!rc || attempt == 1 || !use_pool) break;
    // out of device memory with idle entries pooled: give them back and try once more
    if (e->d_pts) (void)hipFree(e->d_pts);
    if (e->d_sc) (void)hipFree(e->d_sc);
    if (e->plan) mlhip_msm_plan_destroy(e->plan);
    e->d_pts = e->d_sc = nullptr;
    e->plan = nullptr;
    (void)hipGetLastError();
    mlhip_release_cache();
  }
  if (!rc && hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess)
    rc = mlhip_rt::fail(MLHIP_EHIP, "hipStreamCreate failed");
  if (rc) {
    pool_free_entry(e);
    return nullptr;
  }
  (void)hipMemGetInfo(&free_after, &total_mem);
  e->bytes = free_before > free_after ? free_before - free_after : 0;
  if (use_pool) {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    size_t count = 0;
    for (PoolEntry* o : g_pool) count += o->device == e->device;
    if (count < POOL_MAX) {
      e->pooled = true;
      e->stamp = ++g_pool_clock;
      g_pool.push_back(e);
    }
  }
  return e;
}

void pool_release(PoolEntry* e, bool failed) {
  if (e->pooled && failed) {  // do not keep an entry whose last run ended in an error
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (size_t i = 0; i < g_pool.size(); i++)
      if (g_pool[i] == e) {
        g_pool.erase(g_pool.begin() + i);
        break;
      }
    e->pooled = false;
  }
  if (!e->pooled) {
    pool_free_entry(e);
    return;
  }
  std::lock_guard<std::mutex> lk(g_pool_mu);
  e->busy = false;
}

// The window_c of an entry point that returns its result in host memory or over a device list: MLHIP_WINDOW_DEVICE_RESULT is
// not for it (checked before anything is written).
int reject_device_result(int window_c, const char* who) {
  if (window_c > 0 && (window_c & MLHIP_WINDOW_DEVICE_RESULT))
    return mlhip_rt::fail(MLHIP_EINVAL, std::string(who) + ": MLHIP_WINDOW_DEVICE_RESULT is for mlhip_msm_plan_create, mlhip_bases_create and mlhip_bases_create_device");
  return 0;
}

// MLHIP_GROUP_SUBGROUP(group) of include/mlhip.h taken apart (mlhip_scalar_mul / _device only): true and the plain group
// for the two flagged values, otherwise false and `group` as it came -- so every other value is rejected as before.
bool take_subgroup_promise(int& group) {
  if (group != MLHIP_GROUP_SUBGROUP(MLHIP_GROUP_G1) && group != MLHIP_GROUP_SUBGROUP(MLHIP_GROUP_G2)) return false;
  group &= 0xFF;
  return true;
}

// MLHIP_CURVE_SUBGROUP_POINTS(curve_id) of include/mlhip.h taken apart (mlhip_msm_batch / _device only): true and the plain
// curve id for the three flagged values, otherwise false and `curve` as it came -- so every other value is unknown as before.
bool take_subgroup_points_promise(int& curve) {
  if (curve < MLHIP_CURVE_SUBGROUP_POINTS(0) || curve > MLHIP_CURVE_SUBGROUP_POINTS(2)) return false;
  curve &= 0xFF;
  return true;
}

// A launch on `st`: remembered for the finish of a device-result plan, whose previous finish may still be queued on
// ANOTHER stream -- the new stream then waits for it on the device (the slot, d_out and the sort buffers are being read).
int plan_begin_on(mlhip_msm_plan* p, hipStream_t st) {
  p->pending_stream = st;
  if (p->device_result && p->done_queued && p->done_stream != st) HIPCHK(hipStreamWaitEvent(st, p->done, 0));
  return 0;
}

// the unfinished work of a device-result plan (nothing to wait for on a host-result plan: its finish has waited)
void plan_wait_done(mlhip_msm_plan* p) {
  if (p->device_result && p->done_queued) (void)hipEventSynchronize(p->done);
}

// the phase times of a device-result plan's last profiled finish, read once its work is done (plan_finish reads them in the
// call itself for a host-result plan); [5] is the tail kernel's time
int plan_read_device_times(mlhip_msm_plan* p) {
  if (!p->device_result || !p->times_stale || p->pending) return 0;
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(hipEventSynchronize(p->done));
  p->times_stale = false;
  if (p->timed_n != 0 && p->tiles_timed >= 0)
    if (int rc_times = plan_read_phase_times(p)) return rc_times;
  HIPCHK(hipEventElapsedTime(&p->ms[5], p->ev_tail[0], p->ev_tail[1]));
  return 0;
}

// can this plan run the segment train (msm_plan.h: plan_stream_train)?  The condition stream_begin checks.
bool plan_can_stream(const mlhip_msm_plan* p) {
  return p->aux && p->d_points28;
}

// After a failed launch on `st`: `done` may never have been recorded, and what was queued may still read the caller's
// buffers.  Wait for every stream a launch queues work on -- `st` (sorts, accumulation, reduction, the copy of the partial
// sums), each plan's auxiliary stream (uploads, point conversion) and its sort-ahead stream -- and leave the k plans
// reusable.  The error text survives: none of these calls goes through fail().
void drain_failed_launch(mlhip_msm_plan* const* plans, int k, hipStream_t st) {
  (void)hipStreamSynchronize(st);
  for (int j = 0; j < k; j++)
    if (plans[j]->aux) (void)hipStreamSynchronize(plans[j]->aux);
  for (int j = 0; j < k; j++)
    if (plans[j]->sort_stream) (void)hipStreamSynchronize(plans[j]->sort_stream);
  (void)hipGetLastError();
  for (int j = 0; j < k; j++) {
    plans[j]->pending = false;
    plans[j]->upload_src = nullptr;
  }
}

// The G1 MSM and the G2 MSM of ONE scalar vector (BASELINE configs[3], a Groth16 prover's B-query): the train of the two
// plans -- every tile is sorted once, in the G1 plan, and accumulated twice.  h_* = nullptr: everything is already at the d_*
// pointers; else the caller's pageable memory, staged through d_*: the scalars and the G1 points of a tile travel on the G1
// plan's auxiliary stream, the G2 points on the G2 plan's, under the kernels of the tile before.
int plan_shared(mlhip_msm_plan* g1, mlhip_msm_plan* g2, void* d1, void* d2, void* dsc, const void* h1, const void* h2,
                const void* hsc, int mont, size_t n, hipStream_t st) {
  mlhip_msm_plan* ps[2] = {g1, g2};
  void* dp[2] = {d1, d2};
  const void* hp[2] = {h1, h2};
  int rc = 0;
  if (g1->c != g2->c || g1->W != g2->W || g1->M != g2->M || g1->bits != g2->bits)
    rc = mlhip_rt::fail(MLHIP_EINVAL, "the two plans of a shared-scalar MSM need the same window width and scalar width");
  // (plans over shifted-base tables belong to resident-bases handles: their shared-scalar MSM is a set's, mlhip_bases_set_create)
  else if (g1->fold || g2->fold)
    rc = mlhip_rt::fail(MLHIP_EINVAL, "shared-scalar MSM: plans with shifted-base tables are not supported");
  else
    rc = curve_ops(g1->curve)->plan_train(ps, dp, hp, 2, dsc, hsc, mont, n, shared_segments(hsc != nullptr, n), false, st);
  if (rc) drain_failed_launch(ps, 2, st);
  return rc;
}

// ---- mlhip_g1_sum / mlhip_g2_sum: host loop or device route (point_sum.h) ------------------------------------------------
// Smallest n that goes to the device, per group: the smallest measured size (a power of two) from which the device route,
// upload included, is ahead of the host loop by more than 4 % at every larger size on all three curves: at 2^12 G1 is a
// tie (0.96 .. 1.08x), G2 2.5x ahead (tools/perf_point_sum.py, profiles/point_sum_ab.txt).  MLHIP_SUM_DEVICE_MIN=n overrides both: 0 = never,
// 1 = always.  Far above the handful of per-device partials the multi-GPU combine adds, which must not touch a device.
constexpr size_t SUM_DEVICE_MIN_G1 = (size_t)1 << 14, SUM_DEVICE_MIN_G2 = (size_t)1 << 12;

// does this sum take the device route?  False below the threshold without a single HIP call; at or above it, false when
// the thread has no usable device (the host loop serves every size: these two entry points never need a GPU).
bool sum_on_device(int group, size_t n) {
  size_t min_n = group == MLHIP_GROUP_G1 ? SUM_DEVICE_MIN_G1 : SUM_DEVICE_MIN_G2;
  if (const char* e = getenv("MLHIP_SUM_DEVICE_MIN")) {
    char* end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (end != e) min_n = (size_t)v;
  }
  if (min_n == 0 || n == 0 || n < min_n) return false;
  return ensure_device() == 0;
}

// upload, pass 0, sum passes, download of one point -- on a leased stream; n >= 1, ensure_device() has succeeded
int device_group_sum(const CurveOps* ops, int group, const void* pts, size_t n, void* out) {
  const size_t ptsz = ops->point_size(group);
  HostCall hc;
  hc.reserve(n * ptsz + ptsz);
  void* dp = hc.up(pts, n * ptsz);
  void* dout = hc.dev(ptsz);
  if (hc.rc) return hc.rc;
  int rc = ops->point_sum(group, dp, n, dout, hc.l.st);
  if (rc) return rc;
  return hc.down(out, dout, ptsz);
}

}  // namespace

namespace mlhip_rt {
// measured optimum on one MI355X (tools/sweep_window.py, profiles/r02_sweep_window.txt).  With the balanced window
// layout (msm_body.h: msm_win_layout) every width splits the scalar evenly, so the mid sizes no longer have to jump
// from 8 to 16: 13-14 bits win from 2^11 to 2^15 points (2^14: 0.81 ms instead of 1.11), 16 from 2^16 on.  For large n on
// the curves whose 254 / 255 scalar bits fit 15 windows of 17 bits (BLS12-377, BN254) one window less is one addition
// per scalar less (BLS12-377 2^22: 12.5 ms instead of 13.5); BLS12-381's 256 bits need 16 windows either way.
// Round 4 (profiles/r04_sweep_window.txt, the same sweep on this round's kernels): 10 bits from 2^10 to 2^11 points
// (0.47 / 0.49 ms against 0.50 at c = 8 / 0.53 at c = 13), and for BN254 (254-bit order, 10-limb field: its reduction weighs
// more against its additions) 15 bits from 2^16 to 2^17 points (0.505 / 0.587 ms against 0.554 / 0.617 at c = 16) -- not for
// BLS12-377, whose 253 bits also fit 17 windows of 15: 0.93 / 1.14 ms against 0.88 / 1.00 at c = 16.
int pick_window(size_t n, int fr_bits) {
  if (n <= 128) return 4;
  if (n <= 512) return 8;
  if (n <= 2048) return 10;
  if (n <= 8192) return 13;
  if (n <= 32768) return 14;
  if (n < ((size_t)1 << 18) && fr_bits == 254) return 15;
  if (n >= ((size_t)1 << 22) && msm_num_windows(fr_bits, 17) < msm_num_windows(fr_bits, 16)) return 17;
  return 16;
}

// The width for n scalars of `bits` bits (short-scalar plans: mlhip_msm_plan_create_bits, mlhip_msm_bits).  Full width is
// pick_window itself.  Below it the starting rule is pick_window's width for the size, which the plan then normalises to
// c' = ceil((bits + 1) / W) (msm_body.h: msm_effective_c): the same number of windows, fewer buckets each.  That rule is the
// measured optimum for small inputs only (tools/perf_msm_bits.py --sweep, profiles/msm_bits_ab.txt: G1 on BLS12-381 and
// BN254 from 2^12 to 2^22 points, G2 on BLS12-381 up to 2^18, at 32 / 64 / 128 bits).  With few windows the buckets are few
// and their chains of dependent additions long -- 2^20 points, 64 bits, 5 windows of 13 bits: 2.9 ms of accumulation, where
// 4 windows of 17 bits take 0.76 (and 0.32 instead of 0.13 ms of reduction) -- so from a size that grows with the number of
// windows the pick is 17 bits: fewer, fuller windows, 2^16 buckets each, still on the two-level sort.  Measured crossovers,
// by W17 = ceil((bits + 1) / 17):  G1  W17 <= 2: 2^16 points, <= 4: 2^17, <= 8: 2^18;  G2 (its reduction of a 17-bit window
// costs 1.6 ms against 0.6 at 13 bits)  W17 <= 2: 2^17, <= 8: 2^19 -- the G2 sizes above 2^18 are extrapolated, not measured.
// The wide pick is taken only where its windows come out 16 or 17 bits wide and there are at most the 8 of the widest
// measured width (128 bits); other widths keep the starting rule.
int pick_window_bits(size_t n, int bits, int fr_bits, int group) {
  const int c = pick_window(n, fr_bits);
  if (bits >= fr_bits) return c;
  const int start = std::max(4, msm_effective_c(bits, c));
  const int w17 = msm_num_windows(bits, 17), wide = msm_effective_c(bits, 17);
  if (wide < 16 || wide <= start || w17 > 8) return start;
  int lg_min;
  if (group == MLHIP_GROUP_G2)
    lg_min = w17 <= 2 ? 17 : 19;
  else
    lg_min = w17 <= 2 ? 16 : w17 <= 4 ? 17 : 18;
  return n >= ((size_t)1 << lg_min) ? wide : start;
}

// normalised scalar width: 0 or >= fr_bits (up to 256) = fr_bits; -1 = out of range
int scalar_width(int scalar_bits, int fr_bits) {
  if (scalar_bits < 0 || scalar_bits > 256) return -1;
  return (scalar_bits == 0 || scalar_bits >= fr_bits) ? fr_bits : scalar_bits;
}

// MLHIP_WINDOW_BITS(window_c, scalar_bits) of include/mlhip.h taken apart: the window width in the low 8 bits, the scalar
// width above them (0 = full width; the macro's 0x3FF for an out-of-range width, and anything else above 256, comes out as
// -1, which scalar_width rejects).  A plain window_c is its own packed form.
void unpack_window(int packed, int& window_c, int& scalar_bits) {
  if (packed < 0) {  // (never a packed value: the window check reports it)
    window_c = packed;
    scalar_bits = 0;
    return;
  }
  window_c = packed & 0xFF;
  scalar_bits = packed >> 8;
  if (scalar_bits > 256) scalar_bits = -1;
}

// fold_tile != 0: a plan over shifted-base tables (msm_fold.h, mlhip_internal.h) -- window_c is the digit width, the
// 2^(c-1) buckets all digits share are cut into groups of at most 2^15 for the reduction; the table itself is built by
// mlhip_tu_plan_fold_build_* (mlhip_bases_create).
// device_result: the plan leaves its result in device memory (include/mlhip.h, "device results"; msm_tail.h)
int plan_create_ex(int curve, int group, size_t max_n, int window_c, size_t fold_tile, mlhip_msm_plan** out, int scalar_bits,
                   bool device_result) {
  if (!out) return mlhip_rt::fail(MLHIP_EINVAL, "null plan pointer");
  *out = nullptr;
  const CurveOps* ops = curve_ops(curve);
  if (!ops) return mlhip_rt::fail(MLHIP_EINVAL, "unknown curve id");
  if (!ops->point_size(group)) return mlhip_rt::fail(MLHIP_EINVAL, "group must be 1 (G1) or 2 (G2)");
  if (max_n == 0 || max_n > ((size_t)1 << 27)) return mlhip_rt::fail(MLHIP_EINVAL, "max_n out of range (1 .. 2^27)");
  // (shifted-base tables keep full width: the table rows are the bases shifted by the full-width digit offsets)
  const int bits = fold_tile ? ops->fr_bits : scalar_width(scalar_bits, ops->fr_bits);
  if (bits < 0) return mlhip_rt::fail(MLHIP_EINVAL, "scalar_bits out of range (0 .. 256)");
  if (window_c == 0) window_c = pick_window_bits(max_n, bits, ops->fr_bits, group);
  if (window_c < 4 || window_c > 20) return mlhip_rt::fail(MLHIP_EINVAL, "window_c out of range (4 .. 20)");
  // a short plan's W = ceil((bits + 1) / c) windows need c' = ceil((bits + 1) / W) bits each: the plan's width is c'
  // (never below 4, the smallest width the reduction's chunks of 8 buckets take: a few bits only; W stays the same, since
  // ceil(B / 4) lies between ceil(B / c) and ceil(B / c'))
  if (bits < ops->fr_bits) window_c = std::max(4, msm_effective_c(bits, window_c));
  const int digits = msm_num_windows(bits, window_c);
  // sorted-entry offsets, cursors and scans are 32-bit: W * max_n entries must be addressable
  if (!fold_tile && (size_t)digits * max_n > 0xFFFFFFFFull)
    return mlhip_rt::fail(MLHIP_EINVAL, "window_c too small for max_n: W * max_n entries exceed 2^32 - 1");
  if (fold_tile) {
    // an entry = table row index (below Wd fold_tile) | sign: 31 bits + 1; the tiles of one MSM are its segments
    if ((size_t)digits * fold_tile > ((size_t)1 << 30)) return mlhip_rt::fail(MLHIP_EINVAL, "shifted-base tables: tile too long");
    // the sort's per-block bin counts are 16-bit and a block of 1024 scalars may put all its 1024 Wd entries into one bin
    if ((size_t)digits * 1024 >= 65536) return mlhip_rt::fail(MLHIP_EINVAL, "shifted-base tables: digit width below 5 bits");
    if ((max_n + fold_tile - 1) / fold_tile > MLHIP_MAX_SEGMENTS) return mlhip_rt::fail(MLHIP_EINVAL, "shifted-base tables: too many tiles");
  }
  int rc = ensure_device();
  if (rc) return rc;
  mlhip_msm_plan* p = new mlhip_msm_plan();
  p->curve = curve;
  p->group = group;
  p->device = call_device();
  p->c = window_c;
  p->bits = bits;
  p->Wd = digits;
  p->max_n = max_n;
  p->device_result = device_result;
  if (fold_tile) {
    p->fold = 1;
    p->fold_tile = fold_tile;
    const uint32_t nbuckets = 1u << (window_c - 1);
    p->M = nbuckets < 32768u ? nbuckets : 32768u;
    p->W = (int)(nbuckets / p->M);
  } else {
    p->W = digits;
    p->M = 1u << (window_c - 1);
  }
  // buckets per level-1 reduction chunk: 16 for G1 (the quad-lane kernels are bound by work, and a longer chunk
  // halves the second level), 8 for tiny windows
  // (and for small bucket sets, where the chunk pass is a dependent chain rather than work: 2^12 points, c = 13:
  // reduction 0.25 -> 0.22 ms)
  // G2 (carry-free lane-pair reduction): 16 as well -- BLS12-381: reduction 1.43 -> 1.31 ms at c = 16
  p->lgL = (p->M >= 256 && (size_t)p->W * p->M >= ((size_t)1 << 17)) ? 4 : 3;
  if (const char* e = getenv("MLHIP_CHUNK_LOG2")) {
    int v = atoi(e);
    if (v >= 1 && v <= 6 && (1u << v) <= p->M) p->lgL = v;
  }
  p->L = 1 << p->lgL;
  p->T = p->M / p->L;
  p->nb = ilog2(p->T);
  p->nsel = 4 + p->nb;  // two half-sums of W0, two of A, nb bit-masked sums
  rc = ops->plan_alloc(p);
  if (!rc && p->fold && (p->lists.sort_low <= 0 || !p->reduce28))
    rc = mlhip_rt::fail(MLHIP_EINVAL, "shifted-base tables need the two-level sort and the carry-free kernels");
  if (rc) {
    mlhip_msm_plan_destroy(p);
    return rc;
  }
  *out = p;
  return 0;
}

// Room for the twisted Edwards form of the points (168-byte Niels triples instead of 112-byte rows) in a plan that may take
// that path; called when the SRS promise is made, with nothing in flight on the plan.  A failed allocation is not an error:
// the plan keeps (or gets back) the smaller buffer and stays on the Weierstrass kernels (plan_use_edwards checks the size).
void plan_reserve_edwards(mlhip_msm_plan* p) {
  if (!p->points28_elem_ed || p->points28_elem >= p->points28_elem_ed || !p->d_points28 || p->fold) return;
  const char* e = getenv("MLHIP_EDWARDS");
  if (e && e[0] == '0') return;
  (void)hipSetDevice(p->device);
  if (p->aux) (void)hipStreamSynchronize(p->aux);
  void* bigger = nullptr;
  if (hipMalloc(&bigger, p->max_n * p->points28_elem_ed) != hipSuccess) {
    (void)hipGetLastError();
    return;
  }
  (void)hipFree(p->d_points28);
  p->d_points28 = bigger;
  p->points28_elem = p->points28_elem_ed;
  p->conv_src = nullptr;
}

// Number of segments a host-buffer MSM is streamed in (msm_segments.h; 1 = one upload, one pass)
int stream_segments(int group, size_t n, const mlhip_msm_plan* plan) {
  return mlhip::stream_segments(plan->aux && plan->d_points28, group == MLHIP_GROUP_G1, n);
}

// the train of one plan (msm_plan.h: plan_stream_train, k = 1): a host-buffer MSM streamed in `segments` >= 2 segments
int plan_stream(mlhip_msm_plan* p, void* d_pts, void* d_sc, const void* points, const void* scalars, int mont, size_t n,
                int segments, hipStream_t st) {
  int rc = curve_ops(p->curve)->plan_train(&p, &d_pts, &points, 1, d_sc, scalars, mont, n, segments, true, st);
  if (rc) drain_failed_launch(&p, 1, st);  // (copies from the caller's buffers may still be queued)
  return rc;
}

// a class of a set of resident-bases handles (api_bases.hip): the plan runs the segment train, on the two-level sort
bool plan_can_train(const mlhip_msm_plan* p) { return plan_can_stream(p) && p->lists.sort_low > 0; }

// k plans of one geometry over one scalar vector (msm_plan.h: plan_stream_train); h_scalars = nullptr: they are at d_scalars
int plan_train(mlhip_msm_plan* const* plans, void* const* d_points, int k, void* d_scalars, const void* h_scalars, int mont,
               size_t n, int segments, hipStream_t st) {
  for (int j = 0; j < k; j++)
    if (int rc_order = plan_begin_on(plans[j], st)) return rc_order;
  int rc = curve_ops(plans[0]->curve)->plan_train(plans, d_points, nullptr, k, d_scalars, h_scalars, mont, n, segments, true, st);
  if (rc) drain_failed_launch(plans, k, st);
  return rc;
}

int host_group_sum(int curve, int group, const void* pts, size_t n, void* out) {
  return group == MLHIP_GROUP_G1 ? mlhip_g1_sum(curve, pts, n, out) : mlhip_g2_sum(curve, pts, n, out);
}

// offsets of a batch: k + 1 nondecreasing host entries from 0 (k = 0: nothing to check)
int check_batch_offsets(const uint64_t* offsets, size_t k) {
  if (k == 0) return 0;
  if (!offsets) return mlhip_rt::fail(MLHIP_EINVAL, "msm batch: offsets is null");
  if (offsets[0] != 0) return mlhip_rt::fail(MLHIP_EINVAL, "msm batch: offsets[0] must be 0");
  for (size_t i = 0; i < k; i++)
    if (offsets[i + 1] < offsets[i]) return mlhip_rt::fail(MLHIP_EINVAL, "msm batch: offsets decrease");
  return 0;
}

// MLHIP_SCALARS_UNIT of include/mlhip.h taken apart (mlhip_msm_batch*, mlhip_bases_msm_batch* only): every scalar is 1, so
// there is no scalar array and no other bit of scalars_mont.  Without the flag nothing is checked: scalars_mont as it was.
int take_unit_scalars(int scalars_mont, const void* scalars, bool* unit) {
  *unit = (scalars_mont & MLHIP_SCALARS_UNIT) != 0;
  if (!*unit) return 0;
  if (scalars_mont != MLHIP_SCALARS_UNIT) return mlhip_rt::fail(MLHIP_EINVAL, "MLHIP_SCALARS_UNIT takes no other bit of scalars_mont");
  if (scalars) return mlhip_rt::fail(MLHIP_EINVAL, "unit scalars take no scalar array");
  return 0;
}


void release_plan_pool() {
  std::vector<PoolEntry*> idle;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (size_t i = 0; i < g_pool.size();)
      if (!g_pool[i]->busy) {
        idle.push_back(g_pool[i]);
        g_pool.erase(g_pool.begin() + i);
      } else {
        i++;
      }
  }
  for (PoolEntry* e : idle) pool_free_entry(e);
}
}  // namespace mlhip_rt

namespace {
int msm_host_buffers(int curve, int group, const void* points, const void* scalars, int mont, size_t n, int window_c,
                     void* out, int scalar_bits = 0);

// One MSM over several devices (reference semantics math.go:960-969 /
// driver/gurvy/bls12381/bls12-381.go:766-783): contiguous shards of the pairs, one host thread per device running the
// whole single-device pipeline on its shard (its own pooled plan, its own PCIe link), the per-device partial sums --
// already in host memory, where each shard's Horner tail leaves them -- added on the host.  The caller wants the sum in
// host memory, so there is nothing for a device-side collective to do here; the RCCL all-gather lives in the
// process-per-GPU form (mathlib_amd/dist.py), where every rank wants the total.
int msm_multi(const std::vector<int>& devs, int curve, int group, const void* points, const void* scalars, int mont,
              size_t n, int window_c, void* out, size_t ptsz) {
  std::vector<char> partial(devs.size() * ptsz);
  int rc = run_on_devices(devs, n, [&](size_t r, size_t lo, size_t hi) {
    return msm_host_buffers(curve, group, (const char*)points + lo * ptsz, (const char*)scalars + lo * 32, mont, hi - lo,
                            window_c, &partial[r * ptsz]);
  });
  if (rc) return rc;
  return host_group_sum(curve, group, partial.data(), devs.size(), out);
}

// scalar_bits: mlhip_msm_bits' width (0 = full: mlhip_msm_g1 / _g2).  A short call runs on the calling thread's first device.
int msm_host_buffers(int curve, int group, const void* points, const void* scalars, int mont, size_t n, int window_c,
                     void* out, int scalar_bits) {
  const CurveOps* ops = curve_ops(curve);
  if (!ops) return mlhip_rt::fail(MLHIP_EINVAL, "unknown curve id");
  if (!out) return mlhip_rt::fail(MLHIP_EINVAL, "null output pointer");
  const size_t ptsz = ops->point_size(group);
  if (!ptsz) return mlhip_rt::fail(MLHIP_EINVAL, "group must be 1 (G1) or 2 (G2)");
  const int bits = scalar_width(scalar_bits, ops->fr_bits);
  if (bits < 0) return mlhip_rt::fail(MLHIP_EINVAL, "scalar_bits out of range (0 .. 256)");
  if (n == 0) {
    // the point at infinity, as gnark's MultiExp gives for empty slices (and, via the dropped
    // error, for mismatched lengths: bls12-381.go:777)
    memset(out, 0, ptsz);
    return 0;
  }
  if (!points || !scalars) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  if (bits == ops->fr_bits) {
    const std::vector<int> devs = spread_devices(n, false);
    if (!devs.empty()) return msm_multi(devs, curve, group, points, scalars, mont, n, window_c, out, ptsz);
  }
  if (window_c == 0) window_c = pick_window_bits(n, bits, ops->fr_bits, group);
  int rc = ensure_device();
  if (rc) return rc;
  PoolEntry* e = pool_acquire(curve, group, window_c, bits, n, ptsz, rc);
  if (!e) return rc;
  const int segments = stream_segments(group, n, e->plan);
  do {
    if (segments > 1) {
      // large G1 MSMs: upload, sort and accumulate segment by segment, so the PCIe transfer hides under the kernels
      rc = plan_stream(e->plan, e->d_pts, e->d_sc, points, scalars, mont, n, segments, e->stream);
      if (!rc) rc = mlhip_msm_finish(e->plan, out, nullptr);
      break;
    }
    // scalars first (the sort needs only them); the points follow on the plan's auxiliary stream while the sort runs
    if (hipMemcpy(e->d_sc, scalars, n * 32, hipMemcpyHostToDevice) != hipSuccess) {
      rc = mlhip_rt::fail(MLHIP_EHIP, "hipMemcpy of MSM scalars failed");
      break;
    }
    e->plan->upload_src = points;
    e->plan->upload_bytes = n * ptsz;
    rc = mlhip_msm_run(e->plan, e->d_pts, e->d_sc, mont, n, e->stream, out, nullptr);
    e->plan->upload_src = nullptr;
  } while (0);
  pool_release(e, rc != 0);
  return rc;
}

}  // namespace

extern "C" {

int mlhip_msm_multi(int curve, int group, const int* devices, int n_devices, const void* points, const void* scalars,
                    int scalars_mont, size_t n, int window_c, void* out_affine) {
  const CurveOps* ops = curve_ops(curve);
  if (!ops) return mlhip_rt::fail(MLHIP_EINVAL, "unknown curve id");
  const size_t ptsz = ops->point_size(group);
  if (!ptsz) return mlhip_rt::fail(MLHIP_EINVAL, "group must be 1 (G1) or 2 (G2)");
  if (!out_affine) return mlhip_rt::fail(MLHIP_EINVAL, "null output pointer");
  if (n_devices < 1 || n_devices > 64 || !devices) return mlhip_rt::fail(MLHIP_EINVAL, "device list: 1 .. 64 entries");
  if (int rc_flag = reject_device_result(window_c, "mlhip_msm_multi")) return rc_flag;
  if (n == 0) {
    memset(out_affine, 0, ptsz);
    return 0;
  }
  if (!points || !scalars) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  std::vector<int> devs(devices, devices + n_devices);
  for (int d : devs)
    if (d < 0 || d >= MLHIP_MAX_DEVICES) return mlhip_rt::fail(MLHIP_EINVAL, "device list: index out of range (0 .. 63)");
  if (devs.size() > n) devs.resize(n);
  return msm_multi(devs, curve, group, points, scalars, scalars_mont, n, window_c, out_affine, ptsz);
}

int mlhip_msm_plan_create(int curve, int group, size_t max_n, int window_c, mlhip_msm_plan** out) {
  // (window_c may carry MLHIP_WINDOW_DEVICE_RESULT, taken off first, and a scalar width: MLHIP_WINDOW_BITS)
  const bool device_result = window_c > 0 && (window_c & MLHIP_WINDOW_DEVICE_RESULT);
  if (device_result) window_c &= ~MLHIP_WINDOW_DEVICE_RESULT;
  int c = 0, bits = 0;
  unpack_window(window_c, c, bits);
  return plan_create_ex(curve, group, max_n, c, 0, out, bits, device_result);
}

int mlhip_msm_plan_destroy(mlhip_msm_plan* p) {
  if (!p) return 0;
  (void)hipSetDevice(p->device);
  plan_wait_done(p);  // (a device-result plan: its last finish may still be running)
  entry_lists_free(&p->lists);
  void* ptrs[] = {p->d_result, p->d_biglist, p->d_buckets, p->d_A, p->d_W0, p->d_out, p->d_points28, p->d_state28, p->d_bigprefix, p->d_bigpart};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  if (p->h_out) (void)hipHostFree(p->h_out);
  for (int i = 0; i < 5; i++)
    if (p->ev[i]) (void)hipEventDestroy(p->ev[i]);
  for (int i = 0; i < 2; i++)
    if (p->ev_tail[i]) (void)hipEventDestroy(p->ev_tail[i]);
  if (p->done) (void)hipEventDestroy(p->done);
  if (p->ev_fork) (void)hipEventDestroy(p->ev_fork);
  if (p->ev_join) (void)hipEventDestroy(p->ev_join);
  for (hipEvent_t e : p->ev_seg)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : p->ev_seg_sc)
    if (e) (void)hipEventDestroy(e);
  for (auto& tile : p->ev_tile)
    for (hipEvent_t e : tile)
      if (e) (void)hipEventDestroy(e);
  if (p->aux) (void)hipStreamDestroy(p->aux);
  for (int i = 0; i < 2; i++) {
    if (p->sort_helper[i]) {
      entry_lists_free(p->sort_helper[i]);
      delete p->sort_helper[i];
    }
    if (p->ev_sorted[i]) (void)hipEventDestroy(p->ev_sorted[i]);
    if (p->ev_lists_free[i]) (void)hipEventDestroy(p->ev_lists_free[i]);
  }
  if (p->sort_stream) (void)hipStreamDestroy(p->sort_stream);
  delete p;
  return 0;
}

int mlhip_msm_launch(mlhip_msm_plan* p, const void* d_points, const void* d_scalars, int scalars_mont, size_t n,
                     void* stream) {
  if (!p) return mlhip_rt::fail(MLHIP_EINVAL, "null plan");
  if (p->pending) return mlhip_rt::fail(MLHIP_EINVAL, "plan already has a pending launch; call mlhip_msm_finish first");
  if (n > p->max_n) return mlhip_rt::fail(MLHIP_EINVAL, "n exceeds the plan's max_n");
  if (n && (!d_points || !d_scalars)) return mlhip_rt::fail(MLHIP_EINVAL, "null device pointer");
  HIPCHK(hipSetDevice(p->device));
  hipStream_t st = (hipStream_t)stream;
  if (int rc_order = plan_begin_on(p, st)) return rc_order;
  int rc = curve_ops(p->curve)->plan_launch(p, d_points, d_scalars, scalars_mont, n, st);
  if (rc) drain_failed_launch(&p, 1, st);  // (a later finish must not read h_out)
  return rc;
}

int mlhip_msm_launch_shared(mlhip_msm_plan* g1, mlhip_msm_plan* g2, const void* d_points_g1, const void* d_points_g2,
                            const void* d_scalars, int scalars_mont, size_t n, void* stream) {
  if (!g1 || !g2) return mlhip_rt::fail(MLHIP_EINVAL, "null plan");
  if (g1->group != MLHIP_GROUP_G1 || g2->group != MLHIP_GROUP_G2 || g1->curve != g2->curve || g1->device != g2->device)
    return mlhip_rt::fail(MLHIP_EINVAL, "shared-scalar MSM needs a G1 plan and a G2 plan of one curve on one device");
  if (g1->pending || g2->pending)
    return mlhip_rt::fail(MLHIP_EINVAL, "plan already has a pending launch; call mlhip_msm_finish first");
  if (n > g1->max_n || n > g2->max_n) return mlhip_rt::fail(MLHIP_EINVAL, "n exceeds a plan's max_n");
  if (n && (!d_points_g1 || !d_points_g2 || !d_scalars)) return mlhip_rt::fail(MLHIP_EINVAL, "null device pointer");
  const bool share = n != 0 && g1->c == g2->c && g1->W == g2->W && g1->bits == g2->bits && plan_can_stream(g1) && plan_can_stream(g2);
  if (!share) {  // nothing to share (or a plan on a second-implementation path): two ordinary launches, one after the other
    int rc = mlhip_msm_launch(g1, d_points_g1, d_scalars, scalars_mont, n, stream);
    if (rc) return rc;
    rc = mlhip_msm_launch(g2, d_points_g2, d_scalars, scalars_mont, n, stream);
    if (rc) {  // leave neither plan pending: the caller gets one error for the pair
      (void)hipStreamSynchronize((hipStream_t)stream);
      g1->pending = false;
    }
    return rc;
  }
  HIPCHK(hipSetDevice(g1->device));
  hipStream_t st = (hipStream_t)stream;
  void *p1 = const_cast<void*>(d_points_g1), *p2 = const_cast<void*>(d_points_g2), *sc = const_cast<void*>(d_scalars);
  if (int rc_order = plan_begin_on(g1, st)) return rc_order;
  if (int rc_order = plan_begin_on(g2, st)) return rc_order;
  return plan_shared(g1, g2, p1, p2, sc, nullptr, nullptr, nullptr, scalars_mont, n, st);
}

int mlhip_msm_g1g2(int curve, const void* points_g1, const void* points_g2, const void* scalars, int scalars_mont, size_t n,
                   int window_c, void* out_g1, void* out_g2) {
  const CurveOps* ops = curve_ops(curve);
  if (!ops) return mlhip_rt::fail(MLHIP_EINVAL, "unknown curve id");
  if (!out_g1 || !out_g2) return mlhip_rt::fail(MLHIP_EINVAL, "null output pointer");
  if (int rc_flag = reject_device_result(window_c, "mlhip_msm_g1g2")) return rc_flag;
  if (n == 0) {  // the points at infinity, as for mlhip_msm_g1 / _g2
    memset(out_g1, 0, ops->g1);
    memset(out_g2, 0, ops->g2);
    return 0;
  }
  if (!points_g1 || !points_g2 || !scalars) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  if (!spread_devices(n, false).empty()) {
    // spread over the device list: every device sorts its own shard anyway -- two sharded MSMs; the caller's window_c
    // travels as given (0 = each shard picks the width of its own size)
    int rc = msm_host_buffers(curve, MLHIP_GROUP_G1, points_g1, scalars, scalars_mont, n, window_c, out_g1);
    if (rc) return rc;
    return msm_host_buffers(curve, MLHIP_GROUP_G2, points_g2, scalars, scalars_mont, n, window_c, out_g2);
  }
  if (window_c == 0) window_c = pick_window(n, ops->fr_bits);
  int rc = ensure_device();
  if (rc) return rc;
  PoolEntry* e1 = pool_acquire(curve, MLHIP_GROUP_G1, window_c, ops->fr_bits, n, ops->g1, rc);
  if (!e1) return rc;
  PoolEntry* e2 = pool_acquire(curve, MLHIP_GROUP_G2, window_c, ops->fr_bits, n, ops->g2, rc);
  if (!e2) {
    pool_release(e1, false);
    return rc;
  }
  if (plan_can_stream(e1->plan) && plan_can_stream(e2->plan)) {
    rc = plan_shared(e1->plan, e2->plan, e1->d_pts, e2->d_pts, e1->d_sc, points_g1, points_g2, scalars, scalars_mont, n,
                        e1->stream);
    if (!rc) rc = mlhip_msm_finish(e1->plan, out_g1, nullptr);
    if (!rc) rc = mlhip_msm_finish(e2->plan, out_g2, nullptr);
    if (rc) {  // (a finish failed, or the launch, drained already: whatever is still queued reads the caller's buffers)
      mlhip_msm_plan* ps[2] = {e1->plan, e2->plan};
      drain_failed_launch(ps, 2, e1->stream);
    }
    pool_release(e2, rc != 0);
    pool_release(e1, rc != 0);
    return rc;
  }
  // a second-implementation path (MLHIP_ACC32=1 ...): nothing to share
  pool_release(e2, false);
  pool_release(e1, false);
  rc = msm_host_buffers(curve, MLHIP_GROUP_G1, points_g1, scalars, scalars_mont, n, window_c, out_g1);
  if (rc) return rc;
  return msm_host_buffers(curve, MLHIP_GROUP_G2, points_g2, scalars, scalars_mont, n, window_c, out_g2);
}

int mlhip_msm_finish(mlhip_msm_plan* p, void* out_affine, void* out_xyzz) {
  if (!p || !out_affine) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  HIPCHK(hipSetDevice(p->device));
  return curve_ops(p->curve)->plan_finish(p, out_affine, out_xyzz);
}

int mlhip_msm_run(mlhip_msm_plan* p, const void* d_points, const void* d_scalars, int scalars_mont, size_t n,
                  void* stream, void* out_affine, void* out_xyzz) {
  if (!p || !out_affine) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  int rc = mlhip_msm_launch(p, d_points, d_scalars, scalars_mont, n, stream);
  if (rc) return rc;
  return mlhip_msm_finish(p, out_affine, out_xyzz);
}

int mlhip_msm_plan_set_profiling(mlhip_msm_plan* p, int on) {
  if (!p) return mlhip_rt::fail(MLHIP_EINVAL, "null plan");
  p->profiling = on != 0;
  return 0;
}

int mlhip_msm_plan_assume_srs(mlhip_msm_plan* p, int on) {
  if (!p) return mlhip_rt::fail(MLHIP_EINVAL, "null plan");
  if (p->pending) return mlhip_rt::fail(MLHIP_EINVAL, "mlhip_msm_plan_assume_srs with a launch pending");
  if (p->fold) return mlhip_rt::fail(MLHIP_EINVAL, "mlhip_msm_plan_assume_srs: this plan reads the tables of a mlhip_bases handle");
  (void)hipSetDevice(p->device);
  plan_wait_done(p);  // (a device-result plan: unfinished work still reads the carry-free copy this call gives up)
  p->conv_src = nullptr;  // whatever carry-free copy the plan holds was made under the other promise
  p->points_static = p->trust_subgroup = on != 0;
  if (on) plan_reserve_edwards(p);
  return 0;
}

int mlhip_msm_plan_timings(mlhip_msm_plan* p, float* ms, int cap) {
  if (!p || !ms) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  if (int rc_times = plan_read_device_times(p)) return rc_times;
  int k = cap < 13 ? cap : 13;
  for (int i = 0; i < k && i < 6; i++) ms[i] = p->ms[i];
  if (k >= 7) ms[6] = p->tiles_timed > 0 ? (float)p->tiles_timed : 1.0f;
  if (k >= 8) ms[7] = (float)p->c;
  if (k >= 9) ms[8] = (float)p->Wd;
  if (k >= 10) ms[9] = p->last_ed ? 1.0f : 0.0f;
  if (k >= 11) ms[10] = p->fold ? 1.0f : 0.0f;
  if (k >= 12) ms[11] = (float)p->bits;  // the plan's scalar width (fr_bits: full width)
  if (k >= 13) ms[12] = p->device_result ? 1.0f : 0.0f;  // the result stays in device memory ("device results")
  return k;
}

int mlhip_msm_g1(int curve, const void* points, const void* scalars, int scalars_mont, size_t n, int window_c,
                 void* out_affine) {
  if (int rc_flag = reject_device_result(window_c, "mlhip_msm_g1")) return rc_flag;
  int c = 0, bits = 0;  // (window_c may carry a scalar width: MLHIP_WINDOW_BITS)
  unpack_window(window_c, c, bits);
  return msm_host_buffers(curve, MLHIP_GROUP_G1, points, scalars, scalars_mont, n, c, out_affine, bits);
}

int mlhip_msm_g2(int curve, const void* points, const void* scalars, int scalars_mont, size_t n, int window_c,
                 void* out_affine) {
  if (int rc_flag = reject_device_result(window_c, "mlhip_msm_g2")) return rc_flag;
  int c = 0, bits = 0;
  unpack_window(window_c, c, bits);
  return msm_host_buffers(curve, MLHIP_GROUP_G2, points, scalars, scalars_mont, n, c, out_affine, bits);
}

int mlhip_scalar_mul_device(int curve, int group, const void* d_points, size_t point_stride, const void* d_scalars,
                            int mont, size_t n, void* d_out, void* stream) {
  const bool subgroup = take_subgroup_promise(group);
  if (group != MLHIP_GROUP_G1 && group != MLHIP_GROUP_G2) return mlhip_rt::fail(MLHIP_EINVAL, "group must be 1 or 2");
  if (point_stride > 1) return mlhip_rt::fail(MLHIP_EINVAL, "point_stride must be 0 or 1");
  if (subgroup) {  // a promised call checks what it can before it asks for a device (n = 0: nothing to do, nothing read)
    if (n == 0) return 0;
    if (!curve_ops(curve)) return mlhip_rt::fail(MLHIP_EINVAL, "unknown curve id");
    if (!d_points || !d_scalars || !d_out) return mlhip_rt::fail(MLHIP_EINVAL, "null device pointer");
  }
  int rc = ensure_device();
  if (rc) return rc;
  if (n == 0) return 0;
  const CurveOps* ops = curve_ops(curve);
  if (!ops) return mlhip_rt::fail(MLHIP_EINVAL, "unknown curve id");
  return ops->scalar_mul(group, d_points, point_stride, d_scalars, mont, n, d_out, (hipStream_t)stream, subgroup);
}

int mlhip_scalar_mul(int curve, int group, const void* points, size_t point_stride, const void* scalars, int mont,
                     size_t n, void* out) {
  const int group_arg = group;  // (with the promise, as mlhip_scalar_mul_device takes it)
  const bool subgroup = take_subgroup_promise(group);
  if (subgroup && n == 0) return 0;
  const CurveOps* ops = curve_ops(curve);
  if (!ops) return mlhip_rt::fail(MLHIP_EINVAL, "unknown curve id");
  const size_t ptsz = ops->point_size(group);
  if (!ptsz) return mlhip_rt::fail(MLHIP_EINVAL, "group must be 1 or 2");
  if (n == 0) return 0;
  if (!points || !scalars || !out) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  if (subgroup && point_stride > 1) return mlhip_rt::fail(MLHIP_EINVAL, "point_stride must be 0 or 1");
  int rc = ensure_device();
  if (rc) return rc;
  const size_t npts = point_stride ? n : 1;
  HostCall hc;
  hc.reserve(npts * ptsz + n * 32 + n * ptsz);
  void* dp = hc.up(points, npts * ptsz);
  void* ds = hc.up(scalars, n * 32);
  void* dout = hc.dev(n * ptsz);
  if (hc.rc) return hc.rc;
  rc = mlhip_scalar_mul_device(curve, group_arg, dp, point_stride, ds, mont, n, dout, hc.l.st);
  if (rc) return rc;
  return hc.down(out, dout, n * ptsz);
}

int mlhip_msm_batch_device(int curve, int group, const void* d_points, const void* d_scalars, int scalars_mont,
                           const uint64_t* offsets, size_t k, void* d_out_affine, void* stream) {
  const bool subgroup = take_subgroup_points_promise(curve);
  bool unit = false;
  int rc = take_unit_scalars(scalars_mont, d_scalars, &unit);
  if (rc) return rc;
  const CurveOps* ops = curve_ops(curve);
  if (!ops) return mlhip_rt::fail(MLHIP_EINVAL, "unknown curve id");
  if (!ops->point_size(group)) return mlhip_rt::fail(MLHIP_EINVAL, "group must be 1 or 2");
  rc = check_batch_offsets(offsets, k);
  if (rc) return rc;
  if (k == 0) return 0;
  if (!d_out_affine || (offsets[k] && (!d_points || (!d_scalars && !unit)))) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  rc = ensure_device();
  if (rc) return rc;
  // plain sums (msm_sum_batch.h): no scalar to split, so the subgroup promise changes nothing
  if (unit) return ops->sum_batch(group, d_points, false, nullptr, offsets, k, d_out_affine, (hipStream_t)stream);
  return ops->msm_batch(group, d_points, d_scalars, scalars_mont, offsets, k, d_out_affine, (hipStream_t)stream, subgroup);
}

int mlhip_msm_batch(int curve, int group, const void* points, const void* scalars, int scalars_mont, const uint64_t* offsets,
                    size_t k, void* out_affine) {
  const int curve_arg = curve;  // (with the promise, as mlhip_msm_batch_device takes it)
  take_subgroup_points_promise(curve);
  bool unit = false;
  int rc = take_unit_scalars(scalars_mont, scalars, &unit);
  if (rc) return rc;
  const CurveOps* ops = curve_ops(curve);
  if (!ops) return mlhip_rt::fail(MLHIP_EINVAL, "unknown curve id");
  const size_t ptsz = ops->point_size(group);
  if (!ptsz) return mlhip_rt::fail(MLHIP_EINVAL, "group must be 1 or 2");
  rc = check_batch_offsets(offsets, k);
  if (rc) return rc;
  if (k == 0) return 0;
  const size_t n = offsets[k];
  if (!out_affine || (n && (!points || (!scalars && !unit)))) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  rc = ensure_device();
  if (rc) return rc;
  HostCall hc;
  hc.reserve(n * ptsz + (unit ? 0 : n * 32) + k * ptsz);
  void* dp = hc.up(points, n * ptsz);
  void* ds = unit ? nullptr : hc.up(scalars, n * 32);
  void* dout = hc.dev(k * ptsz);
  if (hc.rc) return hc.rc;
  rc = mlhip_msm_batch_device(curve_arg, group, dp, ds, scalars_mont, offsets, k, dout, hc.l.st);
  if (rc) return rc;
  return hc.down(out_affine, dout, k * ptsz);
}

int mlhip_g1_sum(int curve, const void* pts, size_t n, void* out) {
  if (!out || (n && !pts)) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  const CurveOps* ops = curve_ops(curve);
  if (!ops) return mlhip_rt::fail(MLHIP_EINVAL, "unknown curve id");
  if (sum_on_device(MLHIP_GROUP_G1, n)) return device_group_sum(ops, MLHIP_GROUP_G1, pts, n, out);
  return ops->g1_sum(pts, n, out);
}

int mlhip_g2_sum(int curve, const void* pts, size_t n, void* out) {
  if (!out || (n && !pts)) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  const CurveOps* ops = curve_ops(curve);
  if (!ops) return mlhip_rt::fail(MLHIP_EINVAL, "unknown curve id");
  if (sum_on_device(MLHIP_GROUP_G2, n)) return device_group_sum(ops, MLHIP_GROUP_G2, pts, n, out);
  return ops->g2_sum(pts, n, out);
}

}  // extern "C"

// mlhip_rt.h -- what the host-only units of the C ABI share (rt.hip, api_msm.hip, api_bases.hip, api_pairing.hip,
// api_codec.hip): the calling thread's device, the sharding threads, the leased stream + scratch arena of a host-buffer
// call, and the few MSM-plan helpers the resident-bases handles use.  No kernels in any of them.
#pragma once
#include <functional>
#include <vector>

#include "mlhip_internal.h"

namespace mlhip_rt {
constexpr int MLHIP_MAX_DEVICES = 64;  // device indices 0 .. 63 (the per-device tables of rt.hip are indexed by them)

// ---- rt.hip ---------------------------------------------------------------------------------------------------------------
// Selects the device this thread's call runs on (mlhip_set_device, else the first of the process's list) and makes it
// current; call_device() is that device from then on.  The thread_local state itself lives in rt.hip.
int ensure_device();
int& call_device();
// Devices a call of `units` items issued by this thread is spread over: empty = stay on one device.
std::vector<int> spread_devices(size_t units, bool pairing);
// fn(shard, lo, hi) runs on one host thread per listed device, with that device selected for the thread: contiguous
// shards [n r / D, n (r + 1) / D).  A device may be listed more than once (two shards in flight on it).
int run_on_devices(const std::vector<int>& devs, size_t n, const std::function<int(size_t, size_t, size_t)>& fn);

// ---- one host-buffer call: a leased non-blocking stream with its own scratch arena ------------------------------
// hipMalloc / hipFree per call and the null stream would serialize concurrent callers (hipFree waits for the whole
// device).  Every host-buffer entry point leases a (stream, arena) pair from a small per-device free list (rt.hip):
// device buffers are bump-allocated from the arena (one hipMalloc, grown when a call needs more), copies and kernels
// go to the leased stream, and the call waits for that stream only.  (hipMallocAsync was tried first and gave
// intermittently wrong results on this runtime.)
struct Lease {
  hipStream_t st = nullptr;
  char* arena = nullptr;
  size_t cap = 0;
};
struct HostCall {
  int device;
  Lease l;
  size_t used = 0;
  int rc = 0;
  HostCall();   // leases on call_device()
  ~HostCall();  // waits for the stream: nothing of this call is left in flight when the caller gets its buffers back
  HostCall(const HostCall&) = delete;
  HostCall& operator=(const HostCall&) = delete;
  void reserve(size_t bytes);  // call once, before the first dev() / up(): the total number of device bytes this call needs
  void* dev(size_t bytes);
  void* up(const void* src, size_t bytes);
  int down(void* dst, const void* dsrc, size_t bytes);
};

// ---- api_msm.hip ----------------------------------------------------------------------------------------------------------
int pick_window(size_t n, int fr_bits);
// fold_tile != 0: a plan over shifted-base tables (msm_fold.h, mlhip_internal.h)
// scalar_bits: 0 or >= the curve's fr_bits = full width; 1 .. fr_bits - 1 = a short-scalar plan (ignored when fold_tile != 0)
// device_result: the plan leaves its result in device memory (include/mlhip.h, "device results")
int plan_create_ex(int curve, int group, size_t max_n, int window_c, size_t fold_tile, mlhip_msm_plan** out, int scalar_bits = 0,
                   bool device_result = false);
// the window width the library picks for n scalars of `bits` bits in `group` (bits == fr_bits: pick_window(n, fr_bits))
int pick_window_bits(size_t n, int bits, int fr_bits, int group = MLHIP_GROUP_G1);
void plan_reserve_edwards(mlhip_msm_plan* p);
// Number of segments a host-buffer MSM is streamed in (1 = one upload, one pass), and the segment train itself
int stream_segments(int group, size_t n, const mlhip_msm_plan* plan);
int plan_stream(mlhip_msm_plan* p, void* d_pts, void* d_sc, const void* points, const void* scalars, int mont, size_t n,
                int segments, hipStream_t st);
// a set of resident-bases handles: can the plan be a member of a class (msm_set.h), and the train of one class
bool plan_can_train(const mlhip_msm_plan* p);
int plan_train(mlhip_msm_plan* const* plans, void* const* d_points, int k, void* d_scalars, const void* h_scalars, int mont,
               size_t n, int segments, hipStream_t st);
int host_group_sum(int curve, int group, const void* pts, size_t n, void* out);
// offsets of a batch: k + 1 nondecreasing host entries from 0 (k = 0: nothing to check)
int check_batch_offsets(const uint64_t* offsets, size_t k);
// MLHIP_SCALARS_UNIT of include/mlhip.h taken apart (the four batch entry points only): *unit = the flag is set; nonzero: the
// flag beside other bits of scalars_mont, or beside a scalar array
int take_unit_scalars(int scalars_mont, const void* scalars, bool* unit);
void release_plan_pool();  // mlhip_release_cache: the idle pooled plans
}  // namespace mlhip_rt

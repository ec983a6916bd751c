// mlhip_internal.h -- shared declarations of libmlhip.so's translation units (one per curve and
// kernel family, so the build parallelises; see mathlib_amd/build.py).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>

#include "../../include/mlhip.h"

namespace mlhip_rt {
int fail(int code, const std::string& msg);
// out[j] = fn(in, j) for j = 0 .. njobs - 1 on the library's host worker threads and the calling thread; returns when
// all are there.  fn must be a pure function of the `in_bytes` bytes at `in` (the call copies them: a worker never touches
// the caller's memory) writing `out_stride` bytes.  The workers are started on first use (MLHIP_HOST_THREADS = threads per
// call incl. the caller, default min(8, cores); 1 = none); a call that finds them busy with another caller's jobs, or
// njobs < 2, computes everything itself, and a job a worker is slow with is computed by the caller as well (rt.hip).
// Used by the host tail of an MSM (msm_plan.h: host_tail): the per-window sums are independent of each other.
void host_parallel(int njobs, void (*fn)(const void*, int, void*), const void* in, size_t in_bytes, void* out, size_t out_stride);
}

#define HIPCHK(x)                                                                                             \
  do {                                                                                                        \
    hipError_t e_ = (x);                                                                                      \
    if (e_ != hipSuccess) return mlhip_rt::fail(MLHIP_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

#include "msm_segments.h"  // MLHIP_MAX_SEGMENTS, and how an MSM is cut into segments / tiles
#include "msm_set.h"       // ... and how the members of a set of resident-bases handles share their sorts

// MLHIP_BUILD_ALT=1 (python -m mathlib_amd.build --alt -> libmlhip_alt.so): the test build.  It also contains the second
// implementations the parity tests compare the default kernels with -- boundary-form (32-bit limb) bucket accumulation and
// reduction, the one-point-per-lane reduction, G2 buckets split by coordinate, one-lane / saturated-limb pairing and G2.Mul
// kernels -- behind their MLHIP_* switches (include/mlhip.h, "2nd impl").  The product library is built without it: those
// kernels are not instantiated, their switches are ignored, and mlhip_version() has bit 16 clear.
#ifndef MLHIP_BUILD_ALT
#define MLHIP_BUILD_ALT 0
#endif
constexpr bool kBuildAlt = MLHIP_BUILD_ALT != 0;
// an alternate-implementation switch: set to '1' AND compiled in
static inline bool mlhip_alt_switch(const char* name) {
  if (!kBuildAlt) return false;
  const char* e = getenv(name);
  return e && e[0] == '1';
}

// The entry lists of one sort: what launch_sort needs and what it leaves for the accumulation (msm_plan.h).  A plan owns one
// (`lists`); a sort-ahead record is another of the plan's geometry (sort_ahead_prepare), and the later plans of a
// shared-scalar train read the first plan's.  entry_lists_alloc (msm_plan.h) fills it, entry_lists_free empties it.
struct MsmEntryLists {
  // the sort geometry, as the owning plan's fields of the same names (msm_plan.h: plan_entry_lists)
  int c = 0, bits = 0, W = 0, Wd = 0, fold = 0;
  uint32_t M = 0;
  size_t fold_tile = 0;
  size_t cap = 0;  // scalars one sort may cover
  int device = 0;
  uint32_t *d_digits = nullptr, *d_sorted = nullptr, *d_zero = nullptr, *d_offsets = nullptr;
  int sort_low = 0, sort_idx_bits = 0;  // two-level sort: fine bits per coarse bin (0 = legacy path)
  uint32_t sort_nb = 0;
  uint32_t *d_coarse_count = nullptr, *d_coarse_cursor = nullptr, *d_coarse_off = nullptr;
  uint16_t* d_blockhist = nullptr;  // per-block coarse histograms (k_coarse_hist -> k_coarse_scatter)
  uint32_t *d_order = nullptr, *d_hist = nullptr, *d_tilesums = nullptr;
  // views into d_zero, which is zeroed ahead of every sort.  d_bigcount is written by the ACCUMULATION of a tile, always
  // through the accumulating plan's own lists, whoever sorted the tile
  uint32_t *d_counts = nullptr, *d_cursor = nullptr, *d_bigcount = nullptr;
  size_t zero_bytes = 0;
  uint32_t* d_binprefix = nullptr;  // coarse bins sorted by several workgroups: slice prefix
};

// gives back whatever entry_lists_alloc got, a half-filled record included
inline void entry_lists_free(MsmEntryLists* l) {
  (void)hipSetDevice(l->device);
  void* ptrs[] = {l->d_digits, l->d_sorted,   l->d_zero,       l->d_offsets,   l->d_order,
                  l->d_hist,   l->d_tilesums, l->d_coarse_off, l->d_blockhist, l->d_binprefix};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  *l = MsmEntryLists();
}

struct mlhip_msm_plan {
  int curve, group, device, c, W, L, lgL, nb, nsel;
  size_t max_n;
  uint32_t M, T;
  // the scalar width the window layout covers (bits + 1 bits in Wd windows): the curve's fr_bits, or less for a plan made by
  // mlhip_msm_plan_create_bits, whose kernels mask every canonical scalar to its low `bits` bits (msm_body.h: fr_mask_bits)
  int bits = 0;
  // Shifted-base tables (msm_fold.h; resident bases only).  Wd = digits per scalar.  A plain plan has one bucket set per
  // digit position: Wd == W windows of M = 2^(c-1) buckets.  A FOLDED plan (fold != 0) has ONE set of 2^(c-1) buckets for
  // all Wd digits -- digit j of scalar i adds row (j, i) = 2^off(j) P_i of the table (off(j) = first bit of digit j) instead of P_i -- cut into W groups of
  // M consecutive buckets for the reduction kernels; the host tail then has lg M doublings instead of one per scalar bit,
  // the reduction 2^(c-1) buckets instead of Wd 2^(c-1), and c can grow (fewer digits = fewer additions).
  // The table is tile-major: bases [k fold_tile, (k + 1) fold_tile) own rows [(k Wd + j) fold_tile + i_local], so that an
  // entry index (i_local + j fold_tile) stays below Wd fold_tile whatever the number of bases; a sorted segment of scalars
  // never crosses a tile.
  int Wd = 0, fold = 0;
  size_t fold_tile = 0, fold_n = 0;  // rows per digit block; bases tabulated
  size_t fold_rows = 0;              // rows allocated in d_points28 (tiles x Wd x fold_tile): carry-free rows or Niels triples
  // the W groups' sums are combined on the device into the sums of one window of W T chunks (msm_reduce.h: group_combine_body);
  // d_out / h_out then hold fold_nsel2 = 4 + nb + lg W more entries behind the W x nsel ones, and the host tail reads those
  int fold_nsel2 = 0;
  size_t pt_size, xyzz_size;
  MsmEntryLists lists;  // the plan's own sort buffers, for max_n scalars (a folded plan: one tile of its table)
  uint32_t* d_biglist = nullptr;
  void *d_buckets = nullptr, *d_A = nullptr, *d_W0 = nullptr, *d_out = nullptr;
  void* h_out = nullptr;
  uint32_t* d_bigprefix = nullptr;  // long buckets: slice counts (prefix) and slice sums
  void* d_bigpart = nullptr;
  void* d_points28 = nullptr;  // G1: the points in the carry-free 28-bit-limb form (ec28.h), rewritten every MSM
  // bytes per point d_points28 was allocated with, and what the twisted Edwards form (Niels triples, ed28.h) would need
  // (0: this curve / group has none).  A BLS12-377 G1 plan starts with the 112-byte Weierstrass rows and grows to 168 bytes
  // only when the caller makes the SRS promise (api_msm.hip: plan_reserve_edwards) -- at 2^24 points that is 0.9 GB not spent
  // on plans that never take the Edwards path
  size_t points28_elem = 0, points28_elem_ed = 0;
  bool profiling = false;
  // which reduction form launch_reduce picks (msm_reduce.h: "reduction forms")
  bool reduce_one_lane = false;  // LaneForm (test build)
  bool reduce28 = false;  // the reduction reads the carry-free bucket state (d_state28): Quad28Form / Pair28Form; else QuadForm / PairForm
  int red_block = 256;  // workgroup size of the quad forms' chunk kernels (MLHIP_RED_BLOCK)
  int acc_block = 64;  // workgroup size of the bucket-accumulation kernel (MLHIP_ACC_BLOCK)
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  hipEvent_t done = nullptr;
  hipStream_t aux = nullptr;  // the point conversion runs here, beside the sort kernels
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // host-buffer entry points: points still in host memory, uploaded on `aux` beside the sort (cleared per launch)
  const void* upload_src = nullptr;
  size_t upload_bytes = 0;
  // resident bases (mlhip_bases_*): the library owns the point buffer, so its carry-free copy is made once
  bool points_static = false;
  const void* conv_src = nullptr;
  size_t conv_n = 0;
  bool conv_ed = false;  // ... and it holds the twisted Edwards form (ed28.h) rather than the Weierstrass one
  // the caller vouches that every point handed to this plan lies in the prime-order subgroup (or is the point at infinity):
  // curves with C::HAS_EDWARDS may then sum their G1 buckets in twisted Edwards coordinates (mlhip_msm_plan_assume_srs)
  bool trust_subgroup = false;
  bool last_ed = false;  // the last launch summed its buckets in twisted Edwards coordinates (mlhip_msm_plan_timings [9])
  // streamed host-buffer MSMs (plan_stream_train): raw carry-free bucket accumulators between segments, one event per segment
  void* d_state28 = nullptr;
  hipEvent_t ev_seg[MLHIP_MAX_SEGMENTS] = {};
  hipEvent_t ev_seg_sc[MLHIP_MAX_SEGMENTS] = {};  // ... and one after the segment's SCALARS alone (the sort needs only them)
  // tiles of device-resident inputs under profiling: before the sort / after it / after the accumulation of each tile
  hipEvent_t ev_tile[MLHIP_MAX_SEGMENTS][3] = {};
  int tiles_timed = 0;  // > 0: the last launch was tiled and recorded ev_tile[0 .. tiles_timed)
  bool pending = false;
  size_t pending_n = 0;
  float ms[6] = {0, 0, 0, 0, 0, 0};
  // A device-result plan (include/mlhip.h, "device results"; msm_tail.h): mlhip_msm_finish queues the tail kernel behind the
  // pending launch, on its stream, and returns without waiting.  The kernel writes [affine | XYZZ] into d_result; the
  // caller's device pointers receive copies of it.  No h_out.  `done` is recorded by that finish: a launch on another
  // stream waits for it on the device, destroy / assume_srs / timings wait for it on the host.
  bool device_result = false;
  void* d_result = nullptr;
  hipStream_t pending_stream = nullptr;  // the stream of the pending launch (set by mlhip_msm_launch / _launch_shared)
  hipStream_t done_stream = nullptr;     // the stream `done` was last recorded on
  bool done_queued = false;              // ... and whether it ever was
  hipEvent_t ev_tail[2] = {nullptr, nullptr};  // around the tail kernel, under profiling: [5] of mlhip_msm_plan_timings
  bool times_stale = false;  // a profiled finish whose events mlhip_msm_plan_timings has not read yet
  size_t timed_n = 0;        // ... and its n (0: no phase events but the tail's)
  // tiles of device-resident inputs: the entry lists of tile s + 1 are sorted on `sort_stream`, into one of two further
  // records, while tile s accumulates (msm_plan.h: sort_ahead_*).  A record is registered here only once it is complete.
  MsmEntryLists* sort_helper[2] = {nullptr, nullptr};
  hipStream_t sort_stream = nullptr;
  hipEvent_t ev_sorted[2] = {nullptr, nullptr}, ev_lists_free[2] = {nullptr, nullptr};
};

// ms[0..4] of the last profiled launch from its phase events: digits / sort / accumulate / reduce / total.  Tiles
// (tiles_timed > 0): the digits are part of each tile's sort, and accumulate is the sum over the tiles' kernels.  The caller
// has waited for `done` and knows tiles_timed >= 0 (a streamed host-buffer MSM records no phase events); ms[5] is its own.
inline int plan_read_phase_times(mlhip_msm_plan* p) {
  if (p->tiles_timed > 0) {
    p->ms[0] = p->ms[1] = p->ms[2] = 0;
    for (int s = 0; s < p->tiles_timed; s++) {
      float a = 0, b = 0;
      HIPCHK(hipEventElapsedTime(&a, p->ev_tile[s][0], p->ev_tile[s][1]));
      HIPCHK(hipEventElapsedTime(&b, p->ev_tile[s][1], p->ev_tile[s][2]));
      p->ms[1] += a;
      p->ms[2] += b;
    }
    HIPCHK(hipEventElapsedTime(&p->ms[3], p->ev[3], p->ev[4]));
  } else {
    for (int i = 0; i < 4; i++) HIPCHK(hipEventElapsedTime(&p->ms[i], p->ev[i], p->ev[i + 1]));
  }
  HIPCHK(hipEventElapsedTime(&p->ms[4], p->ev[0], p->ev[4]));
  return 0;
}

// the per-base fixed-window tables of a mlhip_bases handle for mlhip_bases_msm_batch (msm_bases_batch.h): rows of bases
// [0, n_tabled) at width w, on the handle's device; freed by mlhip_bases_destroy
struct mlhip_bases_batch_tables {
  char* buf = nullptr;
  size_t n_tabled = 0;
  int w = 0;
};

// the device state of a mlhip_g2_prepared handle (pairing_prepared_kernels.h), on the handle's device; read-only once built,
// freed by mlhip_g2_prepared_destroy
struct mlhip_g2_prepared_tables {
  void* d_q = nullptr;       // the m affine points
  int32_t* d_t28 = nullptr;  // every line of every point in the carry-free form
  void* d_t32 = nullptr;     // ... and in the boundary form (test build only)
  uint32_t* d_inf = nullptr;  // [m]: the point is the point at infinity
  size_t m = 0;
};

// ---- the per-curve operations -------------------------------------------------------------------------------------------
// One line per operation: X(curve, result, name, (parameters)) declares mlhip_tu_<name>_<Curve> for the three curves, gives
// CurveOps its `name` member and fills that member's slot in the three rows of the table (rt.hip).  The bodies are written
// once, against MLHIP_TU_CURVE, in tu_msm.inc / tu_pairing.inc / tu_codec.inc; tu_<kind>_<curve>.hip instantiates them.
#define MLHIP_TU_OPS(X, C)                                                                                                \
  X(C, int, plan_alloc, (mlhip_msm_plan * p))                                                                             \
  X(C, int, plan_launch,                                                                                                  \
    (mlhip_msm_plan * p, const void* d_points, const void* d_scalars, int mont, size_t n, hipStream_t st))                \
  X(C, int, plan_finish, (mlhip_msm_plan * p, void* out_affine, void* out_xyzz))                                          \
  /* the segment train (msm_plan.h: plan_stream_train): k plans of one geometry, of either group, over one scalar vector; \
     h_points null, or per plan the host points its tiles upload (null: resident); `schedule`: stream_schedule may cut */   \
  X(C, int, plan_train,                                                                                                   \
    (mlhip_msm_plan* const* plans, void* const* d_points, const void* const* h_points, int k, void* d_scalars,            \
     const void* h_scalars, int mont, size_t n, int segments, bool schedule, hipStream_t st))                             \
  X(C, int, pairing,                                                                                                      \
    (int what, const void* d_g1, const void* d_g2, size_t ppp, size_t n, const void* d_in, void* d_out, hipStream_t st))  \
  X(C, int, fp_mul, (const void* d_a, const void* d_b, size_t n, int repeat, void* d_out, hipStream_t st))                \
  X(C, int, gt_mul, (const void* d_a, const void* d_b, size_t n, void* d_out, hipStream_t st))                            \
  X(C, int, gt_exp, (const void* d_in, const void* d_scalars, int mont, size_t n, void* d_out, hipStream_t st))           \
  /* the same for inputs the caller promises to lie in Gt (gt_exp_cyclo.h) */                                            \
  X(C, int, gt_exp_cyclo, (const void* d_in, const void* d_scalars, int mont, size_t n, void* d_out, hipStream_t st))     \
  /* Gt wire codec, membership test and inverse (gt_codec.h); d_decoded: null, or the values to zero where the test fails */ \
  X(C, int, gt_decode, (const void* d_wire, size_t n, int subgroup_check, void* d_out, void* d_status, hipStream_t st))   \
  X(C, int, gt_encode, (const void* d_in, size_t n, void* d_wire, hipStream_t st))                                        \
  X(C, int, gt_is_member, (const void* d_in, size_t n, void* d_status, void* d_decoded, hipStream_t st))                  \
  X(C, int, gt_inverse, (const void* d_in, size_t n, void* d_out, hipStream_t st))                                        \
  X(C, int, wire_codec,                                                                                                   \
    (int group, int encode, const void* d_in, size_t n, int compressed, int subgroup, void* d_out, void* d_status,        \
     hipStream_t st))                                                                                                     \
  X(C, int, scalar_mul,                                                                                                   \
    (int group, const void* d_points, size_t point_stride, const void* d_scalars, int mont, size_t n, void* d_out,        \
     hipStream_t st, bool subgroup))                                                                                      \
  X(C, int, plan_fold_build, (mlhip_msm_plan * p, const void* d_points, size_t n, hipStream_t st))                        \
  X(C, int, msm_batch,                                                                                                    \
    (int group, const void* d_points, const void* d_scalars, int mont, const uint64_t* offsets, size_t k, void* d_out,    \
     hipStream_t st, bool subgroup))                                                                                      \
  X(C, int, bases_batch,                                                                                                  \
    (int group, mlhip_bases_batch_tables* t, const void* d_pts, size_t n_bases, const void* d_scalars, int mont,          \
     const uint32_t* base_index, const uint64_t* offsets, size_t k, size_t need, void* d_out, hipStream_t st))            \
  /* d_out = the affine sum of the n >= 1 affine points at d_points (point_sum.h: mlhip_g1_sum / mlhip_g2_sum) */        \
  X(C, int, point_sum, (int group, const void* d_points, size_t n, void* d_out, hipStream_t st))                          \
  /* K plain sums (msm_sum_batch.h: the batch calls with MLHIP_SCALARS_UNIT): position i reads d_points[i], or, bases set,   \
     the handle's point base_index[i] / (base_index null) its position in the segment */                                 \
  X(C, int, sum_batch,                                                                                                    \
    (int group, const void* d_points, bool bases, const uint32_t* base_index, const uint64_t* offsets, size_t k,          \
     void* d_out, hipStream_t st))                                                                                        \
  /* what = -1: build t's tables from t->d_q ; 0 / 2: Miller loops / fused pairings of n products against them */         \
  X(C, int, g2_prepared,                                                                                                  \
    (mlhip_g2_prepared_tables * t, int what, const void* d_g1, const uint32_t* q_index, size_t ppp, size_t n,             \
     void* d_out, hipStream_t st))                                                                                        \
  /* n products of m > 4 pairs (pairing_products_run.h): t null = against the n m points d_g2, else against t's points by   \
     q_index; what 0 / 2 = Miller values / their final exponentiation, -1 = free the scratch (mlhip_release_cache) */      \
  X(C, int, miller_products,                                                                                              \
    (const mlhip_g2_prepared_tables* t, int what, const void* d_g1, const void* d_g2, const uint32_t* q_index, size_t m,  \
     size_t n, void* d_out, hipStream_t st))                                                                              \
  X(C, void, release_cache, (void))

#define MLHIP_OP_DECLARE(C, ret, name, params) ret mlhip_tu_##name##_##C params;
#define MLHIP_OP_MEMBER(C, ret, name, params) ret(*name) params;
#define MLHIP_OP_ROW(C, ret, name, params) mlhip_tu_##name##_##C,
MLHIP_TU_OPS(MLHIP_OP_DECLARE, Bn254)
MLHIP_TU_OPS(MLHIP_OP_DECLARE, Bls381)
MLHIP_TU_OPS(MLHIP_OP_DECLARE, Bls377)
// G1 points outside the prime-order subgroup (or off the curve) in an array of affine points: mlhip_bases_create's check
int mlhip_tu_g1_count_outside_subgroup_Bls377(const void* d_pts, size_t n, uint32_t* d_bad, hipStream_t st);

// mlhip_tu_<name>_<MLHIP_TU_CURVE>: the name a tu_*.inc body defines
#define MLHIP_TU_PASTE_(name, C) mlhip_tu_##name##_##C
#define MLHIP_TU_PASTE(name, C) MLHIP_TU_PASTE_(name, C)
#define MLHIP_TU_FN(name) MLHIP_TU_PASTE(name, MLHIP_TU_CURVE)

namespace mlhip_rt {
// what the API layer knows about a curve: plain static data, one row per curve id (rt.hip)
struct CurveOps {
  size_t fp, g1, g2, gt;  // bytes of an Fp element, an affine G1 / G2 point, a Gt value
  int fr_bits;
  MLHIP_TU_OPS(MLHIP_OP_MEMBER, )
  int (*g1_sum)(const void* pts, size_t n, void* out);  // host sums of n affine points (mlhip_g1_sum / mlhip_g2_sum)
  int (*g2_sum)(const void* pts, size_t n, void* out);
  int (*g1_count_outside_subgroup)(const void* d_pts, size_t n, uint32_t* d_bad, hipStream_t st);  // null except BLS12-377
  // bytes of an affine point of `group`; 0: the group is neither MLHIP_GROUP_G1 nor MLHIP_GROUP_G2
  size_t point_size(int group) const { return group == MLHIP_GROUP_G1 ? g1 : group == MLHIP_GROUP_G2 ? g2 : 0; }
};
const CurveOps* curve_ops(int curve);  // null: unknown curve id
}  // namespace mlhip_rt

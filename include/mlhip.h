/* mlhip.h -- C ABI of libmlhip.so: the MI355X (gfx950) backend for the data-parallel hot path of
 * IBM/mathlib (batched G1/G2 multi-scalar multiplication, Miller loop, final exponentiation).
 *
 * This is the boundary a Go `driver/hip` package binds through cgo (INTEGRATION.md shows the stub).
 * Every entry point replaces one call the reference's drivers make into gnark-crypto / kilic:
 *
 *   mlhip_msm_g1          driver/gurvy/bls12381/bls12-381.go:766-783 (G1Jac.MultiExp + FromJacobian),
 *                         driver/gurvy/bn254.go:232-245, driver/gurvy/bls12-377.go:229-242,
 *                         driver/kilic/bls12-381.go:247-254
 *   mlhip_msm_g2          additive (no G2 MSM in driver/math.go); semantics = sum of G2.Mul + Add,
 *                         driver/gurvy/bls12381/bls12-381.go:342-358
 *   mlhip_miller_loop     Pairing / Pairing2: bls12-381.go:448-464, bn254.go:247-263, bls12-377.go:244-260
 *   mlhip_final_exp       FExp: bls12-381.go:466-468, bn254.go:265-267, bls12-377.go:262-264
 *   mlhip_pairing_batch   FExp(Pairing(g2[i], g1[i])) element-wise (kilic's Pairing is this composition:
 *                         driver/kilic/bls12-381.go:260-267)
 *
 * Memory layout (in and out) is gnark-crypto's in-memory layout, so Go passes unsafe.Pointer(&slice[0])
 * with no conversion: Fp = k little-endian uint64 limbs in Montgomery form (k = 6 for BLS12-381/377,
 * 4 for BN254; evidence: driver/gurvy/custom.go:24-40, driver/kilic/custom.go:24-29); G1 affine = {X,Y};
 * G2 affine = {X.A0,X.A1,Y.A0,Y.A1}; infinity = all-zero; Gt = E12 {C0{B0{A0,A1},B1,B2},C1{..}}
 * (12 Fp); scalar = 4 uint64 limbs, either fr.Element (Montgomery, scalars_mont = 1) or a plain
 * little-endian integer (scalars_mont = 0; any 256-bit value, reduced mod r on the device the way
 * fr.Element.SetBigInt does for the reference's BaseZr scalars, driver/gurvy/bn254.go:239).
 *
 * Conventions: every function returns 0 on success and a negative MLHIP_E* code otherwise;
 * mlhip_last_error() gives the message for the calling thread.  The library is re-entrant
 * (perf_test.go:382-404 calls Curve methods from many goroutines); it keeps no caller pointer after
 * return.  There is NO CPU fallback: without a usable HIP device every compute entry point fails
 * with MLHIP_ENODEVICE (the Go shim panics, matching the reference's driver convention,
 * driver/gurvy/bn254.go:249-251).
 */
#ifndef MLHIP_H
#define MLHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the functions declared here with MLHIP_API are its whole dynamic
 * symbol table (tests/test_abi.py compares `nm -D --defined-only` with this header). */
#define MLHIP_API __attribute__((visibility("default")))

#define MLHIP_CURVE_BN254 0
#define MLHIP_CURVE_BLS12_381 1
#define MLHIP_CURVE_BLS12_377 2

#define MLHIP_OK 0
#define MLHIP_EINVAL (-1)    /* bad argument (unknown curve, window out of range, null pointer) */
#define MLHIP_ENODEVICE (-2) /* no usable HIP device */
#define MLHIP_EHIP (-3)      /* a HIP runtime call failed; see mlhip_last_error() */
#define MLHIP_ENOMEM (-4)

#define MLHIP_GROUP_G1 1
#define MLHIP_GROUP_G2 2

/* ---- library / device ---------------------------------------------------------------------- */
MLHIP_API int mlhip_version(void);
MLHIP_API const char* mlhip_last_error(void);
MLHIP_API int mlhip_device_count(int* count);
/* Pins the calling thread's subsequent calls to one device (-1 undoes it: the thread follows the process's device
 * list again, whose first entry -- device 0 when there is no list -- serves calls that are not spread).  Nothing
 * touches the GPU before the first compute call (the reference computes GenGt at package init, math.go:142-255:
 * importing the backend must not need a GPU). */
MLHIP_API int mlhip_set_device(int device);

/* ---- several devices in one process (one host thread per device, the ABI takes a device list) ------
 * mlhip_init sets the process's device list (n_devices = 0: every visible device; the environment variable
 * MLHIP_DEVICES="0,1,2,3" | "all" does the same without a call).  With two or more devices listed, the host-buffer
 * entry points a Go caller reaches through math.Curve.MultiScalarMul (math.go:960-969,
 * driver/gurvy/bls12381/bls12-381.go:766-783) -- mlhip_msm_g1 / mlhip_msm_g2 / mlhip_bases_create + mlhip_bases_msm
 * from MLHIP_MULTI_MIN pairs (default 2^21), and mlhip_miller_loop / mlhip_final_exp / mlhip_pairing_batch from
 * MLHIP_MULTI_MIN_PAIRINGS elements (default 2^17) -- cut the call into contiguous shards, one per listed device, each
 * run by its own host thread through the whole single-device pipeline (own pooled plan, own PCIe link); the
 * per-device partial sums (already in host memory, where each shard's host tail leaves them) are added on the host.
 * No device-side collective is involved: the caller wants the result in host memory.  (The process-per-GPU form,
 * mathlib_amd/dist.py, exchanges the partials with one RCCL all-gather because there every rank wants the total.)
 * Threads pinned with mlhip_set_device are never spread.  A device may be listed more than once.  Device indices are
 * 0 .. 63 and below the device count; anything else is MLHIP_EINVAL (mlhip_init, mlhip_set_device, the explicit
 * lists below), and a MLHIP_DEVICES value that does not parse makes every compute call and mlhip_get_devices fail
 * with MLHIP_EINVAL instead of silently running on device 0.
 * STATUS: spreading is opt-in (nothing is spread unless the caller lists two or more devices) and has so far run only
 * on lists that repeat device 0 of a one-GPU box (tests/test_multi_device.py); see DESIGN.md section 5. */
MLHIP_API int mlhip_init(const int* devices, int n_devices);
MLHIP_API int mlhip_get_devices(int* devices, int cap); /* returns the length of the list, or MLHIP_EINVAL (malformed MLHIP_DEVICES) */
/* frees every cached plan / arena and forgets the device list; the next call reads MLHIP_DEVICES again */
MLHIP_API int mlhip_shutdown(void);
/* The same MSM with an explicit device list, whatever its size (group: MLHIP_GROUP_G1 / _G2). */
MLHIP_API int mlhip_msm_multi(int curve, int group, const int* devices, int n_devices, const void* points, const void* scalars,
                    int scalars_mont, size_t n, int window_c, void* out_affine);

/* sizes in bytes for a curve: Fp element, G1 affine, G2 affine, Gt, scalar (always 32) */
MLHIP_API int mlhip_sizes(int curve, size_t* fp, size_t* g1, size_t* g2, size_t* gt);

/* ---- host-buffer entry points (what the cgo shim binds) ------------------------------------- */
/* out = sum_i [scalars[i]] points[i].  window_c = 0 picks a window from n; BASELINE config 2 uses 16.
 * n = 0 gives the point at infinity (the reference's MultiExp on empty slices).  Plans and input buffers are pooled
 * between calls (mlhip_release_cache below).  G1 calls of 2^19 pairs and more (G2: 2^18) are streamed over PCIe in
 * segments of 2^18 (2^17) pairs: upload of one segment under the kernels of the one before;
 * MLHIP_STREAM_SEGMENTS=K fixes the count, 0 = one pass.  Smaller calls upload the points beside the sort of the
 * scalars. */
MLHIP_API int mlhip_msm_g1(int curve, const void* points, const void* scalars, int scalars_mont, size_t n, int window_c,
                 void* out_affine);
MLHIP_API int mlhip_msm_g2(int curve, const void* points, const void* scalars, int scalars_mont, size_t n, int window_c,
                 void* out_affine);
/* out_g1 = sum_i [scalars[i]] points_g1[i] and out_g2 = sum_i [scalars[i]] points_g2[i] over ONE scalar vector
 * (additive: BASELINE configs[3]; in the reference's terms MultiScalarMul(a1, b), driver/gurvy/bls12381/bls12-381.go:766-783,
 * and the G2 sum of g2.Mul(b[i]), :342-358, over the same b): the scalars travel and are sorted once, both groups
 * accumulate from the same entry lists.  Same results as mlhip_msm_g1 + mlhip_msm_g2. */
MLHIP_API int mlhip_msm_g1g2(int curve, const void* points_g1, const void* points_g2, const void* scalars, int scalars_mont, size_t n,
                   int window_c, void* out_g1, void* out_g2);

/* out[k] = prod_{j < pairs_per_product} MillerLoop(g1[k*ppp + j], g2[k*ppp + j]); Pairing = 1, Pairing2 = 2.
 * pairs_per_product is 1 .. 4 as a plain number, or MLHIP_PRODUCT_PAIRS(m) for any m ("products of any length" below).
 * Pairs holding an infinity contribute 1.  NOT final-exponentiated: like gurvy's Pairing the value is only meaningful
 * after mlhip_final_exp. */
MLHIP_API int mlhip_miller_loop(int curve, const void* g1, const void* g2, size_t pairs_per_product, size_t n_products,
                      void* out_gt);
/* out[i] = in[i]^(k (p^12-1)/r), k = 3 (BLS12 curves) or 2x(6x^2+3x+1) (BN254): gnark's and kilic's value */
MLHIP_API int mlhip_final_exp(int curve, const void* in_gt, size_t n, void* out_gt);
/* out[i] = FExp(Pairing(g2[i], g1[i])) */
MLHIP_API int mlhip_pairing_batch(int curve, const void* g1, const void* g2, size_t n, void* out_gt);
/* out[i] = a[i] * b[i] in Gt (Gt.Mul, driver/gurvy/bls12381/bls12-381.go:417-419), element-wise over n */
MLHIP_API int mlhip_gt_mul(int curve, const void* a_gt, const void* b_gt, size_t n, void* out_gt);
/* out[i] = 1 / in[i] in Fp12 (Gt.Inverse, driver/gurvy/bls12381/bls12-381.go:413-415), element-wise over n: any Fp12 value, as
 * gnark's E12.Inverse, not only members of Gt; the inverse of 0 is 0.  curve_id is a MLHIP_CURVE_* value. */
MLHIP_API int mlhip_gt_inverse(int curve_id, const void* in_gt, size_t n, void* out_gt);

/* out[i] = in[i]^(scalars[i]) in Gt (Gt.Exp, driver/gurvy/bls12381/bls12-381.go:399-407), element-wise over n;
 * valid for any Gt value.  Scalars as for the MSM entry points. */
MLHIP_API int mlhip_gt_exp(int curve, const void* in_gt, const void* scalars, int scalars_mont, size_t n, void* out_gt);
/* out[i] = in[i]^(scalars[i]) for in[i] in Gt (the subgroup of order r): same bytes as mlhip_gt_exp on such inputs, in a
 * fraction of the time -- cyclotomic squarings and a split of the scalar over the Frobenius map.
 * The caller PROMISES membership (FExp outputs, GenGt, products / powers of members; 1 is a member); for a value that arrived
 * as bytes or from another party, mlhip_gt_is_member (or mlhip_gt_from_bytes with the check) earns the promise.  An input
 * outside Gt gives an undefined RESULT, never a fault.  curve_id is a MLHIP_CURVE_* value; scalars as for mlhip_gt_exp (scalars_mont, any
 * 256-bit value, reduced mod r). */
MLHIP_API int mlhip_gt_exp_cyclo(int curve_id, const void* in_gt, const void* scalars, int scalars_mont, size_t n, void* out_gt);
/* out = FExp( prod_i MillerLoop(g1[i], g2[i]) ): a multi-pairing product with ONE shared final exponentiation
 * (what a verifier computes before IsUnity: perf_test.go:254-259).  n Miller loops run one per lane, the
 * product is a log-depth tree of Gt multiplications on the device. */
MLHIP_API int mlhip_pairing_product(int curve, const void* g1, const void* g2, size_t n, void* out_gt);

/* ---- device-resident entry points (points / scalars already in HBM; resident SRS) ----------- */
typedef struct mlhip_msm_plan mlhip_msm_plan;
/* Workspace for MSMs of up to max_n points on the calling thread's device. */
MLHIP_API int mlhip_msm_plan_create(int curve, int group, size_t max_n, int window_c, mlhip_msm_plan** plan);
MLHIP_API int mlhip_msm_plan_destroy(mlhip_msm_plan* plan);
/* d_points / d_scalars are device pointers; stream is a hipStream_t (NULL = default stream).
 * out_affine is HOST memory; the call returns after the result is there.  When out_xyzz is non-NULL
 * the un-normalised partial sum (X,Y,ZZ,ZZZ) is written there too (multi-GPU combine): x = X/ZZ, y = Y/ZZZ is out_affine,
 * but the representation is not canonical -- two runs of one MSM can give different bytes for the same point.
 * (A device-result plan: see "device results" below -- both outputs are DEVICE pointers and the call returns once
 * everything is queued, in order on `stream`.) */
MLHIP_API int mlhip_msm_run(mlhip_msm_plan* plan, const void* d_points, const void* d_scalars, int scalars_mont, size_t n,
                  void* stream, void* out_affine, void* out_xyzz);
/* The same in two halves, so consecutive MSMs pipeline: mlhip_msm_launch enqueues the kernels and the
 * D2H of the window sums on `stream` and returns; mlhip_msm_finish waits for them and runs the O(1) host
 * tail.  With two plans on two streams the sort of MSM k+1 overlaps the bucket accumulation of MSM k and
 * the host tail of MSM k overlaps GPU work (a Groth16 prover issues 4-5 MSMs back to back).
 * (A device-result plan: see "device results" below -- mlhip_msm_finish queues the tail as a kernel and does not wait.) */
MLHIP_API int mlhip_msm_launch(mlhip_msm_plan* plan, const void* d_points, const void* d_scalars, int scalars_mont, size_t n,
                     void* stream);
MLHIP_API int mlhip_msm_finish(mlhip_msm_plan* plan, void* out_affine, void* out_xyzz);
/* The G1 MSM and the G2 MSM of ONE scalar vector (additive: BASELINE configs[3] "G1 + G2 MSM, shared scalars"; in the
 * reference's terms MultiScalarMul(a1, b) -- driver/gurvy/bls12381/bls12-381.go:766-783 -- and the G2 sum of
 * g2.Mul(b[i]) -- :342-358 -- over the same b).  Both plans: same curve, device and window width; the (window, bucket)
 * entry lists depend on the scalars only, so they are sorted once and both groups accumulate from them.  Finish each
 * plan with mlhip_msm_finish.  Plans that cannot share (different widths, a second-implementation path) run one after
 * the other with the same results. */
MLHIP_API int mlhip_msm_launch_shared(mlhip_msm_plan* g1_plan, mlhip_msm_plan* g2_plan, const void* d_points_g1,
                            const void* d_points_g2, const void* d_scalars, int scalars_mont, size_t n, void* stream);
/* Phase timings of the last run with profiling on (HIP events on the plan's stream), milliseconds:
 * [0] digits [1] sort (histogram scan + scatter) [2] bucket accumulation [3] bucket reduction
 * [4] device total [5] host tail [6] the number of tiles the accumulation ran in (device-resident inputs from 2^22 / 2^23
 * points on are accumulated tile by tile; [1] and [2] are then sums over the tiles' launches).  A streamed host-buffer
 * MSM (mlhip_msm_g1 and friends on a pooled plan) records no phase events: [0..5] are then 0.  [7] and [8] are not times:
 * the window width c the plan runs with (the library's pick when it was created with window_c = 0) and its number of
 * windows W; [9] is 1 when the last launch summed its buckets in twisted Edwards coordinates (a subgroup-trusted
 * BLS12-377 G1 plan or table with the SRS promise, mlhip_msm_plan_assume_srs), else 0; [10] is 1 when the plan reads the
 * shifted-base tables of a mlhip_bases handle ([8] is then the number of digits a scalar is cut into).  Returns the number of
 * values written (at most `cap`, at most 11).
 * (With cap >= 12 a twelfth value, with cap >= 13 a thirteenth: "short scalars" and "device results" below.) */
MLHIP_API int mlhip_msm_plan_set_profiling(mlhip_msm_plan* plan, int on);
/* The caller declares (on != 0) that this plan's points are a fixed SRS: (1) the point buffer at a given device address
 * holds the same points at every launch until the promise is taken back (the plan keeps its converted copy of them and
 * converts nothing on later launches), and (2) every point lies in the prime-order subgroup or is the point at infinity --
 * what gnark's SetBytes checks on the way in, and what an SRS is by construction.  The reference's MultiScalarMul
 * (driver/gurvy/bls12-377.go:229-242, gnark MultiExp) accepts any curve points in fresh slices, and so does a plan without
 * this promise.  With it, a BLS12-377 G1 plan sums its buckets in twisted Edwards coordinates (7 field products per
 * addition instead of 10; that addition law is complete on the subgroup only): same result bytes, less time.  On the other
 * curves and for G2 only (1) matters.  mlhip_bases_create makes the same promise for its own table after checking (2) on
 * the device.  A promise that does not hold gives an undefined RESULT, never a fault. */
MLHIP_API int mlhip_msm_plan_assume_srs(mlhip_msm_plan* plan, int on);
MLHIP_API int mlhip_msm_plan_timings(mlhip_msm_plan* plan, float* ms, int cap);

/* ---- short scalars: plans and a host-buffer call that know the scalar width --------------------------------------------
 * For callers whose scalars are short by construction (the 64- or 128-bit randomisers of a batch verifier, small weights,
 * bit-decomposed witnesses).
 *
 * Result.  out = sum_i [s_i'] P_i with s_i' = (s_i mod r) mod 2^scalar_bits: scalars_mont and unreduced 256-bit inputs are
 * handled as everywhere else, then the canonical value is masked to its low scalar_bits bits.  The result is therefore
 * defined for every input; a caller who keeps the promise s_i < 2^scalar_bits gets exactly mlhip_msm_g1's / _g2's bytes.
 *
 * How it is said.  The library's dynamic symbol table does not grow (the tests pin it): the width travels in the window_c
 * argument of the existing entry points -- mlhip_msm_plan_create, mlhip_msm_g1, mlhip_msm_g2 -- as
 * MLHIP_WINDOW_BITS(window_c, scalar_bits) below, and a plan reports it as a twelfth value, [11], of
 * mlhip_msm_plan_timings when cap >= 12 (the curve's fr_bits for a full-width plan; the call then returns 12, and with
 * cap <= 11 exactly what it returned before).  include/mlhip_bits.h wraps this in three inline functions for C, C++ and cgo
 * callers: mlhip_msm_plan_create_bits(curve_id, group, max_n, window_c, scalar_bits, &plan),
 * mlhip_msm_plan_scalar_bits(plan, &scalar_bits) and mlhip_msm_bits(curve_id, group, points, scalars, scalars_mont,
 * scalar_bits, n, window_c, out_affine); the names below mean those.  The packed value is taken apart in those three
 * entry points and nowhere else: every other one that takes a window_c (mlhip_msm_multi, mlhip_msm_g1g2,
 * mlhip_bases_create*) rejects it as it rejects any window_c above 20, and nothing inside the library calls the three.
 *
 * Range.  scalar_bits = 0, or any value from the curve's fr_bits (253 / 254 / 255) up to 256, means full width: the packed
 * window_c is then the plain one -- same geometry, same bytes, same code path (full width is the short path with the
 * width at fr_bits).  A negative value or one above 256 is MLHIP_EINVAL (the plan pointer is left NULL).  Otherwise
 * 1 .. fr_bits - 1.
 *
 * Geometry.  B = scalar_bits + 1 bits are covered (the spare bit absorbs the last signed-digit carry) by W = ceil(B / c)
 * windows; the plan's effective width is c' = ceil(B / W) <= c, with 2^(c'-1) buckets per window (B = 129, c = 16: 9 windows
 * of 15 / 14 bits and 2^14 buckets each; c' is never taken below 4).  ceil(B / c') = W again, so c' is simply the plan's
 * width: mlhip_msm_plan_timings [7] and [8] report c' and W.  Digits, sort, bucket arrays, reduction and the host tail all
 * scale with this W; W * max_n must stay below 2^32.  window_c = 0: the library picks from (n, scalar_bits, group) -- the
 * width it would pick for full-width scalars, or, from a size that grows with the number of windows, 17 bits: fewer, fuller
 * windows, whose buckets are many enough to keep the chip busy (api_msm.hip: pick_window_bits).
 *
 * A short plan runs through mlhip_msm_run / _launch / _launch_shared / _finish like any other (one pass, tiles, profiling,
 * mlhip_msm_plan_assume_srs, out_xyzz).  mlhip_msm_launch_shared shares one sort only between plans of the same curve,
 * width, window count AND scalar width; others run one after the other with the same results.  mlhip_msm_bits uses the
 * plan pool (a pooled full-width plan never serves a short call, nor the reverse), streams large inputs in segments like
 * mlhip_msm_g1, runs on the calling thread's first device (a short call is never spread over a device list), and gives the
 * point at infinity for n = 0.  Plans over the shifted-base tables of a mlhip_bases handle, mlhip_msm_batch*,
 * mlhip_scalar_mul* and the Gt exponentiations keep full width.
 * curve_id is a MLHIP_CURVE_* value (an unknown one is MLHIP_EINVAL, "unknown curve id").
 * Measured: profiles/msm_bits_ab.txt, DESIGN.md section 14 -- 2^20 BLS12-381 G1 points, scalars below 2^bits, short plan
 * against full-width plan: 0.656 / 0.707 / 0.833 of its time at 32 / 64 / 128 bits (the additions count alone would predict
 * 0.125 / 0.25 / 0.5: the full-width plan already skips zero digits). */
#define MLHIP_WINDOW_BITS(window_c, scalar_bits) \
  ((int)((window_c) < 0 || (window_c) > 255 ? 0xFF : (window_c)) | (int)(((scalar_bits) < 0 || (scalar_bits) > 256 ? 0x3FF : (scalar_bits)) << 8))

/* ---- device results: plans and handles that leave their result in device memory --------------------------------------------
 * For callers who hold device pointers and a stream and want to keep both: a batch verifier that hands sum r_k A_k and
 * sum r_k B_k straight to mlhip_pairing_prepared_device, a prover with several MSMs in flight on one plan's stream, K results
 * gathered in one device array and fetched with one copy.  The launch half of an MSM never waited for the host; with this
 * flavour the tail (per-window sums, the Horner pass over the windows, the conversion to an affine point) is a kernel too
 * (msm_tail.h), and nothing waits.
 *
 * How it is said.  The symbol table does not grow: a flag travels in window_c,
 *     MLHIP_WINDOW_DEVICE_RESULT, OR-ed onto a plain window_c or onto MLHIP_WINDOW_BITS(window_c, scalar_bits),
 * and is ACCEPTED by exactly three entry points -- mlhip_msm_plan_create, mlhip_bases_create, mlhip_bases_create_device --
 * which take it off and read the rest of window_c as before (the handles still reject a scalar-width packing, as a width
 * above 20; mlhip_bases_create with the flag never spreads over a device list).  mlhip_msm_g1, mlhip_msm_g2, mlhip_msm_g1g2,
 * mlhip_msm_multi and mlhip_bases_create_multi -- results in host memory or over a device list -- REJECT it with
 * MLHIP_EINVAL: no handle, nothing written.  mlhip_msm_plan_timings reports the flavour as a thirteenth value, [12], when
 * cap >= 13 (1 for a device-result plan, else 0; the call then returns 13, and with cap <= 12 exactly what it returned
 * before).  include/mlhip_device_result.h wraps this in inline functions for C, C++ and cgo:
 * mlhip_msm_plan_create_device_result(curve_id, group, max_n, window_c, scalar_bits, &plan),
 * mlhip_msm_plan_is_device_result(plan, &on), mlhip_msm_run_device(plan, d_points, d_scalars, scalars_mont, n, stream,
 * d_out_affine, d_out_xyzz), mlhip_msm_finish_device(plan, d_out_affine, d_out_xyzz),
 * mlhip_bases_create_device_result(curve_id, group, points, points_on_device, n, window_c, &bases) and
 * mlhip_bases_msm_to_device(bases, d_scalars, scalars_mont, n, stream, d_out_affine).
 *
 * A device-result plan.  mlhip_msm_launch and mlhip_msm_launch_shared are what they are for every plan (in a shared launch
 * each plan may be of either flavour and is finished in its own way).  mlhip_msm_finish(plan, d_out_affine, d_out_xyzz):
 * both are DEVICE pointers on the plan's device, d_out_xyzz may be NULL; the call queues the tail kernel on the stream of the
 * pending launch, queues the delivery of the result, records the plan's completion event and returns WITHOUT waiting.
 * mlhip_msm_run is launch + finish: asynchronous and in order on `stream`, like every other _device form.  The kernel writes the
 * affine point and the XYZZ value into a slot the plan owns; delivery is one asynchronous copy of that slot per requested
 * output, on the same stream -- no kernel of the library dereferences the caller's output pointers.  n = 0 takes the same
 * path: the all-zero affine point (and the XYZZ form of infinity) arrive in stream order.  The bytes are those of a
 * host-result plan of the same geometry.
 *
 * Ordering.  Work on one stream is in order.  A launch on a plan whose previous work was queued on ANOTHER stream makes the
 * new stream wait for that work on the device (never the host).  mlhip_msm_plan_destroy, mlhip_msm_plan_assume_srs and -- with
 * profiling on -- mlhip_msm_plan_timings wait for the plan's unfinished work on the host; [5] is then the time of the tail
 * kernel.  The caller's inputs may be rewritten, and the output read, by work queued behind the call on the same stream.
 * One MSM at a time per plan, as always: launch, finish, launch.  Capture into a hipGraph is neither promised nor tested.
 *
 * A device-result handle (mlhip_bases_create / _create_device with the flag; mlhip_bases_plan shows [12] = 1).
 * mlhip_bases_msm_device(bases, d_scalars, scalars_mont, n, stream, d_out_affine) is asynchronous and in order on `stream`
 * with a DEVICE output; n = 0 writes the all-zero point in stream order; the handle's lock covers the enqueue only.
 * mlhip_bases_msm (host scalars, host result) on such a handle is MLHIP_EINVAL -- use mlhip_bases_msm_device.
 * mlhip_bases_msm_batch*, mlhip_bases_checked_subgroup and mlhip_bases_batch_tabled are what they are for every handle.
 * curve_id is a MLHIP_CURVE_* value.  Measured: profiles/msm_device_result_ab.txt, DESIGN.md section 16. */
#define MLHIP_WINDOW_DEVICE_RESULT (1 << 20) /* OR-ed onto a plain window_c or onto MLHIP_WINDOW_BITS(c, bits) */

/* ---- products of any length: K products of m pairs each, for any m ------------------------------------------------------------
 * For callers with K independent products of MORE than four pairs: K aggregated signatures over m messages each, K
 * pairing-product equations of five to nine pairs, a batch of multi-openings, a verifier that folds m proofs into each of K
 * checks.
 *
 * Result.  out[k] = prod_{j < m} MillerLoop(g1[k m + j], g2[k m + j]); for the prepared forms the G2 point of slot j is
 * Q[q_index[j]] (q_index: m HOST entries shared by all products, read before the call returns, repeats allowed), and a NULL
 * q_index pairs slot j with point j, which needs m <= the handle's count.  A pair with an infinity on either side contributes
 * 1; a product of such pairs only is 1 (mlhip_pairing_prepared*: FExp(1) = 1).  The Miller value is the exact Fp12 product,
 * however the library groups the pairs: its bytes are those of the library's own calls with at most four pairs multiplied
 * together with mlhip_gt_mul.  n_products = 0 returns 0 and launches nothing; n_products * m overflowing size_t, or a null
 * pointer in a non-empty batch, is MLHIP_EINVAL before anything is launched.  A RAGGED batch (products of different
 * lengths) is a uniform one padded with infinity pairs (all-zero points): there is no offsets array.
 *
 * How it is said.  The library's dynamic symbol table does not grow (the tests pin it): the length travels in the
 * pairs_per_product / ppp argument of exactly six entry points -- mlhip_miller_loop, mlhip_miller_loop_device,
 * mlhip_miller_loop_prepared, mlhip_miller_loop_prepared_device, mlhip_pairing_prepared, mlhip_pairing_prepared_device -- as
 * MLHIP_PRODUCT_PAIRS(m) below: bit 63 set, m in the low 32 bits.  It is taken apart in those six and nowhere else.
 * include/mlhip_products.h wraps this in six inline functions for C, C++ and cgo callers, with m as a plain size_t:
 * mlhip_miller_loop_products[_device], mlhip_miller_loop_prepared_products[_device], mlhip_pairing_prepared_products[_device].
 *   - A PLAIN value keeps its meaning exactly: 1 .. 4 accepted, anything else MLHIP_EINVAL ("pairs_per_product must be 1..4").
 *   - MLHIP_PRODUCT_PAIRS(m) with m <= 4 is the plain call: same path, same bytes.
 *   - m = 0 or m >= 2^32 packs to a value that every entry point rejects with MLHIP_EINVAL.
 *
 * How it runs.  A product is cut into groups of `per` pairs (and a shorter tail); one launch runs the
 * Miller loops of all groups of all products -- the kernels of the plain calls, quads or lane pairs by the number of groups
 * -- into a per-device scratch buffer, log2-many launches fold each product's values into one (Gt products on the device),
 * and the fused forms then run the final exponentiation on the K folded values.  per = 1 while K m pairs leave the chip
 * under-filled, 4 from 2^17 pairs on (mlhip_pairing_product's rule; profiles/miller_products_ab.txt);
 * MLHIP_MILLER_GROUP=1|2|4 forces it.  The scratch is kept between calls (mlhip_release_cache frees it) and never exceeds
 * 1 GiB: a larger call runs in slabs of products, one after the other on the same stream, and a single product whose partial
 * values alone exceed 1 GiB is MLHIP_EINVAL.  The _device forms are asynchronous and in order on `stream` like every other
 * _device form; calls on different streams share the scratch and are ordered on the device by an event.  A long product is
 * never spread over a device list: it runs on the calling thread's first device (the prepared forms: the handle's).
 * MLHIP_G2_PREPARED_GENERAL does not apply to m > 4. */
#define MLHIP_PRODUCT_PAIRS(m) \
  (((size_t)1 << 63) | ((m) >= 1 && (unsigned long long)(m) <= 0xFFFFFFFFull ? (size_t)(m) : (size_t)0))

/* The device forms of the entry points above (and the _device forms further down, unless their comment says otherwise): device
 * pointers in and out; they enqueue their kernels on `stream` and return, so the work runs in order on `stream` (NULL = the
 * default stream) -- after whatever the caller queued there before, which may still be producing the inputs, and before
 * whatever it queues afterwards, which may overwrite them.  Arrays documented as HOST memory (offsets, base_index, q_index) are
 * read before the call returns (tests/test_stream_order_gpu.py calls every one of them on a busy stream). */
MLHIP_API int mlhip_miller_loop_device(int curve, const void* d_g1, const void* d_g2, size_t pairs_per_product,
                             size_t n_products, void* d_out_gt, void* stream);
MLHIP_API int mlhip_final_exp_device(int curve, const void* d_in_gt, size_t n, void* d_out_gt, void* stream);
MLHIP_API int mlhip_pairing_batch_device(int curve, const void* d_g1, const void* d_g2, size_t n, void* d_out_gt,
                               void* stream);
MLHIP_API int mlhip_gt_mul_device(int curve, const void* d_a_gt, const void* d_b_gt, size_t n, void* d_out_gt, void* stream);
MLHIP_API int mlhip_gt_inverse_device(int curve_id, const void* d_in_gt, size_t n, void* d_out_gt, void* stream);
MLHIP_API int mlhip_gt_exp_device(int curve, const void* d_in_gt, const void* d_scalars, int scalars_mont, size_t n,
                        void* d_out_gt, void* stream);
MLHIP_API int mlhip_gt_exp_cyclo_device(int curve_id, const void* d_in_gt, const void* d_scalars, int scalars_mont, size_t n,
                                        void* d_out_gt, void* stream);

/* out[i] = [scalars[i]] points[i * point_stride]: batched single-scalar multiplication (G1.Mul / G2.Mul,
 * driver/gurvy/bls12381/bls12-381.go:238-247, :342-351).  point_stride = 0 multiplies one base point by
 * every scalar (how the synthetic benchmark inputs [k_i]G are produced); from 2^12 scalars on that case builds a table
 * of [m 2^(wj)]P on the device (w = 12; MLHIP_FB_WINDOW overrides) and spends ceil(256 / w) mixed
 * additions per scalar instead of 256 doublings + 64 additions (MLHIP_FIXED_BASE_MIN=n moves the threshold, 0 = never).
 * The table stays on the device: the next call with the same curve, group and base point skips the build (the comparison
 * runs on the device, the call stays asynchronous; MLHIP_FB_CACHE=0 builds it every time).  Device pointers. */
MLHIP_API int mlhip_scalar_mul_device(int curve, int group, const void* d_points, size_t point_stride, const void* d_scalars,
                            int scalars_mont, size_t n, void* d_out_affine, void* stream);
/* host-buffer form */
MLHIP_API int mlhip_scalar_mul(int curve, int group, const void* points, size_t point_stride, const void* scalars,
                     int scalars_mont, size_t n, void* out_affine);

/* ---- points promised in G1 / G2: batched Mul over the curve's endomorphisms ------------------------------------------------
 * For callers who know where their points come from: decoded with subgroup_check = 1, outputs of MSMs over checked bases,
 * generators and their multiples, the r_k A_k of a batch verifier.  The reference's own G1.Mul / G2.Mul are defined for every
 * point of the curve, and the endomorphisms act as multiplications by known scalars on the prime-order subgroup ONLY -- so
 * the library never takes this route by itself.
 *
 * Result.  With the promise kept -- every point is in the prime-order subgroup or is the point at infinity (all zero) --
 * the bytes of the plain call on the same inputs: scalars_mont, unreduced 256-bit scalars (reduced mod r first), infinity in,
 * s = 0 mod r, point_stride 0 or 1.  A point outside the subgroup gives an undefined RESULT for its own product and for no
 * other, never a fault: no address depends on point data.
 *
 * How it is said.  The symbol table does not grow: the promise travels in the `group` argument of exactly two entry points,
 * the host-buffer batched Mul and its _device form above, as MLHIP_GROUP_SUBGROUP(group) below; they take the flag off
 * and read the rest as before.  include/mlhip_subgroup.h wraps this in two inline functions for C, C++ and cgo, which take a
 * plain group: the batched Mul with the suffix _subgroup (curve_id, group, points, point_stride, scalars, scalars_mont, n,
 * out_affine) and with _subgroup_device (.., d_out_affine, stream).  Every other entry point that takes a group -- the plan
 * and handle constructors, the MSM over a device list, the batched MSMs -- rejects the flagged value as it rejects any
 * group other than 1 or 2, and nothing inside the library produces it.
 *
 * Range.  group = MLHIP_GROUP_G1 or _G2; anything else makes the macro -1, which is MLHIP_EINVAL.  n = 0 returns 0 before
 * any pointer or device is looked at.  A null pointer, an unknown curve id and point_stride > 1 are MLHIP_EINVAL before
 * anything is launched.  The _device form is asynchronous and in order on `stream`, like the plain one.
 *
 * How it runs (msm_scalar_mul_endo.h).  G1 of the BLS12 curves: s = a + b x^2 with a, b < 2^128,
 * [s]P = [a]P + [b](beta Px, -Py), joint signed 4-bit windows -- 128 doublings and at most 66 additions instead of 256 and
 * 65.  G2 of every curve: the digits of s in base |x| (BLS12, four) or 6 x^2 (BN254, two) over Q, psi(Q), .., a 15-entry
 * table of their sums, 64 steps of one doubling (BN254: two) and at most one addition.  G1 of BN254:
 * s = k1 + k2 lambda with lambda = 36 x^4 - 1 and |k1|, |k2| < 2^127 from a lattice reduction, [s]P = [k1]P + [k2](beta Px, Py),
 * the chain of the BLS12 curves over the two magnitudes and their signs.  E(Fp) has prime order there, so the promise holds
 * for EVERY point of the curve (and infinity): any caller of BN254 G1 may set the flag.  A point that is not on the curve
 * gives an undefined result for its own product and for no other, never a fault.  One route the flag never changes:
 * point_stride = 0 from MLHIP_FIXED_BASE_MIN scalars on, where the fixed-base table has no doubling to save: accepted and
 * ignored.  MLHIP_SCALAR_MUL_ENDO=0 sends every flagged call to the plain kernels (second implementation, A/B).
 * Measured: profiles/scalar_mul_endo_ab.txt, DESIGN.md section 17 -- 2^20 products of per-point bases on one MI355X, flagged call
 * against plain call in one process, same bytes, on two machines: G1 0.69 - 0.70 (BLS12-381) / 0.67 (BLS12-377) of the plain
 * call's time, G2 0.54 - 0.58 / 0.53 - 0.56 and 0.72 - 0.76 on BN254 (the operation counts predict 0.67, 0.5 and 0.65); within
 * 0.05 of that from 2^10 products on.  Every (curve, group) that has a split is ahead by far more than two identical plain
 * runs differ (at most 0.012 of their time at 2^20), so all of them take it.  BN254 G1 (profiles/scalar_mul_glv_ab.txt, DESIGN.md
 * section 20): 0.66 - 0.69 of the plain call's time from 2^10 to 2^20 products (counted: 0.66), spread at most 0.010. */
#define MLHIP_GROUP_SUBGROUP(group) ((group) == 1 || (group) == 2 ? ((group) | 0x100) : -1)

/* K independent MSMs in one call: out[k] = sum_{offsets[k] <= i < offsets[k+1]} [scalars[i]] points[i] (the batched form of
 * MultiScalarMul / Mul2: an idemix or BBS verifier's many proofs of a few pairs each).
 * offsets: K+1 nondecreasing entries in HOST memory, offsets[0] = 0, offsets[K] = total pairs; anything else, or a null
 * pointer in a non-empty batch, is MLHIP_EINVAL before anything is launched.  K = 0 returns 0 and does nothing.
 * An empty segment gives the point at infinity.  group = MLHIP_GROUP_G1 or _G2.  Scalars as in mlhip_msm_g1
 * (scalars_mont, not necessarily reduced).  Affine output in this header's layout (infinity = all zero).
 * Every segment is cut into chunks of at most P pairs, one lane (G1) or lane pair (G2) per chunk runs an interleaved
 * signed 4-bit-window double-and-add (256 / P + 71 group operations per pair), and the chunk sums of each segment are
 * added in passes of at most 32 per lane.  P = 4 (MLHIP_MSM_BATCH_CHUNK = 1, 2, 4 or 8 overrides; below ~2^17 pairs in all
 * the device is not filled and P = 1 is faster).
 * Segments of MLHIP_MSM_BATCH_BUCKET_MIN pairs or more (default 512 for G1, 256 for G2; 0 = never, 1 .. 8 mean 9) take a
 * bucket route instead: slices of at most S pairs, signed windows of 7 bits (G1: one bucket per lane of a wave) or 6 bits (G2:
 * one bucket per lane pair, 43 windows), one wave per (slice, window), an in-wave reduction and one Horner lane (pair) per
 * slice; the slice sums join the chunk sums of the passes above.  S is the largest power of two from 256 to 4096 (G2: to
 * 1024) that still gives 4096 waves (MLHIP_MSM_BATCH_BUCKET_SLICE=s fixes it).  Same bytes as the chunks for every input
 * (infinities, repeated points, P beside -P, points outside the subgroup).  Scratch: 37 (G2: 43) bytes per pair of a slice +
 * as many XYZZ per slice; a call that would need more than 1 GiB of it runs chunks only.  Measured:
 * G1 (profiles/msm_batch_bucket_ab.txt), from 2^18 pairs per call on, 1.2-1.5x the chunks at 512 pairs per segment and
 * 1.4-2.1x from 1024 on; a batch of 16 384-pair segments is level with or ahead of single mlhip_msm_g1 calls, from 65 536
 * pairs per segment on single calls are ahead.  G2 (profiles/msm_batch_bucket_g2_ab.txt), at 2^16 and 2^18 pairs per call,
 * 1.07-1.4x at 256 pairs per segment, 1.35-1.5x at 512 and 1.4-1.6x from 1024 on.  The table-free path of
 * mlhip_bases_msm_batch* takes the same route (same switches, its group's defaults).
 * Runs on the first listed device.  Device pointers; the offsets are read on the host. */
MLHIP_API int mlhip_msm_batch_device(int curve, int group, const void* d_points, const void* d_scalars, int scalars_mont,
                                     const uint64_t* offsets, size_t k, void* d_out_affine, void* stream);
/* host-buffer form */
MLHIP_API int mlhip_msm_batch(int curve, int group, const void* points, const void* scalars, int scalars_mont,
                              const uint64_t* offsets, size_t k, void* out_affine);

/* ---- batched MSMs over points promised in G1 / G2: endomorphism-split Straus chunks ------------------------------------------
 * The promise of "points promised in G1 / G2" above for mlhip_msm_batch / mlhip_msm_batch_device: a verifier's points are
 * decoded with subgroup_check = 1, are issuer keys or generators, or come out of earlier MSMs.  The library never takes
 * this route by itself.
 *
 * Result.  With the promise kept -- every point is in the prime-order subgroup or is the point at infinity (all zero) --
 * the bytes of the plain call on the same inputs: every offsets shape, scalars_mont, unreduced 256-bit scalars, empty
 * segments, every chunk length.  A point outside the subgroup gives an undefined RESULT for the segment that holds it and
 * for no other, never a fault: no address depends on point data.
 *
 * How it is said.  The symbol table does not grow, and `group` stays what it was (both batch entry points go on rejecting
 * MLHIP_GROUP_SUBGROUP values): the promise travels in the CURVE ID of exactly these two entry points, as
 * MLHIP_CURVE_SUBGROUP_POINTS(curve_id) below; they take the flag off and read the rest as before.  Everywhere else the
 * flagged ids are unknown curves, as they were here, and nothing inside the library produces them.  include/mlhip_subgroup.h
 * wraps this in two inline functions that take a plain curve id: mlhip_msm_batch_subgroup(curve_id, group, points, scalars,
 * scalars_mont, offsets, k, out_affine) and mlhip_msm_batch_subgroup_device(.., d_out_affine, stream).
 *
 * Range.  curve_id = 0, 1 or 2; anything else makes the macro -1, which is MLHIP_EINVAL ("unknown curve id").  Every other
 * argument rule is the plain call's.
 *
 * How it runs (msm_batch_endo.h).  Only the Straus chunks change; segments on the bucket route, the sum
 * passes and the scratch are the plain call's.  Per pair, where the plain chunk spends 256 / P + 71 group operations: G1 of
 * the BLS12 curves 128 / P + 7 + <= 66 (s = a + b x^2, joint signed 4-bit windows over one table, b's additions scale X by
 * beta and flip Y); G2 of the BLS12 curves 64 / P + 11 + <= 64 (four digits base |x| over Q .. psi^3 Q, a 15-entry table, 64
 * steps of one doubling); G2 of BN254 128 / P + 13 + <= 64 (two digits base 6 x^2, 64 steps of two doublings).  The G2 table
 * is 15 XYZZ per pair in scratch, so the split chunks are compiled for P = 1, 2, 4 there: at MLHIP_MSM_BATCH_CHUNK=8 a flagged
 * G2 call runs the plain chunk kernel.  G1 of BN254 128 / P + 7 + <= 66: the G1 chunk of the BLS12 curves over the lattice
 * split s = k1 + k2 lambda, |k1|, |k2| < 2^127, the signs of k1, k2 per pair.  E(Fp) has prime order
 * there, so the promise holds for every point of the curve; a point that is not on the curve gives an undefined result for
 * its own segment and for no other, never a fault.
 * MLHIP_MSM_BATCH_ENDO=0 sends every flagged call to the plain chunk kernels (second implementation, A/B).
 * Measured (profiles/msm_batch_endo_ab.txt): flagged call against plain call in one process on one
 * MI355X, same device buffers, same bytes in every cell; 2^10 .. 2^16 segments of 2 .. 64 pairs.  Flagged / plain time at the
 * default P = 4, smallest .. largest over the grid (counted from the operations above): G1 0.79 .. 0.90 BLS12-381 and
 * 0.78 .. 0.89 BLS12-377 (0.78); G2 0.65 .. 0.86 and 0.64 .. 0.84 (0.67), BN254 0.79 .. 0.97 (0.81); from 2^20 pairs per call on,
 * the device full, 0.88 / 0.86, 0.86 / 0.84 and 0.97.  At P = 1: G1 0.68 .. 0.77 (0.61), G2 0.51 .. 0.62 (0.43), BN254 0.71 .. 0.80
 * (0.63).  The measured ratios lie above the counted ones because the split removes doublings only, the cheapest operation
 * (9 field products against 14 of an addition), and G2 builds 11 or 13 more table entries per pair.  Every (curve, group) with
 * a split is ahead of the plain call in every cell at the default P by more than two identical plain runs differ (at most
 * 0.015), so all five take it.  BN254 G1 (profiles/msm_batch_glv_ab.txt): 0.76 .. 0.88 at P = 4 (0.78),
 * 0.67 .. 0.80 at P = 1 (0.61), ahead in all 12 cells at the default P by more than the spread (at most 0.013): it takes the
 * split too.  Flagged calls keep the default P = 4: below ~2^17 pairs in all P = 1 is
 * faster, as for the plain call, but from 2^18 pairs on it falls behind the plain call at its default. */
#define MLHIP_CURVE_SUBGROUP_POINTS(curve_id) ((curve_id) >= 0 && (curve_id) <= 2 ? ((curve_id) | 0x100) : -1)

/* ---- K independent point sums in one call: the batch calls with every scalar 1 ------------------------------------------------
 * The batched twin of mlhip_g1_sum / mlhip_g2_sum: K committees' public keys, K aggregate signatures, K folded proofs, the
 * pairwise A[k] + B[k] between two device stages.  out[k] = the sum of the points of segment k; over a handle the points are
 * B[idx(i)], idx as in mlhip_bases_msm_batch.
 *
 * How it is said.  The symbol table does not grow: the flag MLHIP_SCALARS_UNIT below travels in `scalars_mont` of exactly four
 * entry points -- mlhip_msm_batch, mlhip_msm_batch_device, mlhip_bases_msm_batch, mlhip_bases_msm_batch_device -- and nowhere
 * else (every other entry point reads scalars_mont as before).  With the flag, scalars_mont must equal it exactly and
 * `scalars` must be NULL ("unit scalars take no scalar array"); both are MLHIP_EINVAL otherwise.  Every other argument rule
 * is the plain call's (offsets, K = 0 returns 0, empty segment = all-zero point, unknown curve / group, null points or output
 * in a non-empty batch, index >= the handle's n, a segment longer than n without base_index, a set or a sharded handle), all
 * checked before a device is asked for.  MLHIP_CURVE_SUBGROUP_POINTS(curve) beside the flag is accepted and changes nothing:
 * there is no scalar to split.  No CPU fallback: MLHIP_ENODEVICE without a device, as for mlhip_msm_batch.
 * include/mlhip_sum_batch.h wraps this in four inline functions: mlhip_sum_batch(curve_id, group, points, offsets, k,
 * out_affine), mlhip_sum_batch_device(.., d_out_affine, stream), mlhip_bases_sum_batch(bases, base_index, offsets, k,
 * out_affine) and mlhip_bases_sum_batch_device(bases, base_index, offsets, k, stream, d_out_affine).
 *
 * Result.  The canonical affine form of each segment's sum: the bytes of the plain call with an explicit array of
 * plain-integer ones and of mlhip_g1_sum / mlhip_g2_sum per segment, for any points of the curve in any order and multiplicity
 * (inside or outside the subgroup, (0,0) = infinity, one point m times, P beside -P).  A point off the curve gives an
 * undefined result for its own segment only, never a fault: no address depends on point data.
 *
 * How it runs (msm_sum_batch.h).  A segment of m points is cut into c = ceil(m / S) slices, slice j
 * reading the points j, j + c, j + 2 c, .. of the segment; one lane (G1) or lane pair (G2) per slice adds its points with the
 * complete mixed addition of the plain sums (1 group operation per point, no table, no doubling), and the slice sums go
 * through mlhip_msm_batch's sum passes: 1 + ~1.4 / S operations per point where the plain call with ones spends ~9 (the
 * {1..8} P table and one addition), uploads 32 bytes of scalar per point and sends long segments to buckets.  A flagged call
 * never takes the Straus chunks or the bucket route and needs no scalar memory; on a handle it neither builds nor reads
 * batch tables (mlhip_bases_batch_tabled is unchanged by it).
 * S is a power of two per call: the largest of 4, 8, 16, 32 that still gives 2^13 slices, counting total / S of them, else 4
 * (S = 4 below 2^16 points per call, 32 from 2^18 on); MLHIP_SUM_BATCH_SLICE=s (a power of two, 1 .. 4096) forces it.  The rule
 * is the one the grid of profiles/sum_batch_ab.txt supports (tools/perf_sum_batch.py runs every cell at S = 4, 8, 16, 32 as
 * well): the first candidate, "as many slices as the device keeps lanes" (2^16; G2 2^15 lane pairs), stayed at S = 4 up to
 * 2^18 points, where S = 8 or 16 takes 19 - 27 % less time -- a small call waits for its chain of dependent additions, about
 * 10 us each, and 2^13 slices already hide it.
 * Measured (one MI355X, profiles/sum_batch_ab.txt): mlhip_sum_batch_device against
 * mlhip_msm_batch_device with a resident array of ones in one process, same device buffers, same bytes in every cell;
 * K = 2^10, 2^14, 2^16 segments of 2 .. 4096 points, at most 2^22 points per call.  Flagged / plain time (counted: 0.12 - 0.15):
 * about 0.3 - 0.55 up to 2^18 points per call in segments of 2 .. 64 points, where the flagged call is a few launches of
 * 0.14 - 0.8 ms in all; about 0.2 at 2^20 points; 0.01 - 0.07 for 2^22 points per call and for segments of 512 and 4096 points, where the plain
 * call builds 2^22 tables or sorts its ones into buckets (2^10 segments of 4096 BLS12-381 G1 points: about 2.2 ms against
 * 260 ms).  BLS12-381 G1 and G2 and BN254 G1 alike; over a 4096-base handle with an index list 0.4 - 0.55.  Ahead of the plain
 * call in every cell by more than two identical plain runs differ (at most 0.10).  2^10 lists of 64 G1 points from host
 * memory: one call 0.6 - 0.75 ms against 26 ms for 2^10 mlhip_g1_sum calls. */
#define MLHIP_SCALARS_UNIT 0x400 /* `scalars_mont` of the four batch entry points: every scalar is 1, `scalars` must be NULL */

/* ---- resident bases (upload-once point table, only the scalars travel per call) ----------
 * For callers that cannot hold device pointers themselves (the Go shim): the points are uploaded once, every
 * mlhip_bases_msm() uploads n x 32 bytes of scalars and returns sum_i [s_i] P_i over the first n bases (n <= the
 * count given at creation).  Calls on one handle from several threads are serialized inside the library (one MSM at a
 * time per handle); handles are independent of each other. */
typedef struct mlhip_bases mlhip_bases;
/* window_c = 0 leaves the geometry to the library, and lets it keep SHIFTED-BASE TABLES for the handle (tables of at least
 * 2^10 bases that fit a quarter of the free device memory; MLHIP_BASES_TABLES=0 never, =1 always): besides P_i the device
 * holds 2^off(j) P_i for every digit position j (first bit off(j)) of a signed-digit scalar (13 rows a base from 2^16 bases
 * on -- 20-bit digits, 1.5 GB for 2^20 BLS12-381 G1 bases, built once in ~60 ms --, 16 to 20 rows below), so that all digits
 * of all scalars add into ONE set of 2^(c-1) buckets: a wider digit at the same reduction cost (19 % fewer bucket additions)
 * and a host tail of at most 19 doublings instead of 256.  Same result bytes.
 * An explicit window_c asks for that Pippenger geometry over the plain table (what BASELINE's "c = 16" names).  The
 * reference has no counterpart: its MultiScalarMul takes fresh slices (driver/gurvy/bls12381/bls12-381.go:766-783). */
MLHIP_API int mlhip_bases_create(int curve, int group, const void* points, size_t n, int window_c, mlhip_bases** bases);
/* the same handle from n affine points that are already in the current device's memory (a copy is taken; the caller's
 * buffer may be reused at once): always one device, never spread */
MLHIP_API int mlhip_bases_create_device(int curve, int group, const void* d_points, size_t n, int window_c, mlhip_bases** bases);
/* the table cut into contiguous shards over an explicit device list (mlhip_bases_create does this by itself with the
 * process's list from MLHIP_MULTI_MIN bases on): every mlhip_bases_msm then moves each device's scalars over its own
 * PCIe link and adds the per-device partial sums on the host */
MLHIP_API int mlhip_bases_create_multi(int curve, int group, const int* devices, int n_devices, const void* points, size_t n,
                             int window_c, mlhip_bases** bases);
MLHIP_API int mlhip_bases_msm(mlhip_bases* bases, const void* scalars, int scalars_mont, size_t n, void* out_affine);
/* the same MSM with the n scalars already in device memory (a prover whose witness was computed on the device); `stream`
 * as in mlhip_msm_run; single-device handles only (MLHIP_EINVAL for a table spread over several devices)
 * (a device-result handle: see "device results" above -- out_affine is a DEVICE pointer, written in order on `stream`) */
MLHIP_API int mlhip_bases_msm_device(mlhip_bases* bases, const void* d_scalars, int scalars_mont, size_t n, void* stream,
                           void* out_affine);
/* the plan a single-device handle runs its MSMs on (NULL otherwise) -- for mlhip_msm_plan_set_profiling /
 * mlhip_msm_plan_timings only; it stays owned by the handle */
MLHIP_API mlhip_msm_plan* mlhip_bases_plan(mlhip_bases* bases);
/* 1 when mlhip_bases_create verified, on the device, that every point of the table is on the curve and in the prime-order
 * subgroup (or the point at infinity) -- done for BLS12-377 G1 tables, whose MSMs then sum their buckets in twisted
 * Edwards coordinates (see mlhip_msm_plan_assume_srs); 0 otherwise (other curves, G2, a table with a point outside the
 * subgroup, MLHIP_EDWARDS=0): such tables take the Weierstrass kernels and give the reference's result for any input. */
MLHIP_API int mlhip_bases_checked_subgroup(mlhip_bases* bases);
MLHIP_API int mlhip_bases_destroy(mlhip_bases* bases);
/* ---- sets of handles: the MSMs of several resident tables over ONE scalar vector (a Groth16 prover's A, B1 and B2 queries
 * over the witness).  A SET of 1..4 single-device handles of one curve on one device, any mix of G1 and G2: a handle itself.
 * The members are NOT owned: they must outlive the set and stay usable on their own, before, between and after set calls;
 * mlhip_bases_destroy(set) frees the set only.  Refused with MLHIP_EINVAL: k = 0 or k > 4, a null or repeated member, a set
 * as a member, members of different curves or devices, a member spread over several devices, a device-result member.
 *   mlhip_bases_msm(set, scalars, mont, n, out) and mlhip_bases_msm_device(set, d_scalars, mont, n, stream, out) compute every
 *   member's MSM over the same first n scalars (n <= the smallest member's count) and write the affine results back to back
 *   in member order, each at its own point size, into HOST memory; n = 0 writes all-zero points.  Both return when the
 *   results are there.  A set call takes every member's mutex, in address order.
 *   mlhip_bases_plan(set) is NULL; mlhip_bases_checked_subgroup(set) is 1 iff it is 1 for every member;
 *   mlhip_bases_msm_batch*, mlhip_bases_batch_tabled are MLHIP_EINVAL: batches run on the members.
 * What a set call shares: the entry lists of a tile depend on the scalars and the plan's geometry only, not on the group.
 * Members whose plans have the same geometry (tables or not, digit width, digits, tile, bucket groups, scalar width) form a
 * CLASS: every tile is sorted once and accumulated once per member (shifted-base tables included: each member gathers from
 * its own table through the shared lists); a member of another geometry is a class of its own.  Host scalars cross PCIe once
 * per call whatever the number of classes.  Same result bytes as the members' own calls.
 * MLHIP_BASES_SET_SHARE=0: every member runs exactly what its own mlhip_bases_msm[_device] would, in member order (the second
 * implementation, and the A/B of tools/perf_bases_set.py); =1: the shared route at every size; unset: the shared route from
 * 2^12 host scalars / 2^16 device scalars on, the per-member route below (MLHIP_SET_SHARE_MIN_N_HOST / _DEVICE of
 * mathlib_amd/csrc/msm_set.h: the smallest measured sizes from which the set call is level with or ahead of the k separate
 * calls in every cell of profiles/bases_set_ab.txt -- 2^20 scalars, tables on: {G1, G2} 0.80-0.89 of the separate calls with
 * host scalars and 0.96-0.98 with device scalars, {G1, G1, G2} 0.77-0.86 and 0.93-0.97).
 * Not offered: per-member scalar offsets, device-result sets, sets over sharded handles. */
#define MLHIP_GROUP_SET 0x200     /* `group` of mlhip_bases_create: `points` is an array of n member handles (curve, window_c unused) */
#define MLHIP_MSM_SET_ROUTE 0x100 /* `scalars_mont` of mlhip_bases_msm on a set with scalars = NULL: no MSM, the route report */
/* include/mlhip_bases_set.h has the two as inline functions over mlhip_bases_create / mlhip_bases_msm, in the house style of
 * MLHIP_GROUP_SUBGROUP and MLHIP_WINDOW_BITS (the dynamic symbol table stays what it was):
 *   mlhip_bases_set_create(members, k, &set)
 *   mlhip_bases_set_route(set, info, cap) -- how the set's last MSM ran: info[0] = members, info[1] = sort trains per tile
 *   (geometry classes), info[2] = host-to-device copies of the scalar vector (0 for device scalars), info[3] = 1 iff every
 *   member read tables; returns the number of entries written (<= cap).  Recorded by the code path that ran: the per-member
 *   route reports (k, k, k or 0, .). */
/* K independent MSMs over the resident bases of a handle (an idemix or BBS verifier checking many proofs against one issuer
 * key: most pairs of every proof multiply the same few dozen bases):
 *   out[k] = sum_{offsets[k] <= i < offsets[k+1]} [scalars[i]] B[idx(i)]
 * idx(i) = base_index[i] when base_index != NULL; otherwise i - offsets[k] (pair j of a segment takes base j).
 * Semantics as mlhip_msm_batch (offsets rules, K = 0 does nothing, empty segment = infinity, scalars_mont, scalars not
 * necessarily reduced, affine output with infinity all zero), in the group the handle was created with.  offsets and
 * base_index are HOST memory in both forms.  MLHIP_EINVAL before anything is launched for malformed offsets, an index >= the
 * handle's n, a segment longer than n without base_index, or a handle spread over several devices (not supported).
 * The first call that reads base m - 1 builds per-base fixed-window tables T_b[j][m'-1] = [m' 2^(wj)] B_b for the bases
 * [0, m) on the device (a later call that reads further extends them); every pair then costs ceil(256 / w) mixed additions
 * and no doubling.  Width w = 12 (MLHIP_BASES_BATCH_WINDOW = 4 .. 12), ceil(256 / w) 2^(w-1) rows of
 * 112 B (BLS12 G1; G2 twice) per base: 5 MB at w = 12, 459 KB at w = 8.  Chunks of P pairs per lane: the largest of
 * 1, 2, 4, 8, 16 that still fills 2^16 lanes (MLHIP_BASES_BATCH_CHUNK overrides).  The tables are owned by the handle (freed
 * by mlhip_bases_destroy, untouched by mlhip_release_cache) and capped at MLHIP_BASES_BATCH_MAX_MB (1024) per handle -- 212
 * BLS12-381 G1 or 106 G2 bases at w = 12: a call whose tables would pass the cap (or MLHIP_BASES_BATCH_MAX_MB=0) runs
 * mlhip_msm_batch's variable-base kernels on the handle's points instead (the table-free path): Straus chunks, and for
 * segments of MLHIP_MSM_BATCH_BUCKET_MIN pairs or more its bucket route, reading each pair's base through base_index
 * (G1 with 4096 bases: 1.3-1.5x the chunks at 512 pairs per segment, 1.7-2.1x from 1024 on).  The tabled path never takes
 * the bucket route: 22 mixed additions per pair beat it.
 * Growing the tables briefly holds the old and the new ones.  A handle that never sees a batch call allocates nothing.
 * Calls on one handle are serialized, as for mlhip_bases_msm. */
MLHIP_API int mlhip_bases_msm_batch(mlhip_bases* bases, const void* scalars, int scalars_mont, const uint32_t* base_index,
                                    const uint64_t* offsets, size_t k, void* out_affine);
/* the same with the scalars in device memory and the outputs written to device memory, in order on `stream` */
MLHIP_API int mlhip_bases_msm_batch_device(mlhip_bases* bases, const void* d_scalars, int scalars_mont, const uint32_t* base_index,
                                           const uint64_t* offsets, size_t k, void* stream, void* d_out_affine);
/* number of leading bases of the handle that currently have batch tables (0: none; every batch call takes the
 * table-free path) */
MLHIP_API int mlhip_bases_batch_tabled(mlhip_bases* bases, size_t* n_tabled);

/* ---- prepared G2 handles: pairings against FIXED G2 points ("G2Prepared") ------------------------------------------------
 * The reference's verifier calls Pairing2(g, sig, pk, h) + FExp with the same two G2 arguments in every call
 * (driver/gurvy/bls12381/bls12-381.go:448-468); so do BBS+ and idemix verification.  The line coefficients of the Miller loop
 * depend on Q alone: a handle computes them once for each of its m points -- 68 lines of three Fp2 per BLS12-381 point, 23 KB,
 * stored in loop order in the limb form the kernels multiply in -- and keeps them, with the affine points, on the device that
 * is current at creation.  A prepared Miller loop then carries no G2 point at all.
 * m >= 1; the points are affine G2 points in the layout of mlhip_miller_loop, infinity all zero.  A point on the curve but
 * outside the subgroup gives what mlhip_miller_loop gives for it (the same arithmetic); a point off the curve gives an
 * undefined result, never a fault.  The tables are read-only after creation: calls on one handle from several threads run
 * concurrently, there is no per-handle lock.  mlhip_release_cache does not touch a handle.  No CPU fallback: MLHIP_ENODEVICE
 * without a device. */
typedef struct mlhip_g2_prepared mlhip_g2_prepared;
/* bls12-381.go:448-468: the G2 arguments of Pairing / Pairing2, prepared once (host points) */
MLHIP_API int mlhip_g2_prepared_create(int curve, const void* g2_points, size_t m, mlhip_g2_prepared** h);
/* bls12-381.go:448-468: the same from device memory; a copy is taken, the caller's buffer is free again on return */
MLHIP_API int mlhip_g2_prepared_create_device(int curve, const void* d_g2_points, size_t m, mlhip_g2_prepared** h);
/* bls12-381.go:448-468: the number of points m of the handle */
MLHIP_API int mlhip_g2_prepared_count(mlhip_g2_prepared* h, size_t* m);
MLHIP_API int mlhip_g2_prepared_destroy(mlhip_g2_prepared* h);
/* bls12-381.go:448-464 (Pairing / Pairing2 without FExp):
 *   out[k] = prod_{j < ppp} MillerLoop(g1[k ppp + j], Q[idx(j)]),   idx(j) = q_index ? q_index[j] : j
 * not final-exponentiated (raw values are defined up to what FExp kills, as for mlhip_miller_loop; after mlhip_final_exp they
 * are byte-identical to mlhip_final_exp(mlhip_miller_loop(..)) on the expanded pairs).  q_index is HOST memory in both forms
 * and has ppp entries that ALL products share: slot j of every product pairs with the same Q, which keeps the line reads
 * uniform across a wave.  ppp = 1 .. 4, or MLHIP_PRODUCT_PAIRS(m) for any length ("products of any length" above).  A G1
 * argument at infinity, or a Q at infinity, contributes 1.  n_products = 0 does nothing.  MLHIP_EINVAL before anything is
 * launched for a null handle, a plain ppp outside 1 .. 4, an index >= m, ppp > m without q_index.
 * Kernels: one product per quad of lanes up to 2^14 products (BLS12-377: 2^15, its Miller loop at every size), per lane pair
 * above -- the sizes the general entry points switch at; MLHIP_PAIRING_QUAD=0|1 forbids / forces the quads.  Switch to the
 * general kernels: at no size, on any curve.  In the A/B against the general entry points on an MI355X
 * (tools/perf_g2_prepared.py -> profiles/g2_prepared_ab.txt: ppp 1, 2 x 1, 2^10, 2^14, 2^16 products; DESIGN.md section 10 has
 * the table) the prepared kernels are ahead at every grid point; at 2^16 products of two pairs the Miller loop takes about two
 * thirds of the general one's time on every curve.  prepared_general_range() (pairing_prepared_kernels.h) is where a losing
 * size would go: inside it the general kernels run on the Qs expanded from the handle's affine copy, same bytes after FExp.
 * MLHIP_G2_PREPARED_GENERAL=1 selects that path at every size (0: never); it allocates and frees its scratch per call, so a
 * _device call through it returns only when its work is done and cannot be captured into a graph.
 * The _device forms launch on the handle's device and leave the caller's current device as it was; `stream` and the device
 * pointers must belong to the handle's device. */
MLHIP_API int mlhip_miller_loop_prepared(mlhip_g2_prepared* h, const void* g1, const uint32_t* q_index, size_t ppp,
                                         size_t n_products, void* out_gt);
/* bls12-381.go:448-464: the same on device pointers, in order on `stream` */
MLHIP_API int mlhip_miller_loop_prepared_device(mlhip_g2_prepared* h, const void* d_g1, const uint32_t* q_index, size_t ppp,
                                                size_t n_products, void* d_out_gt, void* stream);
/* bls12-381.go:448-468: out[k] = FExp of the same product -- the verifier's whole Pairing2 + FExp in one launch */
MLHIP_API int mlhip_pairing_prepared(mlhip_g2_prepared* h, const void* g1, const uint32_t* q_index, size_t ppp,
                                     size_t n_products, void* out_gt);
/* bls12-381.go:448-468: the same on device pointers, in order on `stream` */
MLHIP_API int mlhip_pairing_prepared_device(mlhip_g2_prepared* h, const void* d_g1, const uint32_t* q_index, size_t ppp,
                                            size_t n_products, void* d_out_gt, void* stream);

/* The host-buffer MSM entry points above keep up to 16 plans + input buffers (at most 32 GB) alive between calls (creating and
 * destroying them costs as much as a 2^20-point MSM); this frees the idle ones.  MLHIP_NO_PLAN_CACHE=1 disables the pool. */
MLHIP_API int mlhip_release_cache(void);

/* ---- wire format (bulk NewG1FromBytes / NewG1FromCompressed and G1.Bytes / G1.Compressed,
 * driver/gurvy/bls12381/bls12-381.go:531-569, :286-296) --------------------------------------------------
 * Decode n points of gnark's wire format (BLS12 curves: zcash 3-bit header; BN254: 2-bit header), all of the
 * same form: compressed (fp bytes each) or uncompressed (2 x fp bytes).  Every point gets a status byte:
 * 0 ok | 1 malformed (flags, coordinate >= p, bad infinity) | 2 not on the curve | 3 not in the r-torsion
 * subgroup; out_affine[i] is (0,0) unless status[i] == 0.  subgroup_check: 0 skips the test (gnark's SetBytes always
 * does it), 1 runs the fastest exact test (BLS12 curves: phi(P) = [-x^2]P for G1, psi(Q) = [x]Q for G2; BN254 G2:
 * [x+1]Q + psi([x]Q) + psi^2([x]Q) = psi^3([2x]Q) -- 64-bit ladders, the criteria gnark uses), 2 forces the plain [r]P ladder (kept for cross-checking). */
MLHIP_API int mlhip_g1_from_bytes(int curve, const void* wire, size_t n, int compressed, int subgroup_check, void* out_affine,
                        unsigned char* status);
MLHIP_API int mlhip_g1_to_bytes(int curve, const void* affine, size_t n, int compressed, void* wire);
MLHIP_API int mlhip_g1_from_bytes_device(int curve, const void* d_wire, size_t n, int compressed, int subgroup_check,
                               void* d_out_affine, unsigned char* d_status, void* stream);
MLHIP_API int mlhip_g1_to_bytes_device(int curve, const void* d_affine, size_t n, int compressed, void* d_wire, void* stream);
/* G2 (NewG2FromBytes / NewG2FromCompressed, bls12-381.go:541-569): 2 / 4 fp-sized big-endian values per point in
 * the order X.A1, X.A0 [, Y.A1, Y.A0]; y recovered by a square root in Fp2; subgroup_check as for G1. */
MLHIP_API int mlhip_g2_from_bytes(int curve, const void* wire, size_t n, int compressed, int subgroup_check, void* out_affine,
                        unsigned char* status);
MLHIP_API int mlhip_g2_to_bytes(int curve, const void* affine, size_t n, int compressed, void* wire);
MLHIP_API int mlhip_g2_from_bytes_device(int curve, const void* d_wire, size_t n, int compressed, int subgroup_check,
                               void* d_out_affine, unsigned char* d_status, void* stream);
MLHIP_API int mlhip_g2_to_bytes_device(int curve, const void* d_affine, size_t n, int compressed, void* d_wire, void* stream);
/* Gt (NewGtFromBytes, driver/gurvy/bls12381/bls12-381.go:571-579; Gt.Bytes, :432-436): gnark's GT.Bytes() -- 12 fp-sized
 * big-endian values per element in the order C1.B2.A1, C1.B2.A0, ..., C0.B0.A0 (always 12 x fp bytes; there is no compressed
 * form).  Status byte per element, the codes of the point decoders: 0 ok | 1 malformed (a coordinate >= p) | 3 not in Gt; 2 is
 * never returned for Gt.  Malformed takes precedence; out_gt[i] is all zero unless status[i] == 0.  subgroup_check: 0 only
 * decodes, as gnark's SetBytes does (status 0 or 1); 1 also runs the membership test of mlhip_gt_is_member.  curve_id is a
 * MLHIP_CURVE_* value. */
MLHIP_API int mlhip_gt_from_bytes(int curve_id, const void* wire, size_t n, int subgroup_check, void* out_gt, unsigned char* status);
MLHIP_API int mlhip_gt_to_bytes(int curve_id, const void* gt, size_t n, void* wire);
MLHIP_API int mlhip_gt_from_bytes_device(int curve_id, const void* d_wire, size_t n, int subgroup_check, void* d_out_gt,
                                         unsigned char* d_status, void* stream);
MLHIP_API int mlhip_gt_to_bytes_device(int curve_id, const void* d_gt, size_t n, void* d_wire, void* stream);
/* status[i] = 0 if gt[i] (in-memory layout) lies in Gt, the subgroup of order r of Fp12* -- exactly: 0 iff gt[i]^r = 1 --
 * and 3 otherwise (gnark's GT.IsInSubGroup; the counterpart of the subgroup checks of the point decoders).  The test:
 * gt != 0, frob^2(frob^2(f)) f = frob^2(f) (the cyclotomic subgroup) and frob(f) = f^x (BLS12) / f^(6 x^2) (BN254) by
 * cyclotomic squarings; any Fp12 value gives a status, never a fault.  A value that passes may be
 * handed to mlhip_gt_exp_cyclo. */
MLHIP_API int mlhip_gt_is_member(int curve_id, const void* gt, size_t n, unsigned char* status);
MLHIP_API int mlhip_gt_is_member_device(int curve_id, const void* d_gt, size_t n, unsigned char* d_status, void* stream);

/* ---- group helpers: out = sum of n affine points (n = 0: the point at infinity).  Two routes, one result:
 *   host loop     below the threshold -- the handful of per-GPU partial results combined after the RCCL all-gather.  No HIP
 *                 call is made: a rank that must not initialise a device may call it.
 *   device route  from the threshold on (aggregating 10^4 .. 10^6 signatures or keys, folding proofs), when the thread has a
 *                 usable device: upload, strided slices per lane (pair), segmented sums, download of one point, on a leased
 *                 stream.  Without a usable device the host loop serves every n: these two functions
 *                 never return MLHIP_ENODEVICE.
 *   threshold     MLHIP_SUM_DEVICE_MIN=n (0 = never the device, 1 = always when there is one); default 2^14 points for G1
 *                 and 2^12 for G2: from there on the device route, PCIe upload included, is ahead of the host loop at every
 *                 measured size on all three curves (profiles/point_sum_ab.txt).
 *   inputs        any points of the curve, inside or outside the prime-order subgroup, and (0,0) = infinity, in any order
 *                 and multiplicity (one point n times, P next to -P): both routes give the same bytes, the canonical affine
 *                 form of the sum.  A point off the curve gives an undefined result on the device route, never a fault
 *                 (no address depends on the data). */
MLHIP_API int mlhip_g1_sum(int curve, const void* affine_points, size_t n, void* out_affine);
MLHIP_API int mlhip_g2_sum(int curve, const void* affine_points, size_t n, void* out_affine);

/* ---- field kernel (parity / roofline probe): out[i] = a[i] * b[i] (Montgomery), device pointers */
MLHIP_API int mlhip_fp_mul_device(int curve, const void* d_a, const void* d_b, size_t n, int repeat, void* d_out,
                        void* stream);

/* ---- environment switches (all of them; none is needed for normal use) ---------------------------------------------------
 * Read by the library at the point named.  "2nd impl" = selects a slower second implementation of the same result that the
 * parity tests run against the default one; it never changes a result byte.
 *
 *   devices and threads (read once per process)
 *     MLHIP_DEVICES="0,1,.." | "all"   the process's device list (see mlhip_init)
 *     MLHIP_MULTI_MIN, MLHIP_MULTI_MIN_PAIRINGS   smallest host-buffer MSM / pairing batch that is spread over the list (2^21, 2^17)
 *     MLHIP_HOST_THREADS=N             threads of the host-tail pool per call incl. the caller (default: min(8, cores of the
 *                                      affinity mask / LOCAL_WORLD_SIZE, halved when ranks share the host); 1 = none)
 *     MLHIP_NO_PLAN_CACHE=1            host-buffer MSMs create and destroy their plan per call
 *   MSM geometry and schedules (read per plan or per launch)
 *     MLHIP_STREAM_SEGMENTS=K          host-buffer MSMs in K equal segments (0 / 1 = one upload, one pass)
 *     MLHIP_STREAM_SCHEDULE="w0,w1,.." ... in segments of these relative lengths (default for resident bases: "3,13")
 *     MLHIP_TILE_LOG2=t                device-resident MSMs in tiles of 2^t pairs (0 = never; default 2^21 G1 / 2^20 G2 from 2^22 / 2^23)
 *     MLHIP_SORT_AHEAD=0, MLHIP_SORT_AHEAD_PRIO=0   tiles: sort of tile s+1 in line / on a default-priority stream
 *     MLHIP_SORT_TILE, MLHIP_CHUNK_LOG2, MLHIP_ACC_BLOCK, MLHIP_RED_BLOCK   kernel tile / chunk / workgroup sizes (sweeps)
 *     MLHIP_FIXED_BASE_MIN=n, MLHIP_FB_WINDOW=w, MLHIP_FB_CACHE=0   batched Mul of one base: table from n scalars on, width, no reuse
 *     MLHIP_EDWARDS=0                  BLS12-377 G1 over a checked SRS: keep the Weierstrass bucket sums
 *     MLHIP_BASES_TABLES=0|1           mlhip_bases_create: never / always keep shifted-base tables (default: see there)
 *     MLHIP_FOLD_WINDOW=c, MLHIP_FOLD_TILE_LOG2=t   ... their digit width (default 13 .. 20 by size) and tile (2^20 bases)
 *     MLHIP_BASES_SET_SHARE=0|1        MSMs on a set of handles: every member's own MSM in turn (also the A/B switch) / one upload
 *                                      and one sort train per geometry class at every size (default: see mlhip_bases_set_create)
 *     MLHIP_MSM_BATCH_CHUNK=P          mlhip_msm_batch*: pairs per chunk, 1, 2, 4 or 8 (default 4; 1 = one product per lane)
 *     MLHIP_MSM_BATCH_BUCKET_MIN=n     mlhip_msm_batch* and the table-free path of mlhip_bases_msm_batch*: segments of n pairs
 *                                      or more take the bucket route (default 512 for G1, 256 for G2; 0 = never, 1 .. 8 mean 9)
 *     MLHIP_MSM_BATCH_BUCKET_SLICE=s   ... pairs per slice of such a segment (default: 256 .. 4096, G2 256 .. 1024, by the size
 *                                      of the batch)
 *     MLHIP_SUM_DEVICE_MIN=n           mlhip_g1_sum / mlhip_g2_sum: smallest list summed on the device (0 = never, 1 = always;
 *                                      default 2^14 G1 / 2^12 G2)
 *     MLHIP_SUM_BATCH_SLICE=s          the batch calls with MLHIP_SCALARS_UNIT: points per slice, a power of two 1 .. 4096
 *                                      (default: the largest of 4 .. 32 that still fills the device's lanes, else 4)
 *     MLHIP_BASES_BATCH_WINDOW=w, MLHIP_BASES_BATCH_CHUNK=P   mlhip_bases_msm_batch*: table width 4 .. 12 (default 12), pairs
 *                                      per chunk on the table path, 1, 2, 4, 8 or 16 (default: the largest that fills 2^16 lanes)
 *     MLHIP_BASES_BATCH_MAX_MB=m       ... tables per handle at most m MB (default 1024; 0 = never: the table-free path)
 *     MLHIP_PAIRING_QUAD=0|1           BLS12-381: never / always one pairing per quad of lanes (default: up to 2^14 elements)
 *     MLHIP_G2_PREPARED_GENERAL=1      mlhip_*_prepared*: the general kernels on the Qs expanded from the handle (same bytes after FExp)
 *     MLHIP_MILLER_GROUP=1|2|4         products of more than four pairs (MLHIP_PRODUCT_PAIRS): pairs per Miller loop (default: 1 below
 *                                      2^17 pairs per call, 4 from there on)
 *   2nd impl (parity tests; DESIGN.md section 2 lists which test runs which)
 *     MLHIP_ACC32=1                    boundary-form (32-bit limb) bucket accumulation, G1 and G2
 *     MLHIP_REDUCE32=1, MLHIP_REDUCE_ONE_LANE=1   boundary-form / one-point-per-lane bucket reduction
 *     MLHIP_LEGACY_SORT=1              global-atomic sort (also the default above 2^24 pairs at c = 16)
 *     MLHIP_SCATTER_STAGED=0           round-1 coarse scatter (one store per entry)
 *     MLHIP_NO_QUAD_ACC=1              small MSMs: one bucket per lane instead of per quad
 *     MLHIP_G2_KC=1                    G2 buckets split by coordinate (one-lane Karatsuba Fp2 products; measured 3-5 % slower)
 *     MLHIP_PAIRING_ONE_LANE=1, MLHIP_PAIRING_SAT=1, MLHIP_SCALAR_MUL_ONE_LANE=1   one-lane / saturated-limb pairing and G2.Mul kernels
 *     MLHIP_SCALAR_MUL_ENDO=0          batched Mul with MLHIP_GROUP_SUBGROUP: the plain double-and-add kernels (also the A/B switch)
 *     MLHIP_MSM_BATCH_ENDO=0           mlhip_msm_batch* with MLHIP_CURVE_SUBGROUP_POINTS: the plain chunk kernels (also the A/B switch)
 *   tests only
 *     MLHIP_FAULT_INJECT=sort_helper_alloc   the sort-ahead helper allocation "fails" (tests/test_gpu_parity.py)
 */

#ifdef __cplusplus
}
#endif
#endif /* MLHIP_H */

// msm_kernels.h -- Pippenger MSM kernels and their launch sequence (gfx950).  Included by the per-curve
// translation units tu_msm_<curve>.hip.  Pipeline and data layout: DESIGN.md section 3.
//   k_coarse_hist / k_coarse_scatter / k_fine_sort   two-level LDS counting sort of the (window, bucket) keys
//                 (k_digits / k_scan / k_scatter: the global-atomic variant for n > 2^24, MLHIP_LEGACY_SORT=1)
//   k_order_*     buckets ordered by population, so that a wave's lanes run equally long loops
//   bucket accumulation: three steps, each written once over a bucket form (msm_accumulate.h: "bucket forms") --
//                 accumulate_seg_body: one bucket per lane (G2: per lane pair), acc += points28[idx] (mixed additions,
//                 gathered reads), on the state the segments before left; big_slices_body / accumulate_big_body: buckets
//                 longer than the threshold (skewed scalars) in slices of 4096 entries, one workgroup per slice (LDS
//                 tree), then the slice sums of each bucket into its state.  Forms and their kernels:
//     G1Form28    k_points_to28 / k_accumulate28_seg / k_big_slices28<.., false> / k_accumulate_big_seg   carry-free
//                 Weierstrass rows (fp28.h, ec28.h)
//     EdForm28    k_points_to_ed28 / k_accumulate_ed28_seg / k_big_slices28<.., true> / k_accumulate_big_seg_ed   G1 of a
//                 subgroup-trusted plan on a curve with a twisted Edwards model (BLS12-377): 7-product unified mixed
//                 additions (ed28.h, msm_ed.h), buckets handed on in extended coordinates
//     G2Form28    k_points_to28_g2 / k_accumulate28_lp_seg / k_big_slices_lp28 / k_accumulate_big_seg_g2   two lanes per
//                 bucket, one Fp2 component each (ec28_lp.h); G2KcForm28 / k_accumulate28_kc_seg: one coordinate pair each
//                 (ec28_kc.h; test build)
//   k_accumulate / k_accumulate_lp / k_big_slices / k_big_slices_lp   the same on 32-bit Montgomery limbs, written out by
//                 themselves: the second implementation the parity tests compare with (MLHIP_ACC32, test build); the
//                 slices also serve plain plans, whose long buckets gather the caller's boundary-form points
//   k_accumulate_q28   one bucket per quad of lanes for MSMs with few buckets (msm_accumulate.h)
//   bucket reduction: three levels and the LDS tree over a workgroup's lane groups, each written once over a reduction
//                 form (msm_reduce.h: "reduction forms") -- reduce_chunks_body: per 16 consecutive buckets sum and locally
//                 weighted sum; reduce_masked_body: per window the half / bit-masked sums of the chunk sums
//                 (msm_body.h: reduce_sel_index); group_combine_body: the groups of a folded plan into one window;
//                 group_tree_sum.  Forms and their kernels:
//     Quad28Form  k_chunks_q28 / k_masked_sums_q28 (<.., true>: Edwards)   G1, one point per quad of lanes on the
//                 accumulation's carry-free bucket state (ec_quad28.h)
//     Pair28Form  k_chunks_lp28   G2, lane pairs on the carry-free state (ec28_lp.h); k_masked_sums_lp28 is written out
//                 beside it (msm_g2.h: on the shared body it needed more scratch), as is the quad tree of the long G1
//                 buckets, block_tree_sum_q (msm_reduce.h)
//     QuadForm / PairForm   k_group_combine_q / _lp and the trees of the long buckets, in the boundary form; with
//                 k_chunks_q / k_masked_sums_q / k_chunks_lp / k_masked_sums_lp the test build's MLHIP_REDUCE32
//     LaneForm    k_chunks / k_masked_sums   one lane per point (MLHIP_REDUCE_ONE_LANE, test build)
//   k_msm_batch_chunk / k_msm_batch_sum (+ _lp for G2)   many small MSMs per call: Straus chunks of <= P pairs per lane,
//                 then segmented sums of <= 32 partials per lane (msm_batch.h)
//   k_msm_batch_chunk_endo (+ _lp)   the chunks of a call whose points are promised to be in G1 / G2: the scalar splits of
//                 msm_scalar_mul_endo.h per pair, half (G1, BN254 G2) or a quarter (BLS12 G2) of the shared doublings
//                 (msm_batch_endo.h)
//   k_msm_bucket_digits / k_msm_bucket_accumulate / k_msm_bucket_combine   the segments of such a call that are long enough
//                 for buckets: 7-bit digit bytes per slice, one wave per (slice, window) with one bucket per lane and an
//                 in-wave reduction, Horner per slice into the slice's row of the partials (msm_batch_bucket.h); _lp for G2
//                 (6-bit digits, one bucket per lane pair), _at / MsmBucketIndexed for the bases of a handle
//   k_bases_batch_chunk (+ _lp)   the same over a mlhip_bases handle: per-base fixed-window tables, ceil(256 / w) mixed
//                 additions per pair, no doubling (msm_bases_batch.h)
//   k_point_sum (+ _lp)   plain sums of many points (mlhip_g1_sum / mlhip_g2_sum above their threshold): strided slices per
//                 lane, then k_msm_batch_sum over the lanes' partials (point_sum.h)
//   k_sum_batch_slice (+ _lp)   K plain sums per call (mlhip_msm_batch* / mlhip_bases_msm_batch* with MLHIP_SCALARS_UNIT):
//                 strided slices of <= S points of one segment per lane, then k_msm_batch_sum (msm_sum_batch.h)
//   host tail     Horner over <= W*c bit positions + one inversion (O(1) work, 64-bit limbs)
// Launch sequence (msm_plan.h): plan_launch runs an MSM in one pass, stream_begin / stream_tile / stream_end as a train of
// segments or tiles cut by msm_segments.h (stream_segments, resident_tiles, shared_segments, stream_schedule,
// segment_cuts).  Both are orchestration of streams and events around the same steps: launch_sort, launch_convert (points
// into the carry-free form), launch_accumulate (THE choice of bucket kernel, with the long-bucket step: launch_big_slices
// and the kernel that adds the slice sums), launch_reduce, finish_train (reduce, copy to h_out, `done`).  What one pass does
// differently from a tile hangs on launch_accumulate's `one_pass` and is listed there and at plan_launch: it skips the
// long-bucket step below big_bucket_threshold, may take the quad kernel or the test build's MLHIP_ACC32 kernels,
// uploads a host-buffer call's points itself, sets the conv_* cache after every conversion, and places ev[0..3] / the wait
// for ev_join where the tiles place ev_tile / the waits for ev_seg.
// Replaces gnark-crypto's MultiExp behind MultiScalarMul (reference
// driver/gurvy/bls12381/bls12-381.go:766-783, driver/gurvy/bn254.go:232-245, driver/gurvy/bls12-377.go:229-242).
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include <type_traits>

#include "ec28.h"
#include "ec_jac.h"
#include "ed28.h"
#include "ec28_lp.h"
#include "ec28_kc.h"
#include "ec_quad.h"
#include "ec_quad28.h"
#include "fp2_lanes.h"
#include "mlhip_internal.h"
#include "msm_body.h"
#include "msm_fold_body.h"

namespace mlhip {

constexpr size_t QUAD_ACC_MAX_BUCKETS = 32768;  // up to here a G1 MSM accumulates one bucket per quad of lanes (k_accumulate_q28)
constexpr uint32_t BIG_BUCKET_MIN = 256;  // a bucket goes to the sliced long-bucket path above max(this, 8 x the mean length)
constexpr int CHUNK_L = 8;            // buckets per level-1 reduction thread

}  // namespace mlhip

#include "msm_sort.h"
#include "msm_reduce.h"
#include "msm_accumulate.h"
#include "msm_ed.h"
#include "msm_g2.h"
#include "msm_scalar_mul_endo.h"
#include "msm_scalar_mul.h"
#include "msm_batch.h"
#include "msm_batch_endo.h"
#include "msm_batch_bucket.h"
#include "point_sum.h"
#include "msm_sum_batch.h"
#include "msm_bases_batch.h"
#include "msm_fold.h"
#include "msm_tail.h"
#include "msm_plan.h"

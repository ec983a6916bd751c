// msm_plan.h -- host side of the MSM: plan allocation (entry_lists_alloc: the sort buffers, an MsmEntryLists; plan_alloc: the
// rest), the launch steps both sequences share (launch_sort, launch_convert, launch_accumulate, launch_reduce, finish_train),
// the two sequences themselves (plan_launch: one pass; plan_stream_train: the one train of segments or tiles over
// stream_begin / stream_tile / stream_end, cut by msm_segments.h, for one plan or a class of plans) and the host tail.
// Part of msm_kernels.h.
#pragma once
// (included by msm_kernels.h after its common headers and constants; msm_segments.h comes with mlhip_internal.h)

namespace mlhip {

// G2 runs in the carry-free lane-pair form (ec28_lp.h: bucket loop, segment / tile state, lane-pair reduction) on every curve
// since round 3 -- BLS12-381 first (-14 % accumulation), then BLS12-377 (u^2 = -5: 2^20 points 12.35 -> 9.45 ms) and BN254
// (10 limbs: 5.25 -> 4.95 ms); MLHIP_ACC32=1 keeps the boundary-form kernels as the second implementation

// G2 bucket accumulation (carry-free form): lane pairs split by component with dual products (k_accumulate28_lp_seg, default)
// or by coordinate with one-lane Karatsuba Fp2 products (k_accumulate28_kc_seg, MLHIP_G2_KC=1: 16 % fewer multiplier
// instructions per addition, but three 64-bit column combinations per product column and 130 spilled registers instead of
// 63 -- measured 3-5 % SLOWER; kept as a second implementation for the parity tests).  Read per launch
// so that a test can switch paths; both leave bit-identical bucket states.
static inline bool g2_split_by_coordinate() { return mlhip_alt_switch("MLHIP_G2_KC"); }

// Does this plan sum its buckets in twisted Edwards coordinates (ed28.h)?  G1 of a curve with the model, the SRS promise
// (mlhip_msm_plan_assume_srs, or a table mlhip_bases_create has checked: every point in the subgroup, and the converted copy
// made once -- converting per launch costs what the cheaper additions save: 0.95 ms for 2^20 points), the carry-free
// state the reduction reads, and enough buckets for one lane each (the quad-lane kernel of small MSMs stays on XYZZ).
// MLHIP_EDWARDS=0: never (the Weierstrass kernels stay the second implementation).
template <class C, class F>
inline bool plan_use_edwards(const mlhip_msm_plan* p) {
  if constexpr (C::HAS_EDWARDS && std::is_same<F, FpField<C>>::value) {
    const char* e = getenv("MLHIP_EDWARDS");
    return p->trust_subgroup && p->points_static && p->reduce28 && p->d_points28 && (size_t)p->W * p->M > QUAD_ACC_MAX_BUCKETS &&
           p->points28_elem >= sizeof(EdNiels28<C>) && !(e && e[0] == '0');
  }
  return false;
}

// Scalars one sort of a plan covers: all max_n, or -- a folded plan (msm_fold.h) sorts one tile of its table at a time -- at
// most fold_tile of them, Wd entries each, whose indices run over the Wd fold_tile rows of the tile.
inline size_t plan_sort_capacity(const mlhip_msm_plan* p) { return p->fold ? std::min(p->max_n, p->fold_tile) : p->max_n; }
// Entries one scalar puts into ONE set of 2^(c-1) buckets: a folded plan's digits all share the set.
inline size_t entries_per_bucket_set(const mlhip_msm_plan* p) { return p->fold ? (size_t)p->Wd : 1; }

// An empty record of p's sort geometry for sorts of up to `cap` scalars: the plan's own, or a sort-ahead record.  The one
// place that copies the geometry.
inline MsmEntryLists plan_entry_lists(const mlhip_msm_plan* p, size_t cap) {
  MsmEntryLists l;
  l.c = p->c;
  l.bits = p->bits;
  l.W = p->W;
  l.Wd = p->Wd;
  l.M = p->M;
  l.fold = p->fold;
  l.fold_tile = p->fold_tile;
  l.cap = cap;
  l.device = p->device;
  return l;
}

// the buffers launch_sort works in, for the geometry and capacity the record holds; on failure entry_lists_free takes
// back what was allocated
inline int entry_lists_alloc(MsmEntryLists* p) {
  const size_t nbuckets = (size_t)p->W * p->M;
  const size_t sort_n = p->cap;
  HIPCHK(hipMalloc(&p->d_digits, (size_t)p->Wd * sort_n * 4));
  HIPCHK(hipMalloc(&p->d_sorted, (size_t)p->Wd * sort_n * 4));
  {
    // sort parameters: packed entry = fine bits | sign | index must fit 32 bits, coarse bins must fit LDS
    int idx_bits = 1;
    while (((size_t)1 << idx_bits) < (p->fold ? (size_t)p->Wd * p->fold_tile : p->cap)) idx_bits++;
    int low = p->c - 1 < 8 ? p->c - 1 : 8;
    if (low > 31 - idx_bits) low = 31 - idx_bits;
    const char* legacy = getenv("MLHIP_LEGACY_SORT");
    uint32_t nb = low >= 1 ? (uint32_t)(nbuckets >> low) : 0;  // (plain plan: W << (c - 1 - low))
    if (low < 1 || nb > 4096 || (legacy && legacy[0] == '1' && !p->fold)) {
      p->sort_low = 0;
      p->sort_nb = 0;
    } else {
      p->sort_low = low;
      p->sort_nb = nb;
    }
    p->sort_idx_bits = idx_bits;
  }
  // zeroed every run: [counts | cursor | bigcount(4) | coarse_count | coarse_cursor]
  p->zero_bytes = (2 * nbuckets + 4 + 2 * (size_t)p->sort_nb) * 4;
  HIPCHK(hipMalloc(&p->d_zero, p->zero_bytes));
  p->d_counts = p->d_zero;
  p->d_cursor = p->d_zero + nbuckets;
  p->d_bigcount = p->d_zero + 2 * nbuckets;
  p->d_coarse_count = p->d_zero + 2 * nbuckets + 4;
  p->d_coarse_cursor = p->d_coarse_count + p->sort_nb;
  HIPCHK(hipMalloc(&p->d_coarse_off, ((size_t)p->sort_nb + 1) * 4));
  HIPCHK(hipMalloc(&p->d_binprefix, ((size_t)p->sort_nb + 2) * 4));
  if (p->sort_nb) {
    static_assert(SORT_TILE_MAX < 65536, "a block puts at most one entry per scalar into a coarse bin: the count fits 16 bits");
    const size_t blocks = (sort_n + SORT_TILE - 1) / SORT_TILE;
    HIPCHK(hipMalloc(&p->d_blockhist, blocks * p->sort_nb * sizeof(uint16_t)));
  }
  HIPCHK(hipMalloc(&p->d_offsets, nbuckets * 4));
  HIPCHK(hipMalloc(&p->d_order, nbuckets * 4));
  {
    const size_t nblk = (nbuckets + 255) / 256;
    const size_t hist_n = (size_t)ORDER_BINS * nblk;
    HIPCHK(hipMalloc(&p->d_hist, hist_n * 4));
    const size_t tiles = (std::max(nbuckets, hist_n) + SCAN_TILE - 1) / SCAN_TILE;
    HIPCHK(hipMalloc(&p->d_tilesums, (tiles + 1) * 4));
  }
  return 0;
}

template <class F>
int plan_alloc(mlhip_msm_plan* p) {
  const size_t nbuckets = (size_t)p->W * p->M;
  p->pt_size = sizeof(Affine<F>);
  p->xyzz_size = sizeof(XYZZ<F>);
  {
    p->lists = plan_entry_lists(p, plan_sort_capacity(p));
    int rc_sort = entry_lists_alloc(&p->lists);
    if (rc_sort) return rc_sort;
  }
  HIPCHK(hipMalloc(&p->d_biglist, nbuckets * 4));
  {
    // long buckets: at most W n / BIG_BUCKET_MIN of them, and W n / BIG_SLICE + one more slice per bucket
    const size_t entries = (size_t)p->Wd * plan_sort_capacity(p);
    const size_t nbig_max = std::min(nbuckets, entries / BIG_BUCKET_MIN + 1);
    HIPCHK(hipMalloc(&p->d_bigprefix, (nbig_max + 2) * 4));
    HIPCHK(hipMalloc(&p->d_bigpart, (entries / BIG_SLICE + nbig_max + 2) * p->xyzz_size));
  }
  if (const char* e = getenv("MLHIP_RED_BLOCK")) {
    const int v = atoi(e);
    if (v == 64 || v == 128 || v == 256) p->red_block = v;
  }
  if (const char* e = getenv("MLHIP_ACC_BLOCK")) {
    const int v = atoi(e);
    if (v == 64 || v == 128 || v == 256) p->acc_block = v;
  }
  {
    p->reduce_one_lane = mlhip_alt_switch("MLHIP_REDUCE_ONE_LANE");  // =1: the one-point-per-lane reduction kernels
  }
  if constexpr (std::is_same<F, FpField<typename F::Curve>>::value) {
    // G1 accumulation runs in the carry-free form (fp28.h): -24 % time for the 12-limb fields, -7 % for BN254.
    // MLHIP_ACC32=1 selects the boundary-form kernel (kept as the second implementation the tests compare with).
    const bool want28 = !mlhip_alt_switch("MLHIP_ACC32");
    // (a curve with a twisted Edwards model grows the buffer to the Niels triples' 168 B a point when the SRS promise is made)
    constexpr size_t kPoint28 = sizeof(Affine28<typename F::Curve>);
    if (want28 && p->fold) {
      p->points28_elem = 0;  // the table is allocated by plan_fold_build, in the form the plan will read
      p->points28_elem_ed = F::Curve::HAS_EDWARDS ? sizeof(EdNiels28<typename F::Curve>) : 0;
    } else if (want28) {
      HIPCHK(hipMalloc(&p->d_points28, p->max_n * kPoint28));
      p->points28_elem = kPoint28;
      p->points28_elem_ed = F::Curve::HAS_EDWARDS ? sizeof(EdNiels28<typename F::Curve>) : 0;
    }
    // ... and so does the quad-lane reduction, on the accumulators as the kernel leaves them (MLHIP_REDUCE32=1: the
    // boundary-form reduction kernels, kept as the second implementation)
    p->reduce28 = want28 && !p->reduce_one_lane && !mlhip_alt_switch("MLHIP_REDUCE32");
    if (p->reduce28) HIPCHK(hipMalloc(&p->d_state28, nbuckets * sizeof(XYZZ28<typename F::Curve>)));
  }
  if constexpr (std::is_same<F, Fp2Field<typename F::Curve>>::value) {
    // G2 in the carry-free form (above)
    if (!mlhip_alt_switch("MLHIP_ACC32")) {
      if (!p->fold) HIPCHK(hipMalloc(&p->d_points28, p->max_n * sizeof(AffineG2_28<typename F::Curve>)));
      // ... and the lane-pair reduction reads the accumulators as the kernel leaves them (MLHIP_REDUCE32=1: boundary form)
      p->reduce28 = !mlhip_alt_switch("MLHIP_REDUCE32");
      if (p->reduce28) HIPCHK(hipMalloc(&p->d_state28, nbuckets * 2 * sizeof(XYZZ28L<Fp28<typename F::Curve>>)));
    }
  }
  HIPCHK(hipMalloc(&p->d_buckets, nbuckets * p->xyzz_size));
  {
    size_t chunk_size = p->xyzz_size;
    if constexpr (std::is_same<F, FpField<typename F::Curve>>::value)
      chunk_size = std::max(chunk_size, sizeof(XYZZ28<typename F::Curve>));
    else
      chunk_size = std::max(chunk_size, 2 * sizeof(XYZZ28L<Fp28<typename F::Curve>>));
    HIPCHK(hipMalloc(&p->d_A, (size_t)p->W * p->T * chunk_size));
    HIPCHK(hipMalloc(&p->d_W0, (size_t)p->W * p->T * chunk_size));
  }
  if (p->fold && p->W > 1 && p->W <= 32 && p->reduce28) {  // (group_combine_body: G1 on quads, G2 on lane pairs)
    int lgW = 0;
    while ((1 << lgW) < p->W) lgW++;
    p->fold_nsel2 = 4 + p->nb + lgW;
  }
  HIPCHK(hipMalloc(&p->d_out, ((size_t)p->W * p->nsel + p->fold_nsel2) * p->xyzz_size));
  if (p->device_result) {
    // a device-result plan (msm_tail.h): no host copy of the partial sums; the tail kernel writes [affine | XYZZ] here
    HIPCHK(hipMalloc(&p->d_result, p->pt_size + p->xyzz_size));
    for (int i = 0; i < 2; i++) HIPCHK(hipEventCreate(&p->ev_tail[i]));
  } else {
    HIPCHK(hipHostMalloc(&p->h_out, ((size_t)p->W * p->nsel + p->fold_nsel2) * p->xyzz_size, hipHostMallocDefault));
  }
  for (int i = 0; i < 5; i++) HIPCHK(hipEventCreate(&p->ev[i]));
  HIPCHK(hipEventCreateWithFlags(&p->done, hipEventDisableTiming));
  {  // the auxiliary stream: point conversion beside the sort, and the uploads of a streamed host-buffer MSM
    HIPCHK(hipStreamCreateWithFlags(&p->aux, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&p->ev_join, hipEventDisableTiming));
  }
  return 0;
}

// total = sum_w 2^off(w) V_w,  V_w = out[w][0..3] summed + 2^lgL sum_k 2^k out[w][4+k]
// (window w starts at bit off(w): msm_win_layout, widths differ by at most one bit).  The V_w are independent chains of
// nb + lgL doublings and nb + 4 additions each -- two thirds of the tail's field products -- and run on the library's host
// workers (mlhip_rt::host_parallel); what stays sequential is the Horner pass over the windows, one doubling per scalar
// bit.  2^20 points, c = 16: 0.20 -> 0.10 ms.  MLHIP_HOST_THREADS=1 keeps everything on the calling thread.
// (host_parallel copies its input blob: {nb, lgL, nsel} then the W x nsel partial sums as the device left them)
// A folded plan (msm_fold.h): job g < W is the weighted sum V_g of bucket group g (as a window's), job W + g its PLAIN sum
// S_g = out[g][2] + out[g][3] (the two halves of sum_t A[g][t]).  Bucket b of group g has weight g M + b + 1, so
//   total = sum_g V_g + M sum_g g S_g
// -- lg M doublings in all, where the windows of a plain plan need one per scalar bit.
template <class F>
void host_tail_group(const void* in, int job, void* out) {
  const HostTailHeader& h = *static_cast<const HostTailHeader*>(in);
  const int W = h.pad;
  if (job < W) {
    host_tail_window<F>(in, job, out);
    return;
  }
  const XYZZ<F>* o = reinterpret_cast<const XYZZ<F>*>(static_cast<const unsigned char*>(in) + sizeof(HostTailHeader)) + (size_t)(job - W) * h.nsel;
  XYZZ<F> acc = o[2];
  xyzz_add<F>(acc, o[3]);
  memcpy(out, &acc, sizeof(acc));
}
template <class F>
void host_tail_fold(const mlhip_msm_plan* p, XYZZ<F>& total) {
  if (p->fold_nsel2) {
    // the device has combined the groups (group_combine_body): one window of W T chunks, summed on this thread
    const size_t sums2 = (size_t)p->fold_nsel2 * sizeof(XYZZ<F>);
    std::vector<unsigned char> blob2(sizeof(HostTailHeader) + sums2);
    const HostTailHeader h2{p->fold_nsel2 - 4, p->lgL, p->fold_nsel2, 0};
    memcpy(blob2.data(), &h2, sizeof(h2));
    memcpy(blob2.data() + sizeof(h2), static_cast<const XYZZ<F>*>(p->h_out) + (size_t)p->W * p->nsel, sums2);
    host_tail_window<F>(blob2.data(), 0, &total);
    return;
  }
  const size_t sums = (size_t)p->W * p->nsel * sizeof(XYZZ<F>);
  std::vector<unsigned char> blob(sizeof(HostTailHeader) + sums);
  const HostTailHeader h{p->nb, p->lgL, p->nsel, p->W};
  memcpy(blob.data(), &h, sizeof(h));
  memcpy(blob.data() + sizeof(h), p->h_out, sums);
  const int W = p->W;
  std::vector<XYZZ<F>> VS(2 * (size_t)W);
  mlhip_rt::host_parallel(W > 1 ? 2 * W : 1, host_tail_group<F>, blob.data(), blob.size(), VS.data(), sizeof(XYZZ<F>));
  // sum_g g S_g as a running sum from the top group down (run += S_g; hi += run), then the lg M doublings
  XYZZ<F> run, hi;
  xyzz_set_inf<F>(run);
  xyzz_set_inf<F>(hi);
  for (int g = W - 1; g >= 1; g--) {
    xyzz_add<F>(run, VS[(size_t)W + g]);
    xyzz_add<F>(hi, run);
  }
  int lgM = 0;
  while ((1u << lgM) < p->M) lgM++;
  const int down0 = lgM;
  horner_jac<F>(total, &hi, 1, &down0);  // total = 2^lgM hi
  for (int g = 0; g < W; g++) xyzz_add<F>(total, VS[g]);
}

template <class F>
void host_tail(const mlhip_msm_plan* p, XYZZ<F>& total) {
  if (p->fold) {
    host_tail_fold<F>(p, total);
    return;
  }
  const size_t sums = (size_t)p->W * p->nsel * sizeof(XYZZ<F>);
  std::vector<unsigned char> blob(sizeof(HostTailHeader) + sums);
  const HostTailHeader h{p->nb, p->lgL, p->nsel, 0};
  memcpy(blob.data(), &h, sizeof(h));
  memcpy(blob.data() + sizeof(h), p->h_out, sums);
  std::vector<XYZZ<F>> V(p->W);
  mlhip_rt::host_parallel(p->W, host_tail_window<F>, blob.data(), blob.size(), V.data(), sizeof(XYZZ<F>));
  // the sequential part: one doubling per scalar bit.  In Jacobian coordinates since round 4 (ec_jac.h: 2M + 5S a doubling
  // instead of 6M + 3S; the 16 additions are dearer and do not matter)
  std::vector<int> down(p->W, 0);
  msm_window_shifts(p->bits, p->c, down.data());  // (a short-scalar plan: its own, shorter layout)
  horner_jac<F>(total, V.data(), p->W, down.data());
}

// slice sums of the long buckets listed by the accumulation kernel (nothing to do, two near-empty launches, when
// there are none)
// (`row0`: a folded plan keeps carry-free rows only -- the slices gather from d_points28 + row0, in the form the table holds;
// `sv`: the entry lists (sorted / offsets / counts) that describe this tile; the long-bucket count is p's own)
template <class F>
void launch_big_slices(mlhip_msm_plan* p, const Affine<F>* d_points, hipStream_t st, const MsmEntryLists* sv, size_t row0) {
  typedef typename F::Curve C;
  constexpr bool kG2 = std::is_same<F, Fp2Field<C>>::value;
  constexpr int BLOCK = 256;  // one XYZZ<F> of LDS per lane (G2: per lane pair): 48 KB for both groups
  k_big_prefix<<<dim3(1), dim3(1024), 0, st>>>(sv->d_counts, p->d_biglist, p->lists.d_bigcount, p->d_bigprefix);
  auto slices = [&](auto kernel, auto rows) {
    kernel<<<dim3(1024), dim3(BLOCK), (BLOCK / (kG2 ? 2 : 1)) * sizeof(XYZZ<F>), st>>>(
        rows, sv->d_sorted, sv->d_offsets, sv->d_counts, p->d_biglist, p->lists.d_bigcount, p->d_bigprefix, (XYZZ<F>*)p->d_bigpart);
  };
  if (!p->fold) {  // a plain plan: the boundary-form rows the caller gave
    if constexpr (kG2)
      slices(k_big_slices_lp<C, BLOCK>, d_points);
    else
      slices(k_big_slices<F, BLOCK>, d_points);
    return;
  }
  // a folded plan: the carry-free rows of its table, in the form the table holds
  if constexpr (kG2) {
    slices(k_big_slices_lp28<C, BLOCK>, (const AffineG2_28<C>*)p->d_points28 + row0);
  } else {
    if constexpr (C::HAS_EDWARDS) {
      if (p->conv_ed) return slices(k_big_slices28<C, BLOCK, true>, (const void*)((const EdNiels28<C>*)p->d_points28 + row0));
    }
    slices(k_big_slices28<C, BLOCK, false>, (const void*)((const Affine28<C>*)p->d_points28 + row0));
  }
}

// digits -> entries sorted by (window, bucket) in d_sorted / d_offsets / d_counts, and the bucket order by population
// (`p`: the record sorted into, zeroed by the caller; `ev_digits`: recorded once the digits are taken -- null: no event)
template <class C>
int launch_sort(const MsmEntryLists* p, const void* d_scalars, int mont, size_t n, hipStream_t st, hipEvent_t ev_digits) {
  const size_t nbuckets = (size_t)p->W * p->M;
  const int Wd = p->Wd;  // entries per scalar (== W on a plain plan)
  const uint32_t fold_stride = p->fold ? (uint32_t)p->fold_tile : 0u;
  if (p->fold && (p->sort_low <= 0 || n > p->fold_tile))
    return mlhip_rt::fail(MLHIP_EINVAL, "folded plan: a sort covers at most one tile of the table, on the two-level path");
  if (p->sort_low > 0) {
    // two-level LDS counting sort (no per-key global atomics)
    int tile = sort_tile_for(n);
    // (a folded plan's digits share the bins: a block may put tile * Wd entries into one bin, and the count is 16-bit)
    // (plan_create_ex admits only digit counts for which the smallest tile fits: Wd SORT_TILE < 65536)
    while (p->fold && tile > SORT_TILE && (size_t)tile * Wd >= 65536) tile /= 2;
    const uint32_t NB = p->sort_nb;
    // entries staged in LDS and written bin by bin (k_coarse_scatter_staged) when a block's tile * W entries fit beside
    // the three bin tables -- the tile shrinks to make them fit; MLHIP_SCATTER_STAGED=0: one store per entry (round 1)
    const char* staged_env = getenv("MLHIP_SCATTER_STAGED");  // read per launch so that a test can switch paths
    const bool staged_on = !(staged_env && staged_env[0] == '0');
    constexpr size_t kLdsMax = 160 * 1024 - 256;
    auto staged_lds = [&](int t) { return (3 * (size_t)NB + (size_t)t * Wd) * 4; };
    bool staged = false;
    if (staged_on) {
      int t = tile;
      while (t > 1024 && staged_lds(t) > kLdsMax) t /= 2;
      if (staged_lds(t) <= kLdsMax) {
        tile = t;
        staged = true;
      }
    }
    const unsigned blocks = (unsigned)((n + tile - 1) / tile);
    k_coarse_hist<C><<<dim3(blocks), dim3(256), NB * 4, st>>>((const uint32_t*)d_scalars, n, mont, p->c, Wd, p->sort_low, NB,
                                                            p->d_coarse_count, p->d_blockhist, tile, fold_stride, p->bits);
    if (ev_digits) HIPCHK(hipEventRecord(ev_digits, st));
    launch_scan(p->d_coarse_count, p->d_coarse_off, p->d_tilesums, NB, st);
    if (staged) {
      int group = 1;  // lanes per bin in the write-out: the mean run length, rounded down to a power of two
      while (group < 64 && (size_t)group * 2 * NB <= (size_t)tile * Wd) group *= 2;
      HIPCHK(hipFuncSetAttribute((const void*)k_coarse_scatter_staged<C>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
      k_coarse_scatter_staged<C><<<dim3(blocks), dim3(1024), staged_lds(tile), st>>>(
          (const uint32_t*)d_scalars, n, mont, p->c, Wd, p->sort_low, p->sort_idx_bits, NB, p->d_coarse_off, p->d_coarse_cursor,
          p->d_digits, p->d_blockhist, tile, group, fold_stride, p->bits);
    } else {
      k_coarse_scatter<C><<<dim3(blocks), dim3(256), NB * 8, st>>>((const uint32_t*)d_scalars, n, mont, p->c, Wd, p->sort_low,
                                                                 p->sort_idx_bits, NB, p->d_coarse_off, p->d_coarse_cursor,
                                                                 p->d_digits, p->d_blockhist, tile, fold_stride, p->bits);
    }
    // bins more than 8x the mean (and at least 32768 entries) are sorted by many workgroups
    const uint32_t big_bin = (uint32_t)std::min<size_t>(std::max<size_t>(32768, 8 * ((size_t)Wd * n / NB)), 0x7fffffffu);
    k_fine_sort<<<dim3(NB), dim3(256), 0, st>>>(p->d_digits, p->d_coarse_off, p->d_coarse_count, p->c, p->sort_low,
                                               p->sort_idx_bits, big_bin, p->d_counts, p->d_offsets, p->d_sorted);
    if ((size_t)Wd * n > big_bin) {  // a bin holds at most all W n entries: small MSMs skip three near-empty launches
      k_bigbin_prefix<<<dim3(1), dim3(1024), 0, st>>>(p->d_coarse_count, NB, big_bin, p->d_binprefix);
      k_bigbin_hist<<<dim3(1024), dim3(256), 0, st>>>(p->d_digits, p->d_coarse_off, p->d_coarse_count, p->d_binprefix, NB,
                                                     p->sort_low, p->sort_idx_bits, p->d_counts);
      k_bigbin_place<<<dim3(1024), dim3(256), 0, st>>>(p->d_digits, p->d_coarse_off, p->d_coarse_count, p->d_binprefix, NB,
                                                      p->sort_low, p->sort_idx_bits, p->d_counts, p->d_cursor, p->d_offsets,
                                                      p->d_sorted);
    }
  } else {
    // legacy path (very large n or MLHIP_LEGACY_SORT=1): digits array + global-atomic histogram / scatter
    {
      size_t blocks = (n + 255) / 256;
      if (blocks > 65536) blocks = 65536;
      k_digits<C><<<dim3((unsigned)blocks), dim3(256), 0, st>>>((const uint32_t*)d_scalars, n, mont, p->c, p->W, p->M,
                                                                 p->d_digits, p->d_counts, p->bits);
    }
    if (ev_digits) HIPCHK(hipEventRecord(ev_digits, st));
    launch_scan(p->d_counts, p->d_offsets, p->d_tilesums, nbuckets, st);
    {
      size_t total_e = (size_t)p->W * n;
      size_t blocks = (total_e + 255) / 256;
      if (blocks > 262144) blocks = 262144;
      k_scatter<<<dim3((unsigned)blocks), dim3(256), 0, st>>>(p->d_digits, n, p->W, p->M, p->d_offsets, p->d_cursor,
                                                               p->d_sorted);
    }
  }
  {
    const unsigned nblk = (unsigned)((nbuckets + 255) / 256);
    k_order_hist<<<dim3(nblk), dim3(256), 0, st>>>(p->d_counts, nbuckets, p->d_hist);
    launch_scan(p->d_hist, p->d_hist, p->d_tilesums, (size_t)ORDER_BINS * nblk, st);
    k_order_place<<<dim3(nblk), dim3(256), 0, st>>>(p->d_counts, nbuckets, p->d_hist, p->d_order);
  }
  return 0;
}

// LDS of a masked-sum block of RB threads: one slot per lane group, half of that where the form's tree hands over first
template <class R, int RB>
constexpr size_t reduce_masked_lds() {
  return (size_t)(RB / R::LANES / (R::TREE_HAND_OVER ? 2 : 1)) * R::MEMS * sizeof(typename R::Mem);
}

// One path of the reduction over the form R: chunk sums, masked sums (RB threads a block) and, for a folded plan, the
// combine of the groups' sums into one window's (`combine` null: the path has none).  MLHIP_RED_BLOCK sizes the chunk
// blocks of the quad kernels.
template <class R, int RB>
void launch_reduce_kernels(mlhip_msm_plan* p, hipStream_t st, const void* buckets,
                           void (*chunks)(const typename R::Mem*, size_t, int, typename R::Mem*, typename R::Mem*),
                           void (*masked)(const typename R::Mem*, const typename R::Mem*, uint32_t, int, XYZZ<typename R::BF>*),
                           void (*combine)(const XYZZ<typename R::BF>*, int, int, int, XYZZ<typename R::BF>*),
                           unsigned combine_threads, size_t combine_lds) {
  typedef typename R::Mem Mem;
  typedef XYZZ<typename R::BF> X;
  const size_t n_chunks = (size_t)p->W * p->T;
  const unsigned cb = R::LANES == 4 ? (unsigned)p->red_block : 256u;
  chunks<<<dim3((unsigned)((R::LANES * n_chunks + cb - 1) / cb)), dim3(cb), 0, st>>>((const Mem*)buckets, n_chunks, p->L,
                                                                                     (Mem*)p->d_A, (Mem*)p->d_W0);
  masked<<<dim3((unsigned)(p->W * p->nsel)), dim3(RB), reduce_masked_lds<R, RB>(), st>>>(
      (const Mem*)p->d_A, (const Mem*)p->d_W0, p->T, p->nsel, (X*)p->d_out);
  if (combine && p->fold_nsel2)
    combine<<<dim3((unsigned)p->fold_nsel2), dim3(combine_threads), combine_lds, st>>>(
        (const X*)p->d_out, p->W, p->nsel, p->nb, (X*)p->d_out + (size_t)p->W * p->nsel);
}

// bucket sums in d_buckets (boundary form) or d_state28 (the accumulation's carry-free state, MLHIP_SEG_KEEP28) -> W x nsel
// partial sums in d_out (two levels: chunks of L buckets, bit-masked sums): picks the reduction form (msm_reduce.h)
template <class C, class F>
int launch_reduce(mlhip_msm_plan* p, hipStream_t st) {
  typedef XYZZ<F> X;
  constexpr int RB = 512;  // 128 quads or 256 lane pairs a block
  if constexpr (std::is_same<F, Fp2Field<C>>::value) {  // G2: two lanes per bucket
    // the combine: one lane pair per input slot
    const unsigned gthreads = (unsigned)(4 * p->W);
    const size_t glds = 2 * p->W * sizeof(X);
    if (p->reduce28) {
      static_assert(reduce_masked_lds<Pair28Form<C>, RB>() == (RB / 4) * 2 * sizeof(XYZZ28L<Fp28<C>>), "128 slots x 448 B = 56 KB");
      launch_reduce_kernels<Pair28Form<C>, RB>(p, st, p->d_state28, k_chunks_lp28<C>, k_masked_sums_lp28<C, RB>,
                                               k_group_combine_lp<C, 128>, gthreads, glds);
    } else if constexpr (kBuildAlt) {  // (boundary-form lane pairs: MLHIP_REDUCE32 / MLHIP_ACC32, test build only)
      static_assert(reduce_masked_lds<PairForm<C>, RB>() == (RB / 4) * sizeof(X), "128 slots x 384 B = 48 KB");
      launch_reduce_kernels<PairForm<C>, RB>(p, st, p->d_buckets, k_chunks_lp<C>, k_masked_sums_lp<C, RB>, nullptr, 0, 0);
    } else {
      return mlhip_rt::fail(MLHIP_EINVAL, "G2 reduction: the carry-free bucket state is missing");
    }
  } else {
    // the combine: one quad per input slot, at least a wave; a slot for every quad of its launch bound
    constexpr int GB = 256;
    const unsigned gthreads = (unsigned)std::max(64, 8 * p->W);
    constexpr size_t glds = GB / QuadForm<C>::LANES * sizeof(X);
    static_assert(glds == 64 * sizeof(X), "64 slots");
    if (p->reduce28) {
      static_assert(reduce_masked_lds<Quad28Form<C, false>, RB>() == (RB / 4) * sizeof(XYZZ28<C>), "128 slots: 28 KB");
      if constexpr (C::HAS_EDWARDS) {
        if (p->last_ed) {  // the buckets are in extended twisted Edwards coordinates (msm_ed.h): the same kernels on that addition
          launch_reduce_kernels<Quad28Form<C, true>, RB>(p, st, p->d_state28, k_chunks_q28<C, true>, k_masked_sums_q28<C, RB, true>,
                                                         k_group_combine_q<C, GB>, gthreads, glds);
          return 0;  // (both forms leave Weierstrass sums: one combine)
        }
      }
      launch_reduce_kernels<Quad28Form<C, false>, RB>(p, st, p->d_state28, k_chunks_q28<C>, k_masked_sums_q28<C, RB>,
                                                      k_group_combine_q<C, GB>, gthreads, glds);
    } else if constexpr (kBuildAlt) {  // boundary-form reductions: test build only
      if (p->reduce_one_lane) {  // MLHIP_REDUCE_ONE_LANE=1 when the plan was created
        static_assert(reduce_masked_lds<LaneForm<F>, 256>() == 256 * sizeof(X), "256 slots: 48 KB");
        launch_reduce_kernels<LaneForm<F>, 256>(p, st, p->d_buckets, k_chunks<F>, k_masked_sums<F, 256>, nullptr, 0, 0);
      } else {
        static_assert(reduce_masked_lds<QuadForm<C>, RB>() == (RB / 4) * sizeof(X), "128 slots: 24 KB");
        launch_reduce_kernels<QuadForm<C>, RB>(p, st, p->d_buckets, k_chunks_q<C>, k_masked_sums_q<C, RB>, nullptr, 0, 0);
      }
    } else {
      return mlhip_rt::fail(MLHIP_EINVAL, "G1 reduction: the carry-free bucket state is missing");
    }
  }
  return 0;
}

template <class C>
int plan_stream_train(mlhip_msm_plan* const* ps, void* const* d_points, const void* const* h_points, int k, void* d_scalars,
                      const void* h_scalars, int mont, size_t n, int K, bool schedule, hipStream_t st);

// ---- the steps plan_launch (one pass) and stream_tile / stream_end (a train of segments or tiles) share -------------------

// A folded plan's points are its own table (plan_fold_build): a call brings none of its own, and at most fold_n scalars.
inline int fold_check_args(const mlhip_msm_plan* p, size_t n, bool points_travel) {
  if (points_travel || n > p->fold_n || !p->d_points28)
    return mlhip_rt::fail(MLHIP_EINVAL, "folded plan: the points are the plan's table; more scalars than tabulated bases, or no table");
  return 0;
}

// Buckets far longer than the mean (degenerate inputs: equal scalars, tiny scalars) are handed to a whole
// workgroup each; the threshold scales with the mean length len / 2^(c-1) so that large inputs, and the sparser top
// window (2-4x the mean for these group orders), stay on the one-thread-per-bucket path.
// (a folded plan's buckets collect the entries of all Wd digits: the mean is Wd len / 2^(c-1))
inline uint32_t big_bucket_threshold(const mlhip_msm_plan* p, size_t len) {
  const uint32_t t = (uint32_t)std::min<size_t>(((entries_per_bucket_set(p) * len) >> (p->c - 1)) * 8, 1u << 30);
  return t < BIG_BUCKET_MIN ? BIG_BUCKET_MIN : t;
}

// `len` points at `src` into the carry-free form the plan accumulates from, at row `dst_row` of d_points28: G2 lane-pair
// rows, G1 Niels triples (`ed`) or Weierstrass rows.  The caller owns the upload before it, the events around it and the
// conv_* bookkeeping.
template <class C, class F>
void launch_convert(const mlhip_msm_plan* p, const Affine<F>* src, size_t len, size_t dst_row, bool ed, hipStream_t st) {
  if constexpr (std::is_same<F, Fp2Field<C>>::value) {
    k_points_to28_g2<C><<<dim3((unsigned)((4 * len + 255) / 256)), dim3(256), 0, st>>>(src, len, (AffineG2_28<C>*)p->d_points28 + dst_row);
  } else {
    if constexpr (C::HAS_EDWARDS) {
      if (ed) {
        k_points_to_ed28<C><<<dim3((unsigned)(((len + 3) / 4 + 255) / 256)), dim3(256), 0, st>>>(src, len, (EdNiels28<C>*)p->d_points28 + dst_row);
        return;
      }
    }
    k_points_to28<C><<<dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st>>>(src, len, (Affine28<C>*)p->d_points28 + dst_row);
  }
}

// The bucket accumulation of one segment of `len` scalars, and the long-bucket step that belongs to it (k_big_prefix, the
// slices, the kernel that adds the slice sums): the one place that picks these kernels.
//   sv        the entry lists (sorted / offsets / counts / order) that describe the segment: p's own, a sort-ahead record,
//             or those of the first plan of a shared-scalar train.  The count of long buckets is always p's own.
//   row0      first carry-free row of the segment in d_points28 (a folded plan: fold_row of its tile)
//   d_points  the segment's points in the boundary form, read by the MLHIP_ACC32 kernels and the slices of a plain plan
//             (a folded plan gathers from d_points28 + row0 only: a token)
//   flags     MLHIP_SEG_FIRST / _LAST / _KEEP28 for the segment kernels
//   ev_mid    recorded between the accumulation and the long-bucket step (null: no event)
//   one_pass  the segment is the whole MSM, launched by plan_launch.  What a single pass does differently from a tile:
template <class C, class F>
int launch_accumulate(mlhip_msm_plan* p, const MsmEntryLists* sv, size_t row0, const Affine<F>* d_points, int flags, bool ed,
                      size_t len, bool one_pass, hipEvent_t ev_mid, hipStream_t st) {
  typedef XYZZ<F> X;
  constexpr bool kG2 = std::is_same<F, Fp2Field<C>>::value;  // two lanes per bucket
  constexpr int BB = kG2 ? 128 : 256;                        // workgroup of the long-bucket kernels: 48 KB of LDS per block
  static_assert((sizeof(X) <= 192) == !kG2, "BB * sizeof(X) is 48 KB for both groups");
  const size_t nbuckets = (size_t)p->W * p->M;
  const uint32_t big_threshold = big_bucket_threshold(p, len);
  // (1) a bucket holds at most all len entries (Wd len when folded): a small MSM skips the three near-empty launches of
  //     the long-bucket step.  A tile always runs them: whether an MSM has long buckets does not show in one tile's length.
  const bool long_buckets = !one_pass || entries_per_bucket_set(p) * len > big_threshold;
  // (2) too few buckets to fill the chip with one lane each: one bucket per quad of lanes (shorter dependent chains), ahead
  //     of the Edwards test.  The quad kernel keeps no state between segments, so tiles never use it.
  const bool quad = !kG2 && one_pass && p->d_points28 && p->reduce28 && nbuckets <= QUAD_ACC_MAX_BUCKETS && !getenv("MLHIP_NO_QUAD_ACC");
  // (3) every carry-free plan goes through the segment kernels of its bucket form, one pass ("first and last") or tile.  The
  //     test build's boundary-form reductions (MLHIP_REDUCE32 / MLHIP_REDUCE_ONE_LANE) come without MLHIP_SEG_KEEP28: the
  //     last segment leaves d_buckets, and one pass touches no state (such a plan has none before its first train).  Only
  //     MLHIP_ACC32 (no carry-free rows; test build, one pass) takes kernels of its own: the second implementation on
  //     32-bit limbs.  The product build instantiates none of those: nothing is launched, and launch_reduce reports the
  //     missing bucket state.
  const dim3 grid((unsigned)(((kG2 ? 2 : 1) * nbuckets + p->acc_block - 1) / p->acc_block)), block(p->acc_block);
  auto seg = [&](auto kernel, auto rows, auto state, auto... buckets) {
    kernel<<<grid, block, 0, st>>>(rows + row0, sv->d_sorted, sv->d_offsets, sv->d_counts, nbuckets, sv->d_order, big_threshold,
                                   p->d_biglist, p->lists.d_bigcount, state, flags, buckets...);
  };
  if (!p->d_points28) {
    if constexpr (kBuildAlt) {
      if constexpr (kG2)
        k_accumulate_lp<C><<<grid, block, 0, st>>>(d_points, sv->d_sorted, sv->d_offsets, sv->d_counts, nbuckets, sv->d_order,
                                                 big_threshold, p->d_biglist, p->lists.d_bigcount, (X*)p->d_buckets);
      else
        k_accumulate<F><<<grid, block, 0, st>>>(d_points, sv->d_sorted, sv->d_offsets, sv->d_counts, nbuckets, sv->d_order,
                                              big_threshold, p->d_biglist, p->lists.d_bigcount, (X*)p->d_buckets);
    }
  } else if constexpr (kG2) {
    typedef XYZZ28L<Fp28<C>> S;
    bool kc = false;
    if constexpr (C::BETA == -1 && kBuildAlt) {
      if ((kc = g2_split_by_coordinate()))
        seg(k_accumulate28_kc_seg<C>, (const AffineG2_28<C>*)p->d_points28, (S*)p->d_state28, (X*)p->d_buckets);
    }
    if (!kc) seg(k_accumulate28_lp_seg<C>, (const AffineG2_28<C>*)p->d_points28, (S*)p->d_state28, (X*)p->d_buckets);
  } else if (quad) {
    k_accumulate_q28<C><<<dim3((unsigned)((4 * nbuckets + 255) / 256)), dim3(256), 0, st>>>(
        (const Affine28<C>*)p->d_points28 + row0, sv->d_sorted, sv->d_offsets, sv->d_counts, nbuckets, big_threshold, p->d_biglist,
        p->lists.d_bigcount, (XYZZ28<C>*)p->d_state28);
  } else if (ed) {  // (implies reduce28: the last segment leaves its extended coordinates for the reduction)
    if constexpr (C::HAS_EDWARDS) seg(k_accumulate_ed28_seg<C>, (const EdNiels28<C>*)p->d_points28, (XYZZ28<C>*)p->d_state28);
  } else {
    seg(k_accumulate28_seg<C>, (const Affine28<C>*)p->d_points28, (XYZZ28<C>*)p->d_state28, (X*)p->d_buckets);
  }
  if (ev_mid) HIPCHK(hipEventRecord(ev_mid, st));
  if (!long_buckets) return 0;
  // (4) the slices of a plain plan gather from d_points, those of a folded plan from d_points28 + row0
  launch_big_slices<F>(p, d_points, st, sv, row0);
  auto combine = [&](auto kernel, auto state, auto... buckets) {
    kernel<<<dim3(256), dim3(BB), BB * sizeof(X), st>>>(p->d_biglist, p->lists.d_bigcount, p->d_bigprefix, (const X*)p->d_bigpart, state,
                                                        flags, buckets...);
  };
  if constexpr (kG2) {
    combine(k_accumulate_big_seg_g2<C, BB>, (XYZZ28L<Fp28<C>>*)p->d_state28, (X*)p->d_buckets);
  } else {
    if constexpr (C::HAS_EDWARDS) {
      if (ed) {
        combine(k_accumulate_big_seg_ed<C, BB>, (XYZZ28<C>*)p->d_state28);
        return 0;
      }
    }
    combine(k_accumulate_big_seg<C, BB>, (XYZZ28<C>*)p->d_state28, (X*)p->d_buckets);
  }
  return 0;
}

// the tail of both sequences: bucket sums -> partial sums -> h_out, then `done` (plan_finish waits for it)
// (a device-result plan stops at the partial sums: its finish queues the tail kernel behind them and records `done`)
template <class C, class F>
int finish_train(mlhip_msm_plan* p, bool prof, hipStream_t st) {
  if (int rc_red = launch_reduce<C, F>(p, st)) return rc_red;
  if (prof) HIPCHK(hipEventRecord(p->ev[4], st));
  HIPCHK(hipGetLastError());
  if (p->device_result) return 0;
  HIPCHK(hipMemcpyAsync(p->h_out, p->d_out, ((size_t)p->W * p->nsel + p->fold_nsel2) * sizeof(XYZZ<F>), hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(p->done, st));
  return 0;
}

// One pass over all n points: "one segment that is first and last" of the train below, with the differences listed at
// launch_accumulate, and
//   (5) a host-buffer call's points (upload_src) ride the auxiliary stream ahead of the conversion -- or, without the
//       carry-free copy and its stream, a blocking copy first;
//   (6) conv_src / conv_n / conv_ed are set after every conversion (the train clears conv_src at its start unless the copy
//       is cached, and restores it at its end only for resident, static points);
//   (7) events: memset of d_zero, then ev[0]; ev[2] once the conversion is queued; ev[3] between the accumulation and the
//       long buckets (tiles: ev[0] on the first tile ahead of the memset, ev_tile[s][0..2], ev[3] in stream_end);
//   (8) the wait for ev_join sits immediately before the first kernel that reads the points (tiles: ev_seg / ev_seg_sc).
template <class C, class F>
int plan_launch(mlhip_msm_plan* p, const void* d_points, const void* d_scalars, int mont, size_t n, hipStream_t st) {
  typedef Affine<F> A;
  if (p->fold) {
    if (int rc_fold = fold_check_args(p, n, p->upload_src != nullptr)) return rc_fold;
    d_points = p->d_points28;  // (never read as Affine<F>: every kernel of a folded plan gathers from the carry-free rows)
  }
  if (n != 0 && !p->upload_src) {
    const int K = resident_tiles(p->aux && p->d_points28, std::is_same<F, Fp2Field<C>>::value, p->fold, p->fold_tile,
                                 plan_use_edwards<C, F>(p), n);
    if (K > 1) {  // the train of this one plan, everything resident
      void* dp = const_cast<void*>(d_points);
      return plan_stream_train<C>(&p, &dp, nullptr, 1, const_cast<void*>(d_scalars), nullptr, mont, n, K, true, st);
    }
  }
  p->tiles_timed = 0;
  p->pending_n = n;
  p->pending = true;
  p->last_ed = false;
  if (n != 0) {
    const bool prof = p->profiling;
    if (p->upload_src && !p->d_points28) {  // no auxiliary stream on this path: plain upload first
      HIPCHK(hipMemcpy(const_cast<void*>(d_points), p->upload_src, p->upload_bytes, hipMemcpyHostToDevice));
      p->upload_src = nullptr;
    }
    // the conversion of the points is independent of the sort: it runs on the auxiliary stream beside the
    // (LDS-atomic bound) sort kernels.  The fork is recorded now (after the previous MSM's work on `st`); the work
    // itself is queued after the sort launches so that a host-blocking upload cannot delay them.
    if (p->d_points28) HIPCHK(hipEventRecord(p->ev_fork, st));
    HIPCHK(hipMemsetAsync(p->lists.d_zero, 0, p->lists.zero_bytes, st));
    if (prof) HIPCHK(hipEventRecord(p->ev[0], st));
    if (int rc_sort = launch_sort<C>(&p->lists, d_scalars, mont, n, st, prof ? p->ev[1] : nullptr)) return rc_sort;
    // resident bases: the carry-free copy of the first conv_n points of this very buffer is already there
    const bool use_ed = p->fold ? p->conv_ed : plan_use_edwards<C, F>(p);  // (a table is read in the form it was built in)
    p->last_ed = use_ed;
    const bool conv_cached = p->fold || (p->points_static && p->conv_src == d_points && n <= p->conv_n && !p->upload_src && p->conv_ed == use_ed);
    if (p->d_points28 && conv_cached) {
      HIPCHK(hipEventRecord(p->ev_join, st));  // nothing to wait for
    } else if (p->d_points28) {
      HIPCHK(hipStreamWaitEvent(p->aux, p->ev_fork, 0));
      if (p->upload_src) {  // host-buffer call: the upload of the points rides the same stream, ahead of the conversion
        HIPCHK(hipMemcpyAsync(const_cast<void*>(d_points), p->upload_src, p->upload_bytes, hipMemcpyHostToDevice, p->aux));
        p->upload_src = nullptr;
      }
      launch_convert<C, F>(p, (const A*)d_points, n, 0, use_ed, p->aux);
      HIPCHK(hipEventRecord(p->ev_join, p->aux));
      p->conv_src = d_points;
      p->conv_n = n;
      p->conv_ed = use_ed;
    }
    if (prof) HIPCHK(hipEventRecord(p->ev[2], st));
    if (p->d_points28) HIPCHK(hipStreamWaitEvent(st, p->ev_join, 0));
    // (the Edwards form always leaves its state and reads no MLHIP_SEG_KEEP28)
    const int flags = MLHIP_SEG_FIRST | MLHIP_SEG_LAST | (p->reduce28 ? MLHIP_SEG_KEEP28 : 0);
    if (int rc = launch_accumulate<C, F>(p, &p->lists, 0, (const A*)d_points, flags, use_ed, n, true, prof ? p->ev[3] : nullptr, st)) return rc;
    return finish_train<C, F>(p, prof, st);
  }
  return 0;
}

// Host-buffer G1 MSM streamed in K segments (see k_accumulate28_seg): h_points / h_scalars are the caller's pageable
// buffers, d_points / d_scalars the plan-sized device buffers they are staged through.  Uploads and the point
// conversion ride the auxiliary stream; the sort and the accumulation of segment s wait for its event on `st`.
// The host thread blocks inside the pageable copies, which is exactly what overlaps them with the kernels queued before.
//
// The same train serves device-resident inputs cut into TILES (h_scalars == nullptr: the scalars are already at
// d_scalars; h_points == nullptr: the points are already at d_points and are converted tile by tile unless the plan
// holds their carry-free copy).  Every window gathers its points in a different random order, so an MSM re-reads the
// whole point array once per window; once that array outgrows what the chip keeps close (Infinity Cache 256 MB, TLB
// reach) each gather goes to HBM and the additions wait: 0.139 ns per G1 addition at 2^20-2^21 points, 0.165 at 2^24
// (profiles/r02_tiles.txt).  A tile of 2^21-2^22 points keeps all W passes over its points near; the bucket
// accumulators travel through d_state28 between tiles (0.2-0.5 GB per tile, streamed once).
// one streamed / tiled MSM in flight on a plan: what stream_begin fixes for its tiles (the cuts: msm_segments.h)
struct StreamCtx : SegmentCuts {
  void* d_points = nullptr;
  void* d_scalars = nullptr;
  const void* h_points = nullptr;
  const void* h_scalars = nullptr;
  int mont = 0;
  bool resident = false, conv_cached = false, prof = false;
  bool ed = false;  // the buckets are summed in twisted Edwards coordinates (plan_use_edwards)
};

template <class C, class F>
int stream_begin(mlhip_msm_plan* p, StreamCtx& cx, hipStream_t st, int min_K) {
  constexpr bool kG2 = std::is_same<F, Fp2Field<C>>::value;
  if (!p->aux || !p->d_points28)
    return mlhip_rt::fail(MLHIP_EINVAL, "streamed MSM needs the auxiliary stream and the carry-free path");
  constexpr size_t kStateBytes = kG2 ? 2 * sizeof(XYZZ28L<Fp28<C>>) : sizeof(XYZZ28<C>);
  if (cx.n == 0 || cx.K < min_K || cx.K > MLHIP_MAX_SEGMENTS) return mlhip_rt::fail(MLHIP_EINVAL, "bad segment count");
  const size_t nbuckets = (size_t)p->W * p->M;
  if (!p->d_state28) HIPCHK(hipMalloc(&p->d_state28, nbuckets * kStateBytes));
  // resident points (h_points == nullptr): only the scalars travel (or nothing: h_scalars == nullptr); their carry-free
  // copy is either the plan's (resident bases) or made tile by tile
  cx.resident = cx.h_points == nullptr;
  cx.ed = p->fold ? p->conv_ed : plan_use_edwards<C, F>(p);
  p->last_ed = cx.ed;
  cx.conv_cached = cx.resident && p->points_static && p->conv_src == cx.d_points && cx.n <= p->conv_n && p->conv_ed == cx.ed;
  if (p->fold) {
    if (int rc_fold = fold_check_args(p, cx.n, !cx.resident)) return rc_fold;
    cx.conv_cached = true;
    cx.d_points = p->d_points28;  // (a token: never read as Affine<F>)
  }
  cx.prof = p->profiling && cx.h_scalars == nullptr;  // tiles of device-resident inputs: per-tile phase events
  p->pending_n = cx.n;
  p->pending = true;
  if (!cx.conv_cached) p->conv_src = nullptr;  // the carry-free copy is being rewritten
  if (!segment_cuts(cx, p->fold, p->fold_tile)) return mlhip_rt::fail(MLHIP_EINVAL, "folded plan: too many tiles");
  for (int s = 0; s < cx.K; s++) {  // the events of the segments as cut
    if (!p->ev_seg[s]) HIPCHK(hipEventCreateWithFlags(&p->ev_seg[s], hipEventDisableTiming));
    if (cx.h_scalars && cx.h_points && !p->ev_seg_sc[s]) HIPCHK(hipEventCreateWithFlags(&p->ev_seg_sc[s], hipEventDisableTiming));
    if (cx.prof)
      for (int j = 0; j < 3; j++)
        if (!p->ev_tile[s][j]) HIPCHK(hipEventCreate(&p->ev_tile[s][j]));
  }
  p->tiles_timed = cx.prof ? cx.K : -1;  // -1: a streamed host-buffer MSM records no phase events
  HIPCHK(hipEventRecord(p->ev_fork, st));  // the staging buffers are free once the work queued before us is done
  HIPCHK(hipStreamWaitEvent(p->aux, p->ev_fork, 0));
  return 0;
}

// tile s = pairs [off, off + len): uploads / conversion on the auxiliary stream, then sort and accumulation on `st`.
// `sorter` != nullptr: the tile was already sorted into these entry lists -- a sort-ahead record, or the lists of ANOTHER plan
// of the same window geometry over the same scalars (plan_stream_train) -- which are read; nothing is sorted.
template <class C, class F>
int stream_tile(mlhip_msm_plan* p, const StreamCtx& cx, int s, hipStream_t st, const MsmEntryLists* sorter) {
  typedef Affine<F> A;
  const size_t off = cx.bound[s];
  const size_t len = cx.bound[s + 1] - off;
  const bool first = off == 0, last = off + len >= cx.n;
  const int flags = (first ? MLHIP_SEG_FIRST : 0) | (last ? MLHIP_SEG_LAST : 0) | (p->reduce28 ? MLHIP_SEG_KEEP28 : 0);
  const char* hp = (const char*)cx.h_points;
  const char* hs = (const char*)cx.h_scalars;
  char* dsc = (char*)cx.d_scalars + off * 32;
  // where this segment's points start: plain arrays at `off`; a folded plan's table at the tile block that holds base `off`
  const size_t row0 = p->fold ? fold_row(p, off) : off;
  A* dpt = p->fold ? nullptr : (A*)cx.d_points + row0;  // (folded: the slices of long buckets gather from d_points28 + row0)
  const bool prof = cx.prof;
  if (hs) HIPCHK(hipMemcpyAsync(dsc, hs + off * 32, len * 32, hipMemcpyHostToDevice, p->aux));
  // points and scalars both travel: the sort starts when the segment's scalars are there, under the upload of its points
  const bool split = hs && !cx.resident && p->ev_seg_sc[s];
  if (split) HIPCHK(hipEventRecord(p->ev_seg_sc[s], p->aux));
  if (!cx.conv_cached) {
    if (!cx.resident) HIPCHK(hipMemcpyAsync(dpt, hp + off * sizeof(A), len * sizeof(A), hipMemcpyHostToDevice, p->aux));
    launch_convert<C, F>(p, dpt, len, off, cx.ed, p->aux);
  }
  HIPCHK(hipEventRecord(p->ev_seg[s], p->aux));
  if (prof && first) HIPCHK(hipEventRecord(p->ev[0], st));
  HIPCHK(hipMemsetAsync(p->lists.d_zero, 0, p->lists.zero_bytes, st));  // (with a sorter too: the count of long buckets)
  if (prof) HIPCHK(hipEventRecord(p->ev_tile[s][0], st));
  const bool uploads = hs || !cx.resident;
  if (uploads) HIPCHK(hipStreamWaitEvent(st, split ? p->ev_seg_sc[s] : p->ev_seg[s], 0));  // the sort needs the uploaded scalars
  if (!sorter) {
    int rc_sort = launch_sort<C>(&p->lists, dsc, cx.mont, len, st, nullptr);
    if (rc_sort) return rc_sort;
  }
  if (!uploads || split) HIPCHK(hipStreamWaitEvent(st, p->ev_seg[s], 0));  // only the accumulation waits for points / conversion
  if (prof) HIPCHK(hipEventRecord(p->ev_tile[s][1], st));
  if (int rc = launch_accumulate<C, F>(p, sorter ? sorter : &p->lists, row0, dpt, flags, cx.ed, len, false, nullptr, st)) return rc;
  if (prof) HIPCHK(hipEventRecord(p->ev_tile[s][2], st));
  return 0;
}

template <class C, class F>
int stream_end(mlhip_msm_plan* p, const StreamCtx& cx, hipStream_t st) {
  if (cx.resident && !cx.conv_cached && p->points_static) {  // every tile was converted: the copy is whole again
    p->conv_src = cx.d_points;
    p->conv_n = cx.n;
    p->conv_ed = cx.ed;
  }
  if (cx.prof) HIPCHK(hipEventRecord(p->ev[3], st));
  return finish_train<C, F>(p, cx.prof, st);
}

// ---- sorting ahead (round 3) ----------------------------------------------------------------------------------------------
// A tiled device-resident MSM ran sort(0), accumulate(0), sort(1), accumulate(1) ... on one stream: the sort kernels are
// bound by LDS atomics and leave the multipliers idle, the accumulation is the opposite.  The entry lists of tile s + 1
// are now sorted on a second stream, into one of two further MsmEntryLists of the plan's geometry, while tile s accumulates
// on the caller's stream from the other record's lists (the `sorter` argument of stream_tile, as the later plans of a
// shared-scalar train read the first plan's lists).  Events: ev_sorted[b] (sort stream -> accumulation), ev_lists_free[b]
// (accumulation -> the next sort into record b; it also orders consecutive MSMs on the plan).  MLHIP_SORT_AHEAD=0: off.
template <class C>
int sort_ahead_prepare(mlhip_msm_plan* p, size_t seg, bool& on) {
  on = false;
  const char* e = getenv("MLHIP_SORT_AHEAD");
  if (e && e[0] == '0') return 0;
  if (p->lists.sort_low <= 0) return 0;  // the legacy sort shares the digits buffer with the accumulation path: not split
  for (int b = 0; b < 2; b++) {
    MsmEntryLists* h = p->sort_helper[b];
    if (h && h->cap < seg) {  // longer tiles than last time: rebuild
      (void)hipStreamSynchronize(p->sort_stream);
      entry_lists_free(h);
      delete h;
      h = p->sort_helper[b] = nullptr;
    }
    if (!h) {
      // The record is an optimisation: if its buffers do not fit (two copies of the tile's entry lists; plausible at
      // 2^24 pairs) the MSM must still run, with the sort in line as before.  The record is registered only once it is
      // complete -- a half-allocated one left in p->sort_helper would pass the `cap >= seg` test of the next launch
      // and hand null list pointers to launch_sort.  MLHIP_FAULT_INJECT=sort_helper_alloc makes the allocation "fail"
      // (tests/test_gpu_parity.py::test_sort_ahead_helper_allocation_failure).
      h = new MsmEntryLists(plan_entry_lists(p, seg));
      const char* fi = getenv("MLHIP_FAULT_INJECT");
      int rc = (fi && !strcmp(fi, "sort_helper_alloc")) ? MLHIP_ENOMEM : entry_lists_alloc(h);
      if (rc || h->sort_low <= 0) {
        entry_lists_free(h);      // whatever was allocated
        delete h;
        (void)hipGetLastError();  // an out-of-memory error must not surface in the next HIPCHK
        return 0;                 // on = false: the in-line path
      }
      p->sort_helper[b] = h;  // owned by p from here on
    }
    if (!p->ev_sorted[b]) HIPCHK(hipEventCreateWithFlags(&p->ev_sorted[b], hipEventDisableTiming));
    if (!p->ev_lists_free[b]) HIPCHK(hipEventCreateWithFlags(&p->ev_lists_free[b], hipEventDisableTiming));
  }
  if (!p->sort_stream) {
    // the highest priority: a sort is a chain of a dozen short kernels that must find wave slots between the
    // accumulation's one-wave workgroups
    int lo = 0, hi = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    const char* pe = getenv("MLHIP_SORT_AHEAD_PRIO");
    if (pe && pe[0] == '0')
      HIPCHK(hipStreamCreateWithFlags(&p->sort_stream, hipStreamNonBlocking));
    else
      HIPCHK(hipStreamCreateWithPriority(&p->sort_stream, hipStreamNonBlocking, hi));
  }
  on = true;
  return 0;
}
// queue the sort of tile s into record s & 1 (after whatever still reads that record's lists)
template <class C>
int sort_ahead_tile(mlhip_msm_plan* p, const StreamCtx& cx, int s) {
  const int b = s & 1;
  const MsmEntryLists* h = p->sort_helper[b];
  const size_t off = cx.bound[s];
  const size_t len = cx.bound[s + 1] - off;
  HIPCHK(hipStreamWaitEvent(p->sort_stream, p->ev_lists_free[b], 0));  // never recorded yet: no wait
  HIPCHK(hipMemsetAsync(h->d_zero, 0, h->zero_bytes, p->sort_stream));
  int rc = launch_sort<C>(h, (const char*)cx.d_scalars + off * 32, cx.mont, len, p->sort_stream, nullptr);
  if (rc) return rc;
  HIPCHK(hipEventRecord(p->ev_sorted[b], p->sort_stream));
  return 0;
}

// THE train: a class of k plans of ONE window geometry, of either group, over one scalar vector.  Every tile is sorted once
// -- into the first plan's lists, or with sort-ahead into one of its two further records -- and accumulated once per plan,
// plan after plan, on one stream.  stream_end of a plan is queued as soon as its last tile is (the last plan's after the
// loop), so that its reduction, its copy to the host and the host tail of its result run under the next plan's accumulation.
//   d_points[j]   plan j's points in device memory (a folded plan brings none: its table), or the buffer they are staged in
//   h_points      null: every plan's points are resident; else h_points[j] = the caller's pageable points of plan j (or null),
//                 uploaded tile by tile on that plan's auxiliary stream
//   h_scalars     null: the scalars are at d_scalars; else uploaded once, by the first plan's tiles
//   schedule      a G1 first plan whose scalars travel cuts its segments by stream_schedule (msm_segments.h)
// k = 1 is the train of a single plan -- a host-buffer MSM streamed in segments, or a device-resident one cut into tiles --
// and needs at least two segments (one is plan_launch's single pass); a class may run a single tile.
// Folded plans: the cuts are segment_cuts' over the class's fold_tile, row0 = fold_row(p, off) is taken per plan, and the
// slices of long buckets gather from each plan's own d_points28 through the sorter's lists (launch_big_slices).
template <class C>
int plan_stream_train(mlhip_msm_plan* const* ps, void* const* d_points, const void* const* h_points, int k, void* d_scalars,
                      const void* h_scalars, int mont, size_t n, int K, bool schedule, hipStream_t st) {
  typedef FpField<C> F1;
  typedef Fp2Field<C> F2;
  if (k < 1) return mlhip_rt::fail(MLHIP_EINVAL, "shared-scalar MSM: no plan");
  mlhip_msm_plan* p0 = ps[0];
  for (int j = 1; j < k; j++)
    if (ps[j]->fold != p0->fold || ps[j]->c != p0->c || ps[j]->Wd != p0->Wd || ps[j]->fold_tile != p0->fold_tile ||
        ps[j]->W != p0->W || ps[j]->M != p0->M || ps[j]->bits != p0->bits)
      return mlhip_rt::fail(MLHIP_EINVAL, "the plans of a shared-scalar MSM need the same window width and scalar width");
  auto g1 = [&](int j) { return ps[j]->group == MLHIP_GROUP_G1; };
  std::vector<StreamCtx> cx(k);
  bool points_travel = false;
  for (int j = 0; j < k; j++) {
    cx[j].d_points = d_points[j];
    cx[j].d_scalars = d_scalars;
    cx[j].h_points = h_points ? h_points[j] : nullptr;
    cx[j].h_scalars = j == 0 ? h_scalars : nullptr;
    cx[j].mont = mont;
    cx[j].n = n;
    cx[j].K = K;
    points_travel = points_travel || cx[j].h_points != nullptr;
  }
  if (schedule && h_scalars && g1(0)) {
    stream_schedule(cx[0], cx[0].h_points != nullptr, schedule_tile(p0->fold, p0->fold_tile, plan_use_edwards<C, F1>(p0)), p0->fold != 0);
    for (int j = 1; j < k; j++) static_cast<SegmentCuts&>(cx[j]) = cx[0];  // (before segment_cuts: every plan cuts alike)
  }
  const int min_K = k == 1 ? 2 : 1;
  for (int j = 0; j < k; j++) {
    int rc = g1(j) ? stream_begin<C, F1>(ps[j], cx[j], st, min_K) : stream_begin<C, F2>(ps[j], cx[j], st, min_K);
    if (rc) return rc;
  }
  bool ahead = false;
  if (!h_scalars && !points_travel && cx[0].K >= 2) {  // device-resident tiles: nothing to upload, the sorts can run ahead
    int rc = sort_ahead_prepare<C>(p0, cx[0].seg, ahead);
    if (rc) return rc;
  }
  if (ahead) HIPCHK(hipStreamWaitEvent(p0->sort_stream, p0->ev_fork, 0));  // the scalars are ready where `st` stood at launch
  auto end = [&](int j) { return g1(j) ? stream_end<C, F1>(ps[j], cx[j], st) : stream_end<C, F2>(ps[j], cx[j], st); };
  for (int s = 0; s < cx[0].K; s++) {
    const MsmEntryLists* lists = &p0->lists;  // the entry lists the later plans' tiles read
    if (ahead) {
      int rc = sort_ahead_tile<C>(p0, cx[0], s);
      if (rc) return rc;
      HIPCHK(hipStreamWaitEvent(st, p0->ev_sorted[s & 1], 0));
      lists = p0->sort_helper[s & 1];
    }
    for (int j = 0; j < k; j++) {
      const MsmEntryLists* sorter = j == 0 ? (ahead ? lists : nullptr) : lists;
      int rc = g1(j) ? stream_tile<C, F1>(ps[j], cx[j], s, st, sorter) : stream_tile<C, F2>(ps[j], cx[j], s, st, sorter);
      if (rc) return rc;
      if (s + 1 == cx[0].K && j + 1 < k) {
        rc = end(j);
        if (rc) return rc;
      }
    }
    if (ahead) HIPCHK(hipEventRecord(p0->ev_lists_free[s & 1], st));
  }
  return end(k - 1);
}

// What the tail kernel needs of a plan (msm_tail.h: MsmTailArgs).
inline int msm_tail_args(const mlhip_msm_plan* p, MsmTailArgs& a) {
  memset(&a, 0, sizeof(a));
  a.nsel = p->nsel;
  a.lgL = p->lgL;
  a.empty = p->pending_n == 0;
  if (p->fold) {
    // one window and no Horner pass: the combined entries, or the only group's own (host_tail_fold with W = 1 adds V_0 to
    // 2^lgM times an empty sum).  Several groups without the combined entries do not occur: plan_alloc combines whenever
    // W > 1 (a folded plan has the carry-free reduction and at most 16 groups).
    if (!p->fold_nsel2 && p->W != 1) return mlhip_rt::fail(MLHIP_EINVAL, "device-result plan: bucket groups without their combined sums");
    a.W = 1;
    a.first = p->fold_nsel2 ? p->W * p->nsel : 0;
    a.nb = p->fold_nsel2 ? p->fold_nsel2 - 4 : p->nb;
    return 0;
  }
  if (p->W > MSM_TAIL_MAX_W) return mlhip_rt::fail(MLHIP_EINVAL, "device-result plan: more windows than the tail kernel holds");
  a.W = p->W;
  a.nb = p->nb;
  a.horner = 1;
  int down[MSM_TAIL_MAX_W] = {};
  msm_window_shifts(p->bits, p->c, down);  // (a short-scalar plan: its own, shorter layout)
  for (int w = 0; w < p->W; w++) a.down[w] = (unsigned char)down[w];
  return 0;
}

// mlhip_msm_finish of a device-result plan: ONE launch on the stream of the pending launch -- the tail kernel into the
// plan's slot -- then the delivery (a copy of the slot per requested output: no kernel of the library dereferences the
// caller's pointers) and `done`.  No allocation and no host wait; the phase times are read by mlhip_msm_plan_timings.
template <class C, class F>
int plan_finish_device(mlhip_msm_plan* p, void* d_out_affine, void* d_out_xyzz) {
  typedef Affine<F> A;
  typedef XYZZ<F> X;
  constexpr bool kG2 = std::is_same<F, Fp2Field<C>>::value;
  if (!p->pending) return mlhip_rt::fail(MLHIP_EINVAL, "mlhip_msm_finish without a pending mlhip_msm_launch");
  p->pending = false;
  MsmTailArgs a;
  if (int rc = msm_tail_args(p, a)) return rc;
  hipStream_t st = p->pending_stream;
  A* slot_affine = (A*)p->d_result;
  X* slot_xyzz = (X*)((char*)p->d_result + sizeof(A));
  const bool prof = p->profiling;
  if (prof) HIPCHK(hipEventRecord(p->ev_tail[0], st));
  if constexpr (kG2)
    k_msm_tail<TailLanePair<C>, 2><<<dim3(1), dim3(128), 0, st>>>((const X*)p->d_out, a, slot_xyzz, slot_affine);
  else
    k_msm_tail<TailOneLane<F>, 1><<<dim3(1), dim3(64), 0, st>>>((const X*)p->d_out, a, slot_xyzz, slot_affine);
  if (prof) HIPCHK(hipEventRecord(p->ev_tail[1], st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(d_out_affine, slot_affine, sizeof(A), hipMemcpyDefault, st));
  if (d_out_xyzz) HIPCHK(hipMemcpyAsync(d_out_xyzz, slot_xyzz, sizeof(X), hipMemcpyDefault, st));
  HIPCHK(hipEventRecord(p->done, st));
  p->done_stream = st;
  p->done_queued = true;
  p->times_stale = prof;
  p->timed_n = p->pending_n;
  return 0;
}

template <class C, class F>
int plan_finish(mlhip_msm_plan* p, void* out_affine, void* out_xyzz) {
  typedef Affine<F> A;
  typedef XYZZ<F> X;
  if (p->device_result) return plan_finish_device<C, F>(p, out_affine, out_xyzz);
  X total;
  if (!p->pending) return mlhip_rt::fail(MLHIP_EINVAL, "mlhip_msm_finish without a pending mlhip_msm_launch");
  p->pending = false;
  if (p->pending_n == 0) {
    xyzz_set_inf<F>(total);
  } else {
    HIPCHK(hipEventSynchronize(p->done));
    auto t0 = std::chrono::steady_clock::now();
    host_tail<F>(p, total);
    if (p->profiling && p->tiles_timed >= 0) {
      if (int rc_times = plan_read_phase_times(p)) return rc_times;
      p->ms[5] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();  // the host tail
    } else if (p->profiling) {
      for (int i = 0; i < 6; i++) p->ms[i] = 0;  // a streamed host-buffer MSM records no phase events: nothing stale is left
    }
  }
  A r;
  xyzz_to_affine<F>(r, total);
  memcpy(out_affine, &r, sizeof(A));
  if (out_xyzz) memcpy(out_xyzz, &total, sizeof(X));
  return 0;
}

}  // namespace mlhip

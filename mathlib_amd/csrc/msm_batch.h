// msm_batch.h -- many independent small MSMs in one call (mlhip_msm_batch*): out[k] = sum over segment k of [s_i] P_i.
// Part of msm_kernels.h; the layout builder and the per-lane bodies above the kernels are plain C++ / __host__ __device__,
// so tests/hostmath_batch replays them on the CPU.  Cost model and measurements: DESIGN.md section 8.
//
//   chunks     every segment is cut into chunks of at most P consecutive pairs (the last one of a segment may be shorter).
//              One lane (G1) or one lane pair (G2, msm_g2.h) per chunk runs an interleaved (Straus) signed 4-bit-window
//              double-and-add: a table {1..8} P_j per point, then 65 windows of 4 doublings shared by the chunk + up to P
//              table additions -- 256 / P + 64 + 7 group operations per pair instead of k_scalar_mul's 327.  The chunk's
//              partial sum is written in XYZZ.
//   sum passes groups of at most MSM_BATCH_GROUP partials of one segment are summed, one lane (pair) per group, until one
//              group per segment is left; the last pass converts to affine (one inversion per output lane).  No lane runs a
//              chain longer than max(P, MSM_BATCH_GROUP) additions, whatever a segment's length.
//   layout     the chunk table (first pair, pair count) and the groups of every pass are built on the host from the
//              offsets (msm_batch_layout) and uploaded in one copy on the call's stream.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "msm_body.h"

namespace mlhip {

constexpr int MSM_BATCH_GROUP = 32;  // partials per lane in a sum pass
// the compiled chunk lengths (MLHIP_MSM_BATCH_CHUNK picks one per call) and the defaults
constexpr int MSM_BATCH_P_DEFAULT_G1 = 4, MSM_BATCH_P_DEFAULT_G2 = 4;
inline bool msm_batch_p_valid(int p) { return p == 1 || p == 2 || p == 4 || p == 8; }

struct MsmBatchChunk {
  uint64_t first;  // index of the chunk's first pair in points / scalars
  uint32_t count;  // 1 .. P pairs
  uint32_t base0;  // mlhip_bases_msm_batch without an index list: the position of the first pair in its segment (= its base)
};
struct MsmBatchGroup {
  uint32_t begin, count;  // partials [begin, begin + count) of the pass's input, all of one segment
};

// passes[q] = [pass_begin[q], pass_begin[q + 1]) in groups; pass q reads the output of pass q - 1 (pass 0: the chunk
// partials) and writes one partial per group, contiguous per segment.  The last pass has exactly k groups, one per
// segment in order (count 0 = empty segment = the point at infinity), and writes the affine results.
struct MsmBatchLayout {
  std::vector<MsmBatchChunk> chunks;
  std::vector<MsmBatchGroup> groups;
  std::vector<size_t> pass_begin;
  size_t max_mid = 0;  // largest number of groups of a pass before the last one (size of the second partials buffer)
};

// false: the chunk or group indices do not fit 32 bits.  offsets must have been checked (0 first, nondecreasing).
// chunk_len(m) = the chunk length of a segment of m pairs (msm_batch_layout: P for every segment; msm_batch_bucket.h: the
// slice length for the long ones)
template <class ChunkLen>
inline bool msm_batch_layout_by(MsmBatchLayout& L, const uint64_t* offsets, size_t k, int G, ChunkLen chunk_len) {
  L.chunks.clear();
  L.groups.clear();
  L.pass_begin.assign(1, 0);
  L.max_mid = 0;
  std::vector<uint64_t> n(k);  // partials per segment in the current pass's input
  for (size_t s = 0; s < k; s++) {
    const uint64_t a = offsets[s], b = offsets[s + 1];
    const uint64_t P = chunk_len(b - a);
    n[s] = (b - a + P - 1) / P;
    for (uint64_t f = a; f < b; f += P) L.chunks.push_back({f, (uint32_t)(b - f < P ? b - f : P), (uint32_t)(f - a)});
  }
  if (L.chunks.size() >= ((uint64_t)1 << 32)) return false;
  for (;;) {
    uint64_t most = 0;
    for (size_t s = 0; s < k; s++) most = n[s] > most ? n[s] : most;
    const bool last = most <= (uint64_t)G;
    uint64_t in = 0;  // first input partial of segment s
    for (size_t s = 0; s < k; s++) {
      if (last) {
        L.groups.push_back({(uint32_t)in, (uint32_t)n[s]});
      } else {
        for (uint64_t j = 0; j < n[s]; j += (uint64_t)G)
          L.groups.push_back({(uint32_t)(in + j), (uint32_t)(n[s] - j < (uint64_t)G ? n[s] - j : (uint64_t)G)});
      }
      in += n[s];
      if (!last) n[s] = (n[s] + G - 1) / G;
    }
    const size_t mid = L.groups.size() - L.pass_begin.back();
    L.pass_begin.push_back(L.groups.size());
    if (last) break;
    L.max_mid = mid > L.max_mid ? mid : L.max_mid;
  }
  return true;
}
inline bool msm_batch_layout(MsmBatchLayout& L, const uint64_t* offsets, size_t k, int P, int G = MSM_BATCH_GROUP) {
  return msm_batch_layout_by(L, offsets, k, G, [P](uint64_t) { return (uint64_t)P; });
}

// group operations of the per-lane bodies below: the plain formulas (host replay); the kernels pass their own
template <class F>
struct MsmBatchOps {
  MLHIP_HD static void madd(XYZZ<F>& acc, const Affine<F>& q) { xyzz_madd<F>(acc, q, false); }
  MLHIP_HD static void add(XYZZ<F>& acc, const XYZZ<F>& q) { xyzz_add<F>(acc, q); }
  MLHIP_HD static void dbl(XYZZ<F>& r, const XYZZ<F>& p) { xyzz_dbl<F>(r, p); }
};

// acc = sum_{j < count} [s_j] P_j for one chunk (count <= P): scalars = 8 words per pair (fr_canonical: Montgomery or plain,
// not necessarily reduced), load(pt, j) reads P_j.  Interleaved signed 4-bit windows: the digits come from
// signed_windows4, so every branch depends on the scalars alone -- uniform over a lane pair, and over a wave's lanes as far
// as their digits agree.  The accumulator may meet its own table entry (the same pair twice: xyzz_add's doubling branch) or
// its negative (infinity), which xyzz_add handles.
template <class F, int P, class Ops, class Load>
MLHIP_HD void msm_batch_chunk(XYZZ<F>& acc, const uint32_t* scalars, uint32_t count, bool mont, Load load) {
  typedef typename F::Curve C;
  uint32_t sw[P][9];
  XYZZ<F> tab[P][8];
#pragma unroll 1
  for (int j = 0; j < P; j++) {
    uint32_t s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if ((uint32_t)j < count) fr_canonical<C>(s, scalars + 8 * j, mont);
    signed_windows4(sw[j], s);  // s = 0 (a slot past the chunk's end): every digit 0, the table is never read
    if ((uint32_t)j >= count) continue;
    Affine<F> pt;
    load(pt, j);
    xyzz_from_affine<F>(tab[j][0], pt);
#pragma unroll 1
    for (int m = 1; m < 8; m++) {
      tab[j][m] = tab[j][m - 1];
      Ops::madd(tab[j][m], pt);
    }
  }
  xyzz_set_inf<F>(acc);
  bool started = false;
#pragma unroll 1
  for (int w = 64; w >= 0; w--) {
    if (started) {
#pragma unroll 1
      for (int d = 0; d < 4; d++) {
        XYZZ<F> t;
        Ops::dbl(t, acc);
        acc = t;
      }
    }
#pragma unroll 1
    for (int j = 0; j < P; j++) {
      const int d = signed_window4_digit(sw[j], w);
      if (d) {
        XYZZ<F> q = tab[j][(d < 0 ? -d : d) - 1];
        typename F::T ny;
        F::neg(ny, q.y);
        F::select(q.y, d < 0, ny, q.y);
        Ops::add(acc, q);
        started = true;
      }
    }
  }
}

// acc = sum_{i < count} partial_i, load(q, i) reading partial i of one group
template <class F, class Ops, class Load>
MLHIP_HD void msm_batch_sum(XYZZ<F>& acc, uint32_t count, Load load) {
  xyzz_set_inf<F>(acc);
#pragma unroll 1
  for (uint32_t i = 0; i < count; i++) {
    XYZZ<F> q;
    load(q, i);
    Ops::add(acc, q);
  }
}

#if defined(__HIPCC__)
// ---- kernels ---------------------------------------------------------------------------------------------------------
// G1: one lane per chunk / group; the running point stays in registers (as in k_scalar_mul), the table build is out of line
template <class F>
struct MsmBatchOpsG1 {
  __device__ static void madd(XYZZ<F>& acc, const Affine<F>& q) { xyzz_madd_ool<F>(acc, q); }
  __device__ static void add(XYZZ<F>& acc, const XYZZ<F>& q) { xyzz_add<F>(acc, q); }
  __device__ static void dbl(XYZZ<F>& r, const XYZZ<F>& p) { xyzz_dbl<F>(r, p); }
};
// G2: one lane pair per chunk / group, one Fp2 component per lane (as in k_scalar_mul_lp)
template <class C>
struct MsmBatchOpsLp {
  typedef Fp2LField<C> FL;
  __device__ static void madd(XYZZ<FL>& acc, const Affine<FL>& q) { xyzz_madd<FL>(acc, q, false); }
  __device__ static void add(XYZZ<FL>& acc, const XYZZ<FL>& q) { xyzz_add_lp_ool<C>(acc, q); }
  __device__ static void dbl(XYZZ<FL>& r, const XYZZ<FL>& p) { xyzz_dbl<FL>(r, p); }
};

template <class C, int P>
__global__ void __launch_bounds__(64) k_msm_batch_chunk(const Affine<FpField<C>>* __restrict__ points,
                                                        const uint32_t* __restrict__ scalars, int mont,
                                                        const MsmBatchChunk* __restrict__ chunks, uint32_t n_chunks,
                                                        XYZZ<FpField<C>>* __restrict__ partials) {
  typedef FpField<C> F;
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_chunks) return;
  const MsmBatchChunk ch = chunks[c];
  if (ch.count > (uint32_t)P) return;  // a slice of a long segment: the bucket kernels write this row (msm_batch_bucket.h)
  const Affine<F>* pts = points + ch.first;
  XYZZ<F> acc;
  msm_batch_chunk<F, P, MsmBatchOpsG1<F>>(acc, scalars + 8 * ch.first, ch.count, mont != 0,
                                          [&](Affine<F>& p, int j) { p = pts[j]; });
  partials[c] = acc;
}

template <class C, int P>
__global__ void __launch_bounds__(64) k_msm_batch_chunk_lp(const Affine<Fp2Field<C>>* __restrict__ points,
                                                           const uint32_t* __restrict__ scalars, int mont,
                                                           const MsmBatchChunk* __restrict__ chunks, uint32_t n_chunks,
                                                           XYZZ<Fp2Field<C>>* __restrict__ partials) {
  typedef Fp2LField<C> FL;
  const uint32_t c = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;  // both lanes of a pair share the chunk
  if (c >= n_chunks) return;
  const int hi = (int)(threadIdx.x & 1u);
  const MsmBatchChunk ch = chunks[c];
  if (ch.count > (uint32_t)P) return;  // a slice of a long segment (both lanes of the pair leave): msm_batch_bucket.h
  XYZZ<FL> acc;
  msm_batch_chunk<FL, P, MsmBatchOpsLp<C>>(acc, scalars + 8 * ch.first, ch.count, mont != 0,
                                           [&](Affine<FL>& p, int j) { lp_load_affine<C>(p, points, ch.first + j, hi); });
  lp_store_xyzz<C>(partials, c, acc, hi);
}

// one sum pass: dst[g] = sum of the group's partials; out_affine != nullptr (the last pass): the affine result instead
template <class C>
__global__ void __launch_bounds__(64) k_msm_batch_sum(const XYZZ<FpField<C>>* __restrict__ src,
                                                      const MsmBatchGroup* __restrict__ groups, uint32_t n_groups,
                                                      XYZZ<FpField<C>>* __restrict__ dst, Affine<FpField<C>>* __restrict__ out_affine) {
  typedef FpField<C> F;
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups) return;
  const MsmBatchGroup gr = groups[g];
  XYZZ<F> acc;
  msm_batch_sum<F, MsmBatchOpsG1<F>>(acc, gr.count, [&](XYZZ<F>& q, uint32_t i) { q = src[gr.begin + i]; });
  if (out_affine) {
    Affine<F> a;
    xyzz_to_affine<F>(a, acc);
    out_affine[g] = a;
  } else {
    dst[g] = acc;
  }
}

template <class C>
__global__ void __launch_bounds__(64) k_msm_batch_sum_lp(const XYZZ<Fp2Field<C>>* __restrict__ src,
                                                         const MsmBatchGroup* __restrict__ groups, uint32_t n_groups,
                                                         XYZZ<Fp2Field<C>>* __restrict__ dst,
                                                         Affine<Fp2Field<C>>* __restrict__ out_affine) {
  typedef Fp2LField<C> FL;
  const uint32_t g = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;
  if (g >= n_groups) return;
  const int hi = (int)(threadIdx.x & 1u);
  const MsmBatchGroup gr = groups[g];
  XYZZ<FL> acc;
  msm_batch_sum<FL, MsmBatchOpsLp<C>>(acc, gr.count, [&](XYZZ<FL>& q, uint32_t i) { lp_load_xyzz<C>(q, src, gr.begin + i, hi); });
  if (out_affine) {
    Affine<FL> a;
    xyzz_to_affine<FL>(a, acc);
    Fp<C>* o = reinterpret_cast<Fp<C>*>(out_affine + g);
    o[hi] = a.x.v;
    o[2 + hi] = a.y.v;
  } else {
    lp_store_xyzz<C>(dst, g, acc, hi);
  }
}

// device scratch of the batch calls: [chunk table | groups | partials A | partials B], one persistent buffer per device
// (per curve: this header is compiled into one translation unit per curve).  Calls on different streams take it in the
// order they take the lock; each waits on the device for the event the previous one recorded after its last kernel.
struct MsmBatchScratch {
  char* buf = nullptr;
  size_t cap = 0;
  hipEvent_t last = nullptr;
};
static std::mutex g_mb_mu;
static MsmBatchScratch g_mb[64];

static inline void msm_batch_release() {
  std::lock_guard<std::mutex> lk(g_mb_mu);
  int cur = 0;
  const bool have_cur = hipGetDevice(&cur) == hipSuccess;
  for (int dev = 0; dev < 64; dev++) {
    MsmBatchScratch& mb = g_mb[dev];
    if (!mb.buf && !mb.last) continue;
    (void)hipSetDevice(dev);
    if (mb.last) {
      (void)hipEventSynchronize(mb.last);
      (void)hipEventDestroy(mb.last);
      mb.last = nullptr;
    }
    if (mb.buf) (void)hipFree(mb.buf);
    mb.buf = nullptr;
    mb.cap = 0;
  }
  if (have_cur) (void)hipSetDevice(cur);
}

// the chunk length of this call: MLHIP_MSM_BATCH_CHUNK if it names a compiled one, else the group's default
template <class C, class F>
int msm_batch_chunk_len() {
  constexpr bool kG1 = std::is_same<F, FpField<C>>::value;
  if (const char* e = getenv("MLHIP_MSM_BATCH_CHUNK")) {
    const int v = atoi(e);
    if (msm_batch_p_valid(v)) return v;
  }
  return kG1 ? MSM_BATCH_P_DEFAULT_G1 : MSM_BATCH_P_DEFAULT_G2;
}

template <class C, class F, int P>
void msm_batch_launch_chunks(const void* d_points, const void* d_scalars, int mont, const MsmBatchChunk* d_chunks,
                             uint32_t n_chunks, void* d_partials, hipStream_t st) {
  if constexpr (std::is_same<F, FpField<C>>::value)
    k_msm_batch_chunk<C, P><<<dim3((n_chunks + 63) / 64), dim3(64), 0, st>>>(
        (const Affine<FpField<C>>*)d_points, (const uint32_t*)d_scalars, mont, d_chunks, n_chunks, (XYZZ<FpField<C>>*)d_partials);
  else
    k_msm_batch_chunk_lp<C, P><<<dim3((unsigned)((2 * (size_t)n_chunks + 63) / 64)), dim3(64), 0, st>>>(
        (const Affine<Fp2Field<C>>*)d_points, (const uint32_t*)d_scalars, mont, d_chunks, n_chunks, (XYZZ<Fp2Field<C>>*)d_partials);
}

// the passes of one batch call over a built layout: one upload of [chunk table | groups | extra] on the call's stream,
// launch(d_chunks, n_chunks, d_extra, d_partials, d_scratch) queues the chunk kernel (n_chunks >= 1), then the sum passes
// write the k affine results.  extra: extra_bytes of host data the chunk kernel reads (the base indices of
// mlhip_bases_msm_batch, the slice rows of msm_batch_bucket.h); d_scratch: scratch_bytes more of the buffer, 256-byte aligned
template <class C, class F, class Launch>
int msm_batch_run(const MsmBatchLayout& L, const void* extra, size_t extra_bytes, void* d_out, hipStream_t st, Launch launch,
                  size_t scratch_bytes = 0) {
  constexpr bool kG1 = std::is_same<F, FpField<C>>::value;
  const size_t n_chunks = L.chunks.size(), n_groups = L.groups.size();
  const size_t chunk_bytes = n_chunks * sizeof(MsmBatchChunk), group_bytes = n_groups * sizeof(MsmBatchGroup);
  const size_t meta = (chunk_bytes + group_bytes + extra_bytes + 255) & ~(size_t)255;
  const size_t a_bytes = ((n_chunks * sizeof(XYZZ<F>)) + 255) & ~(size_t)255;
  const size_t b_bytes = ((L.max_mid * sizeof(XYZZ<F>)) + 255) & ~(size_t)255;
  const size_t need = meta + a_bytes + b_bytes + scratch_bytes;
  std::vector<char> host(chunk_bytes + group_bytes + extra_bytes);
  if (chunk_bytes) memcpy(host.data(), L.chunks.data(), chunk_bytes);
  memcpy(host.data() + chunk_bytes, L.groups.data(), group_bytes);
  if (extra_bytes) memcpy(host.data() + chunk_bytes + group_bytes, extra, extra_bytes);
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_mb_mu);
  MsmBatchScratch& mb = g_mb[dev & 63];
  if (need > mb.cap) {
    if (mb.buf) HIPCHK(hipFree(mb.buf));  // waits for the device: no earlier call is still reading it
    mb.buf = nullptr;
    mb.cap = 0;
    const size_t want = need + need / 4;
    HIPCHK(hipMalloc((void**)&mb.buf, want));
    mb.cap = want;
  }
  if (!mb.last)
    HIPCHK(hipEventCreateWithFlags(&mb.last, hipEventDisableTiming));
  else
    HIPCHK(hipStreamWaitEvent(st, mb.last, 0));
  HIPCHK(hipMemcpyAsync(mb.buf, host.data(), host.size(), hipMemcpyHostToDevice, st));
  const MsmBatchChunk* d_chunks = (const MsmBatchChunk*)mb.buf;
  const MsmBatchGroup* d_groups = (const MsmBatchGroup*)(mb.buf + chunk_bytes);
  void* bufs[2] = {mb.buf + meta, mb.buf + meta + a_bytes};
  if (n_chunks)
    launch(d_chunks, (uint32_t)n_chunks, (const void*)(mb.buf + chunk_bytes + group_bytes), bufs[0],
           (void*)(mb.buf + meta + a_bytes + b_bytes));
  const size_t passes = L.pass_begin.size() - 1;
  for (size_t q = 0; q < passes; q++) {
    const bool last = q + 1 == passes;
    const uint32_t ng = (uint32_t)(L.pass_begin[q + 1] - L.pass_begin[q]);
    const MsmBatchGroup* gq = d_groups + L.pass_begin[q];
    void* src = bufs[q & 1];
    void* dst = last ? nullptr : bufs[(q + 1) & 1];
    if constexpr (kG1)
      k_msm_batch_sum<C><<<dim3((ng + 63) / 64), dim3(64), 0, st>>>(
          (const XYZZ<FpField<C>>*)src, gq, ng, (XYZZ<FpField<C>>*)dst, last ? (Affine<FpField<C>>*)d_out : nullptr);
    else
      k_msm_batch_sum_lp<C><<<dim3((unsigned)((2 * (size_t)ng + 63) / 64)), dim3(64), 0, st>>>(
          (const XYZZ<Fp2Field<C>>*)src, gq, ng, (XYZZ<Fp2Field<C>>*)dst, last ? (Affine<Fp2Field<C>>*)d_out : nullptr);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(mb.last, st));
  return 0;
}

// msm_batch_endo.h: the split chunk kernel of a call whose points are promised to be in G1 / G2; false: there is none for
// this (curve, group, P), or MLHIP_MSM_BATCH_ENDO=0
template <class C, class F>
bool msm_batch_endo_launch_chunks(int P, const void* d_points, const void* d_scalars, int mont, const MsmBatchChunk* d_chunks,
                                  uint32_t n_chunks, void* d_partials, hipStream_t st);

// the chunk kernel of the compiled chunk length P; subgroup: the caller's promise (MLHIP_CURVE_SUBGROUP_POINTS)
template <class C, class F>
void msm_batch_launch_chunks_p(int P, const void* d_points, const void* d_scalars, int mont, const MsmBatchChunk* d_chunks,
                               uint32_t n_chunks, void* d_partials, hipStream_t st, bool subgroup = false) {
  if (subgroup && msm_batch_endo_launch_chunks<C, F>(P, d_points, d_scalars, mont, d_chunks, n_chunks, d_partials, st)) return;
  switch (P) {
    case 1: msm_batch_launch_chunks<C, F, 1>(d_points, d_scalars, mont, d_chunks, n_chunks, d_partials, st); break;
    case 2: msm_batch_launch_chunks<C, F, 2>(d_points, d_scalars, mont, d_chunks, n_chunks, d_partials, st); break;
    case 4: msm_batch_launch_chunks<C, F, 4>(d_points, d_scalars, mont, d_chunks, n_chunks, d_partials, st); break;
    default: msm_batch_launch_chunks<C, F, 8>(d_points, d_scalars, mont, d_chunks, n_chunks, d_partials, st); break;
  }
}

// Straus chunks for every segment.  offsets: k + 1 checked host entries (api_msm.hip: mlhip_msm_batch_device), k >= 1
template <class C, class F>
int msm_batch_device(const void* d_points, const void* d_scalars, int mont, const uint64_t* offsets, size_t k, void* d_out,
                     hipStream_t st, bool subgroup = false) {
  const int P = msm_batch_chunk_len<C, F>();
  MsmBatchLayout L;
  if (!msm_batch_layout(L, offsets, k, P)) return mlhip_rt::fail(MLHIP_EINVAL, "msm batch: more than 2^32 - 1 chunks");
  return msm_batch_run<C, F>(L, nullptr, 0, d_out, st, [&](const MsmBatchChunk* d_chunks, uint32_t n_chunks, const void*, void* part, void*) {
    msm_batch_launch_chunks_p<C, F>(P, d_points, d_scalars, mont, d_chunks, n_chunks, part, st, subgroup);
  });
}
#endif  // __HIPCC__

}  // namespace mlhip

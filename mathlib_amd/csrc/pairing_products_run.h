// pairing_products_run.h -- K products of m > 4 pairs each (include/mlhip.h: MLHIP_PRODUCT_PAIRS): the
// Miller loops of all groups of all products in one launch (pairing_products.h has the layout), the fold of each product's
// partial values (k_gt_fold, pairing_kernels.h) and, for the fused form, the final exponentiation of the K folded values.
// Included by tu_pairing.inc (one translation unit per curve).
#pragma once
#include <mutex>
#include <vector>

#include "pairing_prepared_kernels.h"

namespace mlhip {

// device scratch of the long products: [index copy | partials], one persistent buffer per device (per curve: this header is
// compiled into one translation unit per curve).  Calls on different streams take it in the order they take the lock; each
// waits on the device for the event the previous one recorded after its last kernel (the pattern of msm_batch_run).
struct MillerProductsScratch {
  char* buf = nullptr;
  size_t cap = 0;
  hipEvent_t last = nullptr;
};
static std::mutex g_mp_mu;
static MillerProductsScratch g_mp[64];

static inline void miller_products_release() {
  std::lock_guard<std::mutex> lk(g_mp_mu);
  int cur = 0;
  const bool have_cur = hipGetDevice(&cur) == hipSuccess;
  for (int dev = 0; dev < 64; dev++) {
    MillerProductsScratch& mp = g_mp[dev];
    if (!mp.buf && !mp.last) continue;
    (void)hipSetDevice(dev);
    if (mp.last) {
      (void)hipEventSynchronize(mp.last);
      (void)hipEventDestroy(mp.last);
      mp.last = nullptr;
    }
    if (mp.buf) (void)hipFree(mp.buf);
    mp.buf = nullptr;
    mp.cap = 0;
  }
  if (have_cur) (void)hipSetDevice(cur);
}

// t: the prepared handle's tables (then q_index: m host entries or null = slot j takes point j; d_g2 unused), or null for the
// general form (d_g2: K m affine points).  what: 0 = Miller values, 2 = their final exponentiation.  m > 4, K >= 1, every
// argument checked by the caller (api_pairing.hip).
template <class C>
int miller_products_run(const mlhip_g2_prepared_tables* t, int what, const void* d_g1, const void* d_g2, const uint32_t* q_index,
                        size_t m, size_t K, void* d_out, hipStream_t st) {
  typedef Affine<FpField<C>> A1;
  typedef Affine<Fp2Field<C>> A2;
  const size_t per = miller_group_pick(K * m, getenv("MLHIP_MILLER_GROUP"));  // read per call: the tests flip it
  const MillerGroups mg = miller_groups(m, per);
  const size_t index_bytes = t ? ((m * sizeof(uint32_t) + 255) & ~(size_t)255) : 0;
  const size_t slab = miller_products_slab(K, mg.g, sizeof(Fp12<C>), index_bytes);
  if (slab == 0) return mlhip_rt::fail(MLHIP_EINVAL, "pairs_per_product: the partial values of one product exceed the 1 GiB scratch");
  const size_t need = index_bytes + slab * mg.g * sizeof(Fp12<C>);
  // the index copy leaves the caller's array before the call returns: staged in pageable host memory the copy below reads
  // synchronously with respect to the host (hipMemcpyAsync from pageable memory returns after the staging copy)
  std::vector<uint32_t> index;
  if (t) {
    index.resize(m);
    for (size_t j = 0; j < m; j++) index[j] = q_index ? q_index[j] : (uint32_t)j;
  }
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_mp_mu);
  MillerProductsScratch& mp = g_mp[dev & 63];
  if (need > mp.cap) {
    if (mp.buf) HIPCHK(hipFree(mp.buf));  // waits for the device: no earlier call is still reading it
    mp.buf = nullptr;
    mp.cap = 0;
    size_t want = need + need / 4;
    if (want > MILLER_PRODUCTS_SCRATCH_CAP) want = need > MILLER_PRODUCTS_SCRATCH_CAP ? need : MILLER_PRODUCTS_SCRATCH_CAP;
    HIPCHK(hipMalloc((void**)&mp.buf, want));
    mp.cap = want;
  }
  if (!mp.last)
    HIPCHK(hipEventCreateWithFlags(&mp.last, hipEventDisableTiming));
  else
    HIPCHK(hipStreamWaitEvent(st, mp.last, 0));
  const uint32_t* d_index = nullptr;
  if (t) {
    HIPCHK(hipMemcpyAsync(mp.buf, index.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    d_index = (const uint32_t*)mp.buf;
  }
  Fp12<C>* part = (Fp12<C>*)(mp.buf + index_bytes);
  // (g2_prepared_run's way to the general kernels; the groups never take it)
  auto general = [](int w, const void* a, const void* b, size_t p, size_t n, const void* in, void* o, hipStream_t s) {
    return pairing_device<C>(w, a, b, p, n, in, o, s);
  };
  int rc = 0;
  for (size_t k0 = 0; k0 < K && !rc; k0 += slab) {
    const size_t ks = K - k0 < slab ? K - k0 : slab, n = ks * mg.g;
    const A1* g1 = (const A1*)d_g1 + k0 * m;
    Fp12<C>* out = (Fp12<C>*)d_out + k0;
    if (t) {
      rc = g2_prepared_run<C>(t, 0, g1, nullptr, per, n, part, st, general, &mg, d_index);
    } else if (per == 1) {
      // groups of one pair ARE the plain call over K m products of one pair
      rc = pairing_device<C>(0, g1, (const A2*)d_g2 + k0 * m, 1, n, nullptr, part, st);
    } else {
      rc = pairing_device<C>(0, g1, (const A2*)d_g2 + k0 * m, per, n, nullptr, part, st, &mg);
    }
    if (!rc) rc = gt_fold_device<C>(part, mg.g, ks, out, st);
    if (!rc && what == 2) rc = pairing_device<C>(1, nullptr, nullptr, 1, ks, out, out, st);
  }
  // (recorded on failure too: whatever was queued still uses the buffer)
  HIPCHK(hipEventRecord(mp.last, st));
  return rc;
}

}  // namespace mlhip

// TEST ARTIFACT -- host (g++, -DMLHIP_HOST_USE_DEVICE_PATH: the 32-bit device field code) build of the GLV lattice split of
// BN254 G1 (mathlib_amd/csrc/msm_scalar_mul_endo.h: g1_glv_split, G1Split, g1_endo_chain) and of the G1 chunk body of
// mathlib_amd/csrc/msm_batch_endo.h over it, replayed lane by lane as tests/hostmath_batch_endo does for the other groups.
// Loaded by tests/test_g1_glv_host.py and tests/test_g1_glv_gpu.py through ctypes and compared with Python integers and
// oracle/pyref.py.  It is NOT part of libmlhip.so.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../mathlib_amd/csrc/msm_batch_endo.h"

using namespace mlhip;

typedef Bn254 C;
typedef FpField<C> F;

struct HostOps {
  static void dbl(XYZZ<F>& r, const XYZZ<F>& p) { xyzz_dbl<F>(r, p); }
  static void add(XYZZ<F>& acc, const XYZZ<F>& q) { xyzz_add<F>(acc, q); }
  static void madd(XYZZ<F>& acc, const Affine<F>& q) { xyzz_madd<F>(acc, q, false); }
};

template <int P>
static int batch(const void* points, const void* scalars, int mont, const uint64_t* offsets, size_t k, void* out) {
  MsmBatchLayout L;
  if (!msm_batch_layout(L, offsets, k, P)) return -1;
  const Affine<F>* pts = (const Affine<F>*)points;
  const uint32_t* sc = (const uint32_t*)scalars;
  std::vector<XYZZ<F>> cur(L.chunks.size()), next;
  for (size_t c = 0; c < L.chunks.size(); c++) {
    const MsmBatchChunk ch = L.chunks[c];
    if (ch.count < 1 || ch.count > (uint32_t)P) return -2;
    const Affine<F>* base = pts + ch.first;
    msm_batch_chunk_endo_g1<F, P, MsmBatchOps<F>>(cur[c], sc + 8 * ch.first, ch.count, mont != 0,
                                                 [&](Affine<F>& p, int j) { p = base[j]; });
  }
  const size_t passes = L.pass_begin.size() - 1;
  for (size_t q = 0; q < passes; q++) {
    const size_t g0 = L.pass_begin[q], g1 = L.pass_begin[q + 1];
    next.assign(g1 - g0, XYZZ<F>());
    for (size_t g = g0; g < g1; g++) {
      const MsmBatchGroup gr = L.groups[g];
      msm_batch_sum<F, MsmBatchOps<F>>(next[g - g0], gr.count, [&](XYZZ<F>& p, uint32_t i) { p = cur[gr.begin + i]; });
    }
    if (q + 1 == passes) {
      if (g1 - g0 != k) return -4;
      Affine<F>* o = (Affine<F>*)out;
      for (size_t s = 0; s < k; s++) xyzz_to_affine<F>(o[s], next[s]);
    }
    cur.swap(next);
  }
  return 0;
}

extern "C" {
// bit 0: G1Glv<C>::AVAILABLE, bit 1: ScalarMulEndo<C, true>::AVAILABLE (which the lattice split leaves as it was)
int glv_available(int curve) {
  switch (curve) {
    case 0: return (G1Glv<Bn254>::AVAILABLE ? 1 : 0) | (ScalarMulEndo<Bn254, true>::AVAILABLE ? 2 : 0);
    case 1: return (G1Glv<Bls381>::AVAILABLE ? 1 : 0) | (ScalarMulEndo<Bls381, true>::AVAILABLE ? 2 : 0);
    case 2: return (G1Glv<Bls377>::AVAILABLE ? 1 : 0) | (ScalarMulEndo<Bls377, true>::AVAILABLE ? 2 : 0);
    default: return -2;
  }
}
// the compiled constants: beta (Montgomery) and lambda, 32 bytes each; A1, B1, A2, B2, 16 bytes each, and their signs; the
// two rounding constants, 32 bytes each
void glv_constants(void* beta, void* lambda, void* basis, int* neg, void* g1, void* g2) {
  memcpy(beta, C::GLV_BETA, 32);
  memcpy(lambda, C::GLV_LAMBDA, 32);
  memcpy((char*)basis, C::GLV_A1, 16);
  memcpy((char*)basis + 16, C::GLV_B1, 16);
  memcpy((char*)basis + 32, C::GLV_A2, 16);
  memcpy((char*)basis + 48, C::GLV_B2, 16);
  neg[0] = C::GLV_A1_NEG;
  neg[1] = C::GLV_B1_NEG;
  neg[2] = C::GLV_A2_NEG;
  neg[3] = C::GLV_B2_NEG;
  memcpy(g1, C::GLV_G1, 32);
  memcpy(g2, C::GLV_G2, 32);
}
// (beta x, y) through the policy the chain reads its beta from
void glv_phi(const void* in, void* out) {
  Affine<F> p;
  memcpy(&p, in, sizeof(p));
  Fp<C> beta;
  G1Split<C>::beta(beta);
  F::mul(p.x, p.x, beta);
  memcpy(out, &p, sizeof(p));
}
// behind fr_canonical, as the kernels run it: a = |k1|, b = |k2| (32 bytes each), neg = their signs, canon = s mod r
void glv_split(const uint32_t* scalar, int mont, uint32_t* a_out, uint32_t* b_out, int* neg, uint32_t* canon_out) {
  uint32_t s[8], a[8], b[8];
  bool na, nb;
  fr_canonical<C>(s, scalar, mont != 0);
  g1_glv_split<C>(a, b, na, nb, s);
  memcpy(a_out, a, sizeof(a));
  memcpy(b_out, b, sizeof(b));
  memcpy(canon_out, s, sizeof(s));
  neg[0] = na;
  neg[1] = nb;
}
// the chain of k_scalar_mul_endo<Bn254>
void glv_g1_mul(const void* in, const uint32_t* scalar, int mont, void* out) {
  Affine<F> p, r;
  memcpy(&p, in, sizeof(p));
  uint32_t s[8];
  fr_canonical<C>(s, scalar, mont != 0);
  XYZZ<F> tab[8], acc;
  xyzz_from_affine<F>(tab[0], p);
  g1_endo_chain<C, F, HostOps>(acc, tab, p, s);
  xyzz_to_affine<F>(r, acc);
  memcpy(out, &r, sizeof(r));
}
// out[s] = the affine sum of segment s by the split chunks of length P.  0 on success, -5: P is not compiled.
int glv_msm_batch(int P, const void* points, const void* scalars, int mont, const uint64_t* offsets, size_t k, void* out) {
  switch (P) {
    case 1: return batch<1>(points, scalars, mont, offsets, k, out);
    case 2: return batch<2>(points, scalars, mont, offsets, k, out);
    case 4: return batch<4>(points, scalars, mont, offsets, k, out);
    case 8: return batch<8>(points, scalars, mont, offsets, k, out);
    default: return -5;
  }
}
}

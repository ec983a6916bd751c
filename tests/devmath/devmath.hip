// TEST ARTIFACT -- device (gfx950) build of the field multipliers that only exist under __HIP_DEVICE_COMPILE__:
// fp_mul_comba.inc (fp_mul_device / fp_mul2_device) and fp28_comba.inc (fp28_mul / sqr / mul2 / k2mul), plus the plain
// C++ around them (fp_add / sub / neg, fp28_normalize / reduce, the boundary conversions, the divsteps inversion).
// tests/test_devmath_gpu.py builds it twice -- libdevmath.so as shipped, libdevmath_portable.so with
// -DMLHIP_FP28_PORTABLE (the device then runs fp28_mont / fp28_k2mul_portable) -- loads both through ctypes and compares
// every output with Python integers.  It is NOT part of libmlhip.so and nothing in the product path links or loads it.
//
// One lane per vector, bounds-guarded, no shared memory, no cross-lane traffic.  Saturated operands are uint32_t[N] per
// vector, carry-free operands RAW limb arrays int32_t[N28] per vector (so a test can feed non-canonical, weighted and
// negative-limbed values); operand i of vector v starts at word v * (N or N28).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fp28.h"

using namespace mlhip;

#define DM_API extern "C" __attribute__((visibility("default")))

// op codes (tests/devmath_cases.py: OPS keeps the same numbers)
enum {
  DM_FP_MUL = 0,      // out-of-line entry fp_mul
  DM_FP_MUL_I = 1,    // inlined entry fp_mul_i
  DM_FP_SQR = 2,      // fp_sqr(a)
  DM_FP_MUL2 = 3,     // fp_mul2_device: a b + c d
  DM_FP_MUL_INLINE = 4,  // the portable CIOS fp_mul_inline, compiled for the device: the second form of the product
  DM_FP_ADD = 5,
  DM_FP_SUB = 6,
  DM_FP_NEG = 7,
  DM_FP_INV = 8,      // fp_inv: the entry every kernel calls (modinv.h: fp_inv_divsteps)
  DM_FP28_MUL = 16,
  DM_FP28_SQR = 17,
  DM_FP28_MUL2 = 18,
  DM_FP28_K2MUL = 19,  // (a, b, c, d) = (a0, a1, b0, b1); out = c0, out2 = c1
  DM_FP28_NORMALIZE = 20,
  DM_FP28_REDUCE = 21,
  DM_FP28_FROM_FP = 22,  // a: uint32_t[N]  -> out: int32_t[N28]
  DM_FP28_TO_FP = 23,    // a: int32_t[N28] -> out: uint32_t[N]
};

template <class C>
__device__ __forceinline__ void ld(Fp<C>& r, const void* p, size_t i) {
  const uint32_t* s = (const uint32_t*)p + i * C::N;
#pragma unroll
  for (int k = 0; k < C::N; k++) r.l[k] = s[k];
}
template <class C>
__device__ __forceinline__ void ld(Fp28<C>& r, const void* p, size_t i) {
  const int32_t* s = (const int32_t*)p + i * C::N28;
#pragma unroll
  for (int k = 0; k < C::N28; k++) r.l[k] = s[k];
}
template <class C>
__device__ __forceinline__ void st(void* p, size_t i, const Fp<C>& v) {
  uint32_t* d = (uint32_t*)p + i * C::N;
#pragma unroll
  for (int k = 0; k < C::N; k++) d[k] = v.l[k];
}
template <class C>
__device__ __forceinline__ void st(void* p, size_t i, const Fp28<C>& v) {
  int32_t* d = (int32_t*)p + i * C::N28;
#pragma unroll
  for (int k = 0; k < C::N28; k++) d[k] = v.l[k];
}

// OP is a template parameter: every op compiles the way the kernels see it (operands in registers, the multiplier inlined
// or called as there), not behind a run-time switch
template <class C, int OP>
__global__ void __launch_bounds__(256) k_devmath(const void* __restrict__ a, const void* __restrict__ b, const void* __restrict__ c,
                                                 const void* __restrict__ d, void* __restrict__ out, void* __restrict__ out2, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
#if defined(__HIP_DEVICE_COMPILE__)  // fp_mul_device / fp_mul2_device do not exist in the host pass
  if constexpr (OP < 16) {
    Fp<C> x, y, z, w, r;
    ld<C>(x, a, i);
    if constexpr (OP != DM_FP_SQR && OP != DM_FP_NEG && OP != DM_FP_INV) ld<C>(y, b, i);
    if constexpr (OP == DM_FP_MUL2) {
      ld<C>(z, c, i);
      ld<C>(w, d, i);
    }
    if constexpr (OP == DM_FP_MUL) fp_mul<C>(r, x, y);
    if constexpr (OP == DM_FP_MUL_I) fp_mul_i<C>(r, x, y);
    if constexpr (OP == DM_FP_SQR) fp_sqr<C>(r, x);
    if constexpr (OP == DM_FP_MUL2) fp_mul2_device<C>(r, x, y, z, w);
    if constexpr (OP == DM_FP_MUL_INLINE) fp_mul_inline<C>(r, x, y);
    if constexpr (OP == DM_FP_ADD) fp_add<C>(r, x, y);
    if constexpr (OP == DM_FP_SUB) fp_sub<C>(r, x, y);
    if constexpr (OP == DM_FP_NEG) fp_neg<C>(r, x);
    if constexpr (OP == DM_FP_INV) fp_inv<C>(r, x);
    st<C>(out, i, r);
  } else if constexpr (OP == DM_FP28_FROM_FP) {
    Fp<C> x;
    Fp28<C> r;
    ld<C>(x, a, i);
    fp28_from_fp<C>(r, x);
    st<C>(out, i, r);
  } else if constexpr (OP == DM_FP28_TO_FP) {
    Fp28<C> x;
    Fp<C> r;
    ld<C>(x, a, i);
    fp28_to_fp<C>(r, x);
    st<C>(out, i, r);
  } else {
    Fp28<C> x, y, z, w, r, r2;
    ld<C>(x, a, i);
    if constexpr (OP == DM_FP28_MUL || OP == DM_FP28_MUL2 || OP == DM_FP28_K2MUL) ld<C>(y, b, i);
    if constexpr (OP == DM_FP28_MUL2 || OP == DM_FP28_K2MUL) {
      ld<C>(z, c, i);
      ld<C>(w, d, i);
    }
    if constexpr (OP == DM_FP28_MUL) fp28_mul<C>(r, x, y);
    if constexpr (OP == DM_FP28_SQR) fp28_sqr<C>(r, x);
    if constexpr (OP == DM_FP28_MUL2) fp28_mul2<C>(r, x, y, z, w);
    if constexpr (OP == DM_FP28_K2MUL) {
      fp28_k2mul<C>(r, r2, x, y, z, w);
      st<C>(out2, i, r2);
    }
    if constexpr (OP == DM_FP28_NORMALIZE) fp28_normalize<C>(r, x);
    if constexpr (OP == DM_FP28_REDUCE) fp28_reduce<C>(r, x);
    st<C>(out, i, r);
  }
#endif
}

template <class C, int OP>
static int launch(const void* a, const void* b, const void* c, const void* d, void* out, void* out2, size_t n) {
  if (n == 0) return 0;
  k_devmath<C, OP><<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0>>>(a, b, c, d, out, out2, n);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return e == hipSuccess ? 0 : 1000 + (int)e;
}

#define DM_CASE(OP) \
  case OP: return launch<C, OP>(a, b, c, d, out, out2, n);

template <class C>
static int run(int op, const void* a, const void* b, const void* c, const void* d, void* out, void* out2, size_t n) {
  const int arity = (op == DM_FP_MUL2 || op == DM_FP28_MUL2 || op == DM_FP28_K2MUL)                         ? 4
                    : (op == DM_FP_SQR || op == DM_FP_NEG || op == DM_FP_INV || op == DM_FP28_SQR || op >= DM_FP28_NORMALIZE) ? 1
                                                                                                                 : 2;
  if (!a || !out || (arity >= 2 && !b) || (arity == 4 && (!c || !d)) || (op == DM_FP28_K2MUL && !out2)) return -3;
  switch (op) {
    DM_CASE(DM_FP_MUL)
    DM_CASE(DM_FP_MUL_I)
    DM_CASE(DM_FP_SQR)
    DM_CASE(DM_FP_MUL2)
    DM_CASE(DM_FP_MUL_INLINE)
    DM_CASE(DM_FP_ADD)
    DM_CASE(DM_FP_SUB)
    DM_CASE(DM_FP_NEG)
    DM_CASE(DM_FP_INV)
    DM_CASE(DM_FP28_MUL)
    DM_CASE(DM_FP28_SQR)
    DM_CASE(DM_FP28_MUL2)
    DM_CASE(DM_FP28_K2MUL)
    DM_CASE(DM_FP28_NORMALIZE)
    DM_CASE(DM_FP28_REDUCE)
    DM_CASE(DM_FP28_FROM_FP)
    DM_CASE(DM_FP28_TO_FP)
    default: return -1;
  }
}

// 0, or -1 unknown op, -2 unknown curve, -3 a missing operand, 1000 + the hipError_t of the launch.  All pointers are
// device pointers to n vectors; unused operands may be null.  Runs on the null stream and returns after the kernel ended.
DM_API int dm_run(int curve, int op, const void* a, const void* b, const void* c, const void* d, void* out, void* out2, size_t n) {
  switch (curve) {
    case 0: return run<Bn254>(op, a, b, c, d, out, out2, n);
    case 1: return run<Bls381>(op, a, b, c, d, out, out2, n);
    case 2: return run<Bls377>(op, a, b, c, d, out, out2, n);
    default: return -2;
  }
}

// 1 when the carry-free products are the generated asm bodies, 0 when they are the portable C++ (-DMLHIP_FP28_PORTABLE)
DM_API int dm_fp28_is_asm(void) {
#ifdef MLHIP_FP28_PORTABLE
  return 0;
#else
  return 1;
#endif
}

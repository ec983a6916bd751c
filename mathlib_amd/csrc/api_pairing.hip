// api_pairing.hip -- the pairing, Gt and prepared-G2 entry points of include/mlhip.h (and the field-multiplication probe):
// argument checking, host-buffer staging and dispatch.  No kernels here.
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "mlhip_rt.h"

using namespace mlhip_rt;

namespace {
// ---- what every entry point with a curve id begins with --------------------------------------------------------------------
// The ops row of the curve, or null with `rc` the status to return at once (0: n == 0, nothing to do).  The ORDER of the
// checks is behaviour (a machine without a device tells the orders apart; tests/test_gt_api_status_host.py):
//   ARGS_THEN_DEVICE  curve, n == 0, null pointers, the device: the host forms and the newer _device forms
//   ARGS_ONLY         curve, n == 0, null pointers: pairing_host, which looks for the device after it has spread the batch
//   DEVICE_N_CURVE    the device, n == 0, the curve, no pointer checks: mlhip_gt_mul_device, _gt_exp_device, _fp_mul_device
//   DEVICE_CURVE      the device, the curve, no pointer checks: the three pairing _device forms (n == 0 is the launcher's)
enum CheckOrder { ARGS_THEN_DEVICE, ARGS_ONLY, DEVICE_N_CURVE, DEVICE_CURVE };
const CurveOps* begin_call(CheckOrder order, int curve, size_t n, bool any_null, int& rc) {
  const bool device_first = order == DEVICE_N_CURVE || order == DEVICE_CURVE;
  rc = device_first ? ensure_device() : 0;
  if (rc || (order == DEVICE_N_CURVE && n == 0)) return nullptr;
  const CurveOps* ops = curve_ops(curve);
  if (!ops) {
    rc = mlhip_rt::fail(MLHIP_EINVAL, "unknown curve id");
    return nullptr;
  }
  if (device_first) return ops;
  if (n == 0) return nullptr;
  if (any_null) {
    rc = mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
    return nullptr;
  }
  if (order == ARGS_THEN_DEVICE) rc = ensure_device();
  return rc ? nullptr : ops;
}

// ---- one host-buffer call on this thread's device: upload, run, download ---------------------------------------------------
// n elements of `each` bytes behind every host pointer, at most MAX_BUFS pointers a list.  The arena is reserved for the sum
// of the two lists, the inputs are uploaded and the outputs allocated in list order, run(d_in, d_out, stream) launches on the
// device copies, and the outputs are brought back: all copies queued, one wait for the stream (HostCall::down) at the end.
struct HostIn {
  const void* p;
  size_t each;
};
struct HostOut {
  void* p;
  size_t each;
};
constexpr size_t MAX_BUFS = 4;
template <class Run>
int staged_call(size_t n, std::initializer_list<HostIn> ins, std::initializer_list<HostOut> outs, Run run) {
  if (ins.size() > MAX_BUFS || outs.size() > MAX_BUFS || outs.size() == 0) return mlhip_rt::fail(MLHIP_EINVAL, "internal: staged_call lists");
  HostCall hc;
  size_t total = 0;
  for (const HostIn& b : ins) total += n * b.each;
  for (const HostOut& b : outs) total += n * b.each;
  hc.reserve(total);
  void *din[MAX_BUFS] = {}, *dout[MAX_BUFS] = {};
  size_t k = 0;
  for (const HostIn& b : ins) din[k++] = hc.up(b.p, n * b.each);
  k = 0;
  for (const HostOut& b : outs) dout[k++] = hc.dev(n * b.each);
  if (hc.rc) return hc.rc;
  const int rc = run(din, dout, hc.l.st);
  if (rc) return rc;
  const HostOut* o = outs.begin();
  for (k = 0; k + 1 < outs.size(); k++)
    if (hipMemcpyAsync(o[k].p, dout[k], n * o[k].each, hipMemcpyDeviceToHost, hc.l.st) != hipSuccess)
      return mlhip_rt::fail(MLHIP_EHIP, "hipMemcpy D2H failed");
  return hc.down(o[k].p, dout[k], n * o[k].each);
}

// host-buffer wrapper around the pairing kernels
int pairing_host(int curve, int what, const void* g1, const void* g2, size_t ppp, size_t n, const void* in, void* out) {
  int rc;
  const CurveOps* ops = begin_call(ARGS_ONLY, curve, n, !out || (what == 1 ? !in : (!g1 || !g2)), rc);
  if (!ops) return rc;
  // independent per element: a large batch is split over the process's devices, no exchange at all
  const std::vector<int> devs = spread_devices(n, true);
  if (!devs.empty())
    return run_on_devices(devs, n, [&](size_t, size_t lo, size_t hi) {
      return pairing_host(curve, what, g1 ? (const char*)g1 + lo * ppp * ops->g1 : nullptr,
                          g2 ? (const char*)g2 + lo * ppp * ops->g2 : nullptr, ppp, hi - lo,
                          in ? (const char*)in + lo * ops->gt : nullptr, (char*)out + lo * ops->gt);
    });
  rc = ensure_device();
  if (rc) return rc;
  if (what == 1)
    return staged_call(n, {{in, ops->gt}}, {{out, ops->gt}}, [&](void* const* d, void* const* o, hipStream_t st) {
      return ops->pairing(what, nullptr, nullptr, ppp, n, d[0], o[0], st);
    });
  return staged_call(n, {{g1, ppp * ops->g1}, {g2, ppp * ops->g2}}, {{out, ops->gt}}, [&](void* const* d, void* const* o, hipStream_t st) {
    return ops->pairing(what, d[0], d[1], ppp, n, nullptr, o[0], st);
  });
}

// the same on device pointers, in order on `stream`
int pairing_device(int curve, int what, const void* d_g1, const void* d_g2, size_t ppp, size_t n, const void* d_in, void* d_out,
                   void* stream) {
  int rc;
  const CurveOps* ops = begin_call(DEVICE_CURVE, curve, n, false, rc);
  return ops ? ops->pairing(what, d_g1, d_g2, ppp, n, d_in, d_out, (hipStream_t)stream) : rc;
}

// ---- pairs_per_product as the six Miller-loop entry points take it (include/mlhip.h): a plain 1 .. 4, or
// MLHIP_PRODUCT_PAIRS(m) -- bit 63 set, m in the low 32 bits.  m <= 4 is the plain call whichever way it was said.
int unpack_pairs(size_t ppp, size_t& m) {
  m = ppp;
  if (!(ppp >> 63)) return ppp < 1 || ppp > 4 ? mlhip_rt::fail(MLHIP_EINVAL, "pairs_per_product must be 1..4") : 0;
  m = ppp & 0xFFFFFFFFu;
  if (((ppp << 1) >> 33) != 0 || m == 0) return mlhip_rt::fail(MLHIP_EINVAL, "MLHIP_PRODUCT_PAIRS(m): m must be 1 .. 2^32 - 1");
  return 0;
}
// n products of m pairs: n m pairs of `each` bytes must be addressable
int check_products(size_t m, size_t n, size_t each) {
  if (n > SIZE_MAX / m || n * m > SIZE_MAX / each) return mlhip_rt::fail(MLHIP_EINVAL, "n_products * pairs_per_product overflows");
  return 0;
}

// K products of m > 4 pairs against per-product G2 points (pairing_products_run.h): on the calling thread's device, never
// spread over the device list
int products_host(int curve, const void* g1, const void* g2, size_t m, size_t n, void* out) {
  int rc;
  const CurveOps* ops = begin_call(ARGS_ONLY, curve, n, !out || !g1 || !g2, rc);
  if (!ops) return rc;
  if ((rc = check_products(m, n, ops->gt)) != 0 || (rc = ensure_device()) != 0) return rc;
  return staged_call(n, {{g1, m * ops->g1}, {g2, m * ops->g2}}, {{out, ops->gt}}, [&](void* const* d, void* const* o, hipStream_t st) {
    return ops->miller_products(nullptr, 0, d[0], d[1], nullptr, m, n, o[0], st);
  });
}
int products_device(int curve, const void* d_g1, const void* d_g2, size_t m, size_t n, void* d_out, void* stream) {
  int rc;
  const CurveOps* ops = begin_call(DEVICE_CURVE, curve, n, false, rc);
  if (!ops || n == 0) return rc;
  if (!d_g1 || !d_g2 || !d_out) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  if ((rc = check_products(m, n, ops->gt)) != 0) return rc;
  return ops->miller_products(nullptr, 0, d_g1, d_g2, nullptr, m, n, d_out, (hipStream_t)stream);
}
}  // namespace

extern "C" {

int mlhip_miller_loop(int curve, const void* g1, const void* g2, size_t ppp, size_t n_products, void* out_gt) {
  size_t m;
  if (int rc = unpack_pairs(ppp, m)) return rc;
  if (m > 4) return products_host(curve, g1, g2, m, n_products, out_gt);
  return pairing_host(curve, 0, g1, g2, m, n_products, nullptr, out_gt);
}

int mlhip_final_exp(int curve, const void* in_gt, size_t n, void* out_gt) {
  return pairing_host(curve, 1, nullptr, nullptr, 1, n, in_gt, out_gt);
}

int mlhip_pairing_batch(int curve, const void* g1, const void* g2, size_t n, void* out_gt) {
  return pairing_host(curve, 2, g1, g2, 1, n, nullptr, out_gt);
}

int mlhip_miller_loop_device(int curve, const void* d_g1, const void* d_g2, size_t ppp, size_t n_products,
                             void* d_out_gt, void* stream) {
  size_t m;
  if (int rc = unpack_pairs(ppp, m)) return rc;
  if (m > 4) return products_device(curve, d_g1, d_g2, m, n_products, d_out_gt, stream);
  return pairing_device(curve, 0, d_g1, d_g2, m, n_products, nullptr, d_out_gt, stream);
}

int mlhip_final_exp_device(int curve, const void* d_in_gt, size_t n, void* d_out_gt, void* stream) {
  return pairing_device(curve, 1, nullptr, nullptr, 1, n, d_in_gt, d_out_gt, stream);
}

int mlhip_pairing_batch_device(int curve, const void* d_g1, const void* d_g2, size_t n, void* d_out_gt, void* stream) {
  return pairing_device(curve, 2, d_g1, d_g2, 1, n, nullptr, d_out_gt, stream);
}

// ---- prepared G2 handles (include/mlhip.h; kernels: pairing_prepared_kernels.h) ---------------------------------------------
struct mlhip_g2_prepared {
  mlhip_g2_prepared_tables t;
  const CurveOps* ops = nullptr;
  int device = 0;
};

int mlhip_g2_prepared_destroy(mlhip_g2_prepared* h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  if (h->t.d_q) (void)hipFree(h->t.d_q);
  if (h->t.d_t28) (void)hipFree(h->t.d_t28);
  if (h->t.d_t32) (void)hipFree(h->t.d_t32);
  if (h->t.d_inf) (void)hipFree(h->t.d_inf);
  delete h;
  return 0;
}

static int g2_prepared_create(int curve, const void* points, bool on_device, size_t m, mlhip_g2_prepared** out) {
  const CurveOps* ops = curve_ops(curve);
  if (!ops) return mlhip_rt::fail(MLHIP_EINVAL, "unknown curve id");
  if (!out) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  *out = nullptr;
  if (m == 0) return mlhip_rt::fail(MLHIP_EINVAL, "mlhip_g2_prepared_create: m must be at least 1");
  if (!points) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  int rc = ensure_device();
  if (rc) return rc;
  mlhip_g2_prepared* h = new mlhip_g2_prepared;
  h->ops = ops;
  h->device = call_device();
  h->t.m = m;
  auto body = [&]() -> int {
    HIPCHK(hipMalloc(&h->t.d_q, m * ops->g2));
    HostCall hc;  // a leased stream: the build does not meet other callers on the null stream
    if (hc.rc) return hc.rc;
    HIPCHK(hipMemcpyAsync(h->t.d_q, points, m * ops->g2, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, hc.l.st));
    int r = ops->g2_prepared(&h->t, -1, nullptr, nullptr, 0, 0, nullptr, hc.l.st);
    if (r) return r;
    HIPCHK(hipStreamSynchronize(hc.l.st));
    return 0;
  };
  rc = body();
  if (rc) {
    mlhip_g2_prepared_destroy(h);
    return rc;
  }
  *out = h;
  return 0;
}

int mlhip_g2_prepared_create(int curve, const void* g2_points, size_t m, mlhip_g2_prepared** h) {
  return g2_prepared_create(curve, g2_points, false, m, h);
}

int mlhip_g2_prepared_create_device(int curve, const void* d_g2_points, size_t m, mlhip_g2_prepared** h) {
  return g2_prepared_create(curve, d_g2_points, true, m, h);
}

int mlhip_g2_prepared_count(mlhip_g2_prepared* h, size_t* m) {
  if (!h || !m) return mlhip_rt::fail(MLHIP_EINVAL, h ? "null pointer" : "null handle");
  *m = h->t.m;
  return 0;
}

// every argument error of the four entry points, before anything is launched; 1 = nothing to do.  ppp: as the caller
// gave it; m: the pairs per product it means (unpack_pairs)
static int g2_prepared_check(const mlhip_g2_prepared* h, const void* g1, const uint32_t* q_index, size_t ppp, size_t n,
                             const void* out, size_t& m) {
  if (!h) return mlhip_rt::fail(MLHIP_EINVAL, "null handle");
  if (int rc = unpack_pairs(ppp, m)) return rc;
  if (q_index) {
    for (size_t j = 0; j < m; j++)
      if (q_index[j] >= h->t.m) return mlhip_rt::fail(MLHIP_EINVAL, "q_index entry beyond the handle's points");
  } else if (m > h->t.m) {
    return mlhip_rt::fail(MLHIP_EINVAL, "pairs_per_product exceeds the handle's points (no q_index)");
  }
  if (n == 0) return 1;
  if (!g1 || !out) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  if (m > 4) return check_products(m, n, h->ops->gt);
  return 0;
}

// the launch: products of at most 4 pairs through the prepared kernels' own dispatcher, longer ones through the groups
static int g2_prepared_launch(mlhip_g2_prepared* h, int what, const void* d_g1, const uint32_t* q_index, size_t m, size_t n,
                              void* d_out, hipStream_t st) {
  if (m > 4) return h->ops->miller_products(&h->t, what, d_g1, nullptr, q_index, m, n, d_out, st);
  return h->ops->g2_prepared(&h->t, what, d_g1, q_index, m, n, d_out, st);
}

static int g2_prepared_device(mlhip_g2_prepared* h, int what, const void* d_g1, const uint32_t* q_index, size_t ppp, size_t n,
                              void* d_out, void* stream) {
  size_t m;
  int rc = g2_prepared_check(h, d_g1, q_index, ppp, n, d_out, m);
  if (rc) return rc < 0 ? rc : 0;
  // the launch needs the handle's device current; the caller gets its own current device back (`stream` and the pointers
  // must belong to the handle's device: multi-device handles are out of scope)
  int prev = h->device;
  (void)hipGetDevice(&prev);
  if (prev != h->device && hipSetDevice(h->device) != hipSuccess) return mlhip_rt::fail(MLHIP_EHIP, "hipSetDevice failed");
  rc = g2_prepared_launch(h, what, d_g1, q_index, m, n, d_out, (hipStream_t)stream);
  if (prev != h->device) (void)hipSetDevice(prev);
  return rc;
}

static int g2_prepared_host(mlhip_g2_prepared* h, int what, const void* g1, const uint32_t* q_index, size_t ppp, size_t n,
                            void* out) {
  size_t m;
  int rc = g2_prepared_check(h, g1, q_index, ppp, n, out, m);
  if (rc) return rc < 0 ? rc : 0;
  if (hipSetDevice(h->device) != hipSuccess) return mlhip_rt::fail(MLHIP_EHIP, "hipSetDevice failed");
  call_device() = h->device;  // thread_local (the device of this thread's call in progress): the call's scratch is leased on the handle's device
  HostCall hc;
  hc.reserve(n * m * h->ops->g1 + n * h->ops->gt);
  void* d1 = hc.up(g1, n * m * h->ops->g1);
  void* dout = hc.dev(n * h->ops->gt);
  if (hc.rc) return hc.rc;
  rc = g2_prepared_launch(h, what, d1, q_index, m, n, dout, hc.l.st);
  if (rc) return rc;
  return hc.down(out, dout, n * h->ops->gt);
}

int mlhip_miller_loop_prepared(mlhip_g2_prepared* h, const void* g1, const uint32_t* q_index, size_t ppp, size_t n_products,
                               void* out_gt) {
  return g2_prepared_host(h, 0, g1, q_index, ppp, n_products, out_gt);
}

int mlhip_miller_loop_prepared_device(mlhip_g2_prepared* h, const void* d_g1, const uint32_t* q_index, size_t ppp,
                                      size_t n_products, void* d_out_gt, void* stream) {
  return g2_prepared_device(h, 0, d_g1, q_index, ppp, n_products, d_out_gt, stream);
}

int mlhip_pairing_prepared(mlhip_g2_prepared* h, const void* g1, const uint32_t* q_index, size_t ppp, size_t n_products,
                           void* out_gt) {
  return g2_prepared_host(h, 2, g1, q_index, ppp, n_products, out_gt);
}

int mlhip_pairing_prepared_device(mlhip_g2_prepared* h, const void* d_g1, const uint32_t* q_index, size_t ppp,
                                  size_t n_products, void* d_out_gt, void* stream) {
  return g2_prepared_device(h, 2, d_g1, q_index, ppp, n_products, d_out_gt, stream);
}

int mlhip_gt_mul_device(int curve, const void* d_a, const void* d_b, size_t n, void* d_out, void* stream) {
  int rc;
  const CurveOps* ops = begin_call(DEVICE_N_CURVE, curve, n, false, rc);
  return ops ? ops->gt_mul(d_a, d_b, n, d_out, (hipStream_t)stream) : rc;
}

int mlhip_gt_mul(int curve, const void* a, const void* b, size_t n, void* out) {
  int rc;
  const CurveOps* ops = begin_call(ARGS_THEN_DEVICE, curve, n, !a || !b || !out, rc);
  if (!ops) return rc;
  return staged_call(n, {{a, ops->gt}, {b, ops->gt}}, {{out, ops->gt}}, [&](void* const* d, void* const* o, hipStream_t st) {
    return ops->gt_mul(d[0], d[1], n, o[0], st);
  });
}

int mlhip_gt_exp_device(int curve, const void* d_in, const void* d_scalars, int mont, size_t n, void* d_out, void* stream) {
  int rc;
  const CurveOps* ops = begin_call(DEVICE_N_CURVE, curve, n, false, rc);
  return ops ? ops->gt_exp(d_in, d_scalars, mont, n, d_out, (hipStream_t)stream) : rc;
}

int mlhip_gt_exp(int curve, const void* in, const void* scalars, int mont, size_t n, void* out) {
  int rc;
  const CurveOps* ops = begin_call(ARGS_THEN_DEVICE, curve, n, !in || !scalars || !out, rc);
  if (!ops) return rc;
  return staged_call(n, {{in, ops->gt}, {scalars, 32}}, {{out, ops->gt}}, [&](void* const* d, void* const* o, hipStream_t st) {
    return ops->gt_exp(d[0], d[1], mont, n, o[0], st);
  });
}

// Gt.Exp for members of Gt (gt_exp_cyclo.h)
int mlhip_gt_exp_cyclo_device(int curve, const void* d_in, const void* d_scalars, int mont, size_t n, void* d_out, void* stream) {
  int rc;
  const CurveOps* ops = begin_call(ARGS_THEN_DEVICE, curve, n, !d_in || !d_scalars || !d_out, rc);
  return ops ? ops->gt_exp_cyclo(d_in, d_scalars, mont, n, d_out, (hipStream_t)stream) : rc;
}

int mlhip_gt_exp_cyclo(int curve, const void* in, const void* scalars, int mont, size_t n, void* out) {
  int rc;
  const CurveOps* ops = begin_call(ARGS_THEN_DEVICE, curve, n, !in || !scalars || !out, rc);
  if (!ops) return rc;
  return staged_call(n, {{in, ops->gt}, {scalars, 32}}, {{out, ops->gt}}, [&](void* const* d, void* const* o, hipStream_t st) {
    return ops->gt_exp_cyclo(d[0], d[1], mont, n, o[0], st);
  });
}

// ---- Gt wire codec, membership test and inverse (gt_codec.h) ---------------------------------------------------------------
int mlhip_gt_from_bytes_device(int curve, const void* d_wire, size_t n, int subgroup_check, void* d_out, unsigned char* d_status,
                               void* stream) {
  int rc;
  const CurveOps* ops = begin_call(ARGS_THEN_DEVICE, curve, n, !d_wire || !d_out || !d_status, rc);
  return ops ? ops->gt_decode(d_wire, n, subgroup_check ? 1 : 0, d_out, d_status, (hipStream_t)stream) : rc;
}

int mlhip_gt_from_bytes(int curve, const void* wire, size_t n, int subgroup_check, void* out, unsigned char* status) {
  int rc;
  const CurveOps* ops = begin_call(ARGS_THEN_DEVICE, curve, n, !wire || !out || !status, rc);
  if (!ops) return rc;
  // (the statuses first: their small copy is queued, the wait is for the values)
  return staged_call(n, {{wire, ops->gt}}, {{status, 1}, {out, ops->gt}}, [&](void* const* d, void* const* o, hipStream_t st) {
    return ops->gt_decode(d[0], n, subgroup_check ? 1 : 0, o[1], o[0], st);
  });
}

int mlhip_gt_to_bytes_device(int curve, const void* d_gt, size_t n, void* d_wire, void* stream) {
  int rc;
  const CurveOps* ops = begin_call(ARGS_THEN_DEVICE, curve, n, !d_gt || !d_wire, rc);
  return ops ? ops->gt_encode(d_gt, n, d_wire, (hipStream_t)stream) : rc;
}

int mlhip_gt_to_bytes(int curve, const void* gt, size_t n, void* wire) {
  int rc;
  const CurveOps* ops = begin_call(ARGS_THEN_DEVICE, curve, n, !gt || !wire, rc);
  if (!ops) return rc;
  return staged_call(n, {{gt, ops->gt}}, {{wire, ops->gt}}, [&](void* const* d, void* const* o, hipStream_t st) {
    return ops->gt_encode(d[0], n, o[0], st);
  });
}

int mlhip_gt_is_member_device(int curve, const void* d_gt, size_t n, unsigned char* d_status, void* stream) {
  int rc;
  const CurveOps* ops = begin_call(ARGS_THEN_DEVICE, curve, n, !d_gt || !d_status, rc);
  return ops ? ops->gt_is_member(d_gt, n, d_status, nullptr, (hipStream_t)stream) : rc;
}

int mlhip_gt_is_member(int curve, const void* gt, size_t n, unsigned char* status) {
  int rc;
  const CurveOps* ops = begin_call(ARGS_THEN_DEVICE, curve, n, !gt || !status, rc);
  if (!ops) return rc;
  return staged_call(n, {{gt, ops->gt}}, {{status, 1}}, [&](void* const* d, void* const* o, hipStream_t st) {
    return ops->gt_is_member(d[0], n, o[0], nullptr, st);
  });
}

int mlhip_gt_inverse_device(int curve, const void* d_in, size_t n, void* d_out, void* stream) {
  int rc;
  const CurveOps* ops = begin_call(ARGS_THEN_DEVICE, curve, n, !d_in || !d_out, rc);
  return ops ? ops->gt_inverse(d_in, n, d_out, (hipStream_t)stream) : rc;
}

int mlhip_gt_inverse(int curve, const void* in, size_t n, void* out) {
  int rc;
  const CurveOps* ops = begin_call(ARGS_THEN_DEVICE, curve, n, !in || !out, rc);
  if (!ops) return rc;
  return staged_call(n, {{in, ops->gt}}, {{out, ops->gt}}, [&](void* const* d, void* const* o, hipStream_t st) {
    return ops->gt_inverse(d[0], n, o[0], st);
  });
}

int mlhip_pairing_product(int curve, const void* g1, const void* g2, size_t n, void* out) {
  const CurveOps* ops = curve_ops(curve);
  if (!ops) return mlhip_rt::fail(MLHIP_EINVAL, "unknown curve id");
  if (!out) return mlhip_rt::fail(MLHIP_EINVAL, "null output pointer");
  if (n && (!g1 || !g2)) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  int rc = ensure_device();
  if (rc) return rc;
  // n == 0: the empty product, FExp(1) = 1; run it through the same kernels with one infinity pair
  const size_t m0 = n ? n : 1;
  HostCall hc;
  hc.reserve(m0 * (ops->g1 + ops->g2 + ops->gt));
  void *d1, *d2;
  if (n) {
    d1 = hc.up(g1, n * ops->g1);
    d2 = hc.up(g2, n * ops->g2);
  } else {
    d1 = hc.dev(ops->g1);
    d2 = hc.dev(ops->g2);
    if (!hc.rc && (hipMemsetAsync(d1, 0, ops->g1, hc.l.st) != hipSuccess || hipMemsetAsync(d2, 0, ops->g2, hc.l.st) != hipSuccess))
      hc.rc = mlhip_rt::fail(MLHIP_EHIP, "hipMemset failed");
  }
  void* dgt = hc.dev(m0 * ops->gt);
  if (hc.rc) return hc.rc;
  // One Miller loop per lane pair while the pairs do not fill the GPU (latency: 7 pairs take 21 ms this way, 45 ms
  // grouped -- measured); beyond 2^17 pairs four pairs share one accumulator's squarings (throughput).
  const size_t per = m0 >= ((size_t)1 << 17) ? 4 : 1;
  const size_t groups = m0 / per, rest = m0 % per;
  rc = ops->pairing(0, d1, d2, per, groups, nullptr, dgt, hc.l.st);
  if (!rc && rest)
    rc = ops->pairing(0, (const char*)d1 + per * groups * ops->g1, (const char*)d2 + per * groups * ops->g2, rest, 1,
                    nullptr, (char*)dgt + groups * ops->gt, hc.l.st);
  // tree product: fold the upper part onto the lower part until one value is left
  size_t m = groups + (rest ? 1 : 0);
  while (m > 1 && rc == 0) {
    size_t half = m / 2;
    rc = mlhip_gt_mul_device(curve, dgt, (const char*)dgt + (m - half) * ops->gt, half, dgt, hc.l.st);
    m -= half;
  }
  if (!rc) rc = ops->pairing(1, nullptr, nullptr, 1, 1, dgt, dgt, hc.l.st);
  if (rc) return rc;
  return hc.down(out, dgt, ops->gt);
}

int mlhip_fp_mul_device(int curve, const void* d_a, const void* d_b, size_t n, int repeat, void* d_out, void* stream) {
  int rc;
  const CurveOps* ops = begin_call(DEVICE_N_CURVE, curve, n, false, rc);
  return ops ? ops->fp_mul(d_a, d_b, n, repeat, d_out, (hipStream_t)stream) : rc;
}

}  // extern "C"

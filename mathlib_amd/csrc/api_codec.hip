// api_codec.hip -- the wire-format entry points of include/mlhip.h (mlhip_g{1,2}_{from,to}_bytes and their device forms).
// No kernels here.
#include <string>

#include "mlhip_rt.h"

using namespace mlhip_rt;

namespace {
int from_bytes_device(int curve, int group, const void* d_wire, size_t n, int compressed, int subgroup_check,
                             void* d_out, unsigned char* d_status, void* stream) {
  int rc = ensure_device();
  if (rc) return rc;
  const CurveOps* ops = curve_ops(curve);
  if (!ops) return mlhip_rt::fail(MLHIP_EINVAL, "unknown curve id");
  return ops->wire_codec(group, 0, d_wire, n, compressed ? 1 : 0, subgroup_check == 2 ? 2 : (subgroup_check ? 1 : 0), d_out, d_status,
                         (hipStream_t)stream);
}

int to_bytes_device(int curve, int group, const void* d_affine, size_t n, int compressed, void* d_wire, void* stream) {
  int rc = ensure_device();
  if (rc) return rc;
  const CurveOps* ops = curve_ops(curve);
  if (!ops) return mlhip_rt::fail(MLHIP_EINVAL, "unknown curve id");
  return ops->wire_codec(group, 1, d_affine, n, compressed ? 1 : 0, 0, d_wire, nullptr, (hipStream_t)stream);
}

int from_bytes_host(int curve, int group, const void* wire, size_t n, int compressed, int subgroup_check, void* out,
                           unsigned char* status) {
  const CurveOps* ops = curve_ops(curve);
  if (!ops) return mlhip_rt::fail(MLHIP_EINVAL, "unknown curve id");
  if (n == 0) return 0;
  if (!wire || !out || !status) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  int rc = ensure_device();
  if (rc) return rc;
  const size_t psz = ops->point_size(group);
  const size_t wlen = compressed ? psz / 2 : psz;
  HostCall hc;
  hc.reserve(n * (wlen + psz + 1));
  void* dw = hc.up(wire, n * wlen);
  void* dout = hc.dev(n * psz);
  void* dst = hc.dev(n);
  if (hc.rc) return hc.rc;
  rc = from_bytes_device(curve, group, dw, n, compressed, subgroup_check, dout, (unsigned char*)dst, hc.l.st);
  if (rc) return rc;
  if (hipMemcpyAsync(status, dst, n, hipMemcpyDeviceToHost, hc.l.st) != hipSuccess)
    return mlhip_rt::fail(MLHIP_EHIP, "hipMemcpy D2H failed");
  return hc.down(out, dout, n * psz);
}

int to_bytes_host(int curve, int group, const void* affine, size_t n, int compressed, void* wire) {
  const CurveOps* ops = curve_ops(curve);
  if (!ops) return mlhip_rt::fail(MLHIP_EINVAL, "unknown curve id");
  if (n == 0) return 0;
  if (!affine || !wire) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  int rc = ensure_device();
  if (rc) return rc;
  const size_t psz = ops->point_size(group);
  const size_t wlen = compressed ? psz / 2 : psz;
  HostCall hc;
  hc.reserve(n * (psz + wlen));
  void* dp = hc.up(affine, n * psz);
  void* dw = hc.dev(n * wlen);
  if (hc.rc) return hc.rc;
  rc = to_bytes_device(curve, group, dp, n, compressed, dw, hc.l.st);
  if (rc) return rc;
  return hc.down(wire, dw, n * wlen);
}

}  // namespace

extern "C" {

int mlhip_g1_from_bytes_device(int curve, const void* d_wire, size_t n, int compressed, int subgroup_check, void* d_out,
                               unsigned char* d_status, void* stream) {
  return from_bytes_device(curve, 1, d_wire, n, compressed, subgroup_check, d_out, d_status, stream);
}
int mlhip_g2_from_bytes_device(int curve, const void* d_wire, size_t n, int compressed, int subgroup_check, void* d_out,
                               unsigned char* d_status, void* stream) {
  return from_bytes_device(curve, 2, d_wire, n, compressed, subgroup_check, d_out, d_status, stream);
}
int mlhip_g1_to_bytes_device(int curve, const void* d_affine, size_t n, int compressed, void* d_wire, void* stream) {
  return to_bytes_device(curve, 1, d_affine, n, compressed, d_wire, stream);
}
int mlhip_g2_to_bytes_device(int curve, const void* d_affine, size_t n, int compressed, void* d_wire, void* stream) {
  return to_bytes_device(curve, 2, d_affine, n, compressed, d_wire, stream);
}
int mlhip_g1_from_bytes(int curve, const void* wire, size_t n, int compressed, int subgroup_check, void* out, unsigned char* status) {
  return from_bytes_host(curve, 1, wire, n, compressed, subgroup_check, out, status);
}
int mlhip_g2_from_bytes(int curve, const void* wire, size_t n, int compressed, int subgroup_check, void* out, unsigned char* status) {
  return from_bytes_host(curve, 2, wire, n, compressed, subgroup_check, out, status);
}
int mlhip_g1_to_bytes(int curve, const void* affine, size_t n, int compressed, void* wire) {
  return to_bytes_host(curve, 1, affine, n, compressed, wire);
}
int mlhip_g2_to_bytes(int curve, const void* affine, size_t n, int compressed, void* wire) {
  return to_bytes_host(curve, 2, affine, n, compressed, wire);
}

}  // extern "C"

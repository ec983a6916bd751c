// The wire codec of one curve (mlhip_internal.h: MLHIP_TU_OPS): tu_codec_<curve>.hip defines MLHIP_TU_CURVE and includes this.
#include "codec_kernels.h"
using namespace mlhip;
int MLHIP_TU_FN(wire_codec)(int group, int encode, const void* d_in, size_t n, int compressed, int subgroup, void* d_out,
                             void* d_status, hipStream_t st) {
  if (group == 2) return wire_codec_device<G2Wire<MLHIP_TU_CURVE>>(encode, d_in, n, compressed, subgroup, d_out, d_status, st);
  return wire_codec_device<G1Wire<MLHIP_TU_CURVE>>(encode, d_in, n, compressed, subgroup, d_out, d_status, st);
}

// MSM kernels instantiated for Bls377 (G1 over Fp, G2 over Fp2).
#define MLHIP_TU_CURVE Bls377
#include "tu_msm.inc"

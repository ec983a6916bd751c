// MSM kernels instantiated for Bn254 (G1 over Fp, G2 over Fp2).
#define MLHIP_TU_CURVE Bn254
#include "tu_msm.inc"

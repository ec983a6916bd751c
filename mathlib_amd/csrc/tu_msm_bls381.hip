// MSM kernels instantiated for Bls381 (G1 over Fp, G2 over Fp2).
#define MLHIP_TU_CURVE Bls381
#include "tu_msm.inc"

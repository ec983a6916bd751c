// Pairing kernels instantiated for Bn254.
#define MLHIP_TU_CURVE Bn254
#include "tu_pairing.inc"

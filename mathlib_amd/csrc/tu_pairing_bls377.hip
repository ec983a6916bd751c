// Pairing kernels instantiated for Bls377.
#define MLHIP_TU_CURVE Bls377
#include "tu_pairing.inc"

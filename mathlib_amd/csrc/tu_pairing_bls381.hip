// Pairing kernels instantiated for Bls381.
#define MLHIP_TU_CURVE Bls381
#include "tu_pairing.inc"

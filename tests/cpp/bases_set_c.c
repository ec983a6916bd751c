/* tests/cpp/bases_set_c.c -- include/mlhip_bases_set.h compiled as C: the two inline functions and the two flags behind plain C
 * symbols that tests/cpp/bases_set_test.cpp calls. */
#include "mlhip_bases_set.h"

int c_bases_set_create(mlhip_bases* const* members, size_t k, mlhip_bases** set) { return mlhip_bases_set_create(members, k, set); }
int c_bases_set_route(mlhip_bases* set, int* info, int cap) { return mlhip_bases_set_route(set, info, cap); }
int c_group_set(void) { return MLHIP_GROUP_SET; }
int c_msm_set_route(void) { return MLHIP_MSM_SET_ROUTE; }

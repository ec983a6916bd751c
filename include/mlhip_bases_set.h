/* mlhip_bases_set.h -- sets of resident-bases handles as inline functions over the entry points of mlhip.h (see its section
 * "sets of handles"): a set is created through the `group` argument of mlhip_bases_create (MLHIP_GROUP_SET) and asked for its
 * route through the `scalars_mont` argument of mlhip_bases_msm (MLHIP_MSM_SET_ROUTE), so the library's dynamic symbol table
 * stays what it was.  C, C++ and cgo. */
#ifndef MLHIP_BASES_SET_H
#define MLHIP_BASES_SET_H

#include "mlhip.h"

/* a SET of 1..4 single-device handles of one curve on one device, any mix of G1 and G2: a handle itself; the members are not
 * owned (mlhip_bases_destroy(set) frees the set only) */
static inline int mlhip_bases_set_create(mlhip_bases* const* members, size_t k, mlhip_bases** set) {
  return mlhip_bases_create(0, MLHIP_GROUP_SET, (const void*)members, k, 0, set);
}
/* how the set's last MSM ran: info[0] = members, info[1] = sort trains per tile (geometry classes),
   info[2] = host-to-device copies of the scalar vector (0 for device scalars), info[3] = 1 iff every member read tables;
   returns the number of entries written (<= cap), or MLHIP_EINVAL (a null pointer, a negative cap, not a set) */
static inline int mlhip_bases_set_route(mlhip_bases* set, int* info, int cap) {
  if (cap < 0) set = 0; /* (a null handle is the library's MLHIP_EINVAL) */
  return mlhip_bases_msm(set, 0, MLHIP_MSM_SET_ROUTE, (size_t)(cap < 0 ? 0 : cap), info);
}

#endif

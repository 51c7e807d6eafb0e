/* mgic_ptag.h -- tagging through the wrap of a periodic domain.
 *
 * libmgic_ptag.so: one gfx950 kernel over libmgic's C ABI.  It is
 * mgic_field_tag_lattice (include/mgic.h) with the periodic flags of the
 * field's grid taken into account.  In a periodic direction d of a level
 * whose domain has n_d cells
 *
 *   the clustering lattice spans the whole domain: lat_lo = dom_lo / c,
 *   lat_n = n_d / c (a domain that is not a multiple of c: MGIC_EBADARG);
 *   a tagged cell's grown range [i - grow, i + grow] is NOT clipped: each
 *   cell index is taken modulo n_d into the domain, so the range sets at
 *   most lat_n[d] lattice cells, and all of them when 2 grow + 1 >= n_d.
 *
 * A non-periodic direction is mgic_field_tag_lattice's: the grown range is
 * clipped to the domain, and the lattice is the bounding box of the level's
 * boxes (every rank's), grown and clipped.  The reference clips with the
 * domain Box in every direction (SetGrids.cpp:201-202); this departs from it
 * on purpose.
 *
 * All local boxes of the level are covered by ONE kernel launch per call.
 * It reaches the field through mgic_field_layout / mgic_field_box /
 * mgic_field_device_ptr and launches on the stream mgic_comm_get_stream
 * returns, so its work is ordered with libmgic's on the same communicator.
 * The library owns its device scratch (grown on demand, freed at unload).
 * Status codes as libmgic; the message of the last failure of the calling
 * thread is mgic_ptag_last_error().
 */
#ifndef MGIC_PTAG_H
#define MGIC_PTAG_H

#include "mgic.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGIC_PTAG_API __attribute__((visibility("default")))

MGIC_PTAG_API const char *mgic_ptag_last_error(void);

/* The two-call protocol of mgic_field_tag_lattice: lat_lo / lat_n are always
 * written; mask_host == NULL is the size query (no device is touched).
 * Otherwise mask_host receives lat_n[0]*lat_n[1]*lat_n[2] bytes (x fastest),
 * 1 where THIS rank's cells set a lattice cell; the call synchronises.  The
 * lattice is the same on every rank, so the masks of the ranks can be OR-ed. */
MGIC_PTAG_API int mgic_ptag_lattice(mgic_comm comm, mgic_field cond, double tag_val, int grow,
                                    int c, int lat_lo[3], int lat_n[3],
                                    unsigned char *mask_host);

/* This library's launch ledger (its own registry, not libmgic's): one
 * "name<TAB>count" line per kernel, sorted by name; every kernel is listed,
 * at 0 until it is launched. */
MGIC_PTAG_API int mgic_ptag_launch_ledger_dump(const char *path);
MGIC_PTAG_API int mgic_ptag_launch_ledger_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* MGIC_PTAG_H */

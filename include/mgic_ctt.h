/* mgic_ctt.h -- the conformal transverse-traceless step of the momentum
 * constraint.
 *
 * libmgic_ctt.so: four fp64 gfx950 kernels over libmgic's C ABI.  It reaches
 * the fields through mgic_field_device_ptr / mgic_field_layout /
 * mgic_field_box and launches on the stream mgic_comm_get_stream returns, so
 * its work is ordered with libmgic's on the same communicator.  Every field
 * of one call must share one layout (domain, dx, boxes, owners).
 *
 * With the total tensor Abar_ij = Abar^BY_ij + LW_ij,
 *
 *   LW_ij = D_i W_j + D_j W_i - (2/3) delta_ij D_k W_k,   W_i = V_i + D_i U,
 *   D_d f = 0.5 / dx * (f(+e_d) - f(-e_d)),
 *
 * where V_i and U are solved for with libmgic's own solvers (Lap V_i = S_i
 * from mgic_field_momentum_source, Lap U = the field of mgic_ctt_div_rhs).
 * Operands are read with ghost layer 1 as stored; outputs are written on the
 * valid cells.  Status codes as libmgic; the message of the last failure of
 * the calling thread is mgic_ctt_last_error().
 */
#ifndef MGIC_CTT_H
#define MGIC_CTT_H

#include "mgic.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGIC_CTT_API __attribute__((visibility("default")))

MGIC_CTT_API const char *mgic_ctt_last_error(void);

/* out = -0.25 * (D_x V_x + D_y V_y + D_z V_z): the right-hand side of U */
MGIC_CTT_API int mgic_ctt_div_rhs(mgic_comm c, const mgic_field v[3], mgic_field out);
/* W_i = V_i + D_i U, three outputs in one pass */
MGIC_CTT_API int mgic_ctt_w(mgic_comm c, const mgic_field v[3], mgic_field u,
                            const mgic_field w[3]);
/* the six LW_ij in the order 11, 12, 13, 22, 23, 33 from W with its ghost layer */
MGIC_CTT_API int mgic_ctt_lw(mgic_comm c, const mgic_field w[3], const mgic_field lw[6]);
/* ghost layer 1 of f across every domain face that is not periodic, by linear
 * extrapolation from the two cells inside: g = 2 f(face cell) - f(next cell
 * in).  Faces only (no edge or corner ghost); nothing else is written.  Every
 * box with a domain face needs two cells along that face's normal. */
MGIC_CTT_API int mgic_ctt_extrap(mgic_comm c, mgic_field f);

/* This library's launch ledger (its own registry, not libmgic's): one
 * "name<TAB>count" line per kernel, sorted by name; every kernel is listed,
 * at 0 until it is launched. */
MGIC_CTT_API int mgic_ctt_launch_ledger_dump(const char *path);
MGIC_CTT_API int mgic_ctt_launch_ledger_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* MGIC_CTT_H */

/* mgic_sample.h -- a field of an AMR hierarchy interpolated at points
 * (DESIGN.md 3o): puncture masses, line-outs.
 *
 * libmgic_sample.so: one fp64 gfx950 kernel over libmgic's C ABI.  fields[l] is
 * one field per AMR level, coarsest first, refinement ratio 2.  Level 0 has N_d
 * cells in direction d (domain low corner 0); level l has N_d 2^l cells, the
 * spacing dx_l its layout reports, and cell centres at
 * (iv + 0.5) dx_l - N_d dx_0 / 2: the coordinates of the puncture table and of
 * mgic_adm.h.  Only valid cells are read: no ghost cell of any field, so
 * nothing needs exchanging beforehand.
 *
 * The rule for one point x (all of it evaluated in the kernel, in fp64, built
 * with -ffp-contract=off; every expression is written as it is evaluated, left
 * to right):
 *
 * 1. A non-finite coordinate gives level_used = -1, order_used = 0, value =
 *    NaN.  Else, per direction, with half_d = N_d * dx_0 / 2.0 and
 *    len_d = N_d * dx_0:  r_d = x_d + half_d.  In a periodic direction
 *    r_d = r_d - floor(r_d / len_d) * len_d, and an r_d the rounding leaves
 *    outside [0, len_d) becomes 0.  In a direction that is not periodic an r_d
 *    outside [0, len_d) gives -1, 0, NaN as above.
 * 2. On level l, q_d = r_d / dx_l and c_d = min(floor(q_d), N_d 2^l - 1) (an r_d
 *    just below len_d can round to q_d = N_d 2^l: the last cell).  The point's level is
 *    the finest l whose boxes hold the cell c and on which c is not covered:
 *    c lies in no box of level l + 1 coarsened by 2 (lo >> 1 .. hi >> 1).  No
 *    such level: -1, 0, NaN.
 * 3. A cell of level l is available when, its index wrapped into
 *    0 .. N_d 2^l - 1 in every periodic direction, it lies in a box of level l
 *    and is not covered by level l + 1.  Covered cells are never read.
 * 4. With s_d = q_d - 0.5, i_d = floor(s_d), t_d = s_d - i_d, the candidates
 *    are tried from the requested order down; the first whose cells are all
 *    available is used, and order_used reports it:
 *      order 4: cells i_d - 1 .. i_d + 2, weights (cubic Lagrange on the nodes
 *               -1, 0, 1, 2), with tm1 = t - 1.0, tm2 = t - 2.0, tp1 = t + 1.0:
 *                 w[0] = -t * tm1 * tm2 / 6.0
 *                 w[1] = tp1 * tm1 * tm2 / 2.0
 *                 w[2] = -tp1 * t * tm2 / 2.0
 *                 w[3] = tp1 * t * tm1 / 6.0
 *      order 2: cells i_d, i_d + 1, weights w[0] = 1.0 - t, w[1] = t
 *      order 1: the cell c itself, value = u[c]
 * 5. value = sum_k wz[k] * (sum_j wy[j] * (sum_i wx[i] * u_ijk)): every sum
 *    starts from its first product and adds the others in increasing index
 *    order, row = wx[0] * u_0jk; row = row + wx[1] * u_1jk; ...; plane =
 *    wy[0] * row_0; ...; value = wz[0] * plane_0; ...
 *
 * Nothing but + - * / and floor is involved, so a restatement that follows
 * this order agrees bit for bit (tests/sample_ref.py).
 *
 * mgic_sample_points launches once on the stream mgic_comm_get_stream returns
 * and returns after it has drained.  It is refused with MGIC_EBADARG, before
 * any launch, for: a NULL pointer; nlev outside 1 .. MGIC_SAMPLE_MAX_LEVELS;
 * npts outside 1 .. MGIC_SAMPLE_MAX_POINTS; an order other than 1, 2 or 4; a
 * level-0 domain whose low corner is not 0; a level whose domain is not the
 * previous one refined by 2, or whose periodicity differs; a box that is not
 * local.  Status codes as libmgic; the message of the last failure of the
 * calling thread is mgic_sample_last_error().
 */
#ifndef MGIC_SAMPLE_H
#define MGIC_SAMPLE_H

#include "mgic.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGIC_SAMPLE_API __attribute__((visibility("default")))

#define MGIC_SAMPLE_MAX_LEVELS 8
#define MGIC_SAMPLE_MAX_POINTS (1 << 20)

MGIC_SAMPLE_API const char *mgic_sample_last_error(void);

/* xyz: host, npts x 3; values, level_used, order_used: host, npts each */
MGIC_SAMPLE_API int mgic_sample_points(mgic_comm c, int nlev, const mgic_field *fields, int npts,
                                       const double *xyz, int order, double *values,
                                       int *level_used, int *order_used);

/* This library's launch ledger (its own registry, not libmgic's): one
 * "name<TAB>count" line per kernel, sorted by name; every kernel is listed,
 * at 0 until it is launched. */
MGIC_SAMPLE_API int mgic_sample_launch_ledger_dump(const char *path);
MGIC_SAMPLE_API int mgic_sample_launch_ledger_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* MGIC_SAMPLE_H */

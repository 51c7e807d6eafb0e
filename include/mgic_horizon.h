/* mgic_horizon.h -- the expansion of a surface at points of an AMR hierarchy
 * (DESIGN.md 3p): apparent horizons of conformally flat data.
 *
 * libmgic_horizon.so: one fp64 gfx950 kernel over libmgic's C ABI.  psi[l] is
 * the regular part of the conformal factor, one field per AMR level, coarsest
 * first, refinement ratio 2; lw is NULL or the six stored LW_ij (11, 12, 13,
 * 22, 23, 33) of every level, lw[6 l + k], on psi[l]'s layout.  The geometry,
 * the coordinates and the rule that only valid cells are read are those of
 * mgic_sample.h; the puncture table (npunct rows m, x, y, z, Px, Py, Pz, Jx,
 * Jy, Jz) is that of the *_punct entry points of mgic.h and of mgic_adm.h.
 *
 * For gamma_ij = psi^4 delta_ij, K_ij = psi^-2 Abar_ij, K = 0 and the unit
 * normal s^i = psi^-2 n^i of a surface with flat unit normal n and flat
 * divergence divn = d_i n^i,
 *
 *     Theta = D_i s^i + K_ij s^i s^j - K
 *           = divn / psi^2 + 4 n . grad psi / psi^3 + Abar_ij n^i n^j / psi^6
 *
 * with psi = psi_reg + sum m / r and Abar_ij = A^BY_ij [+ LW_ij].  The caller
 * supplies the point x, n and divn; the kernel supplies the rest.
 *
 * The rule for one point x (all of it evaluated in the kernel, in fp64, built
 * with -ffp-contract=off; every expression is written as it is evaluated, left
 * to right):
 *
 * 1. - 3. are steps 1 to 3 of mgic_sample.h, for directions that are not
 *    periodic: r_d = x_d + half_d; a non-finite coordinate or an r_d outside
 *    [0, len_d) gives level_used = -1, order_used = 0 and six NaN; on level l
 *    q_d = r_d / dx_l, c_d = min(floor(q_d), N_d 2^l - 1); the point's level is
 *    the finest whose boxes hold c and on which c is not covered (no such
 *    level: -1, 0, NaN); a cell is available when it lies in a box of level l
 *    and is not covered by level l + 1.  No ghost and no covered cell is read.
 * 4. With s_d = q_d - 0.5, i_d = floor(s_d), t_d = s_d - i_d, the candidates
 *    are order 4 (cells i_d - 1 .. i_d + 2), then order 2 (cells i_d, i_d + 1);
 *    the first whose cells are all available is used and order_used reports
 *    it.  Neither: order_used = 0, all six outputs NaN, level_used still the
 *    point's level.  The value weights w are those of mgic_sample.h.  The
 *    derivative weights at order 4, with tm1 = t - 1.0, tm2 = t - 2.0,
 *    tp1 = t + 1.0, a = tm1 * tm2, b = t * tm2, c = t * tm1, d = tp1 * tm2,
 *    e = tp1 * tm1, f = tp1 * t:
 *        dw[0] = -((a + b) + c) / 6.0
 *        dw[1] = ((a + d) + e) / 2.0
 *        dw[2] = -((b + d) + f) / 2.0
 *        dw[3] = ((c + e) + f) / 6.0
 *    and at order 2: dw[0] = -1.0, dw[1] = 1.0.
 * 5. One walk over the stencil, u = psi's cells:
 *        rows:    rv_jk = sum_i wx[i] * u_ijk      rd_jk = sum_i dwx[i] * u_ijk
 *        planes:  pv_k = sum_j wy[j] * rv_jk       px_k = sum_j wy[j] * rd_jk
 *                 py_k = sum_j dwy[j] * rv_jk
 *        totals:  v  = sum_k wz[k] * pv_k          gx = sum_k wz[k] * px_k
 *                 gy = sum_k wz[k] * py_k          gz = sum_k dwz[k] * pv_k
 *    Every sum starts from its first product and adds the others in increasing
 *    index order.  Then g_d = g_d / dx_l.  With lw, each LW_ij is interpolated
 *    as v is (value weights only), on the same cells.
 * 6. The analytic parts at x.  For one puncture (row m, x_n, P, J):
 *        l = x - x_n;  r = sqrt(l0 * l0 + l1 * l1 + l2 * l2);  n = l / r
 *        nP = n0 * P0 + n1 * P1 + n2 * P2;  c = n x J
 *             (c0 = n1 * J2 - n2 * J1, c1 = n2 * J0 - n0 * J2, c2 = n0 * J1 - n1 * J0)
 *        fP = 1.5 / r / r;  fJ = 3.0 / r / r / r;  r3 = r * r * r
 *        psi_n = m / r;  d_n,d = m * l_d / r3
 *        A_n,ij = fP * (n_i * P_j + n_j * P_i + (n_i * n_j - delta_ij) * nP)
 *                 - fJ * (c_i * n_j + c_j * n_i)          for ij = 11 12 13 22 23 33
 *    The table is taken in pairs (an odd count completed by m = P = J = 0 at
 *    the last puncture's position): a pair's term is first + second, the first
 *    pair's term starts each sum and the others are added in pair order.
 * 7. psi   = v + psi_bh
 *    dpsi_d = g_d - d_d
 *    A_ij  = A^BY_ij [ + LW_ij ]
 *    A_nn  = ((n0 * n0 * A11 + n1 * n1 * A22) + n2 * n2 * A33)
 *            + 2.0 * ((n0 * n1 * A12 + n0 * n2 * A13) + n1 * n2 * A23)
 *    p2 = psi * psi;  p3 = p2 * psi;  p6 = p3 * p3
 *    dn = (n0 * dpsi_0 + n1 * dpsi_1) + n2 * dpsi_2
 *    theta = (divn / p2 + 4.0 * dn / p3) + A_nn / p6
 *    (here n is the caller's normal).  A point on a puncture gives non-finite
 *    outputs; it is not refused.
 *
 * out holds MGIC_HORIZON_TERMS doubles per point: theta, psi, dpsi_x, dpsi_y,
 * dpsi_z, A_nn.  Steps 1 to 5 involve nothing but + - * / and floor, so a
 * restatement that follows this order agrees bit for bit in v, g_d and the
 * LW_ij (tests/horizon_ref.py); step 6 has a sqrt and chains of divisions.
 *
 * mgic_horizon_expansion launches once on the stream mgic_comm_get_stream
 * returns, with one device allocation, and returns after the stream has
 * drained.  It is refused with MGIC_EBADARG, before any launch, for: a NULL
 * pointer (lw itself may be NULL; none of its 6 nlev handles may be); nlev
 * outside 1 .. MGIC_HORIZON_MAX_LEVELS; npts outside 1 ..
 * MGIC_HORIZON_MAX_POINTS; a puncture count outside 1 .. MGIC_MAX_PUNCTURES or
 * a table entry that is not finite; a periodic direction; a level-0 domain
 * whose low corner is not 0; a level whose domain is not the previous one
 * refined by 2; a box that is not local; an lw field whose layout is not
 * psi[l]'s.  Status codes as libmgic; the message of the last failure of the
 * calling thread is mgic_horizon_last_error().
 */
#ifndef MGIC_HORIZON_H
#define MGIC_HORIZON_H

#include "mgic.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGIC_HORIZON_API __attribute__((visibility("default")))

#define MGIC_HORIZON_MAX_LEVELS 8
#define MGIC_HORIZON_MAX_POINTS (1 << 20)
#define MGIC_HORIZON_TERMS 6

MGIC_HORIZON_API const char *mgic_horizon_last_error(void);

/* xyz, normal: host, npts x 3; divn: host, npts; out: host, npts x
 * MGIC_HORIZON_TERMS; level_used, order_used: host, npts each */
MGIC_HORIZON_API int mgic_horizon_expansion(mgic_comm c, int nlev, const mgic_field *psi,
                                            const mgic_field *lw, int npunct, const double *table,
                                            int npts, const double *xyz, const double *normal,
                                            const double *divn, double *out, int *level_used,
                                            int *order_used);

/* This library's launch ledger (its own registry, not libmgic's): one
 * "name<TAB>count" line per kernel, sorted by name; every kernel is listed,
 * at 0 until it is launched. */
MGIC_HORIZON_API int mgic_horizon_launch_ledger_dump(const char *path);
MGIC_HORIZON_API int mgic_horizon_launch_ledger_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* MGIC_HORIZON_H */

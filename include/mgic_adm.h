/* mgic_adm.h -- ADM mass, momentum and spin of the solved data as surface
 * integrals over cubes of level 0.
 *
 * libmgic_adm.so: fp64 gfx950 kernels over libmgic's C ABI.  Level 0 has N_d
 * cells in direction d (every N_d even, domain low corner 0), spacing dx, and
 * the coordinates of its cell centres are (iv + 0.5) dx - N_d dx / 2.  A
 * surface is the cell-aligned cube of half-width n cells about the domain
 * centre, cells [N_d/2 - n, N_d/2 + n) in every direction: 6 sides, side =
 * 2 d + (s > 0) for the outward normal s e_d, each (2 n)^2 cell faces (b, a),
 * a fastest, a and b along the two directions other than d in increasing
 * order.  For a face with centre x_f, inner cell `in` and outer cell `out`
 * (geometric units, no factor G):
 *
 *   g    = (psi[out] - psi[in]) / dx + s * d_d psi_bh(x_f)
 *          d_d psi_bh = - sum_n m_n (x_f - x_n)_d / r_n^3
 *   A_kd = A^BY_kd(x_f)  [ + 0.5 * (LW_kd[in] + LW_kd[out]) ]
 *   mass = -(1 / (2 pi)) * g * dx^2
 *   P_i  =  (1 / (8 pi)) * s * A_id * dx^2
 *   J_i  =  (1 / (8 pi)) * s * sum_jk eps_ijk x_f,j A_kd * dx^2
 *
 * A^BY is the Bowen-York tensor of the puncture table (the *_punct entry
 * points' table and pair order) at the real-valued face centre.  Only valid
 * cells are read: no ghost cell of any field, so nothing needs exchanging
 * beforehand.  The 7 sums of a surface are formed in a fixed order (no
 * floating-point atomics) over faces indexed per surface, so they are
 * repeatable bit for bit and do not depend on the box layout of level 0.
 *
 * Both entry points launch on the stream mgic_comm_get_stream returns and
 * return after it has drained.  They are refused with MGIC_EBADARG, before
 * any launch, for: a NULL pointer; nsurf outside 1 .. MGIC_ADM_MAX_SURFACES; a
 * half-width < 1 or > min_d N_d / 2 - 1 (the outer cells stay inside the
 * domain); an odd N_d or a domain whose low corner is not 0; a periodic
 * direction; a box that is not local, or boxes that do not tile the domain
 * (psi is the level-0 field); a bad table (count outside 1 ..
 * MGIC_MAX_PUNCTURES, a non-finite entry); lw fields on another layout.
 * Status codes as libmgic; the message of the last failure of the calling
 * thread is mgic_adm_last_error().
 */
#ifndef MGIC_ADM_H
#define MGIC_ADM_H

#include "mgic.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGIC_ADM_API __attribute__((visibility("default")))

#define MGIC_ADM_MAX_SURFACES 8
#define MGIC_ADM_TERMS 7 /* mass, P1, P2, P3, J1, J2, J3 */

MGIC_ADM_API const char *mgic_adm_last_error(void);

/* *count = the number of doubles mgic_adm_surface_terms writes:
 * sum over the surfaces of 6 * 7 * (2 n)^2.  Only nsurf and the half-widths
 * being >= 1 are checked. */
MGIC_ADM_API int mgic_adm_surface_count(int nsurf, const int *half_widths, long long *count);

/* the 7 terms of every face, laid out (surface, side, 7, b, a), the surfaces
 * concatenated; lw: the six stored LW_ij (11, 12, 13, 22, 23, 33) on psi's
 * layout, or NULL: the Bowen-York tensor alone.  out: host memory, or device
 * memory with out_on_device != 0. */
MGIC_ADM_API int mgic_adm_surface_terms(mgic_comm c, mgic_field psi, int nsurf,
                                        const int *half_widths, int npunct, const double *table,
                                        const mgic_field *lw, double *out, int out_on_device);

/* out[s * 7 + c] (host): the sum of term c over the faces of surface s.
 * Waves of 64 consecutive faces are added by a butterfly (32, 16, .. 1), 4
 * waves to a block of 256 in order, and a surface's blocks in order; lanes
 * past the last face carry +0.0. */
MGIC_ADM_API int mgic_adm_charges(mgic_comm c, mgic_field psi, int nsurf, const int *half_widths,
                                  int npunct, const double *table, const mgic_field *lw,
                                  double *out);

/* This library's launch ledger (its own registry, not libmgic's): one
 * "name<TAB>count" line per kernel, sorted by name; every kernel is listed,
 * at 0 until it is launched. */
MGIC_ADM_API int mgic_adm_launch_ledger_dump(const char *path);
MGIC_ADM_API int mgic_adm_launch_ledger_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* MGIC_ADM_H */

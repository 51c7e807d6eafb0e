/* mgic_cttk.h -- the K(x) field of the CTTK method.
 *
 * libmgic_cttk.so: three fp64 gfx950 kernels over libmgic's C ABI.  In the
 * CTTK method (Aurrekoetxea, Clough & Lim) the conformal factor is chosen and
 * the trace K of the extrinsic curvature varies in space: the Hamiltonian
 * constraint is then algebraic, cell by cell, and the momentum constraint
 * gains the source (2/3) d_i K.  What is here: K from the integrand of
 * mgic_field_nl_integrand_ctt, its gradient added to the momentum source
 * S_i of mgic_field_momentum_source, and the correction of the five
 * constraint fields mgic_field_constraints_ctt wrote at constant_K = 0.
 *
 * All fields of one call share one layout (domain, dx, boxes, owners,
 * strides).  Every call is ONE launch whatever the number of local boxes (a
 * box table in device memory); a level without a local box launches nothing.
 * The library reaches the fields through mgic_field_device_ptr /
 * mgic_field_layout / mgic_field_box and launches on the stream
 * mgic_comm_get_stream returns, so its work is ordered with libmgic's on the
 * same communicator; every call returns with its launch complete.  No ghost
 * cell is written and no LDS is used.  Built with -ffp-contract=off: every
 * expression below is evaluated as written, in that order, in double, so a
 * numpy restatement matches bit for bit (tests/cttk_ref.py).
 *
 * A NULL pointer, fields of different layouts, a field passed twice where
 * the fields must be distinct and a layout with a box that is not local to
 * the calling rank are MGIC_EBADARG before anything is launched (the ledger
 * is unchanged).  Status codes as libmgic; the message of the last failure
 * of the calling thread is mgic_cttk_last_error().
 */
#ifndef MGIC_CTTK_H
#define MGIC_CTTK_H

#include "mgic.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGIC_CTTK_API __attribute__((visibility("default")))

MGIC_CTTK_API const char *mgic_cttk_last_error(void);

/* k_cttk_K.  Per valid cell, v = integrand[cell]:
 *
 *   v >= 0.0:     K[cell] = -sqrt(v)       (IEEE square root; v = 0: -0.0)
 *   otherwise:    K[cell] = 0.0, and the cell is counted
 *
 * "otherwise" is a negative or a NaN value.  *bad_cells is the number of
 * counted cells of the local boxes (an integer atomic on the device: the
 * count does not depend on the order).  integrand and K are distinct. */
MGIC_CTTK_API int mgic_cttk_K(mgic_comm c, mgic_field integrand, mgic_field K,
                              long long *bad_cells);

/* k_cttk_source.  Per valid cell, with h = 0.5 / dx and K read with its
 * ghost layer 1 as stored:
 *
 *   p   = psi[cell];  p2 = p * p;  p6 = (p2 * p2) * p2
 *   c   = (2.0 / 3.0) * p6
 *   D_i = h * (K[cell + e_i] - K[cell - e_i])
 *   S_i[cell] = S_i[cell] + c * D_i                       i = 0, 1, 2
 *
 * in one pass.  psi and K may be any fields but S_i; the S_i are distinct. */
MGIC_CTTK_API int mgic_cttk_source(mgic_comm c, mgic_field psi, mgic_field K,
                                   const mgic_field *S);

/* k_cttk_constraints.  Per valid cell, with h and D_i as above:
 *
 *   t = (2.0 / 3.0) * (K[cell] * K[cell])
 *   ham[cell]     = ham[cell] + t
 *   ham_abs[cell] = ham_abs[cell] + fabs(t)
 *   mom_i[cell]   = mom_i[cell] - (2.0 / 3.0) * D_i      i = 0, 1, 2
 *
 * in one pass.  All six fields are distinct. */
MGIC_CTTK_API int mgic_cttk_constraints(mgic_comm c, mgic_field K, mgic_field ham,
                                        const mgic_field *mom, mgic_field ham_abs);

/* This library's launch ledger (its own registry, not libmgic's): one
 * "name<TAB>count" line per kernel, sorted by name; every kernel is listed,
 * at 0 until it is launched. */
MGIC_CTTK_API int mgic_cttk_launch_ledger_dump(const char *path);
MGIC_CTTK_API int mgic_cttk_launch_ledger_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* MGIC_CTTK_H */

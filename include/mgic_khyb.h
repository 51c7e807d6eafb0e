/* mgic_khyb.h -- K(x) from the matter's energy: the hybrid CTTK choice for
 * decks with holes.
 *
 * libmgic_khyb.so: one fp64 gfx950 kernel over libmgic's C ABI.  In the hybrid
 * CTTK method (Aurrekoetxea, Clough & Lim) the trace K of the extrinsic
 * curvature is chosen cell by cell so that the matter's energy drops out of
 * the Hamiltonian constraint,
 *
 *   (2/3) K^2 = 16 pi G rho,   rho = Pi^2 / 2 + V(phi_0),
 *
 * the conformal factor is solved for as without matter, and the momentum
 * constraint gains the source (2/3) psi^6 d_i K (k_cttk_source of
 * libmgic_cttk.so).  What is here: K from the stored phi_0 and Pi_0.
 *
 * All fields of the call share one layout (domain, dx, boxes, owners,
 * strides).  The call is ONE launch whatever the number of local boxes (a box
 * table in device memory); a level without a local box launches nothing.  The
 * library reaches the fields through mgic_field_device_ptr /
 * mgic_field_layout / mgic_field_box and launches on the stream
 * mgic_comm_get_stream returns, so its work is ordered with libmgic's on the
 * same communicator; the call returns with its launch complete.  No ghost
 * cell is read or written and no LDS is used.  Built with -ffp-contract=off:
 * every expression below is evaluated as written, left to right, in double,
 * so a numpy restatement matches bit for bit (tests/khyb_ref.py).
 *
 * A NULL pointer (but pi), fields of different layouts, K passed as phi or pi
 * and a layout with a box that is not local to the calling rank are
 * MGIC_EBADARG before anything is launched (the ledger is unchanged).  Status
 * codes as libmgic; the message of the last failure of the calling thread is
 * mgic_khyb_last_error().
 */
#ifndef MGIC_KHYB_H
#define MGIC_KHYB_H

#include "mgic.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGIC_KHYB_API __attribute__((visibility("default")))

MGIC_KHYB_API const char *mgic_khyb_last_error(void);

/* k_khyb_K.  pot = {V0, mass, lambda}.  Per valid cell:
 *
 *   p = phi[cell];  q = pi ? pi[cell] : 0.0
 *   V    = V0 + 0.5 * mass * mass * p * p + 0.25 * lambda * p * p * p * p
 *   rho  = 0.5 * q * q + V
 *   m16  = 16.0 * M_PI * G * rho
 *   v    = 1.5 * m16
 *   v >= 0.0:     K[cell] = -sqrt(v)       (IEEE square root; v = 0: -0.0)
 *   otherwise:    K[cell] = 0.0, and the cell is counted
 *
 * V, rho and m16 are the expressions of libmgic's matter kernels
 * (set_m_value at K = 0 is -m16).  "otherwise" is a negative or a NaN value.
 * *bad_cells is the number of counted cells of the local boxes (an integer
 * atomic on the device: the count does not depend on the order).  pi may be
 * NULL (Pi = 0); K is neither phi nor pi. */
MGIC_KHYB_API int mgic_khyb_K(mgic_comm c, mgic_field phi, mgic_field pi, const double *pot,
                              double G, mgic_field K, long long *bad_cells);

/* This library's launch ledger (its own registry, not libmgic's): one
 * "name<TAB>count" line per kernel, sorted by name; every kernel is listed,
 * at 0 until it is launched. */
MGIC_KHYB_API int mgic_khyb_launch_ledger_dump(const char *path);
MGIC_KHYB_API int mgic_khyb_launch_ledger_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* MGIC_KHYB_H */

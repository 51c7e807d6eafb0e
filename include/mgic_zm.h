/* mgic_zm.h -- the zero mode of a periodic level.
 *
 * libmgic_zm.so: one fp64 gfx950 kernel over libmgic's C ABI.  On a periodic
 * domain the operator -beta Lap of the momentum solve (alpha aCoef = 0) is
 * singular: constants are its null space, and a right-hand side is in its
 * range only when it sums to zero.  The sums are libmgic's own
 * (mgic_op_dot with a field of ones); what is here subtracts the mean,
 *
 *   f_n[cell] = f_n[cell] - c_n     on the valid cells of every local box,
 *
 * for n fields that share one layout (domain, dx, boxes, owners).  It reaches
 * the fields through mgic_field_device_ptr / mgic_field_layout /
 * mgic_field_box and launches on the stream mgic_comm_get_stream returns, so
 * its work is ordered with libmgic's on the same communicator.  No ghost
 * cell is written.  Status codes as libmgic; the message of the last failure
 * of the calling thread is mgic_zm_last_error().
 */
#ifndef MGIC_ZM_H
#define MGIC_ZM_H

#include "mgic.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGIC_ZM_API __attribute__((visibility("default")))

MGIC_ZM_API const char *mgic_zm_last_error(void);

/* fields[i] -= consts[i] on the valid cells, i < n; n is 1 or 3 (one pass
 * over the level for all n).  The fields are distinct and share a layout. */
MGIC_ZM_API int mgic_zm_shift(mgic_comm c, int n, const mgic_field *fields, const double *consts);

/* This library's launch ledger (its own registry, not libmgic's): one
 * "name<TAB>count" line per kernel, sorted by name; every kernel is listed,
 * at 0 until it is launched. */
MGIC_ZM_API int mgic_zm_launch_ledger_dump(const char *path);
MGIC_ZM_API int mgic_zm_launch_ledger_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* MGIC_ZM_H */

/* mgic_reflux.h -- the reflux term at coarse-fine faces.
 *
 * libmgic_reflux.so: one fp64 gfx950 kernel (two instantiations) that makes
 * libmgic's composite AMR operator conservative.  For an uncovered cell i of
 * level l whose neighbour n across a face is covered by level l + 1, the
 * coarse stencil's gradient through that face is replaced by the average of
 * the four fine gradients behind it:
 *
 *   G_c   = (phi_c[n] - phi_c[i]) / dx_c          (0 with no coarse field)
 *   g_ab  = (phi_f[in-cell] - phi_f[ghost]) / dx_f
 *   <G_f> = 0.25 * ((g00 + g01) + (g10 + g11))
 *   term  = (<G_f> - G_c) / dx_c
 *   target[i] +/-= ((-beta) * b[i]) * (terms of i's faces, x-lo ... z-hi)
 *
 * The host side (which cells, which fine cells behind them) is libmgic's:
 * AMRSolver builds one table of interface cells and one of their faces per
 * pair of levels (csrc/amr.cpp, FluxRegister) and reaches the launcher here
 * through the function table below.  mgic_reflux_register() hands that table
 * to libmgic (mgic_amr_reflux_register); until it has been called, switching
 * reflux on (mgic_amr_set_reflux, mgic_amr_reflux) fails with MGIC_ESTATE.
 *
 * One launch per pair of levels and call, whatever the number of boxes: one
 * thread per interface cell, the fields reached through their device tables
 * of valid-lo pointers.  Each cell gathers its own terms in a fixed order; no
 * atomics.  Ownership: the tables index local boxes, so every box of the two
 * levels must be local to the calling rank; libmgic refuses reflux otherwise
 * (MGIC_EBADARG, "reflux: every box of levels l and l + 1 must be local").
 */
#ifndef MGIC_REFLUX_H
#define MGIC_REFLUX_H

#include "mgic.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGIC_REFLUX_API __attribute__((visibility("default")))

MGIC_REFLUX_API const char *mgic_reflux_last_error(void);

/* hand this library's launcher to libmgic (idempotent) */
MGIC_REFLUX_API int mgic_reflux_register(void);

/* This library's launch ledger (its own registry, not libmgic's): one
 * "name<TAB>count" line per kernel, sorted by name; every kernel is listed,
 * at 0 until it is launched. */
MGIC_REFLUX_API int mgic_reflux_launch_ledger_dump(const char *path);
MGIC_REFLUX_API int mgic_reflux_launch_ledger_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* MGIC_REFLUX_H */

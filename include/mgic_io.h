/* mgic_io.h -- HDF5 output in the reference's layouts.
 *
 * libmgic_io.so: a host library over libmgic (device fields) and libhdf5
 * (serial, /opt/conda).  It replaces the two writers in Source/WriteOutput.H:
 *
 *   output_final_data  (WriteOutput.H:127-227): the GRChombo checkpoint,
 *     31 components of set_output_data (SetLevelData.cpp:343-396) per level;
 *   output_solver_data (WriteOutput.H:52-123): the per-NL-iteration file of
 *     WriteAMRHierarchyHDF5 with dpsi, rhs and the 8 multigrid_vars.
 *
 * Both write Chombo's AMR HDF5 layout, restated (Chombo's CH_HDF5 / AMRIO
 * are not in the reference tree, so the layout is parity unpinned):
 *   /Chombo_global           attrs SpaceDim, testReal
 *   /                        header attrs (num_levels, num_components,
 *                            component_<c>, ...)
 *   /level_<l>               attrs ref_ratio, dx, dt, time, prob_domain, ...
 *   /level_<l>/boxes         compound {lo_i,lo_j,lo_k,hi_i,hi_j,hi_k}, layout order
 *   /level_<l>/Processors    owner rank per box
 *   /level_<l>/data:offsets=0   long long, nbox + 1 (cumulative doubles)
 *   /level_<l>/data:datatype=0  double, per box: components in order, each
 *                               over the valid box, i fastest (outputGhost 0)
 *   /level_<l>/data_attributes  attrs comps, objectType, ghost, outputGhost
 *
 * Every rank calls the device entry points (collective over the fields'
 * communicator): rank 0 creates the file and the datasets, then each rank in
 * turn writes its own boxes' hyperslabs.  Status codes as libmgic.
 */
#ifndef MGIC_IO_H
#define MGIC_IO_H

#include "mgic.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGIC_IO_API __attribute__((visibility("default")))

MGIC_IO_API const char *mgic_io_last_error(void);

/* output_final_data (WriteOutput.H:127-227).  psi[l] is level l's
 * multigrid_vars psi (the level's grid, dx and domain come from it);
 * bh[13] as mgic_field_binary_bh with bh[12] = constant_K; max_level and
 * ref_ratio[l] as PoissonParameters.  filename NULL: "vcPoissonFinal.3d.hdf5". */
MGIC_IO_API int mgic_io_write_final_data(const char *filename, int nlevels, const mgic_field *psi,
                                         const double bh[13], int max_level,
                                         const int *ref_ratio);

/* output_solver_data (WriteOutput.H:52-123) for NL iteration iter (time =
 * iter, dt = 1).  filename NULL: "vcPoissonOut.3d_<iter>.hdf5". */
MGIC_IO_API int mgic_io_write_solver_data(const char *filename, int nlevels,
                                          const mgic_field *dpsi, const mgic_field *rhs,
                                          const mgic_field *psi, const double bh[13],
                                          const int *ref_ratio, int iter);

/* The two writers with phi_0 stored (mgic.h, "phi_0 as a stored field"):
 * phi[l] is level l's phi_0 field, on psi[l]'s layout.  The "phi" component of
 * the final data and the "phi_0" component of the solver data are copied from
 * it; every other component is as above. */
MGIC_IO_API int mgic_io_write_final_data_phi(const char *filename, int nlevels,
                                             const mgic_field *psi, const mgic_field *phi,
                                             const double bh[13], int max_level,
                                             const int *ref_ratio);
MGIC_IO_API int mgic_io_write_solver_data_phi(const char *filename, int nlevels,
                                              const mgic_field *dpsi, const mgic_field *rhs,
                                              const mgic_field *psi, const mgic_field *phi,
                                              const double bh[13], const int *ref_ratio, int iter);

/* The two writers with the holes taken from a puncture table (mgic.h,
 * "Bowen-York punctures as a table"): npunct punctures, 10 doubles each.  The
 * A_ij and chi components of the final data and the A_ij_0 components of the
 * solver data come from the table; bh's six hole entries are ignored.  phi:
 * one stored phi_0 field per level, or NULL for the analytic Gaussian. */
MGIC_IO_API int mgic_io_write_final_data_punct(const char *filename, int nlevels,
                                               const mgic_field *psi, const mgic_field *phi,
                                               const double bh[13], int npunct,
                                               const double *table, int max_level,
                                               const int *ref_ratio);
MGIC_IO_API int mgic_io_write_solver_data_punct(const char *filename, int nlevels,
                                                const mgic_field *dpsi, const mgic_field *rhs,
                                                const mgic_field *psi, const mgic_field *phi,
                                                const double bh[13], int npunct,
                                                const double *table, const int *ref_ratio,
                                                int iter);

/* The final-data writer with the stored Pi_0 (mgic.h, "Matter"): pi[l] is
 * level l's Pi_0 field on psi[l]'s layout, copied as given into the "Pi"
 * component (26); pi NULL: Pi = 0.  pot[3] = V0, mass, lambda is checked and
 * otherwise unused (no written component depends on it).  Everything else as
 * mgic_io_write_final_data_punct, with the table nullable too (NULL with
 * npunct = 0: the two holes of bh).  A non-finite pot entry and a pi[l] of
 * another layout are MGIC_EBADARG before the file is created.  The solver
 * data (the reference's multigrid_vars) has no Pi component and no _matter
 * form. */
MGIC_IO_API int mgic_io_write_final_data_matter(const char *filename, int nlevels,
                                                const mgic_field *psi, const mgic_field *phi,
                                                const double bh[13], int npunct,
                                                const double *table, const mgic_field *pi,
                                                const double pot[3], int max_level,
                                                const int *ref_ratio);

/* The final-data writer with the diagnostic components filled (mgic.h,
 * "Constraints"): components 27-30 (Ham, Mom1, Mom2, Mom3) carry
 * mgic_field_constraint_vars of the same sources instead of the zeros the
 * writers above put there.  The arguments are those of
 * mgic_io_write_final_data_matter, every optional one nullable: phi NULL (the
 * analytic Gaussian), table NULL with npunct = 0 (the two holes of bh), pot
 * NULL (no matter; pi must then be NULL), pi NULL (Pi = 0).  The other 27
 * components and the file layout are what the writer above that takes the
 * same sources produces.  What the _matter form refuses, and a pi without
 * pot, are MGIC_EBADARG before the file is created. */
MGIC_IO_API int mgic_io_write_final_data_constraints(const char *filename, int nlevels,
                                                     const mgic_field *psi, const mgic_field *phi,
                                                     const double bh[13], int npunct,
                                                     const double *table, const mgic_field *pi,
                                                     const double *pot, int max_level,
                                                     const int *ref_ratio);

/* The final-data writer with the total tensor of the momentum solve (mgic.h,
 * "The momentum constraint"): abar holds six stored fields per level, level
 * l's at abar[6 l .. 6 l + 5] in the order 11, 12, 13, 22, 23, 33 on psi[l]'s
 * layout, added to the Bowen-York tensor in the A11..A33 components (8-13)
 * through mgic_field_grchombo_vars_ctt.  constraints != 0: components 27-30
 * carry mgic_field_constraint_vars_ctt of the same sources (the fields' ghost
 * layer 1 must then be filled), else zeros.  pot and abar are required;
 * everything else as mgic_io_write_final_data_matter.  A NULL field and one
 * of another layout are MGIC_EBADARG before the file is created. */
MGIC_IO_API int mgic_io_write_final_data_ctt(const char *filename, int nlevels,
                                             const mgic_field *psi, const mgic_field *phi,
                                             const double bh[13], int npunct, const double *table,
                                             const mgic_field *pi, const double pot[3],
                                             const mgic_field *abar, int constraints,
                                             int max_level, const int *ref_ratio);

/* The final-data writer of the CTTK method (mgic_cttk.h): K is
 * a stored field, K[l] on psi[l]'s layout.  The file is what
 * mgic_io_write_final_data_ctt writes at constant_K = 0 (bh[12] is ignored)
 * with component 7, "K", copied from K[l]'s valid cells.  cons NULL:
 * components 27-30 are zeros; else cons holds five fields per level, level
 * l's at cons[5 l .. 5 l + 4] in the order Ham, Mom1, Mom2, Mom3, Ham_abs
 * (the corrected fields of mgic_cttk_constraints), and components 27-30 are
 * copied from the first four.  Host code: the stored fields come through
 * mgic_field_download.  What the _ctt form refuses, and a NULL K or cons field
 * or one of another layout, are MGIC_EBADARG before the file is created. */
MGIC_IO_API int mgic_io_write_final_data_cttk(const char *filename, int nlevels,
                                              const mgic_field *psi, const mgic_field *phi,
                                              const double bh[13], int npunct,
                                              const double *table, const mgic_field *pi,
                                              const double pot[3], const mgic_field *abar,
                                              const mgic_field *K, const mgic_field *cons,
                                              int max_level, const int *ref_ratio);

/* The same two layouts from host arrays (tests, and callers whose data is
 * already on the host).  kind 0: final data (31 components), 1: solver data
 * (10).  Level l has nbox[l] boxes (6 ints each, all levels concatenated in
 * `boxes`), domain domains[6 l..], cell size dx[l]; `data` holds every box of
 * every level in that order, each box component-major, i fastest.  iter and
 * max_level as above (iter ignored for kind 0, max_level for kind 1). */
MGIC_IO_API int mgic_io_write_host(const char *filename, int kind, int nlevels, const int *nbox,
                                   const int *boxes, const int *domains, const double *dx,
                                   const int *ref_ratio, const double *data, int max_level,
                                   int iter);

#ifdef __cplusplus
}
#endif
#endif /* MGIC_IO_H */

/*
 * mgic.h -- C ABI of the MI355X-native multigrid library (libmgic.so).
 *
 * The drop-in boundary for the reference's hot path: eugenealim/MG_IC_code
 * hands its V-cycle to Chombo through the operator-plugin API
 *   defineOperatorFactory / VariableCoeffPoissonOperatorFactory
 *     (Source/VariableCoeffPoissonOperatorFactory.H:22-117)
 *   VariableCoeffPoissonOperator  (Source/VariableCoeffPoissonOperator.H:25-170)
 * and the operator reaches its arithmetic through the ChomboFortran C ABI
 * (Source/VariableCoeffPoissonOperatorF_F.H; those host drop-ins are declared
 * in mgic_chf.h).  This header exposes the same surface with plain pointers
 * and integers: every handle-level entry point below names the reference
 * method it replaces.
 *
 * Conventions
 *   - Boxes are 6 ints {lo0, lo1, lo2, hi0, hi1, hi2}, inclusive cell
 *     indices in the level's global index space (Chombo Box).
 *   - Every function returns 0 on success and a negative MGIC_E* code on
 *     failure (the reference aborts through MayDay; this library never
 *     aborts); mgic_last_error() describes the last failure of the thread.
 *   - All device work is enqueued on the communicator's HIP stream; the
 *     functions that return host scalars (dot, norm, iteration norms,
 *     BiCGStab) synchronise that stream.
 *   - Fields are fp64, one component, one ghost layer, device resident.
 */
#ifndef MGIC_H
#define MGIC_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGIC_API __attribute__((visibility("default")))

#define MGIC_OK 0
#define MGIC_EBADARG (-1)
#define MGIC_EHIP (-2)
#define MGIC_ERCCL (-3)
#define MGIC_ESTATE (-4)
#define MGIC_EUNKNOWN (-5)
#define MGIC_UNIQUE_ID_BYTES 128

typedef struct mgic_comm_s *mgic_comm;       /* one rank: RCCL comm + HIP stream */
typedef struct mgic_grid_s *mgic_grid;       /* DisjointBoxLayout + ProblemDomain + dx */
typedef struct mgic_field_s *mgic_field;     /* LevelData<FArrayBox> (1 comp, 1 ghost) */
typedef struct mgic_factory_s *mgic_factory; /* VariableCoeffPoissonOperatorFactory */
typedef struct mgic_op_s *mgic_op;           /* VariableCoeffPoissonOperator */
typedef struct mgic_mg_s *mgic_mg;           /* AMRMultiGrid on one AMR level */
typedef struct mgic_plan_s *mgic_plan;       /* host-side view of a Copier plan */
typedef struct mgic_mixed_s *mgic_mixed;     /* fp32-smoother / fp64-residual V-cycle */
typedef struct mgic_amr_s *mgic_amr;         /* AMR hierarchy (levels > 0, ratio 2) */

/* Operator constants and ParseBC state (params.txt keys alpha, beta, bc_lo,
 * bc_hi, bc_value, coefficient_average_type; [Chombo] statics). */
typedef struct {
  double alpha, beta;          /* default 0, -1 (Factory.cpp:317-322) */
  int bc_lo[3], bc_hi[3];      /* 0 Dirichlet, 1 Neumann, 2 periodic flag */
  double bc_value;
  int coefficient_average_type; /* 0 arithmetic (default), 1 harmonic */
  int prolong_type;             /* 0 piecewise constant, 1 linear (default) */
  int relax_mode;               /* 1 GSRB (default), 4 Jacobi */
  int fused_smoother;           /* fused red+black sweep: 0 off (one launch per colour
                                   pass), 1 kernel by box size, 2 z-streaming, 3 3D blocks */
  int deep_halo;                /* fused sweeps on exchanged layouts: 4-deep ghost shells,
                                   two sweeps per exchange (the first on the box grown by
                                   2 across exchanged faces).  0 off (default), 1 every
                                   level, 2 levels of boxes <= 128^3 cells */
} mgic_op_params;

/* MultiGrid / bottom-solver configuration (MultilevelLinearOp knobs:
 * numMGsmooth, numMGIterations, preCondSolverDepth; BiCGStab defaults). */
typedef struct {
  int max_depth;         /* deepest MG depth, -1: as deep as coarsenable */
  int n_pre, n_post, n_bottom;
  int bottom_solver;     /* 0: relax(n_bottom), 1: BiCGStab */
  int cycles;            /* 1 = V-cycle */
  int agglomerate_below; /* gather to rank 0 once a box side < this; 0 off.  A
                            gathered depth (and every depth below it) runs on
                            rank 0 alone, its BiCGStab reductions included; the
                            other ranks go from the gather to the scatter */
  int bicg_imax;
  double bicg_eps, bicg_reps, bicg_small;
  int bicg_restarts, bicg_norm_type;
} mgic_mg_params;

/* The layout of the parameter structs above and the entry points' argument
 * lists: bumped whenever either changes (round 4 removed fields from the
 * middle of mgic_op_params / mgic_mg_params).  An integrator compiled against
 * this header checks mgic_abi_version() == MGIC_ABI_VERSION once at start-up. */
#define MGIC_ABI_VERSION 2
MGIC_API int mgic_abi_version(void);
MGIC_API const char *mgic_version(void);
MGIC_API const char *mgic_last_error(void);
MGIC_API int mgic_set_device(int device);
MGIC_API int mgic_get_device_count(int *count);
MGIC_API int mgic_device_synchronize(void);
MGIC_API void mgic_op_params_default(mgic_op_params *p);
MGIC_API void mgic_mg_params_default(mgic_mg_params *p);

/* ---- communicator (MPI_Init / process group, Main_PoissonSolver.cpp:261) */
MGIC_API int mgic_comm_unique_id(unsigned char id[MGIC_UNIQUE_ID_BYTES]);
MGIC_API int mgic_comm_create(int rank, int size, const unsigned char *id, int force_rccl,
                              mgic_comm *out);
/* The peer-mapped transport instead of RCCL (no RCCL communicator): every
 * rank maps every other rank's signal page and receive arena through
 * hipIpcOpenMemHandle, and an exchange is two kernels with device-side flags
 * (ranks may share one device).  `allgather` is the host's own collective
 * (MPI_Allgather in a Chombo build), called once inside this function:
 * gather `nbytes` from every rank into out[size * nbytes], rank order, 0 on
 * success; it may be NULL when size == 1.  arena_bytes: one message buffer
 * (0: MGIC_IPC_ARENA_MB, default 64 MB); every rank passes the same value.
 * Replaces the MPI transport of Chombo's Copier (exchange(),
 * VariableCoeffPoissonOperator.cpp:48,131,301) and of its norms. */
typedef int (*mgic_allgather_fn)(const void *in, size_t nbytes, void *out, void *user);
MGIC_API int mgic_comm_create_ipc(int rank, int size, mgic_allgather_fn allgather, void *user,
                                  size_t arena_bytes, mgic_comm *out);
/* transport of a communicator: 0 none (one rank), 1 RCCL, 2 peer-mapped */
MGIC_API int mgic_comm_transport(mgic_comm c, int *transport);
MGIC_API int mgic_comm_destroy(mgic_comm c);
MGIC_API int mgic_comm_set_stream(mgic_comm c, void *hip_stream); /* NULL: own stream */
MGIC_API int mgic_comm_get_stream(mgic_comm c, void **hip_stream);
MGIC_API int mgic_comm_set_self_messages(mgic_comm c, int on);
/* exchanges with messages (peer-mapped or RCCL) issued on this communicator so far:
   a measurement counter (tools/rank_proxy.py charges per-exchange latency with it) */
MGIC_API int mgic_comm_exchanges(mgic_comm c, unsigned long long *count);
MGIC_API int mgic_comm_synchronize(mgic_comm c); /* + raises a transport timeout */
MGIC_API int mgic_comm_rank(mgic_comm c, int *rank, int *size, int *uses_rccl);

/* ---- grids (DisjointBoxLayout(boxes, procs, domain); set_grids,
 *      Source/SetGrids.cpp:54-58) */
MGIC_API int mgic_grid_create(mgic_comm c, const int domain[6], const int periodic[3], double dx,
                              int nbox, const int *boxes, const int *owners, mgic_grid *out);
MGIC_API int mgic_grid_destroy(mgic_grid g);
MGIC_API int mgic_grid_num_local(mgic_grid g, int *n);
MGIC_API int mgic_grid_local_box(mgic_grid g, int n, int lohi[6], int *global_index);
MGIC_API int mgic_grid_coarsen(mgic_grid g, int ratio, mgic_grid *out);

/* ---- copy plans, host side (Copier / exchangeDefine + trimEdges,
 *      Source/VariableCoeffPoissonOperatorFactory.cpp:82-99,179-185).
 *      The exact plan rank `rank` of `size` executes for a layout pair
 *      (exchange: src = dst layout, with_faces = 1; gather/scatter for the
 *      coarse levels: with_valid = 1), computed WITHOUT a GPU so the
 *      multi-rank path can be checked on CPU.  Items are 12 int64 each:
 *      {src, dst, soff, doff, ssy, ssz, dsy, dsz, nx, ny, nz, peer}; src/dst
 *      are local box indices or -1 for the per-peer message buffer, offsets
 *      are in doubles from the box's valid-lo cell (or from the buffer
 *      start), strides in doubles.  which: 0 local copies, 1 pack (send),
 *      2 unpack (receive). */
MGIC_API int mgic_plan_create(int rank, int size, const int domain[6], const int periodic[3],
                              int nsrc, const int *src_boxes, const int *src_owners, int ndst,
                              const int *dst_boxes, const int *dst_owners, int with_valid,
                              int with_faces, mgic_plan *out);
/* the ghost-shell exchange (faces, edges and corners, `depth` deep) of one
 * layout: what the fused sweeps exchange (depth 2; 4 in deep-halo mode) */
MGIC_API int mgic_plan_create_shell(int rank, int size, const int domain[6],
                                    const int periodic[3], int nboxes, const int *boxes,
                                    const int *owners, int depth, mgic_plan *out);
/* the host-side tables transport `transport` (1 RCCL, 2 peer-mapped; the
 * numbering of mgic_comm_transport) builds for this plan before executing
 * it: 0, or an error when that transport cannot execute it (the peer-mapped
 * transport takes at most 32 peers per plan; RCCL has no such limit) */
MGIC_API int mgic_plan_check_transport(mgic_plan p, int transport);
/* the peer-mapped transport's block table of this plan (built as by
 * mgic_plan_check_transport(p, 2)): *n put and get blocks; with rows != NULL,
 * five values per block: side (0 put, 1 get), peer rank, flag, first element
 * in the message, element count.  Both sides of a message must list the same
 * (flag, first, count) rows: a get block waits for the put block of its flag */
MGIC_API int mgic_plan_ipc_blocks(mgic_plan p, int *n, long long *rows);
/* the same table for a block size other than the default: block_elems as
 * MGIC_IPC_BLOCK_ELEMS sets it (a multiple of 512 in [512, 2^20]); a plan's
 * table is built once, so one block size per plan handle */
MGIC_API int mgic_plan_ipc_blocks_per(mgic_plan p, long long block_elems, int *n,
                                      long long *rows);
MGIC_API int mgic_plan_destroy(mgic_plan p);
MGIC_API int mgic_plan_sizes(mgic_plan p, int *n_local, int *n_pack, int *n_unpack, int *n_peers);
MGIC_API int mgic_plan_items(mgic_plan p, int which, long long *items);
/* per peer (ascending rank): send/recv counts and buffer offsets, doubles */
MGIC_API int mgic_plan_peers(mgic_plan p, int *peers, long long *send_cnt, long long *send_off,
                             long long *recv_cnt, long long *recv_off);
/* FabGeom of local box n of the src (layout = 0) or dst (layout = 1)
 * layout: {sy, sz, origin, total} in doubles */
MGIC_API int mgic_plan_geom(mgic_plan p, int layout, int n, long long geom[4]);

/* ---- fields (LevelData<FArrayBox>) */
MGIC_API int mgic_field_create(mgic_grid g, mgic_field *out);
MGIC_API int mgic_field_destroy(mgic_field f);
/* device pointer of the valid-lo cell of local box n and its strides
 * {1, sy, sz} in doubles */
MGIC_API int mgic_field_device_ptr(mgic_field f, int n, double **valid_lo, long strides[3]);
/* host <-> device, contiguous i-fastest over the valid box (with_ghosts=0)
 * or over the valid box grown by one (with_ghosts=1); synchronous */
MGIC_API int mgic_field_upload(mgic_field f, int n, const double *host, int with_ghosts);
MGIC_API int mgic_field_download(mgic_field f, int n, double *host, int with_ghosts);
MGIC_API int mgic_field_set_val(mgic_field f, double v);  /* valid cells */
MGIC_API int mgic_field_set_zero(mgic_field f);           /* valid + ghosts */
MGIC_API int mgic_field_exchange(mgic_field f);           /* LevelData::exchange */
/* LevelData::copyTo: valid -> valid (+ dst face ghosts if with_faces) */
MGIC_API int mgic_field_copy_to(mgic_field src, mgic_field dst, int with_faces);
/* set_a_coef / set_rhs at psi = 1 (SetLevelData.cpp:73-127, :281-325);
 * bh[13] = {domain_length, G_Newton, phi_amplitude, phi_wavelength,
 *           bh1_bare_mass, bh2_bare_mass, bh1_spin, bh2_spin, bh1_offset,
 *           bh2_offset, bh1_momentum, bh2_momentum, constant_K} */
MGIC_API int mgic_field_binary_bh(mgic_field acoef, mgic_field rhs, const double bh[13]);
/* the same at a general conformal factor psi (read with its ghost layer);
 * psi = NULL is psi = 1 (NL iteration 0) */
MGIC_API int mgic_field_nl_coefs(mgic_field psi, mgic_field acoef, mgic_field rhs,
                                 const double bh[13]);
/* set_constant_K_integrand (SetLevelData.cpp:131-180) at psi (NULL: 1):
 * the integrand of the periodic integrability condition for K */
MGIC_API int mgic_field_nl_integrand(mgic_field psi, mgic_field out, const double bh[13]);

/* ---- set_grids (SetGrids.cpp:31-149): the AMR hierarchy from tagging.
 * The condition and the tags are device kernels; clustering, nesting and the
 * owners are host integer code (no device is touched by mgic_regrid_*). */
/* set_regrid_condition (SetLevelData.cpp:190-240) at psi (NULL: 1, what
 * set_grids uses); no ghost cell of psi is read */
MGIC_API int mgic_field_regrid_condition(mgic_field psi, mgic_field out, const double bh[13]);
/* norm(x, ord) of one level over every rank (ord 0 max, 1 sum |x|, 2 root of
 * sum x^2): mgic_op_norm's exact level reduction, for a field that has no
 * operator (set_tag_cells' maxRHS, SetGrids.cpp:184) */
MGIC_API int mgic_field_norm(mgic_field x, int ord, double *out);
/* set_tag_cells (SetGrids.cpp:172-207) onto the clustering lattice of spacing
 * c level cells (lattice index = floor(cell / c)): a cell is tagged iff
 * |cond| >= tag_val; tags grown by `grow` cells and clipped to the domain
 * box set every lattice cell they reach.  The mask covers the lattice
 * bounding box of the level: all of its boxes (every rank's), grown by
 * `grow`, clipped to the domain, rounded out to whole lattice cells.
 * lat_lo / lat_n (always written): its low corner and extents in lattice
 * cells.  mask_host == NULL: the size query.  Otherwise mask_host receives
 * lat_n[0]*lat_n[1]*lat_n[2] bytes (x fastest), 1 where THIS rank's cells
 * set a lattice cell; the call synchronises. */
MGIC_API int mgic_field_tag_lattice(mgic_field cond, double tag_val, int grow, int c,
                                    int lat_lo[3], int lat_n[3], unsigned char *mask_host);
/* c = max(block_factor / 2, 1), maxlen = max(max_grid_size / block_factor, 1);
 * MGIC_EBADARG unless block_factor is a power of two */
MGIC_API int mgic_regrid_lattice(int block_factor, int max_grid_size, int *c, int *maxlen);
/* Berger-Rigoutsos clustering of a byte mask (n[0] fastest) into disjoint
 * boxes in mask indices, at most maxlen a side, sorted by (lo_z, lo_y, lo_x).
 * *nbox = their number; the first min(cap, *nbox) are written to boxes
 * (6 ints each; cap = 0: count only). */
MGIC_API int mgic_regrid_cluster(const unsigned char *mask, const int n[3], double fill_ratio,
                                 int maxlen, int cap, int *nbox, int *boxes);
/* BRMeshRefine::regrid stand-in, top-down with proper nesting: the tag
 * lattices of levels 0 .. nlev-1 (masks[l] over lattice cells lat_lo[3l..] +
 * [0, lat_n[3l..])) -> the boxes of levels 1 .. nlev.  nbox[l] = the number
 * of boxes of level l + 1; boxes = the lists concatenated (cap as above);
 * *new_finest = the highest level with boxes.  MGIC_EBADARG when
 * block_factor is not a power of two or a level's domain is not a multiple
 * of the lattice spacing. */
MGIC_API int mgic_regrid_levels(int nlev, const int domain0[6], const unsigned char *const *masks,
                                const int *lat_lo, const int *lat_n, int block_factor,
                                int max_grid_size, double fill_ratio, int nesting_radius, int cap,
                                int *nbox, int *boxes, int *new_finest);
/* The same with proper nesting through the wrap: in a
 * direction with periodic[d] != 0 the nesting region coarsen(box of level
 * l + 2, 2) +- nesting_radius is not clipped to the level-(l + 1) domain but
 * wrapped round it before it is coarsened onto level l's lattice.
 * Clustering runs inside the domain, so no box crosses a face: a feature on
 * a periodic face becomes boxes on both sides.  periodic = (0, 0, 0) gives
 * mgic_regrid_levels. */
MGIC_API int mgic_regrid_levels_periodic(int nlev, const int domain0[6], const int periodic[3],
                                         const unsigned char *const *masks, const int *lat_lo,
                                         const int *lat_n, int block_factor, int max_grid_size,
                                         double fill_ratio, int nesting_radius, int cap,
                                         int *nbox, int *boxes, int *new_finest);
/* LoadBalance stand-in: box i of the sorted list goes to rank
 * floor(size * (prefix_i + cells_i / 2) / total) */
MGIC_API int mgic_regrid_owners(int nbox, const int *boxes, int size, int *owners);
/* every cell of the allocation, ghosts included (set_initial_conditions
 * sets psi over the whole FAB, SetLevelData.cpp:31-72) */
MGIC_API int mgic_field_set_val_all(mgic_field f, double v);

/* ---- operator factory (defineOperatorFactory, Factory.cpp:29-49) */
MGIC_API int mgic_factory_define(mgic_grid g, const mgic_op_params *p, mgic_field aCoef,
                                 mgic_field bCoef, mgic_factory *out);
MGIC_API int mgic_factory_destroy(mgic_factory f);
/* MGnewOp (Factory.cpp:139-234): returns 1 with *out = NULL when the layout
 * is not coarsenable(2^depth * s_maxCoarse) */
MGIC_API int mgic_factory_mg_new_op(mgic_factory f, int depth, mgic_op *out);
MGIC_API int mgic_factory_amr_new_op(mgic_factory f, mgic_op *out); /* :236-295 */
MGIC_API int mgic_factory_ref_to_finer(mgic_factory f, int *ratio); /* :297-314 */

/* ---- operator (VariableCoeffPoissonOperator) */
MGIC_API int mgic_op_destroy(mgic_op op);
MGIC_API int mgic_op_grid(mgic_op op, mgic_grid *out);
MGIC_API int mgic_op_coef(mgic_op op, int which /* 0 aCoef, 1 bCoef, 2 lambda */,
                          mgic_field *out);
MGIC_API int mgic_op_residual(mgic_op op, mgic_field lhs, mgic_field dpsi, mgic_field rhs,
                              int homogeneous);                                  /* residualI */
MGIC_API int mgic_op_apply_op(mgic_op op, mgic_field lhs, mgic_field dpsi, int homogeneous);
MGIC_API int mgic_op_apply_op_no_boundary(mgic_op op, mgic_field lhs, mgic_field dpsi);
MGIC_API int mgic_op_precond(mgic_op op, mgic_field cor, mgic_field res);        /* preCond */
MGIC_API int mgic_op_relax(mgic_op op, mgic_field e, mgic_field r, int iterations);
MGIC_API int mgic_op_level_gsrb(mgic_op op, mgic_field dpsi, mgic_field rhs);
MGIC_API int mgic_op_level_jacobi(mgic_op op, mgic_field dpsi, mgic_field rhs);
MGIC_API int mgic_op_restrict_residual(mgic_op fine, mgic_field resCoarse, mgic_field dpsiFine,
                                       mgic_field rhsFine);
MGIC_API int mgic_op_prolong_increment(mgic_op fine, mgic_field phiFine, mgic_field corCoarse);
MGIC_API int mgic_op_set_alpha_beta(mgic_op op, double alpha, double beta);
MGIC_API int mgic_op_set_coefs(mgic_op op, mgic_field aCoef, mgic_field bCoef, double alpha,
                               double beta);
MGIC_API int mgic_op_reset_lambda(mgic_op op);
MGIC_API int mgic_op_set_time(mgic_op op, double t);
/* set_update_psi0 (SetLevelData.cpp:236-256): exchange dpsi, its domain
 * ghosts = the inhomogeneous BC image, psi += dpsi over the valid cells and
 * ghost layer 1 */
MGIC_API int mgic_op_update_psi(mgic_op op, mgic_field psi, mgic_field dpsi);
MGIC_API int mgic_op_fill_bc(mgic_op op, mgic_field u, int homogeneous);         /* m_bc */
MGIC_API int mgic_op_set_to_zero(mgic_op op, mgic_field x);
MGIC_API int mgic_op_assign(mgic_op op, mgic_field lhs, mgic_field rhs);
MGIC_API int mgic_op_incr(mgic_op op, mgic_field lhs, mgic_field x, double scale);
MGIC_API int mgic_op_axby(mgic_op op, mgic_field lhs, mgic_field x, mgic_field y, double a,
                          double b);
MGIC_API int mgic_op_scale(mgic_op op, mgic_field lhs, double s);
MGIC_API int mgic_op_dot(mgic_op op, mgic_field x, mgic_field y, double *out);
MGIC_API int mgic_op_norm(mgic_op op, mgic_field x, int ord, double *out);
/* BiCGStab's fused updates (the host loop's; each equals the separate passes
 * bit for bit).  s = r + ca v; e = e + cb pt; *out = norm(s, ord), ord 0/1/2 */
MGIC_API int mgic_op_axpy2_norm(mgic_op op, mgic_field s, mgic_field r, mgic_field v, double ca,
                                mgic_field e, mgic_field pt, double cb, int ord, double *out);
/* *ts = dot(t, s), *tt = dot(t, t) in one pass */
MGIC_API int mgic_op_dot2(mgic_op op, mgic_field t, mgic_field s, double *ts, double *tt);
/* p = ((p * beta) + c v) + 1.0 r */
MGIC_API int mgic_op_bicg_p(mgic_op op, mgic_field p, mgic_field v, mgic_field r, double beta,
                            double c);
/* BiCGStabSolver<LevelData>::solve with this op (bottom solver) */
MGIC_API int mgic_op_bicgstab(mgic_op op, mgic_field phi, mgic_field rhs, int homogeneous,
                              const mgic_mg_params *p, int *iterations);
/* whether the calling thread's last mgic_op_bicgstab ran its loop on the device */
MGIC_API int mgic_op_bicgstab_info(int *device);

/* ---- multigrid (AMRMultiGrid on one AMR level + MultiGrid hierarchy) */
MGIC_API int mgic_mg_create(mgic_factory f, const mgic_mg_params *p, mgic_mg *out);
MGIC_API int mgic_mg_destroy(mgic_mg mg);
MGIC_API int mgic_mg_num_depths(mgic_mg mg, int *n);
MGIC_API int mgic_mg_op(mgic_mg mg, int depth, mgic_op *out);
/* internal fields of depth >= 1: which 0 = correction e, 1 = residual r */
MGIC_API int mgic_mg_level_field(mgic_mg mg, int depth, int which, mgic_field *out);
MGIC_API int mgic_mg_one_cycle(mgic_mg mg, mgic_field e, mgic_field r); /* MultiGrid::oneCycle */
/* e = 0; oneCycle(e, resid); phi += e; resid = rhs - L(phi); *norm (if
 * norm_type >= 0, else not computed and nothing synchronised) */
MGIC_API int mgic_mg_iteration(mgic_mg mg, mgic_field phi, mgic_field rhs, mgic_field resid,
                               int norm_type, int homogeneous, double *norm);
/* `count` iterations (AMRMultiGrid::solve's loop body) from the state
 * mgic_mg_iteration / mgic_mg_init_residual leave; norms[i] (count values,
 * may be NULL) = what the i-th mgic_mg_iteration call would return, bit for
 * bit (the same launches in the same order).  Iteration i's norm is read on
 * the host after iteration i+1's V-cycle has been queued up to its first
 * launch that writes phi and before that launch is queued -- where a stop
 * test on the norm would decide -- so the device does not idle while the
 * host reads it. */
MGIC_API int mgic_mg_iterations(mgic_mg mg, mgic_field phi, mgic_field rhs, mgic_field resid,
                                int count, int norm_type, int homogeneous, double *norms);
MGIC_API int mgic_mg_init_residual(mgic_mg mg, mgic_field phi, mgic_field rhs,
                                   mgic_field resid, int norm_type, int homogeneous,
                                   double *norm);
/* full multigrid on the current resid (as left by init_residual /
 * iteration): resid restricted to every depth, bottom solve, then per finer
 * depth e = P e_coarse and `ncycles` V-cycles; phi += e; resid = rhs - L(phi) */
MGIC_API int mgic_mg_fmg(mgic_mg mg, mgic_field phi, mgic_field rhs, mgic_field resid,
                         int norm_type, int homogeneous, int ncycles, double *norm);
/* HIP events around every BiCGStab bottom solve this rank runs (bottom_solver
 * 1; with a gathered coarsest depth only its owner runs them): on != 0 resets
 * and starts recording; bottom_ms returns their total time and count */
MGIC_API int mgic_mg_bottom_timer(mgic_mg mg, int on);
MGIC_API int mgic_mg_bottom_ms(mgic_mg mg, double *ms, int *calls);
/* BiCGStab iterations summed over the solves timed since mgic_mg_bottom_timer
 * (1), and the smallest / largest norm of the coarse residual they started
 * from (the bench's proof that each timed solve did work) */
MGIC_API int mgic_mg_bottom_iters(mgic_mg mg, long long *iters, double *r0_min, double *r0_max);
/* the last BiCGStab bottom solve this rank ran: on the device (1) or by the
 * host loop (0), its iterations and the norm of the residual it started from */
MGIC_API int mgic_mg_bottom_info(mgic_mg mg, int *device, int *iters, double *r0);
/* the last bottom solve again, n times, each from e = 0 on the same coarse
 * residual: total ms (HIP events), iterations per solve, the residual's norm;
 * *solves = n, or 0 on a rank that does not run the coarsest depth or before
 * a V-cycle has run a bottom solve */
MGIC_API int mgic_mg_bottom_replay(mgic_mg mg, int n, double *ms, int *iters, double *r0,
                                   int *solves);

/* Mixed precision (BASELINE config C5): the same V-cycle schedule with the
 * correction equation in fp32 (GSRB / restrictResidual / prolongIncrement in
 * float, coefficients rounded from the fp64 hierarchy), the fine residual
 * rhs - L(phi) in fp64 rounded once, phi += e in fp64.  Bottom: relax
 * (n_bottom).  agglomerate_below and deep_halo as for the fp64 cycle (fp32
 * gathers / scatters and 4-deep fp32 shells).  resid (fp64) may be NULL
 * unless a norm is requested (norm_type >= 0).  Inhomogeneous BC for the fine
 * residual. */
MGIC_API int mgic_mixed_create(mgic_factory f, const mgic_mg_params *p, mgic_mixed *out);
MGIC_API int mgic_mixed_destroy(mgic_mixed m);
MGIC_API int mgic_mixed_num_depths(mgic_mixed m, int *n);
MGIC_API int mgic_mixed_init_residual(mgic_mixed m, mgic_field phi, mgic_field rhs,
                                      mgic_field resid, int norm_type, double *norm);
MGIC_API int mgic_mixed_iteration(mgic_mixed m, mgic_field phi, mgic_field rhs, mgic_field resid,
                                  int norm_type, double *norm);
MGIC_API int mgic_mixed_fmg(mgic_mixed m, mgic_field phi, mgic_field rhs, mgic_field resid,
                            int norm_type, int ncycles, double *norm);

/* ---- AMR levels > 0 ([Chombo] AMRPoissonOp multi-level
 * operators restated: QuadCFInterp, AMROperator / AMRResidual (reflux a
 * no-op as in the reference unless switched on, mgic_amr_set_reflux below),
 * AMRRestrict, AMRProlong, AMRUpdateResidual,
 * AMRMultiGrid's multi-level V-cycle).  grids[0] tiles its domain; level
 * l+1's domain is level l's refined by 2 and its boxes are properly nested
 * (mgic_grid_create_patches).  Level 0 is solved by its MultiGrid (base). */
MGIC_API int mgic_grid_create_patches(mgic_comm c, const int domain[6], const int periodic[3],
                                      double dx, int nbox, const int *boxes, const int *owners,
                                      mgic_grid *out); /* disjoint boxes inside the domain */
MGIC_API int mgic_amr_create(int nlevels, const mgic_grid *grids, const mgic_field *acoef,
                             const mgic_field *bcoef, const mgic_op_params *op,
                             const mgic_mg_params *base, mgic_amr *out);
MGIC_API int mgic_amr_destroy(mgic_amr a);
MGIC_API int mgic_amr_num_levels(mgic_amr a, int *n);
MGIC_API int mgic_amr_level_op(mgic_amr a, int level, mgic_op *out); /* borrowed */
/* coarse == NULL: homogeneousCFInterp (zero coarse field) */
MGIC_API int mgic_amr_cf_interp(mgic_amr a, int level, mgic_field u, mgic_field coarse);
MGIC_API int mgic_amr_average_down(mgic_amr a, int level, mgic_field coarse, mgic_field fine);
MGIC_API int mgic_amr_operator(mgic_amr a, int level, mgic_field lphi, mgic_field phi,
                               mgic_field phi_coarse, int homogeneous);
MGIC_API int mgic_amr_residual(mgic_amr a, int level, mgic_field r, mgic_field phi,
                               mgic_field phi_coarse, mgic_field rhs, int homogeneous);
MGIC_API int mgic_amr_restrict(mgic_amr a, int level, mgic_field res_coarse, mgic_field res,
                               mgic_field corr, mgic_field corr_coarse);
MGIC_API int mgic_amr_prolong(mgic_amr a, int level, mgic_field corr, mgic_field corr_coarse);
MGIC_API int mgic_amr_update_residual(mgic_amr a, int level, mgic_field res, mgic_field corr,
                                      mgic_field corr_coarse);
/* composite residuals rhs - L(phi) on every level (covered coarse cells
 * zeroed); *norm = max over levels (norm_type >= 0) */
MGIC_API int mgic_amr_init_residual(mgic_amr a, const mgic_field *phi, const mgic_field *rhs,
                                    int norm_type, double *norm);
/* one AMR V-cycle, phi += e on every level, average down, new residuals */
MGIC_API int mgic_amr_iteration(mgic_amr a, const mgic_field *phi, const mgic_field *rhs,
                                int norm_type, double *norm);
MGIC_API int mgic_amr_residual_field(mgic_amr a, int level, mgic_field *out); /* borrowed */
/* MultilevelLinearOp over the hierarchy (Main_PoissonSolver.cpp:103-117,
 * 169-170 with max_level > 0; [Chombo] semantics restated, see amr.hpp):
 * lhs = AMROperator on every level, covered coarse cells zeroed; dot =
 * sum_l dx_l^3 levelDot; norm 0 = max over levels, 1 / 2 = dx_l^3-weighted;
 * dot and norm mask the covered coarse cells of x (MultilevelLinearOp's
 * dotProduct / norm count each physical cell once, on its finest level) */
MGIC_API int mgic_amr_apply_op(mgic_amr a, const mgic_field *lhs, const mgic_field *x,
                               int homogeneous);
/* r = rhs - L(phi) with the same operator (the residual mgic_amr_solve takes),
 * covered coarse cells zeroed */
MGIC_API int mgic_amr_composite_residual(mgic_amr a, const mgic_field *r, const mgic_field *phi,
                                         const mgic_field *rhs, int homogeneous);
MGIC_API int mgic_amr_dot(mgic_amr a, const mgic_field *x, const mgic_field *y, double *out);
MGIC_API int mgic_amr_norm(mgic_amr a, const mgic_field *x, int ord, double *out);
/* computeNorm / computeSum (Main_PoissonSolver.cpp:144-145,208-209): covered
 * coarse cells masked, dx_l^3 weights (x is not modified) */
MGIC_API int mgic_amr_composite_norm(mgic_amr a, const mgic_field *x, int ord, double *out);
MGIC_API int mgic_amr_composite_sum(mgic_amr a, const mgic_field *x, double *out);
/* MultilevelLinearOp::preCond: e = 0, `iters` AMR V-cycle iterations on
 * (e, r) with homogeneous physical BCs */
MGIC_API int mgic_amr_precondition(mgic_amr a, const mgic_field *e, const mgic_field *r, int iters);

/* ---- reflux at coarse-fine faces (include/mgic_reflux.h has
 * the term).  Off by default: the composite operator is then the reference's,
 * not conservative.  On: mgic_amr_apply_op, mgic_amr_init_residual /
 * _iteration, _precondition and _solve add the term to every level that has
 * a finer one, and the V-cycle's downsweep adds the fine correction's to the
 * restricted residual.  mgic_amr_operator / _residual (one level) never do.
 * With the switch on, _apply_op, _init_residual and _solve's residuals first
 * overwrite the covered cells of their input (x, phi) with the average of the
 * finer level, so the result depends on the uncovered cells alone, bit for
 * bit; _iteration and _precondition leave that average there anyway.
 * The kernel is libmgic_reflux.so's, reached through this table: one entry of
 * `cells` per uncovered cell with a covered face neighbour (sorted by box and
 * offset), its faces (bits of `mask`: x-lo ... z-hi) consecutive in `faces`
 * from `first`. */
typedef struct mgic_reflux_cell {
  long long off;  /* the cell, from its box's valid-lo */
  int box;        /* local box of the coarse level */
  int first;      /* its first entry of the face table */
  int mask;       /* its interface faces, bit 0 x-lo ... bit 5 z-hi */
  int pad;
} mgic_reflux_cell;
typedef struct mgic_reflux_face {
  long long foff;   /* fine in-cell (0, 0) behind the face, from its box's valid-lo */
  long long cstep;  /* coarse cell -> its covered neighbour */
  long long fstep;  /* fine in-cell -> the ghost across the face */
  long long ft0;    /* fine stride of the lower tangential direction */
  long long ft1;    /* ... of the higher one */
  int fbox;         /* local box of the fine level */
  int pad;
} mgic_reflux_face;
typedef struct mgic_reflux_table {
  int version; /* 1 */
  /* target[c] = target[c] +/- (coef * b[c]) * sum of c's terms for the
   * ncell cells (device tables; phi_c may be NULL: a zero coarse field);
   * sign > 0 adds; 0, or a negative status with last_error() set */
  int (*apply)(const mgic_reflux_cell *cells, const mgic_reflux_face *faces, long long ncell,
               double *const *target, double *const *phi_c, double *const *phi_f,
               double *const *b, double coef, double dx_c, double dx_f, int sign, void *stream);
  const char *(*last_error)(void);
} mgic_reflux_table;
/* the launcher (libmgic_reflux.so's mgic_reflux_register calls this); the
 * table must outlive every mgic_amr */
MGIC_API int mgic_amr_reflux_register(const mgic_reflux_table *t);
/* on != 0 builds the tables (MGIC_ESTATE without a registered launcher,
 * MGIC_EBADARG when a box of a refined level or its refinement is not
 * local); with one level it changes nothing and needs no launcher */
MGIC_API int mgic_amr_set_reflux(mgic_amr a, int on);
/* the per-level primitive, whatever the switch: level has a finer level;
 * target and phi_coarse live on it, phi_fine on level + 1 with its ghosts as
 * mgic_amr_operator(level + 1) leaves them, phi_coarse's face ghosts as
 * mgic_amr_operator(level) does.  phi_coarse == NULL: a zero coarse field.
 * sign > 0: target += term (an operator); sign < 0: target -= term (a
 * residual) */
MGIC_API int mgic_amr_reflux(mgic_amr a, int level, mgic_field target, mgic_field phi_coarse,
                             mgic_field phi_fine, int sign);

/* ---- output (WriteOutput.H).  For local box n, planes
 * [k0, k0+nk) of its valid box: the components the reference writes,
 * component-major and i fastest (the FArrayBox order of that box's chunk of
 * "data:datatype=0"), into out (host memory, or device memory if
 * out_on_device).
 * grchombo_vars: set_output_data (SetLevelData.cpp:343-396), the 31
 *   GRChombo variables (GRChomboUserVariables.hpp order) from psi, with
 *   constant_K = bh[12];
 * solver_vars: output_solver_data's 10 components (WriteOutput.H:74-100):
 *   dpsi, rhs, psi, A11_0, A12_0, A13_0, A22_0, A23_0, A33_0, phi_0. */
MGIC_API int mgic_field_grchombo_vars(mgic_field psi, int n, int k0, int nk, const double bh[13],
                                      double *out, int out_on_device);
MGIC_API int mgic_field_solver_vars(mgic_field dpsi, mgic_field rhs, mgic_field psi, int n, int k0,
                                    int nk, const double bh[13], double *out, int out_on_device);
/* ---- phi_0 as a stored field (the c_phi_0 component set_initial_conditions
 * fills, SetLevelData.cpp:32-71).  phi holds the scalar-field profile at the
 * centre of every cell of each local box and of the one ghost layer next to
 * each face: loc = (iv + 0.5) dx - L/2, also for ghost cells outside the
 * domain or under a coarse-fine boundary.  It is never exchanged, BC-filled
 * or interpolated.  The *_phi entry points are the ones of the same name
 * above with phi_0 read from phi instead of evaluated as the Gaussian; phi
 * must have the layout of the other fields (MGIC_EBADARG otherwise).  Filled
 * with MGIC_PHI_GAUSSIAN they give the analytic entry points' values bit for
 * bit.  A caller's own profile is uploaded with mgic_field_upload(phi, n,
 * host, 1). */
#define MGIC_PHI_GAUSSIAN 0 /* amplitude exp(-r^2 / wavelength)  (MyPhiFunction.H:14-15) */
#define MGIC_PHI_SINE 1     /* amplitude sum_d sin(2 pi x_d wavelength / L)  (:18-20) */
/* fill phi (valid cells and the ghost shell of depth one) with a built-in
 * profile; bh[13] as mgic_field_binary_bh (domain_length, phi_amplitude and
 * phi_wavelength are read).  An unknown profile is MGIC_EBADARG. */
MGIC_API int mgic_field_fill_phi(mgic_field phi, int profile, const double bh[13]);
MGIC_API int mgic_field_nl_coefs_phi(mgic_field psi, mgic_field phi, mgic_field acoef,
                                     mgic_field rhs, const double bh[13]);
MGIC_API int mgic_field_nl_integrand_phi(mgic_field psi, mgic_field phi, mgic_field out,
                                         const double bh[13]);
MGIC_API int mgic_field_regrid_condition_phi(mgic_field psi, mgic_field phi, mgic_field out,
                                             const double bh[13]);
MGIC_API int mgic_field_grchombo_vars_phi(mgic_field psi, mgic_field phi, int n, int k0, int nk,
                                          const double bh[13], double *out, int out_on_device);
MGIC_API int mgic_field_solver_vars_phi(mgic_field dpsi, mgic_field rhs, mgic_field psi,
                                        mgic_field phi, int n, int k0, int nk, const double bh[13],
                                        double *out, int out_on_device);
/* ---- Bowen-York punctures as a table.  The entry points above place two
 * holes on the x axis with momentum along y and spin along z (bh[4..11]).
 * The *_punct entry points take 1 to MGIC_MAX_PUNCTURES punctures instead,
 * each with any position, momentum and spin: `table` holds 10 doubles per
 * puncture, in the order m, x, y, z, Px, Py, Pz, Jx, Jy, Jz, with positions
 * relative to the domain centre (the coordinates of bh1_offset).
 *
 * The table is taken in pairs, in table order: (0, 1), (2, 3), ...  One pair
 * contributes what get_Aij (SetBinaryBH.H:24-53) gives for two holes with
 * these vectors, l_a = loc - (x_a, y_a, z_a), and psi_bh = m_a / r_a +
 * m_b / r_b; A_ij_0 and psi_bh are the sums over the pairs in pair order,
 * starting from the first pair's value.  An odd count is completed by a
 * puncture with m = P = J = 0 at the last puncture's position.  Punctures get
 * no periodic images.  So the deck's two holes written as the table
 * {m1, off1, 0, 0, 0, mom1, 0, 0, 0, spin1, m2, off2, 0, 0, 0, mom2, 0, 0, 0,
 * spin2} give the bits of the entry points above.
 *
 * bh[13] still carries the domain length, G, the phi parameters and
 * constant_K; its six hole entries bh[4..11] are ignored.  phi: the stored
 * phi_0 on the layout of the other fields, or NULL for the analytic Gaussian.
 * MGIC_EBADARG, before anything is launched, for a count outside 1 ..
 * MGIC_MAX_PUNCTURES, a NULL table or a non-finite entry. */
#define MGIC_MAX_PUNCTURES 8
MGIC_API int mgic_field_nl_coefs_punct(mgic_field psi, mgic_field phi, mgic_field acoef,
                                       mgic_field rhs, const double bh[13], int n,
                                       const double *table);
MGIC_API int mgic_field_nl_integrand_punct(mgic_field psi, mgic_field phi, mgic_field out,
                                           const double bh[13], int n, const double *table);
MGIC_API int mgic_field_regrid_condition_punct(mgic_field psi, mgic_field phi, mgic_field out,
                                               const double bh[13], int n, const double *table);
MGIC_API int mgic_field_grchombo_vars_punct(mgic_field psi, mgic_field phi, int n, int k0, int nk,
                                            const double bh[13], int npunct, const double *table,
                                            double *out, int out_on_device);
MGIC_API int mgic_field_solver_vars_punct(mgic_field dpsi, mgic_field rhs, mgic_field psi,
                                          mgic_field phi, int n, int k0, int nk,
                                          const double bh[13], int npunct, const double *table,
                                          double *out, int out_on_device);
/* ---- Matter: the scalar field's kinetic and potential energy.  set_m_value
 * (SetLevelData.cpp:266-278) reads rho = 0.5 * Pi_field * Pi_field + V_of_phi
 * with both set to 0.0 and a note that V(phi) and Pi may be added later; the
 * entry points above keep those zeros.  The *_matter entry points fill the
 * slot:
 *   V(phi) = V0 + 0.5 * mass * mass * phi * phi
 *               + 0.25 * lambda * phi * phi * phi * phi   (left to right),
 *   rho = 0.5 * Pi * Pi + V(phi_0),
 * phi_0 the cell's scalar field (the stored phi if given, else the Gaussian)
 * and Pi the cell's value of the stored field pi.  m = (2/3) K^2 - 16 pi G rho
 * and every expression that uses it are as written in the reference, so rho
 * has the psi weighting the reference's slot gives it; K is constant_K for
 * the coefficients and 0 for the integrand and the regrid condition.
 *
 * pot[3] = V0, mass, lambda.  pi: one value per cell on the layout of the
 * other fields (only valid cells are read; it is never differenced), or NULL
 * for Pi = 0.  Only Pi * Pi enters, so the sign of pi (GRChombo's Pi is
 * "(minus) conjugate momentum") is the caller's convention;
 * mgic_field_grchombo_vars_matter copies pi as given into component 26 ("Pi")
 * and changes no other component.  Each entry point takes what its _punct
 * form takes, with the table nullable too: NULL with n = 0 means the two
 * holes of bh.  With pot all zero and pi NULL or zero they give the bits of
 * the entry points above.  MGIC_EBADARG, before anything is launched, for
 * what the _punct forms refuse, a non-finite pot entry and a pi of another
 * layout.  These entry points leave the momentum constraint's source
 * Pi d_i phi alone: data with a non-zero Pi and a varying phi_0 violate that
 * constraint by 8 pi G Pi d_i phi.  mgic_field_constraints (below) reports
 * the violation; the *_ctt forms ("The momentum constraint") remove it. */
MGIC_API int mgic_field_nl_coefs_matter(mgic_field psi, mgic_field phi, mgic_field acoef,
                                        mgic_field rhs, const double bh[13], int n,
                                        const double *table, mgic_field pi, const double pot[3]);
MGIC_API int mgic_field_nl_integrand_matter(mgic_field psi, mgic_field phi, mgic_field out,
                                            const double bh[13], int n, const double *table,
                                            mgic_field pi, const double pot[3]);
MGIC_API int mgic_field_regrid_condition_matter(mgic_field psi, mgic_field phi, mgic_field out,
                                                const double bh[13], int n, const double *table,
                                                mgic_field pi, const double pot[3]);
MGIC_API int mgic_field_grchombo_vars_matter(mgic_field psi, mgic_field phi, int n, int k0, int nk,
                                             const double bh[13], int npunct, const double *table,
                                             mgic_field pi, const double pot[3], double *out,
                                             int out_on_device);
/* ---- Constraints: the Hamiltonian and momentum constraints of the data at
 * psi (GRChombo's Constraints for a conformally flat metric and constant K,
 * written in chi = psi_0^-4 and A~_ij = psi_0^-6 Abar_ij).  Per valid cell,
 * with psi_0 = psi + psi_bh, K = constant_K and lap, rho_grad, A2, rho as
 * mgic_field_nl_coefs* forms them:
 *   m       = (2.0/3.0)*(K*K) - 16.0*M_PI*G*rho
 *   Ham     = m - A2*pow(psi_0,-12.0) - 16.0*M_PI*G*rho_grad*pow(psi_0,-4.0)
 *               - 8.0*lap*pow(psi_0,-5.0)
 *   Ham_abs = the sum of the absolute values of (2/3)K^2, 16 pi G rho and the
 *             three other terms of Ham (the scale a residual is judged by)
 *   Mom_i   = pow(psi_0,-6.0) * sum_j 0.5/dx*(Abar_ij(iv+e_j) - Abar_ij(iv-e_j))
 *               + 8.0*M_PI*G*Pi*(0.5/dx*(phi_0(iv+e_i) - phi_0(iv-e_i)))
 * so Ham = (2/3) K^2 - (2/3) * (mgic_field_nl_integrand*'s value).  Abar_ij
 * at the neighbouring cells is the analytic Bowen-York tensor evaluated at
 * their centres: no ghost cell is read for it, and as it is divergence-free
 * away from the punctures that term measures truncation.  psi and a stored
 * phi are read with their first ghost layer as stored (the preconditions of
 * the integrand); pi at valid cells only.  GRChombo's S_i is -Pi d_i phi: Pi
 * enters with the sign it is stored with.
 *
 * Every optional source is nullable: phi NULL, the analytic Gaussian; table
 * NULL with n = 0, the two holes of bh; pot NULL, no matter (the momentum
 * source is the literal zero, and pi must be NULL); pi NULL, Pi = 0.
 * mgic_field_constraints fills five fields on psi's layout, all required and
 * distinct from each other and from the inputs.  mgic_field_constraint_vars
 * gives Ham, Mom1, Mom2, Mom3 of planes [k0, k0 + nk) of local box `box` as
 * (4, nk, ny, nx), the layout of components 27-30 of
 * mgic_field_grchombo_vars*.  MGIC_EBADARG, before anything is launched, for
 * what the _matter forms refuse, a NULL or foreign-layout output, aliased
 * outputs and a pi without pot. */
MGIC_API int mgic_field_constraints(mgic_field psi, mgic_field phi, mgic_field ham,
                                    mgic_field mom1, mgic_field mom2, mgic_field mom3,
                                    mgic_field ham_abs, const double bh[13], int n,
                                    const double *table, mgic_field pi, const double *pot);
MGIC_API int mgic_field_constraint_vars(mgic_field psi, mgic_field phi, int box, int k0, int nk,
                                        const double bh[13], int npunct, const double *table,
                                        mgic_field pi, const double *pot, double *out,
                                        int out_on_device);
/* ---- The momentum constraint: the conformal transverse-traceless step.  The
 * total tensor is Abar_ij = Abar^BY_ij + LW_ij, with LW_ij the longitudinal
 * piece libmgic_ctt (mgic_ctt.h) forms from the solutions of
 *   Lap V_i = S_i,   S_i = -(D_j Abar^BY_ij + pow(psi_0,6.0) * 8 pi G Pi D_i phi_0)
 *   Lap U   = -(1/4) D_k V_k
 * so that D_j Abar_ij cancels the matter current.  mgic_field_momentum_source
 * writes S_1, S_2, S_3 on the valid cells of s1, s2, s3 (the launch of
 * mgic_field_constraints with the psi_0^-6 weight moved onto the source term
 * and the whole negated; pot is required, pi NULL: Pi = 0).
 *
 * The *_ctt forms are the *_matter / constraint entry points of the same name
 * with abar[6], six stored fields on psi's layout in the order 11, 12, 13,
 * 22, 23, 33, added to the Bowen-York components wherever Abar_ij is formed:
 * A2 of the coefficients, the integrand and Ham, d_j Abar_ij of Mom_i, and the
 * A11..A33 components of mgic_field_grchombo_vars_ctt.  The coefficients, the
 * integrand and the output read abar at the cell; the constraints also at
 * its six neighbours, so its ghost layer 1 must be filled.  pot and all six
 * fields are required (MGIC_EBADARG otherwise, and for a field of another
 * layout, before anything is launched); with fields of zeros they give the
 * values of the forms without abar. */
MGIC_API int mgic_field_momentum_source(mgic_field psi, mgic_field phi, mgic_field s1,
                                        mgic_field s2, mgic_field s3, const double bh[13], int n,
                                        const double *table, mgic_field pi, const double pot[3]);
MGIC_API int mgic_field_nl_coefs_ctt(mgic_field psi, mgic_field phi, mgic_field acoef,
                                     mgic_field rhs, const double bh[13], int n,
                                     const double *table, mgic_field pi, const double pot[3],
                                     const mgic_field *abar);
MGIC_API int mgic_field_nl_integrand_ctt(mgic_field psi, mgic_field phi, mgic_field out,
                                         const double bh[13], int n, const double *table,
                                         mgic_field pi, const double pot[3],
                                         const mgic_field *abar);
MGIC_API int mgic_field_grchombo_vars_ctt(mgic_field psi, mgic_field phi, int n, int k0, int nk,
                                          const double bh[13], int npunct, const double *table,
                                          mgic_field pi, const double pot[3],
                                          const mgic_field *abar, double *out,
                                          int out_on_device);
MGIC_API int mgic_field_constraints_ctt(mgic_field psi, mgic_field phi, mgic_field ham,
                                        mgic_field mom1, mgic_field mom2, mgic_field mom3,
                                        mgic_field ham_abs, const double bh[13], int n,
                                        const double *table, mgic_field pi, const double pot[3],
                                        const mgic_field *abar);
MGIC_API int mgic_field_constraint_vars_ctt(mgic_field psi, mgic_field phi, int box, int k0,
                                            int nk, const double bh[13], int npunct,
                                            const double *table, mgic_field pi,
                                            const double pot[3], const mgic_field *abar,
                                            double *out, int out_on_device);
/* the field's layout: domain, periodicity, dx, number of boxes (all ranks),
 * this rank and the job size; box i's extent, owner rank and local index
 * (-1 if not local); a barrier over the field's communicator */
MGIC_API int mgic_field_layout(mgic_field f, int domain[6], int periodic[3], double *dx, int *nbox,
                               int *rank, int *size);
MGIC_API int mgic_field_box(mgic_field f, int i, int lohi[6], int *owner, int *local_index);
MGIC_API int mgic_field_barrier(mgic_field f);
/* page-locked host memory (hipHostMalloc) for staging device output: the
 * D2H copies of mgic_field_*_vars run at full PCIe rate into it */
MGIC_API int mgic_host_alloc(size_t bytes, void **out);
MGIC_API int mgic_host_free(void *p);

/* MultilevelLinearOp::preCond: e = 0, then `iters` AMRMultiGrid iterations
 * on (e, r), homogeneous BC (Main_PoissonSolver.cpp:107-117) */
MGIC_API int mgic_mg_precondition(mgic_mg mg, mgic_field e, mgic_field r, int iters);

/* ---- the linear solve solver.solve(dpsi, rhs) (Main_PoissonSolver.cpp:
 *      103-126, 169-184): BiCGStab over the level operator, preconditioned
 *      by mgic_mg_precondition */
typedef struct {
  int num_mg_iterations; /* numMGIterations (default 1) */
  int max_iterations;    /* max_iterations -> BiCGStab m_imax (default 10) */
  double tolerance;      /* tolerance -> m_eps (default 1e-7) */
  int norm_type;         /* m_normType (0 = max norm) */
} mgic_solve_params;
MGIC_API void mgic_solve_params_default(mgic_solve_params *p);
MGIC_API int mgic_mg_solve(mgic_mg mg, mgic_field phi, mgic_field rhs, const mgic_solve_params *p,
                           int *iterations, double *final_norm);
/* the same solve over an AMR hierarchy (max_level > 0): BiCGStab over
 * mgic_amr_apply_op, preconditioned by mgic_amr_precondition */
MGIC_API int mgic_amr_solve(mgic_amr a, const mgic_field *phi, const mgic_field *rhs,
                            const mgic_solve_params *p, int *iterations, double *final_norm);

/* ---- instrumentation: hipEvents around the smoother launches on boxes of
 * at least min_cells cells (enable 1: a pair per launch; 2: a pair per run of
 * consecutive launches within one relax call -- fewer records in the timed
 * stream); launches / passes = launches timed and the colour passes they
 * performed (1 per-colour launch, 2 one fused sweep, 4 two fused sweeps) */
MGIC_API int mgic_prof_smoother(int enable, long min_cells);
MGIC_API int mgic_prof_smoother_read(int *launches, long *passes, double *total_ms);

/* ---- the launch ledger: a host-side count of launches per compiled kernel
 * instantiation.  Every instantiation the library can launch is listed from
 * load time on, at zero until it runs; a two-sweep instantiation also lists
 * the tile classes its grids contained, as "<name>#em<0|3|12|15>".  dump
 * writes one "name<TAB>count" line per entry, sorted by name; reset zeroes
 * the counts.  With MGIC_LAUNCH_LEDGER=PATH in the environment the library
 * also writes PATH.<pid> when it unloads. */
MGIC_API int mgic_launch_ledger_dump(const char *path);
MGIC_API int mgic_launch_ledger_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* MGIC_H */

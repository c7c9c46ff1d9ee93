/*
 * hmg.h -- C ABI of libhmg_hip.so: matrix-free geometric multigrid on the implicit fine grid,
 * MI355X (gfx950) native.  This is the drop-in boundary for the hot path (level L3) of
 * haampie/Homogenization.jl.  The reference has no FFI seam; its seam is Julia multiple dispatch on
 * `AbstractMatrix` level vectors (src/multigrid.jl:7-13).  Each entry point below names the reference
 * method it replaces (file:line in the reference checkout).  A Julia host binds these with `ccall`
 * (INTEGRATION.md); in this repository the executable host mirror is Python/ctypes
 * (homogenization.jl_amd/api.py).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; hmg_last_error() gives the message
 *     (thread-local).  No exception or longjmp crosses the boundary.
 *   - handles are opaque, created and destroyed by the library.  A vector keeps its grid alive and a grid its context
 *     (reference counts): the hmg_*_destroy calls may come in any order -- e.g. from the finalizers of a garbage-
 *     collected host -- and device memory goes back when the last dependant has been destroyed.
 *   - host arrays use the reference's API layout: level vectors are Nf x Ne column-major FP64 in
 *     the reference's hierarchical node order (src/multilevel_reference.jl:41-61); meshes use
 *     1-based node ids with every cell's tuple ascending (src/implicit_fine_grid.jl:14).
 *   - device work is enqueued on the context's HIP stream; calls that return a scalar to the host
 *     synchronise that stream, all others are asynchronous.
 *   - all COMPUTING calls on one context must come from one host thread at a time.  The hmg_*_destroy calls are the
 *     exception: they may come from any thread at any time (finalizers) -- reference counts, the registry of contexts
 *     and the pool of level-vector memory are guarded by a lock; the memory of a destroyed vector is reused only by
 *     work enqueued later on the context's stream.
 */
#ifndef HMG_H
#define HMG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hmg_ctx hmg_ctx;
typedef struct hmg_grid hmg_grid;
typedef struct hmg_vec hmg_vec;

const char *hmg_last_error(void);
int hmg_version(void);

/* ---- context ------------------------------------------------------------------------------ */
/* stream: a hipStream_t owned by the caller (e.g. torch's current stream) or NULL to create one. */
int hmg_ctx_create(int device, void *stream, hmg_ctx **out);
/* Always runs on the given stream handle, including the null (legacy default) stream -- the handle
 * torch.cuda.current_stream().cuda_stream returns for torch's default stream. */
int hmg_ctx_create_on_stream(int device, void *stream, hmg_ctx **out);
int hmg_ctx_destroy(hmg_ctx *ctx);
int hmg_ctx_sync(hmg_ctx *ctx);
/* Hands the blocks of destroyed level vectors that the context keeps for reuse (option "vec_pool") back to the device;
 * done automatically when an allocation of a level vector fails and when the context goes. */
int hmg_ctx_release_memory(hmg_ctx *ctx);
/* Options of hmg_ctx_set_option: name, default, what the other value changes.
 *
 * Operator apply -- performance only, the same arithmetic per node:
 *   "apply_threads" 0: workgroup size of the apply kernel chosen per level; n: n threads.
 *   "apply_wg512" 1: level-6 cells (6545 nodes, 52 KB of LDS) by 512-thread workgroups, three per CU; 0: 1024 threads, two per CU.
 *   "apply_pack" 1: 3D level-2 cells four to a wave (hmg_apply_small.hip); 0: one cell per wave, as on levels 3-4.
 *   "apply_small" 1: levels 2-4 by the pipelined one-wave kernel where the class-weight cache exists; 0: the generic kernel.
 *   "weight_cache" 1: level 6 takes its class weights from the cache hmg_grid_set_operator fills; 0: combines them per cell.
 *   "weight_cache_classes" 0: every operator of a 3D grid gets a class-weight cache, whatever the number of distinct coefficient
 *       rows (3 840 B per row and level: a field with a row per cell, such as one grain orientation per cube, costs 755 MB per
 *       level at 196 608 cells); n: only operators of at most n distinct rows (1024: the limit this library had before the
 *       option existed), the others keep the kernels that combine their weights per cell.  Read when an operator is set
 *       (hmg_grid_set_operator, hmg_grid_set_operator_tensor) and kept by the grid: hmg_grid_shrink classes the remaining cells
 *       under the limit of its operator, whatever the option says by then, and keeps the memory it has.  A cache that does not
 *       fit the device memory is left out in the same way: hmg_ctx_counter "weight_cache_classes", "weight_cache_refusals".
 *   "apply_wave" 1: level 5 (969 nodes) by one wave per cell where the cache exists and |alpha| = 1 (hmg_apply_wave.hip);
 *       0: the 256-thread kernel.  "wave_grid" 16: its persistent waves per CU; "wave_grid_total": as an absolute number.
 *   "apply_slab2" 1: cells larger than the LDS (level 7) by one persistent 1024-thread workgroup per CU, loader waves
 *       streaming the next k-plane window while evaluator waves work on the current one (hmg_apply_slab.hip); 0: the
 *       rolling-window kernel.  "slab2_grid" 0: one workgroup per CU; n: n workgroups.
 *   "restrict_slab2" 1: the stand-alone restriction of such a level goes through that kernel too; 0: the rolling-window kernel.
 *   "slab2_force" 0; 1 (experiment): level 6 through it as well -- needs HMG_SLAB_LDS_KB <= 30 when the grid is created.
 *   "cell_order" 1: full-grid apply launches of cells of >= 969 nodes walk the cells XCD by XCD; 0: in storage order.
 *
 * CG smoother and V-cycle.  The exact savings (every option below but fuse_cg) drop or fold work whose results the
 * reference's own control flow overwrites before anybody reads them: x, and r of the top level, are the same to the last
 * bit; 0 takes the plain sequence of src/multigrid.jl:46-119.
 *   "fuse_cg" 1: the p-update and both reductions ride in the apply pass; 0: one kernel per statement.  Read when a grid
 *       is created.
 *   "fold_x" 1: the pre-smoother's last x-update rides in the local residual.
 *   "lazy_dead" 1: the pre-smoother's dead last step writes nothing and both pending x-updates ride in the local residual.
 *   "lazy_pre" 1: with three steps or more the step before the dead one leaves its x-update to the local residual as well and
 *       writes its direction into the spare vector of "lazy_top" = 2 (unused during the pre-smoother): three pending updates.
 *       Taken on level 6 where that residual is the register-blocked kernel that restricts in its epilogue ("fold_restrict"),
 *       with "fold_x", "lazy_dead" and "fold_faces" on and the spare vector present; everywhere else -- level 7 (k_apply_slab2),
 *       level 5 and below (k_apply_wave, k_apply_small), 2D -- the two-update form stays.  hmg_ctx_counter "lazy_pre_form".
 *   "swap_rp" 1: CG step 0 takes r itself as p by exchanging the two handles' device pointers (an even number of times).
 *   "fold_faces" 1: the face part of A p's interface sum rides in the CG r-update.
 *   "lean_post" 1: the post-smoothers' dead tails go too: p and Ap, and r below the top level, are scratch on return (the
 *       next smoothing_steps! overwrites them before reading, src/multigrid.jl:46-50); 0: they hold what the reference leaves.
 *   "lazy_post" 1: below the top level the post-smoother's dead last step writes nothing; one pass does both x-updates.
 *   "fold_coarse_x" 1: inside hmg_vcycle the level below a level-6 top level goes further: that pass is dropped and the top level's
 *       first post-smoothing residual, which reads that x as its coarse column anyway, combines the coarse x, p and r columns where
 *       it stages them (the same three roundings per entry).  Needs "lazy_post", "fold_prolong", "prolong_in_image" and "lean_post";
 *       x of that level is then scratch on return from hmg_vcycle, like its r (nothing reads it: the next V-cycle enters the level
 *       with a zero guess).  hmg_vcycle_up takes the caller's coarse x as it is.  hmg_ctx_counter "coarse_x_folds".
 *   "lazy_top" 2: on the top level the last r-update carries the pending x-updates of the last two steps (three steps or
 *       more; the direction of the step before goes to a spare vector of the top level's size, reserved when the first
 *       vector of the finest level is created or wrapped, or by hmg_grid_reserve_spare); 1: of the last step; 0: neither.
 *   "lazy_r" 1: inside hmg_vcycle and hmg_fcg_step the top level's last launch finishes x only (40 instead of 58 B/DOF with the
 *       three-update form, 32 instead of 50 with the two-update form) and the r-update it would have carried stays PENDING on the
 *       grid: r holds r_2, Ap the unsummed A p_2 and a two-double buffer of the grid the step length.  The first call that is
 *       handed r or Ap forms r -- the very launch the eager tail makes (26 B/DOF), so r, its r.r in the scalar bank and every
 *       value derived from them are the same to the last bit -- and a call that cannot have needed it drops the record instead:
 *       the next hmg_vcycle / hmg_fcg_step on the same vectors (its first residual overwrites r), hmg_vec_copy or hmg_vec_fill over
 *       all of r, hmg_vec_destroy of r.  hmg_grid_shrink, hmg_grid_set_smoother, hmg_grid_reserve_spare(grid, 0),
 *       hmg_grid_set_exchange, hmg_grid_set_exchange_async, hmg_grid_set_cut and hmg_level_tune_placement form it first.
 *       A caller that does read r after a cycle would pay 40 + 26 B/DOF for the 58 of the eager tail, so a grid whose last record
 *       was settled by a read takes the eager tail in its next cycle and only notes whether r is read again ("lazy_r_form" 0); the
 *       first cycle whose r goes unread brings the x-only tail back.  Only a call that is handed r or Ap counts as a read, not a
 *       setter that settles the record.
 *       The hmg_*_destroy calls never launch (they may come from a finalizer's thread; the one exception is under "lazy_x"): if Ap is destroyed while r is pending,
 *       its memory stays with the grid until r has been formed or dropped (the grid itself outlives r anyway).  Until then that
 *       block is NOT in the pool of option "vec_pool": an hmg_vec_create that replaces the destroyed Ap at once allocates a new
 *       block ("device_allocs" + 1) and the device holds one more vector of that level for a while -- 10 GB at 1.3e9 entries.
 *       A host that recycles state vectors between V-cycles reads or destroys r first, or keeps Ap.
 *       Needs the "lazy_top" forms; the eager tail runs where the memory can be read behind the library's back (r, p or Ap
 *       wrapped by hmg_vec_wrap, or handed out once by hmg_vec_device_ptr), on a partitioned grid (the deferred sum over the ranks
 *       would be a collective at a place no rank can foresee) and with smoother kinds 1 and 2.  0: the eager tail always.
 *       hmg_ctx_counter "lazy_r_form", "r_materialized", "r_materialized_by_read", "r_dropped".
 *   "lazy_ap" 1: where "lazy_r" leaves the r-update of the three-update form pending (three steps or more, the spare vector
 *       reserved), the CG step in front of it does not store Ap = A p_2 either: it delivers p_2.Ap_2 for the step length (the
 *       pre-smoother's dead launch, 16 instead of 24 B/DOF, and no edge / node interface sum behind it).  That Ap had one reader,
 *       the pending r-update; a record that is dropped unread never needed it.  A record that is settled forms Ap first, by the
 *       launch the eager tail would have made (r_2, the spare vector's p_1, beta_2 from two more doubles of the grid's buffer; 24
 *       B/DOF and the interface sum), then r as above: Ap, r, the scalar bank and every value derived from them are the same to the
 *       last bit.  Three prices: r dropped unread 8 B/DOF and one interface sum less than "lazy_ap" 0; the first read of a solve
 *       16 B/DOF more (one finest-level apply); a caller that reads r after every cycle runs the eager tail from its second cycle
 *       on and pays nothing further.  Such a record also rests on the spare vector, the operator and the kernel choice, so
 *       hmg_grid_set_operator, hmg_grid_set_operator_tensor, hmg_grid_set_lambda and every hmg_ctx_set_option on the grid's
 *       context form it first as well (not a read).  The two-update form, partitioned grids and the other eager cases of
 *       "lazy_r" store Ap as before.  0: Ap is always stored.  hmg_ctx_counter "lazy_ap_form", "ap_rebuilt".
 *   "lazy_x" 1: where "lazy_r" leaves that r-update pending, hmg_vcycle does not launch the x-only tail that remained either: x
 *       lacks its last two (two-update form) or three CG updates, the grid notes on which vectors they rest (x; p_0 in p; p_1 in p
 *       or the spare vector; r_2 in r) and puts their ratios aside (eight doubles of the grid's buffer), and the NEXT hmg_vcycle on
 *       the same states forms x in the load phase of its first residual r = b - A x, which writes x and r in one pass: 56 B/DOF
 *       instead of 40 + 24 and one launch less per cycle.  The same arithmetic in the same order: x, r and every value derived
 *       from them are the same to the last bit.  Every other call that is handed x, p or r (downloads, uploads, norms, dot
 *       products, axpy, fills, samples, integrals, per-cell moments / extrema / fields, hmg_smooth, hmg_vcycle_down / _up,
 *       hmg_vcycle on another top level or other states, hmg_fcg_*), whatever forms or drops the pending r, and
 *       hmg_grid_set_operator*, hmg_grid_set_lambda, hmg_ctx_set_option, hmg_grid_shrink, hmg_grid_set_smoother,
 *       hmg_grid_reserve_spare(grid, 0), hmg_level_tune_placement and the exchange setters run the x-only tail first -- the launch
 *       that was left out, from the ratios put aside.  So does hmg_vec_destroy of p or r (the one launch a destroy makes; x
 *       destroyed or overwritten whole drops the updates).  A caller that reads x after every cycle would pay 40 + 56 B/DOF for
 *       40 + 24: the grid remembers that a call was handed x and finishes x at once in its next cycles ("lazy_x_form" 0) until a
 *       cycle's x goes unread, as "lazy_r" does for r.  hmg_fcg_step, once it has a direction, forms z = x in the pass that computes z.q
 *       (48 B/DOF instead of 40 + 16); its first step after hmg_fcg_start gets a finished x.
 *       Taken where the first residual has the streams: 3D level 6 (the 512-thread register-blocked apply; three updates with
 *       the class weights from the cache); other top levels, and the eager cases of "lazy_r" with x and p added (wrapped, handed
 *       out), keep the x-only tail.  0: always.  hmg_ctx_counter "lazy_x_form", "x_deferred", "x_settled", "x_settled_read".
 *   "fold_prolong" 1: the prolongation rides in the post-smoother's first residual.
 *   "prolong_in_image" 1: on level 6 that residual stages the coarse column at the even nodes of the LDS lattice image
 *       (three workgroups per CU stay resident); 0: in LDS of its own behind it.
 *   "fold_restrict" 1: levels 5 and 6 restrict the local residual in the kernel's epilogue and do not store it.
 *   "zero_entry" 1: a coarse level's zero initial guess is never written; its first residual is the constrained copy of b.
 *
 * Level-1 solve (hmg_coarse_last_iterations):
 *   "coarse_poly" 4: the PCG is preconditioned by that many Chebyshev iterates of the Jacobi-scaled operator; 1: plain Jacobi.
 *   "coarse_maxit" 5000, "coarse_check" 25: the checked solve's limit and the iterations between its looks at the residual.
 *   "coarse_probe" 1: a budgeted solve leaves a probe behind; 0: none (stream-capture experiments).
 *   hmg_ctx_set_option_f64: "coarse_rtol" 1e-13; "coarse_poly_ratio" 20: the preconditioner's interval is [lmax / ratio, lmax].
 *
 * Other:
 *   "vec_pool" 1: hmg_vec_destroy keeps the block for the next hmg_vec_create of the same size (re-allocating freed device
 *       memory costs ~35 ms per GB here); 0: free at once, and release what is held.
 *   "time_apply" 0: off; n: HIP-event timing of the apply launches of levels >= n (hmg_ctx_apply_timing).
 *   "overlap_min_doubles", "comm_rehearsal": multi-GPU, below.
 * Environment: HMG_SLAB_LDS_KB, the LDS window of the slab kernel for cells larger than the LDS (default 70). */
int hmg_ctx_set_option(hmg_ctx *ctx, const char *name, int64_t value);
int hmg_ctx_set_option_f64(hmg_ctx *ctx, const char *name, double value);
/* HIP-event timing of the operator-apply launches of levels >= the value given to option "time_apply"
 * (0 switches it off; setting it resets the counters).  Synchronises the stream. */
int hmg_ctx_apply_timing(hmg_ctx *ctx, int64_t *launches, double *total_ms, double *total_bytes);
/* ... the same, only the launches of one level ("time_apply" = 1 times every level). */
int hmg_ctx_apply_timing_level(hmg_ctx *ctx, int level, int64_t *launches, double *total_ms, double *total_bytes);
/* diagnostic counters: "wave_launches" (launches of the one-wave-per-cell level-5 apply, hmg_apply_wave.hip), "small_launches"
   (levels 2-4, hmg_apply_small.hip), "slab2_launches" (level 7, hmg_apply_slab.hip), "comm_calls", "comm_nranks" (ranks of the RCCL communicator made by hmg_comm_init, 0 without
   one), "device_allocs" (device / pinned allocations the library has made in this process: constant across hmg_vcycle once the
   grid, its operator, its level-1 system and the level vectors exist), "spare_bytes" (spare direction vectors held by this
   context's grids, see hmg_grid_reserve_spare), "weight_cache_classes" (coefficient rows cached by this context's grids: 0 for a
   grid whose rows outnumber option "weight_cache_classes" or whose cache did not fit the device memory), "weight_cache_bytes"
   (bytes those caches hold: rows x 2 x 240 x 8 per 3D level >= 2 when the operator is set; a domain shrink keeps them),
   "weight_cache_refusals" (operators whose cache did not fit the device memory: their grids run the kernels that combine the
   weights per cell, and table "cell_class" is empty) and "weight_cache_launches" (launches of the level-6 apply that took its
   weights from the cache), "lazy_top_form" (the form the last finest-level post-smoother inside hmg_vcycle
   took: 2 = three-update form with the spare vector, 1 = two-update form, 0 = plain), "lazy_pre_form" (the x-updates the
   last pre-smoother of the topmost down leg left to its local residual: 3 with option "lazy_pre" and the spare vector, else 2, 1 or 0), "lazy_r_form" (1: the
   last hmg_vcycle / hmg_fcg_step left its top level's r-update pending, option "lazy_r"; 0: it ran the eager tail), "r_materialized" (pending
   r-updates formed by a later call; "r_materialized_by_read": those of them formed because a call was handed r or Ap, the others
   by hmg_grid_shrink and the other setters, the placement tuner or a V-cycle on other vectors) and "r_dropped" (those that never had to be formed), "lazy_ap_form" (1: that
   pending r-update was left without a stored Ap, option "lazy_ap") and "ap_rebuilt" (pending r-updates that had to run the last CG step's apply again
   before they could be formed), "lazy_x_form" (the x-updates the last hmg_vcycle left pending on its top level's x, option "lazy_x": 3, 2 or 0), "x_deferred"
   (V-cycles that left some), "x_settled" (those of them a later call finished with the x-only tail; the others rode in the next V-cycle's first residual or
   were dropped with x) and "x_settled_read" (of those: because a call was handed x or p), "coarse_x_folds" (residuals
   that finished the coarser level's x on the way, option "fold_coarse_x": one per hmg_vcycle from level 6), "fcg_bytes" (p, q and R of this context's
   hmg_fcg objects), "smoother_diag_bytes" (inverse diagonals held by this context's grids, see hmg_grid_set_smoother) and
   "smoother_diag_builds" (times a grid of this context formed them), the "sample_*" counters listed at hmg_sample (those of
   the locator are process-wide and answered for a NULL context); -1 for an unknown name.  No counterpart in
   the reference. */
int64_t hmg_ctx_counter(hmg_ctx *ctx, const char *name);

/* ---- grid: ImplicitFineGrid(base, levels)  (src/implicit_fine_grid.jl:13-18) ------------------ */
/* Also derives ZeroDirichletConstraint(list_boundary_nodes_edges_faces(base)...)
 * (src/interface.jl:207-284, src/implicit_fine_grid.jl:80-84).
 * nlevels: 1..7 for tetrahedra, 1..11 for triangles (2D levels 9..11: cells larger than the LDS, row-band kernels). */
int hmg_grid_create(hmg_ctx *ctx, int dim, int nlevels, int64_t nnodes, const double *coords /* dim*nnodes */,
                    int64_t ncells, const int64_t *cells /* (dim+1)*ncells, 1-based */, hmg_grid **out);
int hmg_grid_destroy(hmg_grid *grid);
/* L2PlusDivAGrad(diff, mass, constraint, lambda, sigmas)  (src/build_local_operators.jl:26-32) */
int hmg_grid_set_operator(hmg_grid *grid, const double *sigma /* dim*ncells */, double lambda);
/* The same operator with a full symmetric conductivity tensor per cell (no counterpart in the reference): sigma holds
 * dim (dim + 1) / 2 numbers per cell, in the order of the coefficient row -- 3D: 11, 12, 13, 22, 23, 33; 2D: 11, 12, 22.  A
 * partitioned grid takes the GLOBAL field, like hmg_grid_set_operator.  A tensor that is not finite or not positive definite
 * (leading minors) is refused with its cell in hmg_last_error(), and the previous operator stays in force.  Everything that
 * depends on the operator takes the tensor: coefficient rows |J| J^-1 sigma J^-T, the level-1 matrix (g_i . sigma g_j),
 * hmg_rhs_axi_grad (-|J| J^-1 (sigma xi)), hmg_grid_set_lambda, hmg_grid_shrink, cell classes and the weight cache, the
 * Jacobi smoother's diagonal, hmg_fcg_*, hmg_integrate.  A field whose off-diagonal entries are all exactly zero goes through
 * the arithmetic of hmg_grid_set_operator: the same bits in every table. */
int hmg_grid_set_operator_tensor(hmg_grid *grid, const double *sigma /* ncomp*ncells */, double lambda);
int hmg_grid_set_lambda(hmg_grid *grid, double lambda);
/* Domain shrink to a prefix of cells / nodes + new Dirichlet boundary
 * (src/examples/homogenized_coefficients.jl:309-336).  Level vectors keep their storage.  On a partitioned grid
 * the prefix lengths are GLOBAL; every rank keeps its cells below the prefix (a prefix of its own columns) and the
 * cut entities, masks and ownership are re-derived. */
int hmg_grid_shrink(hmg_grid *grid, int64_t ncells_prefix, int64_t nnodes_prefix);
/* The faces on which the constraint holds (no counterpart in the reference, whose constraint is the boundary of the base mesh).
 * faces: dim node ids per face (3D: triangles, 2D: edges), 1-based ids of the base mesh, any order within a face.
 * nfaces = -1 (faces NULL): back to the default, the faces that belong to one cell.  nfaces = 0: no constraint at all.
 * The constrained set is the closure of the chosen faces: a chosen face sets its face bit in the mask of every cell that
 * contains it (one or two), each of its edges the edge bit in every cell around that edge, each of its nodes the node bit in every
 * cell around that node.  The closure alone decides: a face whose nodes are all constrained but which was not chosen stays free.
 * Tables "dmask" and "interior_nodes" and the level-1 system follow the set.  Everything is checked before anything changes: an
 * id out of range, a node twice in a face, a face that no cell has are refused, naming the first offender; duplicates are
 * accepted once.  No kernel changes and no memory is allocated: the new masks go into the buffer the kernels already read.
 * Towards what is cached the call is a new operator (hmg_grid_set_operator): a pending r-update is formed first, hmg_fcg_step
 * asks for hmg_fcg_start, the Jacobi smoother's diagonal goes stale, hmg_coarse_setup is due again; the class-weight cache is
 * kept.  A grid without a device context takes the call.  Refused: a partitioned grid, a grid that has been shrunk; and, while a
 * caller's set is held, hmg_grid_shrink (restore the default first) and, with an empty set and lambda = 0, hmg_coarse_setup (the
 * level-1 matrix is singular).  The default set named face by face is the default set, bit for bit. */
int hmg_grid_set_dirichlet_faces(hmg_grid *grid, int64_t nfaces, const int64_t *faces);
/* the current set (sorted ids within a face, faces in lexicographic order), at most cap ids into out (which may be NULL);
 * returns the number of faces, -1 for a null grid */
int64_t hmg_grid_dirichlet_faces(const hmg_grid *grid, int64_t *out, int64_t cap);
/* A grid on a torus (no counterpart in the reference): the cells name TORUS nodes -- 1-based, every tuple strictly ascending,
 * a node once per cell --, coords holds one representative position per node and period[a] > 0 is the length of the box along
 * axis a.  Periodicity is topology: every interface table is derived from the node ids alone, so opposite sides of the box are
 * shared faces like any other, no face belongs to one cell, no node is constrained (hmg_grid_dirichlet_faces returns 0) and no
 * kernel differs.  Geometry is read through one rule: a cell's vertices relative to its first vertex by the minimal image,
 *     p - p0 - period rint((p - p0) / period)   per axis.
 * Refused, naming the first offending cell, and nothing is created: an edge of a cell with an unwrapped component of
 * period / 2 or more (the image is ambiguous: fewer than three cells along that axis), a face shared by more than two cells, a
 * degenerate cell; and a period that is not positive and finite.  The grid takes hmg_grid_set_operator*, _set_lambda,
 * _set_dirichlet_faces (a plane of fixed potential inside the torus: any faces of the mesh; nfaces = -1 is the empty set here),
 * the smoothers, hmg_fcg_*, the right-hand sides, integrals and per-cell fields.  It refuses, with "periodic" in the message,
 * hmg_grid_shrink and -- until hmg_grid_set_periodic_sampling switches them on -- hmg_grid_locate, hmg_sample and
 * hmg_sample_raster; there is no partitioned form.  hmg_grid_mean_free is 1. */
int hmg_grid_create_periodic(hmg_ctx *ctx, int dim, int nlevels, int64_t nnodes, const double *coords /* dim*nnodes */,
                             int64_t ncells, const int64_t *cells /* (dim+1)*ncells, 1-based */, const double *period /* dim */,
                             hmg_grid **out);
/* The level-1 system with the constants in its kernel.  With the flag on, lambda = 0 and no constrained node, hmg_coarse_setup
 * assembles the singular matrix instead of refusing, and hmg_coarse_solve (hence every V-cycle) takes the plain mean over the
 * level-1 nodes out of its right-hand side before the PCG -- the matrix's range is the complement of the constants -- and out of
 * its solution after it: on the device, in the stream, in a fixed order of additions (the same bits in every run), inside the
 * budget / probe scheme as it stands; the stopping rule is coarse_rtol of the projected right-hand side.  The finer levels need
 * nothing: the smoothers add residual-derived directions only, and the constants of a level are the prolongation of those of
 * level 1.  A solution is then fixed up to a constant; gradients, fluxes and energies do not depend on it.  With lambda > 0 or
 * a constrained node the matrix is regular and the flag changes nothing.  Default: 0 on grids of hmg_grid_create* (whose refusal
 * of the singular matrix stays), 1 on periodic grids.  Towards what is cached the call is hmg_grid_set_dirichlet_faces: pending
 * records are settled, the level-1 system is assembled again, hmg_fcg_step asks for hmg_fcg_start. */
int hmg_grid_set_mean_free(hmg_grid *grid, int on);
int hmg_grid_mean_free(const hmg_grid *grid);   /* 0 / 1; -1 for a null grid */
/* The reference's LevelState holds five vectors per level (src/multigrid.jl:18-25).  With option "lazy_top" = 2 (the default) the
 * finest level's post-smoother inside hmg_vcycle uses a SIXTH vector of that level's size (+20 % on the finest level's footprint)
 * to save 8 B/DOF of traffic per V-cycle.  It belongs to the grid and is setup, not hot-path, memory: reserved automatically when
 * the first vector of the finest level is created or wrapped (if that allocation fails, V-cycles silently-but-reportedly take the
 * two-update form: hmg_ctx_counter "lazy_top_form" / "spare_bytes"), or explicitly here: enable = 1 reserves it now and FAILS if
 * the memory is not there; enable = 0 releases it and keeps it released (the five-vector footprint of the reference). */
int hmg_grid_reserve_spare(hmg_grid *grid, int enable);
/* The smoother of hmg_smooth, hmg_vcycle*, hmg_fcg_*: kind 0 = the reference's CG (src/multigrid.jl:46-71, the default), kind 1 = CG
 * preconditioned by the inverse of the assembled operator's diagonal (no counterpart in the reference):
 *     dinv = 0 on constrained nodes, else 1 / (interface sum of the cell-local diagonal of lambda M + K_sigma)
 *     r = b - A x, constraint, interface sum;  z = dinv o r;  p = z;  rz = dot(r, z)
 *     steps x { Ap = A p, constraint, interface sum;  alpha = rz / dot(p, Ap);  x += alpha p;  r -= alpha Ap;
 *               rz' = dot(r, dinv o r);  p = dinv o r + (rz'/rz) p;  rz = rz' }
 * (dot over the raw storage, copies counted, as hmg_vec_dot).  The V-cycle around it is unchanged.  On a checkerboard of contrast
 * 100 it needs a fraction of the cycles of kind 0 at about 1.5 times the traffic per cycle.
 * Kind 1 reserves one vector per level >= 2 (setup memory, hmg_ctx_counter "smoother_diag_bytes") and FAILS if the memory is not
 * there; kind 0 releases them.  The diagonals go stale with hmg_grid_set_operator, hmg_grid_set_lambda, hmg_grid_shrink,
 * hmg_grid_set_smoother and a change of cut or exchange, and are formed again (kernels only, no allocation) at the next
 * hmg_smooth / hmg_vcycle* / hmg_fcg_start / hmg_fcg_step / hmg_grid_smoother_diag, before that call's first launch -- on a
 * partitioned grid with five cut exchanges per level (the diagonal is summed in fixed point, limb by limb: the same bits whatever the
 * partition), so all ranks make that call together; a level is formed by the first such call that smooths on it.  Changing the smoother counts as a new
 * operator for an hmg_fcg object (hmg_fcg_step then asks for hmg_fcg_start).  A grid without a device context is refused. */
int hmg_grid_set_smoother(hmg_grid *grid, int kind);
int hmg_grid_smoother(const hmg_grid *grid);           /* the kind; -1 for a null grid */
/* out = dinv of the level (2..nlevels), formed first if it is stale; kinds 1 and 2 */
int hmg_grid_smoother_diag(hmg_grid *grid, int level, hmg_vec *out);
/* Kind 2, the Chebyshev-Jacobi smoother: a Chebyshev polynomial in dinv o A on [lambda_lo, lambda_hi], lambda_lo = lambda_hi / ratio,
 * with kind 1's dinv.  No dot product, so no reduction and no sum over ranks inside a smoothing; a fixed linear operator.
 *     theta = (hi + lo) / 2;  delta = (hi - lo) / 2;  sigma1 = theta / delta;  rho_0 = 1 / sigma1
 *     r = b - A x, constraint, interface sum;  d = (1 / theta) dinv o r
 *     steps x { x += d;  Ad = A d, constraint, interface sum;  r -= Ad;
 *               rho_{k+1} = 1 / (2 sigma1 - rho_k);  d = (rho_{k+1} rho_k) d + (2 rho_{k+1} / delta) dinv o r }
 * hmg_smooth leaves the next d in p and A d in Ap.  Inside a V-cycle a smoother whose x alone is read ends with x += d and launches no
 * apply for its last step: `steps` steps cost steps - 1 applies behind the first residual (hmg_ctx_counter "cheb_applies" counts
 * them, "cheb_smoothings" the smoothings of at least one step).
 * lambda_hi of a level must be an upper bound of the largest eigenvalue of dinv o A on the free nodes; an estimate that falls short
 * makes the V-cycle diverge.  Where none is given the library forms, with dinv and stale with it,
 *     lambda_hi = 1.02 * max over free slots i of dinv_i * (interface sum of s_i),   s_i = the absolute row sum of the cell's own
 *                 lambda M + K_sigma at slot i
 * which is at least 1.02 times the Gershgorin bound of the assembled matrix on the free rows (|sum_c a^c_ij| <= sum_c |a^c_ij|), hence an
 * upper bound of the largest eigenvalue.  It has no ceiling of its own: with the default Dirichlet set it stayed below 1.02 (dim + 1) on
 * every mesh tried, but with the constraint lifted (hmg_grid_set_dirichlet_faces, nfaces = 0) a 2D grid of 8 perturbed cells, sigma in
 * {1, 100}, gives 6.39 > 3.06.  It depends on the operator, on lambda, on the domain and on the Dirichlet set (constrained rows leave the
 * maximum) and is formed again after a change of any of them.  A level without a free entry has the maximum 0 and is refused ("the bound
 * of this level is not a positive number"), as is one whose operator holds a NaN or an infinity (the maximum keeps a NaN).  One more
 * kernel, interface sum and maximum per level, and one host read (hmg_ctx_counter "smoother_bound_builds" counts the levels formed).
 * ratio <= 0: the default, 30; otherwise it must be finite and > 1.  lambda_hi: NULL, or nlevels entries,
 * entry l - 1 for level l; an entry > 0 is used as given (no factor, nothing formed), an entry <= 0 asks for the formed bound.
 * A partitioned grid, or one with an interface exchange, is accepted only with entries > 0 for every level >= 2 (the maximum over the
 * ranks would need a hook the exchange does not have); without them the call fails and changes nothing.
 * Memory, staleness, hmg_fcg objects, pending updates and hmg_grid_set_smoother(grid, 0 | 1) afterwards: as for kind 1. */
int hmg_grid_set_smoother_chebyshev(hmg_grid *grid, double ratio, const double *lambda_hi);
/* lambda_lo and lambda_hi of a level (2..nlevels) as kind 2 uses them; forms dinv and the bound first if they are stale (scratch
 * from the context's pool) and synchronises the stream: not for the inside of a V-cycle.  Either pointer may be NULL. */
int hmg_grid_smoother_bounds(hmg_grid *grid, int level, double *lambda_lo, double *lambda_hi);
int64_t hmg_grid_ncells(const hmg_grid *grid);
int64_t hmg_grid_nnodes(const hmg_grid *grid);
int hmg_grid_nlevels(const hmg_grid *grid);
int64_t hmg_grid_nf(const hmg_grid *grid, int level);   /* nnodes(refined_mesh(implicit, level)) */
int64_t hmg_grid_ld(const hmg_grid *grid, int level);   /* device column stride in doubles */
/* Table export for tests / host mirrors. which: "hier2slot" (int32[nf]), "slot_ijk" (int32[3*nf]),
 * "slot_cls" (int32[nf]), "par_a","par_b" (int32[nf]), "ctab" (f64), "dmask","dupmask" (int32[ncells]),
 * "interior_nodes" (int32, 0-based), "coef" (f64[8*ncells]), "cell_class" (int32[ncells]: the cell's class in the class-weight
 * cache, on a host-only grid too; count 0 when the operator has no class table).  Returns the element count via *count. */
int hmg_grid_table_i32(const hmg_grid *grid, int level, const char *which, int32_t *out, int64_t cap, int64_t *count);
int hmg_grid_table_f64(const hmg_grid *grid, int level, const char *which, double *out, int64_t cap, int64_t *count);

/* ---- level vectors: the five matrices of LevelState (src/multigrid.jl:7-25) ------------------- */
int hmg_vec_create(hmg_grid *grid, int level, hmg_vec **out);                 /* zeros(Nf, Ne) */
/* device_ptr must be 16-byte aligned -- the vector kernels move pairs of doubles --; any other pointer is refused. */
int hmg_vec_wrap(hmg_grid *grid, int level, void *device_ptr, hmg_vec **out); /* caller-owned ld*Ne doubles */
int hmg_vec_destroy(hmg_vec *v);
/* The device pointer of the vector.  From this call on the library assumes that the memory is read behind its back: a pending
 * r-update on the vector (option "lazy_r") is formed now, and V-cycles that use the vector as r, p or Ap take the eager tail. */
void *hmg_vec_device_ptr(hmg_vec *v);
int hmg_vec_upload(hmg_vec *v, const double *host);      /* Nf x Ne, hierarchical order */
int hmg_vec_download(hmg_vec *v, double *host);
int hmg_vec_fill(hmg_vec *v, double value);                                   /* fill!           */
int hmg_vec_fill_random(hmg_vec *v, uint64_t seed, int64_t cell_offset);      /* rand! (seeded)  */
int hmg_vec_copy(hmg_vec *dst, hmg_vec *src);                                 /* copyto!         */
int hmg_vec_axpy(double alpha, hmg_vec *x, hmg_vec *y);                       /* axpy!  multigrid.jl:65-66 */
int hmg_vec_xpby(hmg_vec *r, double beta, hmg_vec *p);                        /* p .= r .+ beta.*p  :68   */
int hmg_vec_dot(hmg_vec *x, hmg_vec *y, double *out);    /* dot over raw storage, copies counted  :54 */
int hmg_vec_norm_unique(hmg_vec *r, double *out);        /* norm after zero_out_all_but_one!, r kept */

/* ---- hot-path primitives -------------------------------------------------------------------- */
/* mul!(alpha, base, A::L2PlusDivAGrad, x, y): y += alpha*A*x   (src/apply_local_operators.jl:85-133) */
int hmg_apply(hmg_grid *grid, int level, double alpha, hmg_vec *x, hmg_vec *y);
/* general form behind mul!/local_residual!/the smoother's Ap = A*p: out = (src ? src : 0) + alpha*A*x, then
 * (constrain != 0) apply_constraint!(out).  src may be NULL or alias out. */
int hmg_apply_ex(hmg_grid *grid, int level, double alpha, hmg_vec *x, hmg_vec *src, hmg_vec *out, int constrain);
/* local_residual!: r = b - A*x, then constraint            (src/apply_local_operators.jl:18-27) */
int hmg_residual(hmg_grid *grid, int level, hmg_vec *x, hmg_vec *b, hmg_vec *r);
/* apply_constraint!                                          (src/implicit_fine_grid.jl:94-139) */
int hmg_constraint(hmg_grid *grid, int level, hmg_vec *x);
/* broadcast_interfaces!                                      (src/implicit_fine_grid.jl:209-328) */
int hmg_interface_sum(hmg_grid *grid, int level, hmg_vec *x);
/* zero_out_all_but_one!                                      (src/implicit_fine_grid.jl:334-386) */
int hmg_zero_duplicates(hmg_grid *grid, int level, hmg_vec *x);
/* restrict_to!(b_coarse, P, r_fine) / interpolate_and_sum_to!(x_fine, P, x_coarse), P = interops[level_fine-1]
 *                                                            (src/interpolation.jl:52-74) */
int hmg_restrict(hmg_grid *grid, int level_fine, hmg_vec *r_fine, hmg_vec *b_coarse);
int hmg_prolong_add(hmg_grid *grid, int level_fine, hmg_vec *x_coarse, hmg_vec *x_fine);
/* copy_to_base! / distribute!                                (src/implicit_fine_grid.jl:148-202) */
int hmg_gather_base(hmg_grid *grid, hmg_vec *v1, double *host_u /* nnodes */);
int hmg_scatter_base(hmg_grid *grid, const double *host_u, hmg_vec *v1);

/* ---- driver right-hand sides (run once per outer step) --------------------------------- */
/* rhs_a xi grad v!(b, dphis, implicit, sigmas, xi)   (src/examples/homogenized_coefficients.jl:449-474) */
int hmg_rhs_axi_grad(hmg_grid *grid, const double *xi /* dim */, hmg_vec *b);
/* local_rhs!(b, implicit): b[:, e] = |det J_e| * int phi over the refined reference cell (unit load;
 * src/implicit_fine_grid.jl:391-409, used by checkerboard_hypercube_multigrid, ...homogenized_coefficients.jl:543) */
int hmg_local_rhs(hmg_grid *grid, hmg_vec *b);
/* The driver integrals over the first ncells_subset cells (src/examples/homogenized_coefficients.jl:592-689); M is the level's
 * reference mass matrix, |J_c| the cell's Jacobian determinant, all sums run over the cells c < ncells_subset and the nodes i:
 *
 *   mode  value                                  second                                          reference
 *   0     sum |J_c| v_i (second_i + (M v)_i)     rhs_a xi grad v! for the same xi (*)            integrate_first_term
 *   1     sum |J_c| (v_i + second_i) (M v)_i     the previous iterate v_{k-1}                    integrate_terms
 *   2     sum |J_c| 1' M 1                       unused (v names the level)                      integrate_area
 *   3     sum |J_c| second_i (M v)_i             another corrector; may be v itself              none: mass pairing Mq(v; second)
 *   4     sum |J_c| v_i second_i                 a load vector such as hmg_rhs_axi_grad's        none: load pairing Lq(v; second)
 *
 * (*) hmg_rhs_axi_grad: the reference recomputes dot(dphi_i, P) per node, :621 -- it is that vector entry.
 * So mode 0 = mode 4 + mode 3 with second = v, and mode 1 = mode 3 (v, v) + mode 3 (v, second); modes 3 and 4 are the bilinear
 * forms in two different correctors that the off-diagonal entries of the homogenized tensor need.  Modes 0 and 1 refuse
 * second = v; modes 3 and 4 write nothing and accept it.  Modes 0, 1 and 3 are one 16 B/DOF pass of the operator-apply kernel in
 * reductions-only form, on every level the apply supports; mode 4 is one streaming pass of 16 B/DOF.  None allocates, and the
 * partial sums are folded in a fixed order: the same bits in every run.  ncells_subset = 0 gives 0; any other mode is an error.
 * Partitioned grid: local cells, this rank's share (the host adds the shares). */
int hmg_integrate(hmg_grid *grid, int mode, hmg_vec *v, hmg_vec *second, int64_t ncells_subset, const double *xi,
                  double *out);
/* next_rhs!(b, x, implicit, ops): b = lambda*|J|*M*x  (src/examples/homogenized_coefficients.jl:695-713) */
int hmg_next_rhs(hmg_grid *grid, hmg_vec *x, hmg_vec *b);

/* ---- per-cell gradient moments (no counterpart in the reference) ---------------------------------------------------
 * For every coarse cell c of the grid's current cells (the prefix after hmg_grid_shrink; the local cells of a partitioned grid,
 * nothing is exchanged) the mean gradient and the Gram tensor of the gradient of the level vector v -- or, with xi, of
 * u = xi . x + v:
 *     m(c) = (1/|c|) int_c grad u            G(c) = int_c grad u (x) grad u
 * out[c * nmom ..]: m (dim numbers), then G in the order 11, 12, 13, 22, 23, 33 (2D: 11, 12, 22); nmom = hmg_cell_moments_count =
 * dim + dim (dim + 1) / 2, i.e. 5 in 2D and 9 in 3D.  From these: the mean flux sigma_c m(c) and the flux form of a row of the
 * homogenized tensor, sum_c |c| sigma_c m(c) / |Omega|; the dissipated energy sigma_c : G(c); field moments per phase; and, for
 * the plain Dirichlet cell problem (lambda = 0), the sensitivity d(energy)/d(sigma_c) = G_u(c).
 * The moments are of the vector AS STORED: no operator, no lambda, no Dirichlet mask enters (v should be consistent: every copy
 * of a shared node the same value).  One kernel of its own reads the column once (8 B/DOF) and writes 72 B (2D: 40 B) of
 * reference sums per cell; the host applies the cell's J^-1 and |J|.  The sums are folded in a fixed order: the same bits in every run.
 * It allocates (from the context's pool of level-vector memory) and synchronises: not for the inside of a V-cycle.
 * On a partitioned grid c runs over the LOCAL cells (ascending global ids, the grid's "part_cells"; after a shrink those below the
 * global prefix): out has one row per local cell, and so has every per-cell array the calls of this family take (the form of
 * hmg_cell_extrema) -- whereas hmg_grid_set_operator / hmg_grid_set_operator_tensor take the GLOBAL field.  The rows equal the
 * unpartitioned grid's rows of those cells bit for bit.
 * Served: every level whose cell fits the LDS with its tables -- 3D levels 1 to 6, 2D levels 1 to 8 (level 1: the cell itself, one
 * element).  Larger cells (3D level 7, 2D levels 9-11) are refused with a message naming the level, unless hmg_ctx_set_option "cell_moments_windows" is 1: then such
 * a cell walks through a rolling window of the LDS, as in the operator apply of those levels (slabs of k-planes in 3D, bands of
 * lattice rows in 2D; the pair kernel with v given twice: 8 B/DOF, the same rules, the same bits in every run).  Value 2 sends
 * every level the window kernels can address through them (3D levels 6 and 7, 2D levels from 2: a test and A/B knob); 0 is the
 * default.  hmg_ctx_counter "cell_moments_window_launches" counts their launches, "cell_moments_windows" reads the option back.
 * Refused too: a grid without a device context, a vector of another grid and a null out. */
int hmg_cell_moments(hmg_grid *grid, hmg_vec *v, const double *xi /* dim, or NULL */, double *out /* host, nmom*ncells */);
int hmg_cell_moments_count(const hmg_grid *grid);        /* dim + dim (dim + 1) / 2; works on a host-only grid; -1: null grid */
/* The bilinear counterpart for TWO vectors v, w of one level and grid: per coarse cell the symmetrised cross moment of their
 * gradients -- or, with xi_v / xi_w (each may be NULL, meaning 0), of u = xi_v . x + v and z = xi_w . x + w:
 *     S(c) = 1/2 int_c (grad u (x) grad z + grad z (x) grad u)
 *          = S_vw(c) + |c| sym(xi_v (x) xi_w + xi_v (x) m_w + m_v (x) xi_w),     sym(A) = (A + A^T) / 2, m the mean gradients
 * out[c * nq ..]: S in the order 11, 12, 13, 22, 23, 33 (2D: 11, 12, 22); nq = hmg_cell_pair_moments_count = dim (dim + 1) / 2.
 * Only the symmetric part is defined (the class table stores its off-diagonal stiffness terms symmetrised, and sigma : S with
 * a symmetric sigma needs no more).  S of (v, v) is G of hmg_cell_moments (to rounding; bit for bit only where both calls take the
 * window kernels, which are one kernel and one host transform).  With d correctors
 * u_k = e_k . x + v_k of the plain Dirichlet cell problem: Sigma_kl |Omega| = sum_c sigma_c : S_{u_k u_l}(c), its per-cell
 * energy density, and d(Sigma_kl |Omega|)/d(sigma_c) = S_{u_k u_l}(c).
 * One kernel of its own: only w goes into the LDS image, v is read per node straight from its column -- 16 B/DOF read, 96 B
 * (2D: 56 B) of reference sums written per cell.  w may be v.  Otherwise the rules of hmg_cell_moments: the vectors as stored,
 * the current cells, local cells of a partitioned grid, a fixed summation order (the same bits in every run), allocation from
 * the pool and a synchronisation; the same levels served (3D 1 to 6, 2D 1 to 8) and refused (naming the level), and the same
 * option "cell_moments_windows" for larger cells (only w goes into the window; v is read per node, or from the window's centre
 * tap where v and w are one vector); refused too:
 * a grid without a device context, a null vector or out, a vector of another grid, v and w of different levels. */
int hmg_cell_pair_moments(hmg_grid *grid, hmg_vec *v, hmg_vec *w, const double *xi_v /* dim, or NULL */,
                          const double *xi_w /* dim, or NULL */, double *out /* host, nq*ncells */);
int hmg_cell_pair_moments_count(const hmg_grid *grid);   /* dim (dim + 1) / 2; works on a host-only grid; -1: null grid */

/* ---- per-cell extrema over the fine elements (no counterpart in the reference) ----------------------------------------
 * The per-cell moments above are integrals; this is the pass over the FINE ELEMENTS of every coarse cell.  For every current coarse
 * cell c and every fine element T of it (2^(dim (level-1)) of them, hmg_grid_fine_elements; the P1 gradient is constant on each)
 *     q_T = grad u|_T . Q_c grad u|_T,     u = xi . x + v   (xi = NULL means 0)
 * with a symmetric Q_c per cell in physical coordinates: form[c * nq ..] in the order of hmg_grid_set_operator_tensor (3D 11, 12,
 * 13, 22, 23, 33; 2D 11, 12, 22), any finite symmetric matrix, definite or not; form = NULL means the identity, q = |grad u|^2.
 * Q = sigma_c gives the energy density, Q = sigma_c^T sigma_c the squared flux.
 * out[c * (2 + nthr) ..]: max_T q_T, min_T q_T, then for each j < nthr the number of elements with q_T > thresholds[j], written
 * as a double (an exact integer).  0 <= nthr <= 8; the thresholds are finite and the same for all cells.
 * One kernel of its own reads the column once (8 B/DOF) and one byte of element mask per node; the host folds the cell's J, Q_c
 * and xi into one row of 9 (2D: 5) numbers per cell.  Maxima, minima and integer counts do not depend on any order: the same
 * bits in every run and for every launch shape.
 * Otherwise the rules of hmg_cell_moments: the vector as stored (no operator, no lambda, no mask), the current cells after a
 * shrink, the local cells of a partitioned grid with nothing exchanged; it allocates from the pool (the level's element mask once,
 * at the first call on that level) and synchronises.  hmg_ctx_counter "cell_extrema_kernel_ns": the last call's kernel time.
 * On a partitioned grid form and out are indexed by LOCAL cell (form[c * nq ..] belongs to the c-th local cell: hand in the rows
 * of the global field at the grid's "part_cells"), unlike the sigma of hmg_grid_set_operator*, which is the global field.
 * NaN: max_T q_T and min_T q_T of a cell are NaN exactly when q_T is NaN on some fine element of THAT cell (a NaN entry of the
 * cell's column makes it so on every element that touches the node; so does inf - inf); other cells are not touched.  An
 * infinite q_T is a value like any other: it may be the maximum or the minimum.  The counts keep their meaning: q_T > threshold
 * is false for a NaN, so a NaN element is counted nowhere.  (The moment calls propagate a NaN through their sums.)
 * Served: 3D levels 1 to 6, 2D levels 1 to 8 (level 1: one element per cell, max = min).  Larger cells (3D level 7, 2D levels
 * 9-11) are refused with a message naming the level, unless hmg_ctx_set_option "cell_extrema_windows" is 1: then such a level
 * walks through a rolling window of the LDS (slabs of planes in 3D, bands of lattice rows in 2D; the same 8 B/DOF, the same
 * mask, rows and results).  2 sends every level the window kernels address through them (3D levels 6 and 7, 2D levels 2 to 11):
 * a test and A/B knob -- both kernels evaluate a node with one function, so the bits are those of the default path.  0 is the
 * default; "cell_moments_windows" has no say here.  hmg_ctx_counter "cell_extrema_window_launches" counts the window launches,
 * "cell_extrema_windows" reads the option back.
 * Refused as well, with a message naming the call: a grid without a device context, a null v or out, a vector of another grid,
 * nthr outside 0..8, nthr > 0 with null thresholds, thresholds or form entries that are not finite. */
int hmg_cell_extrema(hmg_grid *grid, hmg_vec *v, const double *xi /* dim, or NULL */,
                     const double *form /* nq*ncells, or NULL */, int nthr, const double *thresholds /* nthr, or NULL */,
                     double *out /* host, (2 + nthr)*ncells */);
int64_t hmg_grid_fine_elements(const hmg_grid *grid, int level);   /* 2^(dim (level-1)); host-only grid too; -1: null grid or bad level */

/* ---- ... and WHERE: the fine elements that hold the maximum and the minimum ---------------------------------------------
 * hmg_cell_extrema_where is hmg_cell_extrema with one more result.  out is what hmg_cell_extrema writes for the same arguments,
 * bit for bit: the values come from the same evaluation and are picked by the same comparisons, whatever the locations are.
 * where[c * 2 (dim + 1) ..]: the dim + 1 vertices of the element that attains max_T q_T of cell c, then the dim + 1 vertices of
 * the element that attains min_T q_T.  Vertices are 0-based HIERARCHICAL node ids -- rows of hmg_vec_download's matrix, the
 * convention of hmg_grid_locate's nodes -- in the element's own order p, p + pi1, p + pi1 + pi2, p + s (2D: p, p + pi1, p + s): p
 * the lexicographically lowest vertex in the lattice coordinates "slot_ijk", pi the permutation of the lattice basis a, b, c
 * ("elem_dirs") that the element's bit k of "elem_mask" names, s = a + b + c.  3D k = 0 .. 5: (a,b,c), (a,c,b), (b,a,c), (b,c,a),
 * (c,a,b), (c,b,a); 2D k = 0, 1: (a,b), (b,a).
 * Ties: elements tie when their values are equal (==: +0 and -0 tie, and then out may carry the sign of another element of the
 * tie than the one reported, as hmg_cell_extrema's does).  Among tied elements the one with the LOWEST CODE slot(p) * 8 + k is
 * reported, slot(p) the storage slot of p (table "hier2slot").  The rule refers to nothing but the values and the grid's tables:
 * the same ints for every launch shape, number of cells, kernel family ("cell_extrema_windows") and run.
 * NaN: a cell whose extrema are NaN (the rule of hmg_cell_extrema) has -1 in all 2 (dim + 1) entries; other cells are not
 * touched.  An infinite q_T is a value like any other and has a location.  Level 1: one element per cell, both locations are it.
 * The same single pass: 8 B/DOF and one launch, the codes ride next to the running extrema in registers and through the folds;
 * 8 bytes more per cell come back, and the host turns the codes into vertices with hmg_grid_element_vertices' decode.
 * Served and refused exactly as hmg_cell_extrema -- the option "cell_extrema_windows" (3D level 7, 2D levels 9-11), partitioned
 * grids (local cells, where indexed by local cell), shrunk grids (current cells), every argument check, in messages that name
 * this call -- and a null where is refused too.  hmg_ctx_counter "cell_extrema_where_launches" counts its launches (a window
 * launch counts in "cell_extrema_window_launches" as well), "cell_extrema_where_kernel_ns" is the last call's kernel time;
 * "cell_extrema_kernel_ns" stays that of the last hmg_cell_extrema.
 *
 * hmg_grid_element_vertices: n codes slot * 8 + k of `level` -> nodes[(dim + 1) * n], the vertices as above.  Host tables only: it
 * works on a grid without a device context.  A code whose slot is out of range (negative codes too) or whose bit k of the slot's
 * mask is clear is refused with a message naming the first such code; nothing is promised about nodes then.  n = 0: success. */
int hmg_cell_extrema_where(hmg_grid *grid, hmg_vec *v, const double *xi /* dim, or NULL */,
                           const double *form /* nq*ncells, or NULL */, int nthr, const double *thresholds /* nthr, or NULL */,
                           double *out /* host, (2 + nthr)*ncells */, int32_t *where /* host, 2*(dim+1)*ncells */);
int hmg_grid_element_vertices(const hmg_grid *grid, int level, int64_t n, const int32_t *codes /* n */,
                              int32_t *nodes /* (dim+1)*n: 0-based HIERARCHICAL row ids */);

/* ---- per-cell histograms over the fine elements (no counterpart in the reference) ---------------------------------------
 * How q_T of hmg_cell_extrema is DISTRIBUTED over the fine elements of every coarse cell: counts per bin, one pass, no threshold
 * to guess.
 * The binning rule.  Bins are floating-point buckets: emin < emax (integers, -1022 <= emin, emax <= 1023) and sub_bits s in
 * 0..5 give nreg = (emax - emin) 2^s regular bins with the edges
 *     E_i = 2^(emin + i div 2^s) (1 + (i mod 2^s) / 2^s),     i = 0 .. nreg          (every edge an exact double)
 * and nbins = nreg + 3:  bin(q) = the number of edges <= q (numpy: searchsorted(E, q, side = "right")) for every q that is no
 * NaN -- bin 0 holds everything below 2^emin (zeros of either sign, negatives, -inf, denormals), bin b = 1..nreg is
 * [E_(b-1), E_b), bin nreg + 1 holds q >= 2^emax (+inf included) -- and a NaN of either sign goes to bin nreg + 2.  The bin is
 * found by integer arithmetic on the double's high word (positive doubles order like their bit patterns): no logarithm, no
 * rounding, one text for host and device.
 * hmg_histogram_nbins: nreg + 3, or -1 (hmg_last_error set) for parameters outside the rule.  hmg_histogram_edges: the nreg + 1
 * edges.  hmg_histogram_bin: the rule's host twin, bins[i] = bin(q[i]) for n values; no grid needed.  All three refuse parameters
 * outside the rule with a message that names the call and the parameter: sub_bits outside 0..5, emin or emax outside
 * -1022..1023, emin >= emax.  These three serve every rule, up to (-1022, 1023, 5); hmg_cell_histogram keeps a cell's histogram
 * in LDS and serves nreg <= 1024 (nbins <= 1027).
 *
 * hmg_cell_histogram: counts[c * nbins + b] = the number of fine elements T of the current coarse cell c with bin(q_T) = b.
 * q_T, xi, form and the row of 9 (2D: 5) numbers per cell are exactly hmg_cell_extrema's -- the same host function folds the
 * rows, the kernel evaluates a node with the same expressions: the values are hmg_cell_extrema's bit for bit, so the number of
 * elements at or above an edge E equals hmg_cell_extrema's count for the threshold nextafter(E, -inf).  Every existing fine
 * element is counted exactly once: a row sums to hmg_grid_fine_elements, and the NaN bin counts the elements hmg_cell_extrema
 * would turn into NaN extrema.
 * One kernel of its own reads the column once (8 B/DOF) and one byte of element mask per node; the histogram of a cell sits in
 * LDS behind the lattice image, is written with LDS integer adds and flushed as one row of nbins 32-bit counts.  No global atomics
 * and no floating-point sums: the same ints in every run and for every launch shape.
 * Otherwise the rules of hmg_cell_extrema: the vector as stored, the current cells after a shrink, the local cells of a
 * partitioned grid with nothing exchanged (form and counts indexed by LOCAL cell), periodic grids served; it allocates from the
 * pool (rows, nbins * ncells 32-bit counts; the level's element mask once) and synchronises.  hmg_ctx_counter
 * "cell_histogram_launches" counts the kernel launches, "cell_histogram_kernel_ns" is the last call's kernel time.
 * Served: 3D levels 1 to 6, 2D levels 1 to 8 -- the levels whose cell fits the LDS together with the largest histogram.  Larger
 * cells (3D level 7, 2D levels 9-11) are refused with a message naming the call and the level, whatever "cell_extrema_windows"
 * says, unless hmg_ctx_set_option "cell_histogram_windows" -- an option of this call's own, 0 by default -- is 1: then such a
 * level walks through a rolling window of the LDS ([window | nbins counters]; slabs of planes in 3D, bands of rows in 2D, one
 * workgroup per cell), each node evaluated and counted with the functions the other kernel calls: the same ints.  2 sends every
 * level the window kernels address through them (3D levels with slab tables, 2D levels 2 and up); the message of the refusal names
 * the option where it would help.  "cell_histogram_window_launches" counts the launches of the window kernels (they count in
 * "cell_histogram_launches" too), "cell_histogram_windows" reads the option back.  Partitioned, shrunk and periodic grids are
 * served as by hmg_cell_extrema with its window option.
 * Refused as well, with a message naming the call: a grid without a device context, a null v or counts, a vector of another grid,
 * bin parameters outside the rule (as above) or more than 1024 regular bins, xi or form entries that are not finite.
 * hmg_ctx_set_option "cell_histogram_variant" (0, 1 = default, 2) chooses how a workgroup brings its counts into LDS -- one add
 * per element, a node's elements combined in registers first, and on top of that the wave's first bin summed across its lanes: a
 * measurement knob, the counts are the same ints from each.  The window kernels have the second form alone; the option has no
 * say there.
 *
 * hmg_cell_histogram_groups: the same pass -- the same checks, kernel choice, options and counters -- whose per-cell rows stay on
 * the device, where a second kernel sums them over groups of cells; ngroups * nbins numbers come down instead of ncells * nbins.
 *   group_of_cell  int32[ncells], values in -1 .. ngroups - 1; -1: the cell is in no group (current / local cells, as counts above)
 *   weights        double[ncells], finite, or NULL
 *   counts         int64[ngroups * nbins], row per group: counts[g * nbins + b] = the sum over the cells c of group g of
 *                  hmg_cell_histogram's counts[c * nbins + b], in 64-bit integers
 *   volume         double[ngroups * nbins], NULL exactly when weights is NULL: volume[g * nbins + b] = sum_c weights[c] *
 *                  counts[c * nbins + b]
 * THE ORDER OF THE FP64 SUM is part of the interface: per (g, b) the cells of group g are taken by ASCENDING CELL ID, s = 0.0,
 * then s = fl(s + fl(weights[c] * (double)count_c)) cell after cell -- product and sum rounded separately, never a fused
 * multiply-add --, cells with a zero count included.  (numpy: s = 0.0; for c in sorted cells: s = s + w[c] * float(n[c, b]).)
 * Independent of launch shape, device and run: the same bits everywhere.  An empty group gives rows of zeros.  No global atomics.
 * Refused before any device work, each with a message naming the call and what failed: ngroups < 1 (or above 65535), a null
 * counts, weights without volume or volume without weights, a null group_of_cell, a group id outside -1 .. ngroups - 1 (the cell
 * is named), a weight that is not finite (the cell is named); then everything hmg_cell_histogram refuses.
 * hmg_ctx_counter "cell_histogram_groups_kernel_ns" is the group-sum kernel's time in the last call; "cell_histogram_kernel_ns"
 * and the launch counters behave as for hmg_cell_histogram. */
int64_t hmg_histogram_nbins(int emin, int emax, int sub_bits);
int hmg_histogram_edges(int emin, int emax, int sub_bits, double *edges /* nreg + 1 */);
int hmg_histogram_bin(int64_t n, const double *q /* n */, int emin, int emax, int sub_bits, int32_t *bins /* n */);
int hmg_cell_histogram(hmg_grid *grid, hmg_vec *v, const double *xi /* dim, or NULL */,
                       const double *form /* nq*ncells, or NULL */, int emin, int emax, int sub_bits,
                       int64_t *counts /* host, nbins*ncells, row per cell */);
int hmg_cell_histogram_groups(hmg_grid *grid, hmg_vec *v, const double *xi /* dim, or NULL */,
                              const double *form /* nq*ncells, or NULL */, int emin, int emax, int sub_bits, int ngroups,
                              const int32_t *group_of_cell /* ncells */, const double *weights /* ncells, or NULL */,
                              int64_t *counts /* host, nbins*ngroups, row per group */,
                              double *volume /* host, nbins*ngroups, or NULL with weights */);

/* ---- sampling a level vector at points and on raster slices (no counterpart in the reference) --------------------------
 * For a point x of physical space, a level and a level vector v of that level, as stored (no interface sum, no mask):
 *   cell      the current coarse cell (the prefix after hmg_grid_shrink) that contains x: all barycentric coordinates of x in it
 *             are >= -tau, tau = 2^-40 in reference coordinates; among several (faces, edges, nodes of the base mesh) the LOWEST
 *             cell id.  No such cell, or a coordinate that is not finite: cell = -1 and every other output of the point is NaN.
 *   value     xi . x + sum_k w_k v[slot_k, cell] over the dim + 1 vertices of ONE fine element of the level that contains x, w_k
 *             its P1 (barycentric) weights there: >= 0 (the slack is clamped away) and summing to 1 within rounding.
 *   gradient  xi + the gradient of the P1 interpolant on that element (constant per element), dim numbers.
 * xi = NULL means 0.  The element: with t = 2^(level-1) x^ (x^ the reference coordinates of x in the cell, negative ones set to 0)
 * and Y = (t_i + t_j + t_k, t_i + t_j, t_i) (2D: (t_i + t_j, t_i)), clamped from the left to m >= Y_0 >= Y_1 >= Y_2, take
 * P_a = min(floor(Y_a), m - 1) and f_a = Y_a - P_a in [0, 1]; the vertices are P, P + e_p1, P + e_p1 + e_p2, P + (1, 1, 1) in
 * that basis, p the order of f descending, EQUAL f IN ASCENDING a.  This rule names an element of the cell for every point of the
 * closed cell (a point on a fine face, edge or node takes the element the rule gives, always the same one); the weights are
 * 1 - f_p1, f_p1 - f_p2, f_p2 - f_p3, f_p3.
 * A vertex whose weight is exactly 0 is not read for the value -- a NaN elsewhere in the column stays out of it --, and
 * hmg_grid_locate reports the element's first vertex in its place.  The gradient belongs to the whole element and reads all its
 * vertices (only when it is asked for).  No reductions, no atomics: the same bits in every run and for every launch shape.
 *
 * hmg_grid_locate runs on the host (a grid without a context too): per point the cell, the dim + 1 vertices as 0-based
 * HIERARCHICAL node ids -- rows of hmg_vec_download's matrix: value = sum_k weights[k] x_host[nodes[k], cell] --, the weights,
 * and, where gweights is not NULL, the vectors g_k (dim each, vertex-major) with gradient = sum_k v_k g_k over the element's own
 * vertices (nodes[] names them wherever all weights are positive).  Points without a cell: nodes -1, weights and gweights NaN.
 * hmg_sample uploads the points, runs one kernel (one thread per point) and downloads what was asked for; each of values
 * (npoints), gradients (dim per point) and cell (npoints) may be NULL, not all three.  hmg_sample_raster forms the points on the
 * device, x(a, b) = fma(b, dv, fma(a, du, origin)) per component for 0 <= a < nu, 0 <= b < nv; outputs at index b * nu + a.
 * device_column is the base address of a level vector of `level` (hmg_vec_device_ptr): it must be device memory with
 * ld(level) * ncells doubles from it inside ONE allocation, or the call is refused before anything is launched (a wrong level
 * or a pointer into the middle of a vector is a message, never a fault).  The calls take no hmg_vec: hmg_vec_device_ptr settles a
 * pending r-update of that vector and marks it exposed, so sampling a grid's r, p or Ap keeps the eager tail of hmg_vcycle for
 * that vector from then on; sampling x, which is what drivers do, changes nothing.
 * The locator (a uniform bin grid over the bounding box of the current cells; per bin the cells that may meet it, ascending) is
 * built at the first of these calls and again after hmg_grid_shrink; its device copy (setup memory, one allocation, plus one
 * lattice table per 3D level used) at the first device call.  Points and results take one block of the context's pool of
 * level-vector memory; the calls synchronise.  Any simplicial base mesh; 3D levels 1-7, 2D levels 1-11.
 * hmg_ctx_counter: "sample_launches", "sample_kernel_ns" and "sample_download_ns" (the last call's kernel, by device events, and
 * its downloads, by the host clock) per context; "sample_locator_builds", "sample_locator_bytes" and
 * "sample_locator_max_candidates" (the longest list of a bin) count locators built in this process and describe the last one:
 * process-wide like "device_allocs" and, unlike every other counter ("device_allocs" too), answered for a NULL context as well --
 * a grid without a context has a locator and nothing else to ask.
 * A raster of any shape up to 2^31 - 1 pixels is one launch: a workgroup takes 16 x 16 pixels, on a raster thinner than 16 pixels
 * one way a tile as thin as the raster (a line of pixels: 256 x 1).
 * Refused with a message, nothing launched and nothing changed: a partitioned grid; a periodic grid on which
 * hmg_grid_set_periodic_sampling has not switched sampling on; a level out of range; null points / origin /
 * du / dv; npoints or nu * nv above 2^31 - 1 or negative (0: success, nothing written); all outputs NULL; and, for the two
 * device calls, a grid without a context or a column that fails the check above. */
/* Sampling on a periodic grid, switched on per grid (default 0: the three calls below refuse a periodic grid).  With it on:
 *   box       the torus is looked at through the box [0, period[a]) per axis, fixed by the period alone -- not by where the
 *             node representatives are stored; a mesh whose nodes are moved by whole periods gives the same bits.
 *   cell      a point is taken modulo the period; whether it lies in a cell is asked of the MINIMAL IMAGE of x - X0 (X0 the
 *             cell's first vertex), d - period rint(d / period) per axis, with the cell's edges unwrapped by the same rule.
 *             Every finite point has a cell; ties go to the lowest cell id, as everywhere.
 *   value     xi . x is taken at the CALLER'S point, not the reduced one: u = xi . x + v grows across periods while v
 *             repeats, and a raster over several periods tiles.  The gradient is periodic.
 * The call launches nothing, touches no vector and no pending record, and drops the locator (the next call that is served
 * builds it).  A grid without a context takes it (hmg_grid_locate is then what it serves).  Refused: a grid that is not
 * periodic; on other than 0 and 1. */
int hmg_grid_set_periodic_sampling(hmg_grid *grid, int on);
int hmg_grid_periodic_sampling(hmg_grid *grid, int *on);
int hmg_grid_locate(hmg_grid *grid, int level, int64_t npoints, const double *points /* point-major, dim each */,
                    int32_t *cell /* npoints */, int32_t *nodes /* (dim+1) per point: 0-based HIERARCHICAL row ids */,
                    double *weights /* (dim+1) per point */, double *gweights /* dim*(dim+1) per point, or NULL */);
int hmg_sample(hmg_grid *grid, int level, const void *device_column /* base of a level vector: ld*Ne doubles */,
               const double *xi /* dim, or NULL */, int64_t npoints, const double *points /* host */,
               double *values, double *gradients, int32_t *cell /* host; each may be NULL */);
int hmg_sample_raster(hmg_grid *grid, int level, const void *device_column, const double *xi,
                      const double *origin, const double *du, const double *dv /* dim each */, int64_t nu, int64_t nv,
                      double *values, double *gradients, int32_t *cell /* nu*nv, index b*nu + a */);

/* ---- fused fast path ------------------------------------------------------------------------ */
/* smoothing_steps!(steps, implicit, ops, curr, k)            (src/multigrid.jl:46-71) */
int hmg_smooth(hmg_grid *grid, int level, int steps, hmg_vec *x, hmg_vec *b, hmg_vec *r, hmg_vec *p, hmg_vec *Ap);
/* Optional, at setup: choose by measurement which memory block plays which role.  `states` as for hmg_vcycle (5 handles
 * per level, level-major); the five hmg_vec_create'd vectors x, b, r, p, Ap of `level` >= 2 (LevelState,
 * src/multigrid.jl:7-25) are tuned, those of level - 1 serve as the coarse side; operator set.  The passes that stream
 * five or six finest-level vectors at once run up to 8 % slower or faster depending on where the blocks lie in HBM
 * relative to each other -- a property of the physical pages, not of anything an address shows --
 * so the library times this level's share of a V-cycle (hmg_vcycle_down + hmg_vcycle_up with `steps` smoothing steps)
 * for `trials` assignments of the five blocks plus `extra` freshly allocated ones to the five roles, keeps the fastest
 * (the handles' device pointers are exchanged; pointers obtained from hmg_vec_device_ptr before are stale), frees the
 * blocks left over and zero-fills the vectors of both levels: CALL IT BEFORE THE VECTORS HOLD DATA.  ms_out (may be
 * NULL): [0] time of the assignment the handles came with, [1] of the one they leave with.  Costs (trials + 3) x that
 * share of a V-cycle; on a partitioned grid every rank must call it with the same arguments. */
int hmg_level_tune_placement(hmg_grid *grid, int level, int steps, hmg_vec **states, int extra, int trials, double *ms_out);
/* Coarse operator for the current sigma/lambda/boundary: replaces
 * cholesky(assemble_checkerboard(base, cond, lambda)[interior, interior])
 * (src/examples/homogenized_coefficients.jl:259-261) by a device-resident CG, preconditioned by Chebyshev iterates of the Jacobi-scaled operator (option "coarse_poly"; 1 = plain Jacobi-PCG). */
int hmg_coarse_setup(hmg_grid *grid);
/* level-1 branch of vcycle!                                  (src/multigrid.jl:74-93) */
int hmg_coarse_solve(hmg_grid *grid, hmg_vec *b1, hmg_vec *x1);
/* Iterations of the last level-1 solve; blocks until its probe has landed.  -1 (hmg_last_error set): that solve did not
 * reach coarse_rtol.  How a solve is policed: the first solve on a new matrix (operator, lambda or domain changed) looks at
 * its residual every "coarse_check" iterations and fails with an error after "coarse_maxit"; later solves enqueue
 * 1.25 x the largest count seen + 4 iterations (plain Jacobi, "coarse_poly" = 1: 1.5 x + 16) without a host round trip
 * and leave a probe behind, which is judged by the next call that synchronises the stream anyway (hmg_vec_norm_unique,
 * hmg_vec_dot, hmg_integrate, hmg_ctx_sync, this function) or by the next solve: an unconverged solve is an ERROR of that call (the V-cycle that used it was inexact),
 * the budget is dropped, and repeating the V-cycle solves the slow, checked way.  The reference's CHOLMOD solve
 * (src/multigrid.jl:84) cannot fail this way; the error keeps that contract visible. */
int hmg_coarse_last_iterations(const hmg_grid *grid);
int64_t hmg_coarse_misses(const hmg_grid *grid);   /* budgeted solves that ran out of iterations so far */
/* vcycle!(implicit, base, ops, levels, k, steps); coarser levels use steps_coarse (the reference
 * does not forward `steps`, src/multigrid.jl:109, so pass 2 for parity).
 * states: 5*nlevels handles ordered level-major as x,b,r,p,Ap of level 1, then level 2, ...
 * On return x of the top level is finished.  Its r is what the reference leaves to every call of this ABI, but with option
 * "lazy_r" (the default) it is formed by the first call that is handed r or Ap: that first read costs one pass of 26 B/DOF,
 * which a run of V-cycles never pays.  p and Ap of the top level are scratch ("lean_post"). */
int hmg_vcycle(hmg_grid *grid, int top_level, int steps, int steps_coarse, hmg_vec **states);
/* The two halves of one level of vcycle! (same `states` layout; only levels `level` and `level - 1` are touched):
 *   down  smoothing_steps!, local_residual!, restrict_to!(next.b, P, curr.r), fill!(next.x, 0)   (src/multigrid.jl:100-106)
 *   up    interpolate_and_sum_to!(curr.x, P, next.x), smoothing_steps!                          (src/multigrid.jl:112-115)
 * hmg_vcycle(k) == down(k); hmg_vcycle(k-1); up(k).  After `down`, x, r (the cell-local residual) and the coarse b
 * hold what the reference leaves; p and Ap are scratch (the library drops the pre-smoother's dead tail).  After `up`,
 * x and r hold what the reference leaves; p and Ap too with option "lean_post" = 0 (see above; `up` acts as the top
 * level of a V-cycle).  With
 * option "swap_rp" each half exchanges the device pointers of the r and p handles once: call them in pairs when
 * r / p wrap caller-owned memory. */
int hmg_vcycle_down(hmg_grid *grid, int level, int steps, hmg_vec **states);
int hmg_vcycle_up(hmg_grid *grid, int level, int steps, hmg_vec **states);

/* ---- V-cycle-preconditioned flexible CG --------------------------------------------------------------
 * Repeating hmg_vcycle is a stationary iteration.  These calls use the same V-cycle as the preconditioner of a flexible
 * conjugate gradient iteration with one retained direction (Notay's FCG(1): the CG smoother makes the V-cycle a slightly
 * non-linear operator, for which the plain PCG recurrence is the wrong one).  No counterpart in the reference.
 *
 *   start   R = b - A_loc x, Dirichlet rows zeroed
 *   step    z = hmg_vcycle on the top level with right-hand side R and a zero initial guess
 *           first step p = z; later beta = -(z.q) / (p.q)_prev, p = z + beta p
 *           q = A_loc p, Dirichlet rows zeroed;  alpha = (p.R) / (p.q);  x += alpha p;  R -= alpha q
 *
 * x, z, p are consistent vectors (all copies of a shared node equal), b, R, q are loads (the copies add up to the global
 * value; A_loc is hmg_apply_ex with constrain = 1, which does no interface sum), so the plain dot products over the
 * storage are the global inner products: the outer iteration has no interface sum and no cut exchange of its own.  On a
 * partitioned grid a step adds two sums over the ranks (z.q; p.q and p.R together) through the grid's scalar_sum hook / the
 * in-library communicator.  alpha and beta are formed on the device: a step enqueues work and returns.
 *
 * The object (an opaque handle, passed as void *) is bound to a grid and a top level and owns p, q and R: three vectors of
 * the top level's size from the context's pool of level-vector memory, allocated by hmg_fcg_create -- setup memory,
 * hmg_ctx_counter "device_allocs" does not move in start / step; their size is counter "fcg_bytes".  A create that does not
 * get the memory fails.  `states` as for hmg_vcycle; the top level's x receives z, its r, p, Ap are scratch, its b is not
 * touched (R takes its place inside the V-cycle, by handle).  x is a vector of the caller's that is none of the top level's
 * five; x must be consistent and constrained (hmg_interface_sum / hmg_constraint) when hmg_fcg_start is called.
 * After hmg_grid_shrink, hmg_grid_set_lambda or hmg_grid_set_operator the residual belongs to the old operator:
 * hmg_fcg_start must be called again, hmg_fcg_step and hmg_fcg_residual_norm fail until it has been.
 * A budgeted level-1 solve that misses its tolerance is reported as for hmg_vcycle (hmg_coarse_last_iterations): by the
 * next synchronising call; the step remains a valid, weaker iterate. */
int hmg_fcg_create(hmg_grid *grid, int top_level, int steps, int steps_coarse, void **out);
int hmg_fcg_destroy(void *fcg);
int hmg_fcg_start(void *fcg, hmg_vec *x, hmg_vec *b, hmg_vec **states);
int hmg_fcg_step(void *fcg, hmg_vec *x, hmg_vec **states);
/* first-copy norm of the interface-summed R (the true residual norm), through the top level's r.  Synchronises. */
int hmg_fcg_residual_norm(void *fcg, hmg_vec **states, double *norm);
/* out[0..4) = alpha, beta, p.q, p.R of the last step (beta = 0 in the first step after a start).  Synchronises. */
int hmg_fcg_scalars(void *fcg, double *out);
/* which: 0 p, 1 q, 2 R -- owned by the object, valid until hmg_fcg_destroy; NULL for anything else */
hmg_vec *hmg_fcg_vec(void *fcg, int which);

/* ---- multi-GPU hooks (one process per GPU; the host layer owns the communicator) ------------------
 * The grid of a rank holds the cells that rank owns.  Entities shared with other ranks are listed by
 * hmg_grid_set_cut(): per cut entity a global cut id and the local first copy.  After the local
 * interface sum the library packs one value per cut DOF into the exchange buffer, calls `exchange`
 * (an in-place sum over ranks, e.g. RCCL allreduce issued by the host on the same stream) and writes
 * the result back to every local copy.  `scalar_sum` does the same for `count` device doubles
 * (the CG dot products). */
typedef int (*hmg_exchange_fn)(void *user, void *device_buf, int64_t count);
int hmg_grid_set_cut(hmg_grid *grid, int64_t ncut_global_faces, int64_t ncut_global_edges, int64_t ncut_global_nodes,
                     int64_t nlocal_faces, const int64_t *face_gid, const int32_t *face_cell_lid,
                     int64_t nlocal_edges, const int64_t *edge_gid, const int32_t *edge_cell_lid,
                     int64_t nlocal_nodes, const int64_t *node_gid, const int32_t *node_cell_lid);
int hmg_grid_set_exchange(hmg_grid *grid, hmg_exchange_fn exchange, hmg_exchange_fn scalar_sum, void *user,
                          void *device_exchange_buf, int64_t exchange_buf_doubles);
/* Asynchronous form of the exchange: begin() starts the in-place sum over ranks of device_buf[0..count) and
 * returns, end() makes the context's stream wait for it.  With it the smoother overlaps the exchange with the
 * apply / interface sums of the cells that do not touch a partition cut (hmg_grid_set_overlap, default on). */
int hmg_grid_set_exchange_async(hmg_grid *grid, hmg_exchange_fn begin, int (*end)(void *user));
int hmg_grid_set_overlap(hmg_grid *grid, int enabled);
/* (context option "overlap_min_doubles", default 524288: levels whose GLOBAL cut -- one value per cut DOF, the same number
 *  on every rank, so that all ranks decide alike and issue their collectives in one order -- is smaller than 4 MiB run in
 *  the plain form even with the overlap on: splitting the launches of a launch-bound small level costs more than its
 *  messages hide) */
/* Exchange among the sharers only (SURVEY 8e's cheaper alternative; the default of hmg_grid_use_comm).  The library groups
 * the cut entities into SEGMENTS by the set of ranks that share them (octants: a quarter of a cut plane = 2 ranks, half an
 * axis line = 4, the centre node = 8), lays this rank's segments out one after the other in the exchange buffer (a segment
 * has the same length and order on each of its members) and, per exchange, hands the transport a list of messages
 * msgs[4 i ..] = {peer rank, buffer offset, count, staging offset} (doubles): send device_buf[offset .. +count) to the
 * peer, receive the peer's partial segment into device_stage[staging offset .. +count).  Two ranks list the segments they
 * share in the same order, so the k-th message a -> b meets the k-th b <- a.  The library then adds the members' partials
 * in ascending rank order (identical bits on every member).  p2p runs on the context's stream; p2p_begin only starts the
 * messages and the `end` of hmg_grid_set_exchange_async joins them.  enabled = 0: back to the all-reduce over the global
 * cut buffer.  hmg_grid_set_exchange still supplies user, the exchange buffer, scalar_sum and `exchange` (level-1 gather). */
typedef int (*hmg_p2p_fn)(void *user, void *device_buf, void *device_stage, int64_t nmsgs, const int64_t *msgs);
int hmg_grid_set_exchange_p2p(hmg_grid *grid, int enabled, hmg_p2p_fn p2p, hmg_p2p_fn p2p_begin, void *device_stage_buf,
                              int64_t stage_buf_doubles);
int64_t hmg_grid_cut_stage_doubles(const hmg_grid *grid);          /* staging capacity needed (max over levels) */
/* the message list of one level: 4 int64 per message (count = numbers written) */
int hmg_grid_exchange_messages(const hmg_grid *grid, int level, int64_t *out, int64_t cap, int64_t *count);
/* level = 0: capacity needed for every level and for the coarse gather */
int64_t hmg_grid_cut_buffer_doubles(const hmg_grid *grid, int level);
void *hmg_ctx_scalar_bank(hmg_ctx *ctx);
/* device_doubles16 = NULL restores the library's own bank (call it before the caller-owned memory goes away) */
int hmg_ctx_set_scalar_bank(hmg_ctx *ctx, void *device_doubles16);
/* the context's HIP stream (a hipStream_t): a host layer that issues its own collectives must issue them here */
void *hmg_ctx_stream(hmg_ctx *ctx);

/* ---- in-library communicator: RCCL over xGMI, one rank per GPU ------------------------------------------------------
 * The reference's exchange point is broadcast_interfaces! (src/implicit_fine_grid.jl:209-328; called at
 * src/multigrid.jl:51,61,75) plus the three dot products of a CG step (src/multigrid.jl:54,64,67).  With a communicator
 * the library does them itself: ncclAllReduce of the packed cut buffer (on a second HIP stream, event-ordered, when the
 * overlap is on) and of the CG scalars (two neighbouring slots of the scalar bank at CG step 0: one call), all enqueued
 * on streams -- no host code runs between two kernels of a V-cycle.  Usage: rank 0 calls hmg_comm_unique_id and hands
 * the 128 bytes to every rank (any channel: MPI, a file, torch.distributed), every rank calls hmg_comm_init on its
 * context, creates its grid with hmg_grid_create_partition and calls hmg_grid_use_comm.  librccl is opened at run time
 * (dlopen), so single-GPU use does not need it. */
#define HMG_COMM_ID_BYTES 128
int hmg_comm_unique_id(void *out128);
int hmg_comm_init(hmg_ctx *ctx, int nranks, int rank, const void *unique_id128);
int hmg_comm_destroy(hmg_ctx *ctx);
int hmg_comm_stats(hmg_ctx *ctx, int64_t *calls, int64_t *doubles);   /* collectives issued so far, doubles moved */
int hmg_grid_use_comm(hmg_grid *grid);
/* sum over ranks of `count` (<= 4) host doubles, in place, blocking: the driver's per-cycle integrals */
int hmg_comm_sum_host(hmg_ctx *ctx, double *vals, int count);
/* Grid of the cells owner[c] == rank of a global base mesh.  The library derives the local mesh, the cut
 * entities (global ids identical on all ranks), global multiplicities and Dirichlet / first-copy masks, and
 * keeps the global mesh for a replicated level-1 solve.  hmg_grid_set_operator takes the GLOBAL sigma.
 * hmg_grid_set_cut is called internally; the host only supplies hmg_grid_set_exchange. */
int hmg_grid_create_partition(hmg_ctx *ctx, int dim, int nlevels, int64_t nnodes, const double *coords, int64_t ncells,
                              const int64_t *cells, const int32_t *owner, int rank, int nranks, hmg_grid **out);
/* Rehearsal of a larger partition on fewer GPUs (measurement / test aid, not a production entry point).
 * cut_owner[c] decides which entities count as cut (their copies' cells differ in cut_owner) while owner[] still decides
 * which cells are local: owner = 0 everywhere, cut_owner = the octant of a cell and a 1-rank communicator walk the
 * cut-first cell lists, pack / unpack kernels, events and the all-reduce of an 8-rank partition with every copy held
 * locally -- results equal the unpartitioned grid's bit for bit.  cut_owner = NULL: as hmg_grid_create_partition.
 * Context option "comm_rehearsal" = 1 lets a grid that holds rank r's share of an N-rank partition use a communicator
 * of another size (timing only: the neighbours' contributions are missing from the sums). */
int hmg_grid_create_partition_rehearsal(hmg_ctx *ctx, int dim, int nlevels, int64_t nnodes, const double *coords,
                                        int64_t ncells, const int64_t *cells, const int32_t *owner, const int32_t *cut_owner,
                                        int rank, int nranks, hmg_grid **out);

/* ---- host-side problem synthesis (threaded; HMG_SETUP_THREADS, default: all cores up to 16) -------------------------
 * hypercube(ElT, n; origin) + order_nodes_and_elements_by_magnitude (src/tet/generate_grid.jl:6-45,
 * src/tri/generate_grid.jl:6-35, src/examples/homogenized_coefficients.jl:21-28) in one call: a box of shape[] unit
 * cubes (6 tetrahedra / 2 triangles each), node ids with the last coordinate fastest.  transposed_lookup = 1 reproduces
 * the reference's corner lookup (first-index-fastest id table, cubes only: the geometry comes out transposed, as in
 * the reference); 0 keeps node id and coordinates aligned (boxes for multi-GPU weak scaling).  ordered = 1 sorts nodes
 * and cells by infinity norm (stable) so that every centred sub-box is a prefix.  cells: 1-based ascending tuples. */
int hmg_checkerboard_mesh_size(int dim, const int64_t *shape, int64_t *nnodes, int64_t *ncells);
int hmg_checkerboard_mesh(int dim, const int64_t *shape, const double *origin, int transposed_lookup, int ordered,
                          double *coords /* dim*nnodes */, int64_t *cells /* (dim+1)*ncells */);
/* shape[] unit cubes on a torus (for hmg_grid_create_periodic with period = shape), the same split into 6 tetrahedra / 2
 * triangles: node ids with the last coordinate fastest, taken modulo shape, nodes at their multi-index; cube q (first index
 * slowest) owns cells 6q .. 6q + 5 (2D: 2q, 2q + 1) in the order of hmg_checkerboard_mesh, so a per-cube conductivity maps to
 * cells without any coordinate; every tuple sorted ascending, 1-based.  shape[a] >= 3. */
int hmg_periodic_mesh_size(int dim, const int64_t *shape, int64_t *nnodes, int64_t *ncells);
int hmg_periodic_mesh(int dim, const int64_t *shape, double *coords /* dim*nnodes */, int64_t *cells /* (dim+1)*ncells */);
/* conductivity_per_element(mesh, sigma, offset) (src/examples/homogenized_coefficients.jl:494-503): sigma[c] =
 * sigma_grid[trunc(centre_c + offset) - 1]; sigma_grid: grid_shape[0] x .. x grid_shape[dim-1] x dim, C order */
int hmg_conductivity_per_element(int dim, int64_t nnodes, const double *coords, int64_t ncells, const int64_t *cells,
                                 const int64_t *grid_shape, const double *sigma_grid, const double *offset, double *sigma);

/* owner[c] = row-major index of the width^dim block (blocks[] of them per axis, counted from origin) that holds the
 * centre of cell c -- the ownership partition of the multi-GPU runs (halves / quadrants / octants about the origin) */
int hmg_block_owner(int dim, int64_t nnodes, const double *coords, int64_t ncells, const int64_t *cells,
                    const int64_t *blocks, double width, const double *origin, int32_t *owner);

#ifdef __cplusplus
}
#endif
#endif /* HMG_H */

// What the host modules of libhmg_hip.so share: the objects behind the handles of include/hmg.h and the functions that cross
// a module boundary, each declared once.  Internal: only .cpp files include it (no kernel file does).
//
//   hmg_context.cpp  lifetimes of contexts, grids and vectors, device memory and the level-vector pool, options, counters
//   hmg_upload.cpp   grid creation: kernel tables to the device (or, on a host-only grid, into the checksum), operator, queries
//   hmg_smooth.cpp   operator apply with its sums, the three smoothers, V-cycle, placement tuner
//   hmg_pending.cpp  the records of a V-cycle's last r-update and x-updates left pending: opened, settled, carried, dropped
//   hmg_coarse.cpp   level-1 system, its PCG and the probes budgeted solves leave behind
//   hmg_comm.cpp     cut exchange, the RCCL communicator and the exchange settings of a grid
//   hmg_fcg.cpp      flexible CG around the V-cycle
//   hmg_fields.cpp   per-cell gradient moments of a level vector and of a pair of them, through the LDS-resident or the window kernels
//   hmg_extrema.cpp  fine-element table of a level; per-cell extrema and exceedance counts of a quadratic form of the gradient
//   hmg_histogram.cpp  the binning rule's host twin; per-cell histograms of that form over the fine elements
//   hmg_sample.cpp   locator of the current cells; a level vector's value, gradient and cell at points and on raster slices
//   hmg_capi.cpp     vector operations, primitives, right-hand sides, integrals: argument checks and one call each
//
// Every extern "C" entry point lives in the module it fronts; hmg_capi.cpp keeps those that front none.
#pragma once

#include "../../include/hmg.h"
#include "hmg_device.hpp"
#include "hmg_host.hpp"

#include <atomic>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

struct ncclComm;        // (<rccl/rccl.h> is hmg_comm.cpp's alone)

using namespace hmg;    // (as every host module does)

#define HIPCHK(expr)                                                                            \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess)                                                                   \
            throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(_e) + " (" #expr ")"); \
    } while (0)

namespace hmg {

// Handles may be destroyed from another thread than the one that computes (finalizers of a garbage-collected host: Julia
// runs them where it likes, Python's weakref.finalize on the collecting thread): reference counts, the registry of live
// contexts and the pooled level-vector blocks are guarded by this lock.  (Recursive: a failed allocation inside a guarded
// region hands the pools back.)  Everything else on one context is for one host thread at a time (include/hmg.h).
std::recursive_mutex &lifetime_mutex();
using LifetimeLock = std::lock_guard<std::recursive_mutex>;

// Device / pinned allocations the library has made so far (hmg_ctx_counter "device_allocs"): after setup -- grid, operator, level-1
// system, level vectors -- a V-cycle makes none (tests/test_gpu_parity.py::test_no_allocation_inside_a_vcycle).
std::atomic<int64_t> &device_allocs();

// hipMalloc; when it fails, every live context hands its pooled level-vector blocks back (they may be what is in the way) and
// it is tried once more.  Counts the allocation; on failure *p stays null and the second attempt's error is returned -- the
// caller says what could not be had.
hipError_t device_malloc(void **p, size_t bytes);

// Host-only grids (hmg_grid_create with a NULL context: table queries, and the CPU sanitizer job of tests/test_sanitizers.py)
// run every table builder as a device grid does; inside a DryUploads scope the uploads keep a running checksum of what WOULD have
// gone to the device instead of touching the HIP runtime (hmg_grid_table_i32 "upload_hash": the same mesh must give the same
// tables whatever the allocator hands out -- an uninitialised read shows up as a checksum that moves with ASan's malloc fill).
struct DryUploads {
    static DryUploads *&current()
    {
        static thread_local DryUploads *c = nullptr;
        return c;
    }
    bool dry;
    uint64_t *hash;
    DryUploads *prev;
    DryUploads(bool dry_, uint64_t *hash_) : dry(dry_), hash(hash_), prev(current()) { current() = this; }
    ~DryUploads() { current() = prev; }
    DryUploads(const DryUploads &) = delete;
    DryUploads &operator=(const DryUploads &) = delete;
    static bool active() { return current() && current()->dry; }
    static void note(const void *data, size_t bytes)
    {
        uint64_t h = *current()->hash ^ (bytes * 0x9e3779b97f4a7c15ull);
        const unsigned char *b = (const unsigned char *)data;
        for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 1099511628211ull;
        *current()->hash = h;
    }
};

template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    void alloc(size_t count)
    {
        release();
        n = count;
        if (!count || DryUploads::active()) return;
        HIPCHK(device_malloc((void **)&p, count * sizeof(T)));
    }
    void upload(const std::vector<T> &h, hipStream_t s)
    {
        alloc(h.size());
        if (DryUploads::active()) {
            DryUploads::note(h.data(), h.size() * sizeof(T));
            return;
        }
        if (!h.empty()) {
            HIPCHK(hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s));
            HIPCHK(hipStreamSynchronize(s));
        }
    }
};

struct LevelBufs {
    DevBuf<uint64_t> meta;
    DevBuf<uint16_t> lpos, sweep_slot;
    DevBuf<int> slab_head, slab_rs_head;
    DevBuf<uint32_t> slab_ld_word, slab_cp_word, slab_rs_word;
    DevBuf<uint16_t> slab_cp_slot, slab_rs_slot;
    DevBuf<double> rtab;   // restriction weights in class-table layout (slab levels)
    int nslab = 0, slab_lds_nodes = 0, slab_max_surf = 0, slab_rs_max_surf = 0, slab_max_int = 0, slab_rs_max_int = 0;
    DevBuf<uint32_t> pos32, pos32w, sweep32, par32, blk_word;
    DevBuf<uint64_t> par64;
    DevBuf<uint16_t> clpos;
    DevBuf<uint32_t> rs_word;
    DevBuf<double> rs_w;
    DevBuf<uint16_t> rs_lp;
    DevBuf<uint16_t> blk_slot;
    // one-wave-per-cell apply of level 5 (k_apply_wave): per-lane tables + the class-weight cache of the current operator
    DevBuf<uint32_t> wave_tab, wave_lpos, wave_par, wave_cl, wave_rs;
    DevBuf<double> wcache;
    DevBuf<double> ctab;
    DevBuf<int32_t> hier2slot, par_a, par_b, rptr, ridx;
    DevBuf<double> dphi;
};

struct CutKind {
    int64_t nglobal = 0;
    int64_t nentries = 0;
    std::vector<int64_t> gid;                    // host: global cut id of every local copy
    std::vector<int32_t> seg;                    // host: segment / index inside it (sharers-only exchange), may be empty
    std::vector<int64_t> sidx;
    DevBuf<int32_t> cell_lid;
    DevBuf<uint8_t> first;
};

// Exchange-buffer layout of one level (built at the first exchange on that level).
//   global layout (all-reduce over every rank): [faces | edges | nodes], a run per GLOBAL cut id -- identical on all ranks;
//   segment layout (exchange among the sharers only): this rank's segments one after the other, inside a segment faces,
//   edges, nodes -- a segment has the same length and order on each of its members.
struct CutLevel {
    bool ready = false;
    DevBuf<int64_t> pos[3];                      // per local cut copy: first buffer position of its run
    int64_t ndoubles = 0;                        // buffer positions used on this level
    // segment layout only:
    std::vector<int64_t> ops;                    // messages, 4 numbers each: peer rank, buffer offset, count, stage offset
    int64_t nstage = 0;                          // staging doubles (the peers' partial segments land there)
    DevBuf<int64_t> plan;                        // k_seg_sum: nseg, then per segment off, size, nmembers, mtab offset; then mtab
};

struct ApplyTimer {
    bool on = false;
    int min_level = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    std::vector<int> ev_level;          // per used event pair: the level of the launch and its algorithmic bytes
    std::vector<double> ev_bytes;
    size_t used = 0;
};

// Field state of a grid (hmg_extrema.cpp): per level the fine-element table, built and checked at grid creation on the host, and
// its device copy, uploaded by the first hmg_cell_extrema on that level -- outside LevelDev, a kernel argument of its own, and
// outside the checksum of a host-only grid (the tables of the operator's kernels are what that pins).
struct FieldState {
    std::vector<ElementTables> elem;                         // [nlevels]
    std::vector<std::unique_ptr<DevBuf<uint8_t>>> d_mask;    // [nlevels], null until used
};

// Sampling state of a grid (hmg_sample.cpp): the locator of the current cells -- built by the first hmg_grid_locate / hmg_sample /
// hmg_sample_raster, and again after hmg_grid_shrink (which clears `ready`) --, per level used the lattice -> slot table, and their
// device copies, made by the first device call.  Like FieldState outside LevelDev / MeshDev and outside the checksum of a
// host-only grid: grid creation and its allocations are what they were.
struct SampleState {
    bool ready = false, on_device = false;
    bool torus = false;                                      // hmg_grid_set_periodic_sampling: a periodic grid is served
    int nb[3] = {1, 1, 1};
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, inv_h[3] = {0, 0, 0};
    std::vector<int32_t> bin_ptr, bin_cell;                  // CSR: per bin its candidate cells, ascending
    std::vector<double> geo;                                 // per cell X0 and J^-1 (row-major)
    DevBuf<double> d_tables;                                 // geo, then bin_ptr and bin_cell: one allocation
    std::vector<char> level_ready;                           // [nlevels] basis and slot formula checked, table built
    std::vector<std::vector<int32_t>> slot_of;               // [nlevels] 3D: lattice node -> storage slot
    std::vector<std::unique_ptr<DevBuf<int32_t>>> d_slot_of; // [nlevels], null until used on the device
};

// state of the last coarse solve, copied to pinned host memory behind the solve and read when somebody asks
struct CoarseProbe {
    double *h = nullptr;            // pinned: S_DONE, S_ITER, S_CRR, b.b
    hipEvent_t ev = nullptr;
    bool pending = false;
    int budget = 0;                 // iterations launched by the solve the probe belongs to
    int generation = 0;             // the level-1 matrix (hmg_grid::coarse_generation) that solve used
};

}  // namespace hmg

// Lifetimes: a vector keeps its grid alive, a grid its context (reference counts, single host thread): hmg_*_destroy
// hands the caller's reference back, the object goes when the last dependant has gone -- the order in which a host
// (finalizers of a garbage-collected language in particular) destroys handles does not matter.
struct hmg_ctx {
    int refs = 1;
    ApplyTimer timer;
    bool fuse_cg_default = true;
    bool fold_x = true;   // V-cycle: pre-smoother's last x-update rides with the local residual
    bool swap_rp = true;  // V-cycle: step 0 of a smoother takes r itself as p (pointer exchange), see smooth_form()
    bool fold_prolong = true;   // V-cycle: prolongation folded into the post-smoother's first residual
    bool lazy_dead = true;      // V-cycle: the pre-smoother's dead last step writes nothing (see smooth_form())
    bool lazy_pre = true;       // ... and with three steps or more the step before it leaves its x-update too, its direction in the spare vector (see smooth_form())
    bool fold_faces = true;     // fused CG: the face part of Ap's interface sum rides in the r-update (all steps but a live last one)
    bool lean_post = true;      // V-cycle: the post-smoother's dead tail is dropped too (see smooth_form())
    bool lazy_post = true;      // ... and below the finest level its dead last step writes nothing: both x-updates in one pass
    bool fold_coarse_x = true;  // ... and the level below the finest leaves them to the finest level's first residual, which reads that x anyway (see coarse_x_folds())
    bool lazy_r = true;         // hmg_vcycle / hmg_fcg_step: the finest level's last r-update only finishes x; r_3 is formed when somebody reads it (PendingR)
    bool lazy_ap = true;        // ... and the CG step in front of it does not store A p_2 (three-update form): the record rebuilds it when r is read (PendingR::ap_stored)
    bool lazy_x = true;         // ... and the x-updates of that launch stay pending too: the next hmg_vcycle's first residual forms x where it reads it (PendingX)
    int lazy_top = 2;           // ... on the finest level its last step leaves both x-updates to the r-update, 2: and the step before its own (see smooth_form())
    bool zero_entry = true;        // V-cycle: a coarse level's zero initial guess is never materialised (see zero_entry_ok())
    bool fold_restrict = true;     // V-cycle: the restriction rides in the epilogue of the local residual, which is then not stored
    bool prolong_in_image = true;  // folded prolongation, level 6: the coarse column is staged at the even nodes of the lattice image
                                   // instead of in LDS of its own behind it (three workgroups per CU stay resident)
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    DevBuf<double> partials, scal, rpart;
    Launch L{};
    int coarse_maxit = 5000;
    int coarse_check = 25;
    bool coarse_probe = true;   // budgeted level-1 solves leave a probe behind (off: stream-capture experiments)
    double coarse_rtol = 1e-13;
    int coarse_poly = 4;            // level-1 PCG: Chebyshev iterates per preconditioner application (1 = plain Jacobi)
    double coarse_poly_ratio = 20.0;   // ... on the interval [lmax / ratio, lmax] of D^-1 A, lmax = its Gershgorin bound
    // in-library communicator (one rank per GPU, RCCL over xGMI): hmg_comm_init
    ncclComm *comm = nullptr;
    int comm_nranks = 1, comm_rank = 0;
    hipStream_t comm_stream = nullptr;       // the overlapped cut exchange runs here
    hipEvent_t ev_packed = nullptr, ev_summed = nullptr;
    int64_t comm_calls = 0, comm_doubles = 0;
    int64_t small_launches = 0;              // launches of the pipelined small-level apply
    int64_t wc_launches = 0;                 // launches of k_apply<.., WC>: class weights from the cache (level 6)
    int64_t wave_launches = 0;               // launches of the one-wave-per-cell apply (hmg_ctx_counter)
    int64_t slab2_launches = 0;              // launches of the role-split slab apply (hmg_apply_slab.hip)
    int64_t rows_launches = 0;               // launches of the row-band apply of 2D cells larger than the LDS (hmg_apply_rows.hip)
    int64_t wc_max_classes = 0;              // option "weight_cache_classes": most distinct coefficient rows that still get a
                                             // class-weight cache (0: no limit by count; 1024: what the library did before)
    int64_t wc_classes = 0, wc_bytes = 0;    // rows cached by this context's grids / bytes of their caches (ensure_weight_cache)
    int64_t wc_refusals = 0;                 // operators whose cache did not fit the device memory (counter "weight_cache_refusals")
    int64_t spare_bytes = 0;                 // spare direction vectors held by this context's grids (reserve_top_spare)
    int64_t fcg_bytes = 0;                   // p, q and R of this context's hmg_fcg objects (hmg_fcg.cpp)
    int64_t smoother_diag_bytes = 0;         // inverse diagonals held by this context's grids (hmg_grid_set_smoother)
    int64_t smoother_diag_builds = 0;        // times a grid of this context formed them (ensure_smoother_diag)
    int64_t smoother_bound_builds = 0;       // level bounds of the Chebyshev smoother formed by this context's grids (ensure_smoother_diag)
    int64_t cheb_applies = 0;                // operator applies launched inside Chebyshev smoothings (the first residual not counted)
    int64_t cheb_smoothings = 0;             // Chebyshev smoothings of at least one step
    int64_t moments_kernel_ns = 0, moments_download_ns = 0;   // the last hmg_cell_moments: its kernel (device events) and the download of its sums (host clock)
    int64_t pair_moments_kernel_ns = 0, pair_moments_download_ns = 0;   // the last hmg_cell_pair_moments, likewise
    int64_t extrema_kernel_ns = 0;           // the last hmg_cell_extrema: its kernel (device events)
    int64_t extrema_where_kernel_ns = 0;     // the last hmg_cell_extrema_where, likewise: a counter of its own, so that one process times both
    int64_t extrema_where_launches = 0;      // launches of the located kernels (hmg_ctx_counter "cell_extrema_where_launches")
    int64_t histogram_kernel_ns = 0;         // the last hmg_cell_histogram: its kernel (device events)
    int64_t histogram_launches = 0;          // launches of k_cell_histogram (hmg_ctx_counter "cell_histogram_launches")
    int histogram_variant = 1;               // option "cell_histogram_variant": how counts reach the LDS histogram (hmg_histogram.hpp: HIST_DEFAULT; the same ints from each)
    int histogram_windows = 0;               // option "cell_histogram_windows": the three values of "cell_extrema_windows" for hmg_cell_histogram and
                                             // its window kernels (hmg_histogram_window.hip); an option of its own, off by default
    int64_t histogram_window_launches = 0;   // launches of those (hmg_ctx_counter "cell_histogram_window_launches")
    int64_t histogram_groups_kernel_ns = 0;  // the last hmg_cell_histogram_groups: its group-sum kernel (device events)
    int64_t sample_launches = 0;             // launches of k_sample (hmg_sample, hmg_sample_raster)
    int64_t sample_kernel_ns = 0, sample_download_ns = 0;   // the last of those calls: its kernel (device events), its downloads (host clock)
    int moments_windows = 0;                 // option "cell_moments_windows": 0 cells larger than the LDS are refused; 1 they take the window
                                             // kernels (hmg_fields_window.hip); 2 so does every level those kernels can address (A/B knob)
    int64_t moments_window_launches = 0;     // launches of the window kernels (hmg_ctx_counter "cell_moments_window_launches")
    int extrema_windows = 0;                 // option "cell_extrema_windows": the same three values for hmg_cell_extrema and its window
                                             // kernels (hmg_extrema_window.hip); an option of its own, so that neither call changes with the other's
    int64_t extrema_window_launches = 0;     // launches of those (hmg_ctx_counter "cell_extrema_window_launches")
    int64_t coarse_x_folds = 0;              // residuals that finished the coarser level's x on the way (option fold_coarse_x)
    int last_pre_form = 0;                   // x-updates the last pre-smoother of a V-cycle's down leg left to its local residual: 0 .. 3
    int last_r_form = 0;                     // what the last hmg_vcycle / hmg_fcg_step left of its top level's r: 0 formed, 1 pending (x-only tail)
    int64_t r_materialized = 0;              // pending residuals formed by a later call (the eager r-update, launched late) ...
    int64_t r_materialized_read = 0;         // ... those of them because a call was handed r or Ap (the others: setters, the tuner)
    int64_t r_dropped = 0;                   // ... and those nobody read: overwritten by the next V-cycle, a copy or a fill, or destroyed
    int last_ap_form = 0;                    // 1: the last hmg_vcycle / hmg_fcg_step left that pending r without a stored Ap (option lazy_ap)
    int64_t ap_rebuilt = 0;                  // pending residuals whose Ap had to be formed first: the last CG step's apply, launched late
    int last_x_form = 0;                     // x-updates the last hmg_vcycle left pending on its top level's x: 0, 2 or 3 (option lazy_x)
    int64_t x_deferred = 0;                  // V-cycles that left them pending ...
    int64_t x_settled = 0;                   // ... those of them a later call had to finish (the eager x-only tail, launched late; the others rode in a first residual)
    int64_t x_settled_read = 0;              // ... of those: because a call was handed x or the direction it rests on
    int last_top_form = 0;                   // form the last finest-level post-smoother inside hmg_vcycle took: 0 plain, 1 two-update, 2 three-update
    // Level-vector memory handed back by hmg_vec_destroy, kept for the next hmg_vec_create of the same size: on this
    // platform hipMalloc of memory the process has freed before costs ~35 ms per GB (tools/dev/alloc_probe.hip: 6 x 10 GB
    // 0.001 s fresh, 2.05 s after a hipFree), i.e. 1.9 s of the 71 GB a second driver call allocates.
    bool vec_pool_on = true;
    std::vector<std::pair<size_t, void *>> vec_pool;
    // rehearsal on fewer GPUs than the partition is meant for: a grid that holds rank r's share of an N-rank partition
    // may use a communicator of another size (the neighbours' contributions are then simply missing from the sums --
    // the work per rank, the message sizes and the stream choreography are the real ones, the numbers are not)
    bool comm_rehearsal = false;
    int64_t overlap_min_doubles = 524288;   // levels whose GLOBAL cut is below 4 MiB (about 1 MiB per rank at octants) are
                                            // exchanged in the plain form (see apply_then_sum)
    // grids of this context whose last budgeted level-1 solve still has its probe in flight: judged at the next call that
    // synchronises the stream anyway (norms, dot products, integrals, hmg_ctx_sync, downloads)
    std::vector<struct hmg_grid *> probe_grids;
    // grids of this context with an open PendingR record: an option that shapes the apply settles them before it takes effect
    std::vector<struct hmg_grid *> pend_grids;
};

// The last r-update of a V-cycle, not launched yet (option lazy_r): r still holds r_2, Ap the unsummed A p_2, the saved block
// (hmg_device.hpp, hmg_grid::pend_alpha()) the step length.  Forming it is launch_cg_rupdate_faces on (r, r, Ap) with the block as its
// scalars, the ratio XS_LAST and its r.r into `slot` --
// the launch the eager tail makes (materialize_r()).  Open on unpartitioned grids and library-owned, never exposed vectors only.
// A caller that reads r after every cycle (a driver that watches the residual norm) would pay for the split: 40 + 26 B/DOF instead of
// 58.  So the grid remembers whether the last V-cycle's r was read (hmg_grid::r_reader): if it was, the next tail runs the eager
// launch and leaves a record that is already `formed` -- nothing left to launch, it only notes whether r is read again; a record
// that is dropped unread clears the flag and the next V-cycle defers again.  The bits do not depend on the path.
// Option lazy_ap (three-update form): the last CG step ran in the dead form -- p_2.Ap_2 for the step length, nothing stored -- and Ap
// holds no A p_2 (ap_stored = false).  Forming r then starts with the launch the eager tail would have made: the fused apply on x = r
// (still r_2), x2 = the spare vector (still p_1), beta_2 = the block's XS_BETA as k_cg_x_tail saved it, out = Ap, the edge / node
// interface sum, p.Ap into S_PAP3.  Such a record rests on the spare vector, the operator (sigma, lambda, masks, class-weight cache)
// and the kernel choice as well: whatever changes one of them settles the record first (hmg_grid_set_operator*, _set_lambda,
// hmg_ctx_set_option through hmg_ctx::pend_grids, a smoother that is about to write the spare vector).  Ap's memory is the column to
// rebuild into, so the rules for r and Ap are the same for both kinds of record.
struct PendingR {
    hmg_vec *r = nullptr, *Ap = nullptr;
    int level = 0;
    int slot = -1;
    bool formed = false;
    bool ap_stored = true;      // false: Ap is still to be rebuilt (option lazy_ap)
    bool orphan_Ap = false;     // Ap's handle was destroyed while r still needs its memory: the record owns it until it closes
};
// (hmg_*_destroy may come from any thread, a finalizer's for one: it launches only where a vector goes that pending x-updates rest on.
//  Whoever touches the records holds the lifetime lock.)

// The x-updates of that last launch, not launched either (option lazy_x): x lacks  x += a0 p0 (form 3 only);  x += a1 p1;
// x += a2 (r2 + b2 p1).  p1 is the p handle's memory (form 2) or the grid's spare vector (form 3, where the p handle holds p0), r2 the r
// handle's -- so the record lives inside an unformed PendingR on the same r, which settles it before r changes -- and the ratios are those
// of the saved block (launch_cg_x_save): saved_updates() says all of this as an XUpdates.  The next hmg_vcycle on the same states forms x in the load phase of its
// first residual (apply_carries_x: the x3 / x4 streams the down leg's local residual has), which writes x and r in one pass; every other
// call that is handed x, p or r, or changes what they rest on, runs the x-only tail first (settle_x()).  The bits do not depend on the path.
// form 0: x was finished at once because the caller read it after the cycle before (hmg_grid::x_reader, as r_reader); the record watches.
struct PendingX {
    hmg_vec *x = nullptr, *p = nullptr, *r = nullptr;
    int level = 0;
    int form = 0;
};

struct hmg_grid {
    int refs = 1;
    hmg_ctx *ctx = nullptr;
    int dim = 0, nlevels = 0;
    std::vector<LevelTables> lt;
    std::vector<std::unique_ptr<LevelBufs>> lb;
    std::vector<LevelDev> ld;
    MeshTables mesh_full, mesh;
    bool shrunk = false;
    bool dir_custom = false;                     // mesh_full's masks are the closure of a caller's faces (hmg_grid_set_dirichlet_faces) ...
    std::vector<int32_t> dir_faces;              // ... these (the form of boundary_faces()); empty with the default set
    MeshDev md{};
    DevBuf<int32_t> d_cells, d_face_pairs, d_face_partner, d_edge_ptr, d_edge_ent, d_node_ptr, d_node_ent, d_node_first;
    DevBuf<uint16_t> d_dmask, d_dupmask;
    DevBuf<uint8_t> d_mult;
    DevBuf<double> d_blockpart;                  // per-cell reduction partials; its last XS_COUNT doubles: the saved block (hmg_device.hpp) of a pending r-update and of pending x-updates
    PendingR pend;
    PendingX pendx;
    bool x_reader = false;                       // a caller's read settled pending x-updates and no V-cycle's x went unread since (see PendingX)
    bool r_reader = false;                       // a caller's read settled a record and none was dropped unread since (see PendingR)
    double *pend_alpha() const { return d_blockpart.p ? d_blockpart.p + d_blockpart.n - XS_COUNT : nullptr; }
    bool fuse_cg = true;
    DevBuf<double> d_coef;
    std::vector<double> sigma, coef;
    int sig_n = 0;                               // numbers per cell in sigma / sigma_global: dim (diagonal tensors,
                                                 // hmg_grid_set_operator) or dim (dim + 1) / 2 (hmg_grid_set_operator_tensor)
    // class-weight cache (k_apply_wave): cells with bitwise equal coefficient rows share a class
    DevBuf<int32_t> d_cell_class;
    DevBuf<double> d_coef_rep;
    int nclasses = 0;
    std::vector<int32_t> cell_class;             // host copy of the class table (hmg_grid_table_i32 "cell_class"), empty: none
    int64_t wc_limit = 0;                        // the context's option "weight_cache_classes" as it stood when the operator was set
                                                 // (a domain shrink re-classes the cells under the same limit)
    bool wc_trim = false;                        // a new operator sizes the cache blocks to its rows; a domain shrink or a new
                                                 // lambda after it keeps the blocks it has (fewer rows of the same operator)
    int64_t wc_counted_classes = 0, wc_counted_bytes = 0;   // this grid's share of the context's "weight_cache_*" counters
    double wc_lambda = 0.0;
    bool wc_ready = false;
    double lambda = 0.0;
    bool has_op = false;
    uint64_t op_epoch = 0;                       // operators this grid has had (new sigma, new lambda, domain shrink): what an
                                                 // hmg_fcg object compares its residual's operator with
    // coarse system
    CoarseMatrix cm;
    CoarseDev cd{};
    bool coarse_ready = false;
    bool mean_free = false;                      // hmg_grid_set_mean_free: a level-1 matrix with the constants in its kernel is solved on their complement ...
    bool coarse_singular = false;                // ... and the matrix coarse_setup assembled last is one (lambda = 0, no constrained node)
    DevBuf<int32_t> c_rowptr, c_colidx, c_interior;
    DevBuf<double> c_val, c_diag, c_b, c_x, c_r, c_z, c_p, c_q, c_u, c_z2, c_d;   // (c_z2, c_d: Chebyshev preconditioner)
    DevBuf<double> top_spare;           // second direction vector of the finest level's post-smoother (smooth(), lazy_top = 2)
    bool top_spare_refused = false;
    // Jacobi-preconditioned CG smoother (hmg_grid_set_smoother): per level >= 2 the inverse of the assembled operator's diagonal,
    // 0 on constrained nodes -- a consistent level vector, reserved by the call (setup memory), formed by ensure_smoother_diag()
    int smoother = 0;                            // 0: CG (src/multigrid.jl:46-71), 1: Jacobi-preconditioned CG, 2: Chebyshev-Jacobi
    // Chebyshev-Jacobi smoother (hmg_grid_set_smoother_chebyshev): a polynomial in dinv o A on [hi / ratio, hi] per level >= 2
    double cheb_ratio = 0.0;                     // lambda_hi / lambda_lo
    std::vector<double> cheb_given;              // [nlevels] the caller's bounds (> 0: used as given, nothing is formed), or empty
    std::vector<double> cheb_hi;                 // [nlevels] the bounds in use; formed with dinv and stale with it (dinv_level_ready)
    std::vector<std::unique_ptr<DevBuf<double>>> dinv;   // [nlevels], empty with smoother 0
    bool dinv_ready = false;                     // false: operator, lambda, domain, cut or exchange changed since they were formed
    std::vector<char> dinv_level_ready;          // [nlevels] formed since then (a level is formed where a call first smooths on it)
    bool dinv_build_counted = false;             // ... and "smoother_diag_builds" has counted this generation
    double c_lmax = 2.0;                         // Gershgorin bound of D^-1 A of the level-1 matrix
    int coarse_last_it = 0;
    int coarse_budget = 0;                       // iterations a solve enqueues blindly (0: not known yet)
    int coarse_generation = 0;                   // counts the level-1 matrices assembled for this grid
    int64_t coarse_misses = 0;                   // budgeted solves that ran out of iterations (each one was reported or, with a
                                                 // new matrix in between, only counted)
    std::unique_ptr<CoarseProbe> probe{new CoarseProbe};
    // multi-GPU
    std::unique_ptr<Partition> part;
    std::vector<double> sigma_global;
    // inputs of the partition analysis, kept for a domain shrink (re-analysis of the prefix mesh)
    std::vector<double> part_coords;
    std::vector<int64_t> part_cells;
    std::vector<int32_t> part_owner, part_cut_owner;     // (part_cut_owner: rehearsal partitions only, else empty)
    bool part_halo = true;                               // partition analysis on this rank's cells + one-cell halo (see create_grid)
    int64_t part_nnodes = 0, part_ncells = 0;
    DevBuf<int32_t> d_nodes_g, d_owned, d_cells_gnode;
    CutKind cut[3];   // faces, edges, nodes
    // Number of cut entities per kind OVER ALL RANKS, agreed once per partition analysis (agree_on_cut): what the overlap
    // decision of apply_then_sum looks at.  (CutKind::nglobal is rank-local after a halo-only analysis.)  -1: no agreement
    // possible (no scalar_sum callback) -- the plain form everywhere.
    int64_t cut_agreed[3] = {0, 0, 0};
    bool cut_agreed_ready = false;
    std::vector<std::unique_ptr<CutLevel>> cutlv;   // [nlevels]
    bool sharers = false;                        // exchange among the sharers of each cut entity (segments) instead of one
                                                 // all-reduce over the global cut buffer; needs a p2p transport (below)
    hmg_exchange_fn exchange = nullptr, scalar_sum = nullptr;
    hmg_exchange_fn ex_begin = nullptr;          // asynchronous form: begin issues the sum, end waits for it
    int (*ex_end)(void *) = nullptr;
    hmg_p2p_fn p2p = nullptr, p2p_begin = nullptr;   // segment layout: the messages of one exchange (sync / begin; ex_end ends it)
    double *stage = nullptr;
    int64_t stage_cap = 0;
    DevBuf<double> own_stage;
    bool overlap = true;
    DevBuf<int32_t> d_cells_cut, d_cells_inner, d_cell_perm;
    void *ex_user = nullptr;
    double *ex_buf = nullptr;
    int64_t ex_cap = 0;
    DevBuf<double> own_exbuf;                    // hmg_grid_use_comm: library-owned exchange buffer

    FieldState fields;                           // fine-element tables of hmg_cell_extrema (hmg_extrema.cpp)
    SampleState sample;                          // locator and lattice tables of hmg_grid_locate / hmg_sample* (hmg_sample.cpp)

    uint64_t upload_hash = 1469598103934665603ull;   // host-only grids: checksum of every table a device grid would upload (DryUploads)

    const MeshTables &cur() const { return shrunk ? mesh : mesh_full; }
};

struct hmg_vec {
    hmg_grid *g = nullptr;
    int level = 0;
    double *d = nullptr;
    bool own = false;
    int64_t alloc_cells = 0;
    size_t bytes = 0;        // own: size of the allocation behind d
    bool exposed = false;    // hmg_vec_device_ptr has handed d out: somebody may read the memory behind the library's back
};

namespace hmg {

inline int fail(const std::exception &e)
{
    last_error() = e.what();
    return 1;
}

#define HMG_TRY try {
#define HMG_END                      \
    }                                \
    catch (const std::exception &e)  \
    {                                \
        return fail(e);              \
    }                                \
    catch (...)                      \
    {                                \
        last_error() = "unknown error"; \
        return 1;                    \
    }                                \
    return 0;

inline void need(bool c, const char *msg)
{
    if (!c) throw std::runtime_error(msg);
}

inline const LevelDev &lev(const hmg_grid *g, int level)
{
    need(g != nullptr, "null grid");
    need(g->ctx != nullptr, "this grid was created without a device context (host tables only): no compute path exists on the CPU");
    need(level >= 1 && level <= g->nlevels, "level out of range");
    return g->ld[level - 1];
}

// ---- hmg_pending.cpp ----
// The pending records of a grid (PendingR, PendingX above).  When the finest level's post-smoother inside hmg_vcycle may leave them:
bool lazy_r_ok(const hmg_grid *g, const hmg_vec *r, const hmg_vec *p, const hmg_vec *Ap);
bool lazy_ap_ok(const hmg_grid *g);
bool lazy_x_ok(const hmg_grid *g, int level, int updates, const hmg_vec *x, const hmg_vec *r, const hmg_vec *p, const hmg_vec *Ap);
// ... and how (slot: where the r-update's r.r goes; form: the x-updates left, 0 for a record that only watches)
void open_pending(hmg_grid *g, int level, hmg_vec *r, hmg_vec *Ap, int slot, bool formed, bool ap_stored = true);
void open_pending_x(hmg_grid *g, int level, hmg_vec *x, hmg_vec *p, hmg_vec *r, int form);
// what a PendingX record with updates to form says is pending: its vectors and the ratios of the grid's saved block
XUpdates saved_updates(const hmg_grid *g, const PendingX &record);
// entry of a V-cycle on top level k with the states st: settles or drops the records; returns the x-updates its first residual is to carry
XUpdates enter_top(hmg_grid *g, int k, hmg_vec **st, bool zero_guess);
// forms it now, if there is one: afterwards vectors and scalar bank are what the eager tail leaves.  read: the caller is about to
// read r or Ap (settle()) -- only that is remembered as a read (hmg_grid::r_reader); a setter that settles the record is not one
void materialize_r(hmg_grid *g, bool read = false);
// a record that has its Ap still to rebuild (option lazy_ap) is settled before what the rebuild rests on changes: the operator, lambda,
// the spare vector, the context's options.  Not a read.  A record that holds its Ap stays open.
// ... and pending x-updates always (the spare vector, the kernel choice)
void settle_x(hmg_grid *g, bool read = false);
// the flexible CG's first pass over z forms them itself: the record on x, if it has updates to form, is handed over (saved_updates() reads
// it) and closed (a record that only watches stays: hmg_fcg_step is a reader of its V-cycle's x like any other, and the next lines say so)
PendingX take_pending_x(hmg_grid *g, const hmg_vec *x);
inline void settle_rebuild(hmg_grid *g)
{
    if (g && g->ctx && g->pendx.x) settle_x(g);
    if (g && g->ctx && g->pend.r && !g->pend.ap_stored) materialize_r(g);
}
// every entry point that is handed a vector goes through one of these three before it touches it:
// the vector is read or partly written -- a pending r or Ap is settled first
// (pending x-updates first, if v is x or a vector they rest on: forming r overwrites one of those)
inline void settle(const hmg_vec *v)
{
    if (!v || !v->g) return;
    const PendingX &px = v->g->pendx;
    if (px.x && (v == px.x || v == px.p || v == px.r)) settle_x(v->g, /*read=*/v != px.r);
    if (v->g->pend.r && (v == v->g->pend.r || v == v->g->pend.Ap)) materialize_r(v->g, /*read=*/true);
}
// every entry of the vector is about to be overwritten unread: a pending r is dropped, a pending Ap settled
void settle_overwritten(const hmg_vec *v);
// hmg_vec_destroy, under the lifetime lock, no launch: a pending r is dropped; true: v is the Ap a pending r still needs -- the
// record keeps the object and its memory, and hands them back (release_vec) when it closes
bool pending_keeps(hmg_vec *v);

// settle_pending = false: the caller settles or drops the record itself (the entries of hmg_vcycle and hmg_fcg_step)
inline void check_vec(const hmg_grid *g, int level, const hmg_vec *v, const char *name, bool settle_pending = true)
{
    if (!v) throw std::runtime_error(std::string("null vector: ") + name);
    if (v->g != g) throw std::runtime_error(std::string("vector belongs to another grid: ") + name);
    if (v->level != level) throw std::runtime_error(std::string("vector has the wrong level: ") + name);
    if (v->alloc_cells < g->md.ncells) throw std::runtime_error(std::string("vector too small: ") + name);
    if (settle_pending) settle(v);
}

inline int64_t vec_len(const hmg_vec *v) { return (int64_t)v->g->ld[v->level - 1].ld * v->g->md.ncells; }

inline bool has_exchange(const hmg_grid *g) { return g->exchange || g->ex_begin || g->p2p || g->p2p_begin; }

// ---- hmg_context.cpp ----
// zero-filled device memory for one level vector, from the context's pool where it has a block of that size
double *vec_alloc(hmg_ctx *c, size_t bytes);
// ... and back into the pool (stream-ordered: what was enqueued on the context's stream before runs before the next owner's work)
void vec_release(hmg_ctx *c, void *p, size_t bytes);
// block partials of the streaming reductions for vectors of nentries entries (allocates where the context's are too few: setup)
void ensure_reduce_scratch(hmg_ctx *c, int64_t nentries);
// what hmg_vec_destroy does with a vector nobody needs any more: memory to the pool, the object, its reference to the grid
void release_vec(hmg_vec *v);
void grid_unref(hmg_grid *grid);
// scal[slot] on the host: synchronises the stream, so the pending probes are judged as well
double read_scalar(hmg_ctx *c, int slot);

// ---- hmg_upload.cpp ----
// (re)forms the class-weight cache when the operator or lambda has changed; called in front of every apply
void ensure_weight_cache(hmg_grid *g);
// hands the cache back (grid destruction, a new class table) and takes its share out of the context's counters
void release_weight_cache(hmg_grid *g);

// ---- hmg_fields.cpp ----
// the level's rolling-window lists (those set_slab hands to the operator apply), without touching the grid's launch state: what
// the window kernels of the per-cell moments and extrema walk
SlabTables slab_tables(const hmg_grid *g, const LevelDev &lv);

// ---- hmg_extrema.cpp ----
// what the calls of the pass over the fine elements share (hmg_cell_extrema, hmg_cell_extrema_where; hmg_histogram.cpp:
// hmg_cell_histogram): the device copy of a level's element mask, uploaded at the first call on that level, and the folded row of
// every current cell -- Q~ = M^T Q M and xi~ = M^-1 xi, cell_extrema_nrow(dim) numbers --, one text of the arithmetic
const uint8_t *device_element_mask(hmg_grid *g, int level);
std::vector<double> cell_form_rows(const std::string &who, const hmg_grid *g, int level, const double *xi, const double *form);

// ---- hmg_sample.cpp ----
// hmg_ctx_counter "sample_locator_builds" (0), "sample_locator_bytes" (1), "sample_locator_max_candidates" (2): locators built in
// this process, and the table bytes and the longest candidate list of the last one.  Process-wide like device_allocs; the only
// counters hmg_ctx_counter answers for a NULL context ("device_allocs" is not: it stays behind the null check)
int64_t sample_locator_counter(int which);

// ---- hmg_smooth.cpp ----
void set_slab(hmg_grid *g, const LevelDev &lv);
// out = (src ? src : 0) + alpha * A x, cell-local (no interface sum); mask: the Dirichlet constraint
void apply(hmg_grid *g, const LevelDev &lv, double alpha, const double *x, const double *src, double *out, int mask);
void restrict_level(hmg_grid *g, int level_fine, const double *rf, double *bc);
void interface_sum(hmg_grid *g, const LevelDev &lv, double *x, bool faces = true);
// the apply with the interface sum of its output and, fused, its reductions into the bank's slot_pap / slot_rr (< 0: not wanted)
void apply_then_sum(hmg_grid *g, const LevelDev &lv, ApplyArgs a, bool fused, int slot_pap, int slot_rr, bool sum_out = true,
                    bool faces = true);
// sum over the ranks of scal[slot .. slot + count) through the grid's scalar_sum callback (nothing on an unpartitioned grid)
void scalar_sum(hmg_grid *g, int slot, int count);
bool reserve_top_spare(hmg_grid *g, bool must);
void release_top_spare(hmg_grid *g);
bool wants_top_spare(const hmg_grid *g, int level);
// forms the stale inverse diagonal of one level of a grid with smoother 1 (kernels and the interface sum's exchange only, no
// allocation): at the entry of every call that smooths on that level, before its first launch.  scratch: a vector of the level
// that the call overwrites anyway (its Ap; the output of hmg_grid_smoother_diag) -- the fixed-point sum needs a second array
void ensure_smoother_diag(hmg_grid *g, int level, double *scratch);
// ... of levels 2 .. top, the scratch of a level being the Ap of its state (states: five handles per level)
void ensure_smoother_diag(hmg_grid *g, int top, hmg_vec **states);
void release_smoother_diag(hmg_grid *g);
// zero_guess (top level only; below it always holds): x is to be taken as zero whatever it holds -- never written where the
// smoother's form allows that (zero_entry_ok), filled first otherwise: the same bits either way
// lazy_x: the caller is not the next reader of the top level's x (hmg_vcycle; hmg_fcg_step reads it at once)
void vcycle(hmg_grid *g, int k, int steps, int steps_coarse, hmg_vec **st, bool top = true, bool zero_guess = false, bool lazy_x = false);

// ---- hmg_coarse.cpp ----
void coarse_solve(hmg_grid *g, hmg_vec *b1, hmg_vec *x1);
void probe_unlist(hmg_grid *g);
void judge_probes(hmg_ctx *c);

// ---- hmg_comm.cpp ----
void exchange_cut(hmg_grid *g, const LevelDev &lv, double *x);
void cut_pack(hmg_grid *g, const LevelDev &lv, double *x, int unpack);
void exchange_prepare(hmg_grid *g, const LevelDev &lv);
void exchange_run(hmg_grid *g, const LevelDev &lv, bool async);
void exchange_finish(hmg_grid *g, const LevelDev &lv, bool async);
// communicator, second stream and events of a context go (errors ignored: the context is on its way out, or they were checked)
void comm_drop(hmg_ctx *c);

}  // namespace hmg

// Contexts, grids and vectors as objects: reference counts, device memory and the pool of level-vector blocks, options and
// counters of a context, with the entry points that front them (hmg_ctx_*, hmg_grid_destroy, hmg_vec_create / wrap / destroy).
#include "../../include/hmg.h"
#include "hmg_objects.hpp"

#include <algorithm>

namespace hmg {

std::recursive_mutex &lifetime_mutex()
{
    static std::recursive_mutex m;
    return m;
}

std::atomic<int64_t> &device_allocs()
{
    static std::atomic<int64_t> n{0};
    return n;
}

namespace {

void vec_pool_trim(hmg_ctx *c)
{
    LifetimeLock lock(lifetime_mutex());
    if (c->vec_pool.empty()) return;
    (void)hipStreamSynchronize(c->stream);
    for (auto &b : c->vec_pool) (void)hipFree(b.second);
    c->vec_pool.clear();
}

std::vector<hmg_ctx *> &live_contexts()
{
    static std::vector<hmg_ctx *> v;
    return v;
}

void release_pooled_memory()
{
    LifetimeLock lock(lifetime_mutex());
    for (hmg_ctx *c : live_contexts()) vec_pool_trim(c);
}

}  // namespace

hipError_t device_malloc(void **p, size_t bytes)
{
    *p = nullptr;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        release_pooled_memory();
        e = hipMalloc(p, bytes);
    }
    if (e == hipSuccess) device_allocs() += 1;
    return e;
}

// (stream-ordered: kernels of a pooled block's previous owner were enqueued on the same stream, or joined to it by events,
//  before the block came back)
double *vec_alloc(hmg_ctx *c, size_t bytes)
{
    LifetimeLock lock(lifetime_mutex());
    void *p = nullptr;
    for (size_t i = 0; i < c->vec_pool.size(); ++i)
        if (c->vec_pool[i].first == bytes) {
            p = c->vec_pool[i].second;
            c->vec_pool[i] = c->vec_pool.back();
            c->vec_pool.pop_back();
            break;
        }
    const bool pooled = p != nullptr;
    if (!pooled) {
        hipError_t e = device_malloc(&p, bytes);  // (pooled blocks of other sizes, any context's, may be what is in the way)
        if (e != hipSuccess)
            throw std::runtime_error(std::string("hipMalloc of a level vector (") + std::to_string(bytes >> 20) +
                                     " MiB) failed: " + hipGetErrorString(e));
    }
    hipError_t e = hipMemsetAsync(p, 0, bytes, c->stream);
    if (e != hipSuccess) {
        (void)hipFree(p);
        throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e));
    }
    return (double *)p;
}

void vec_release(hmg_ctx *c, void *p, size_t bytes)
{
    LifetimeLock lock(lifetime_mutex());
    if (c->vec_pool_on && bytes > 0) {
        c->vec_pool.emplace_back(bytes, p);
        return;
    }
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(p);
}

// scratch of the streaming reductions (one partial per 256-thread block = per 512 entries, see hmg_kernels.hip)
void ensure_reduce_scratch(hmg_ctx *c, int64_t nentries)
{
    const int64_t need_blocks = nentries / 512 + 2;
    if (need_blocks <= 2048 || need_blocks <= c->L.rpart_cap) return;
    HIPCHK(hipStreamSynchronize(c->stream));
    c->rpart.alloc((size_t)need_blocks);
    c->L.rpart = c->rpart.p;
    c->L.rpart_cap = need_blocks;
}

namespace {

void ctx_unref(hmg_ctx *ctx)
{
    LifetimeLock lock(lifetime_mutex());
    if (!ctx || --ctx->refs > 0) return;
    auto &lc = live_contexts();
    lc.erase(std::remove(lc.begin(), lc.end(), ctx), lc.end());
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto &ev : ctx->timer.pool) {
        (void)hipEventDestroy(ev.first);
        (void)hipEventDestroy(ev.second);
    }
    vec_pool_trim(ctx);
    comm_drop(ctx);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

}  // namespace

void grid_unref(hmg_grid *grid)
{
    LifetimeLock lock(lifetime_mutex());
    if (!grid || --grid->refs > 0) return;
    hmg_ctx *c = grid->ctx;
    if (c) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
    }
    probe_unlist(grid);
    if (c) {   // (a record goes with its r, which holds the grid: none is open here; nothing is launched either way)
        c->pend_grids.erase(std::remove(c->pend_grids.begin(), c->pend_grids.end(), grid), c->pend_grids.end());
    }
    release_top_spare(grid);
    release_weight_cache(grid);
    release_smoother_diag(grid);
    if (grid->probe && grid->probe->h) (void)hipHostFree(grid->probe->h);
    if (grid->probe && grid->probe->ev) (void)hipEventDestroy(grid->probe->ev);
    delete grid;
    ctx_unref(c);
}

void release_vec(hmg_vec *v)
{
    if (v->own && v->d) vec_release(v->g->ctx, v->d, v->bytes);
    hmg_grid *g = v->g;
    delete v;
    grid_unref(g);
}

double read_scalar(hmg_ctx *c, int slot)
{
    double h = 0.0;
    HIPCHK(hipMemcpyAsync(&h, c->L.scal + slot, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    judge_probes(c);
    return h;
}

}  // namespace hmg

extern "C" {

const char *hmg_last_error(void) { return last_error().c_str(); }
int hmg_version(void) { return 1; }

static int ctx_create(int device, void *stream, bool use_given, hmg_ctx **out)
{
    HMG_TRY
    need(out != nullptr, "null out pointer");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        throw std::runtime_error("no HIP device available: libhmg_hip needs an MI355X (gfx950); there is no CPU fallback");
    need(device >= 0 && device < ndev, "device index out of range");
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<hmg_ctx> c(new hmg_ctx);
    c->device = device;
    if (use_given) {
        c->stream = (hipStream_t)stream;   // may be the null (legacy default) stream
    } else {
        HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    c->partials.alloc(4096);
    c->scal.alloc(S_COUNT);
    HIPCHK(hipMemsetAsync(c->scal.p, 0, S_COUNT * sizeof(double), c->stream));
    c->L.stream = c->stream;
    c->L.partials = c->partials.p;
    c->L.rpart = nullptr;
    c->L.rpart_cap = 0;
    c->L.scal = c->scal.p;
    c->L.num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    c->L.apply_threads = 0;
    c->L.apply_mass_only = 0;
    c->L.cell_order = 1;
    c->L.weight_cache = 1;  // level 6: class weight rows from the class-weight cache (k_apply<.., WC>)
    c->L.apply_wave = 1;    // level 5: one wave per cell where the class-weight cache exists (hmg_apply_wave.hip)
    c->L.wave_grid = 16 * (int64_t)c->L.num_cu;
    c->L.n_wave_launches = &c->wave_launches;
    c->L.apply_slab2 = 1;   // level 7: one persistent workgroup per CU, loader and evaluator waves (hmg_apply_slab.hip)
    c->L.n_slab2_launches = &c->slab2_launches;
    c->L.n_rows_launches = &c->rows_launches;
    c->L.slab2_grid = 0;
    c->L.slab2_force = 0;
    c->L.restrict_slab2 = 1;
    c->L.apply_pack = 1;    // level 2: four cells per wave
    c->L.apply_small = 1;   // levels 2-4: pipelined one-wave kernel (hmg_apply_small.hip)
    c->L.n_small_launches = &c->small_launches;
    c->L.n_wc_launches = &c->wc_launches;
    c->L.apply_wg512 = 1;   // level 6: three 512-thread workgroups per CU (measured: V-cycle 149.5 -> 141 ms; 3 x 640 threads do not fit the wave slots: 174 ms)
    {
        LifetimeLock lock(lifetime_mutex());
        live_contexts().push_back(c.get());
    }
    *out = c.release();
    HMG_END
}

int hmg_ctx_create(int device, void *stream, hmg_ctx **out) { return ctx_create(device, stream, stream != nullptr, out); }

int hmg_ctx_create_on_stream(int device, void *stream, hmg_ctx **out) { return ctx_create(device, stream, true, out); }

int hmg_ctx_destroy(hmg_ctx *ctx)
{
    HMG_TRY
    ctx_unref(ctx);
    HMG_END
}

int hmg_ctx_sync(hmg_ctx *ctx)
{
    HMG_TRY
    need(ctx != nullptr, "null ctx");
    HIPCHK(hipStreamSynchronize(ctx->stream));
    judge_probes(ctx);
    HMG_END
}

int64_t hmg_ctx_counter(hmg_ctx *ctx, const char *name)
{
    if (!name) return -1;
    const std::string n(name);
    // (process-wide: a host-only grid has a locator and no context)
    if (n == "sample_locator_builds") return sample_locator_counter(0);
    if (n == "sample_locator_bytes") return sample_locator_counter(1);
    if (n == "sample_locator_max_candidates") return sample_locator_counter(2);
    if (!ctx) return -1;
    if (n == "sample_launches") return ctx->sample_launches;                        // launches of k_sample (hmg_sample, hmg_sample_raster)
    if (n == "sample_kernel_ns") return ctx->sample_kernel_ns;                      // the last of those calls: kernel alone
    if (n == "sample_download_ns") return ctx->sample_download_ns;                  // ... and the download of its results
    if (n == "wave_launches") return ctx->wave_launches;
    if (n == "slab2_launches") return ctx->slab2_launches;
    if (n == "rows_launches") return ctx->rows_launches;
    if (n == "small_launches") return ctx->small_launches;
    if (n == "weight_cache_launches") return ctx->wc_launches;
    if (n == "comm_calls") return ctx->comm_calls;
    if (n == "device_allocs") return device_allocs().load();
    if (n == "spare_bytes") return ctx->spare_bytes;
    if (n == "weight_cache_classes") return ctx->wc_classes;
    if (n == "weight_cache_bytes") return ctx->wc_bytes;
    if (n == "weight_cache_refusals") return ctx->wc_refusals;
    if (n == "fcg_bytes") return ctx->fcg_bytes;
    if (n == "smoother_diag_bytes") return ctx->smoother_diag_bytes;
    if (n == "smoother_diag_builds") return ctx->smoother_diag_builds;
    if (n == "smoother_bound_builds") return ctx->smoother_bound_builds;   // level bounds of the Chebyshev smoother formed on the device
    if (n == "cheb_applies") return ctx->cheb_applies;        // operator applies inside Chebyshev smoothings (first residuals not counted)
    if (n == "cheb_smoothings") return ctx->cheb_smoothings;  // Chebyshev smoothings of at least one step
    if (n == "lazy_top_form") return ctx->last_top_form;
    if (n == "lazy_pre_form") return ctx->last_pre_form;
    if (n == "lazy_r_form") return ctx->last_r_form;          // the last hmg_vcycle / hmg_fcg_step: 1 its top level's r-update is (or was) pending
    if (n == "r_materialized") return ctx->r_materialized;    // pending r-updates launched by a later call
    if (n == "r_materialized_by_read") return ctx->r_materialized_read;   // ... of them: by a call that was handed r or Ap
    if (n == "r_dropped") return ctx->r_dropped;              // ... and those that never had to be
    if (n == "lazy_ap_form") return ctx->last_ap_form;        // the last hmg_vcycle / hmg_fcg_step: 1 its record was left without a stored Ap (option lazy_ap)
    if (n == "ap_rebuilt") return ctx->ap_rebuilt;            // pending r-updates that had to run the last CG step's apply again first
    if (n == "lazy_x_form") return ctx->last_x_form;          // the last hmg_vcycle: x-updates it left pending on its top level's x (0, 2, 3; option lazy_x)
    if (n == "x_deferred") return ctx->x_deferred;            // V-cycles that left them pending
    if (n == "x_settled") return ctx->x_settled;              // ... whose x a later call finished with the x-only tail (the others rode in the next first residual)
    if (n == "x_settled_read") return ctx->x_settled_read;    // ... of them: by a call that was handed x or a vector the updates rest on
    if (n == "coarse_x_folds") return ctx->coarse_x_folds;
    if (n == "cell_moments_kernel_ns") return ctx->moments_kernel_ns;       // the last hmg_cell_moments: kernel alone
    if (n == "cell_moments_download_ns") return ctx->moments_download_ns;   // ... and the download of its per-cell sums
    if (n == "cell_pair_moments_kernel_ns") return ctx->pair_moments_kernel_ns;     // the last hmg_cell_pair_moments, likewise
    if (n == "cell_pair_moments_download_ns") return ctx->pair_moments_download_ns;
    if (n == "cell_moments_window_launches") return ctx->moments_window_launches;   // launches of the window kernels (option "cell_moments_windows")
    if (n == "cell_moments_windows") return ctx->moments_windows;                   // ... and that option's value (a caller that sets it for one pass restores it)
    if (n == "cell_extrema_kernel_ns") return ctx->extrema_kernel_ns;               // the last hmg_cell_extrema: kernel alone
    if (n == "cell_extrema_where_kernel_ns") return ctx->extrema_where_kernel_ns;   // the last hmg_cell_extrema_where: kernel alone
    if (n == "cell_extrema_where_launches") return ctx->extrema_where_launches;     // launches of the located kernels, either family
    if (n == "cell_extrema_window_launches") return ctx->extrema_window_launches;   // launches of its window kernels (option "cell_extrema_windows")
    if (n == "cell_extrema_windows") return ctx->extrema_windows;                   // ... and that option's value
    if (n == "cell_histogram_kernel_ns") return ctx->histogram_kernel_ns;           // the last hmg_cell_histogram: kernel alone
    if (n == "cell_histogram_launches") return ctx->histogram_launches;             // launches of its kernel
    if (n == "cell_histogram_variant") return ctx->histogram_variant;               // option of that name
    if (n == "cell_histogram_window_launches") return ctx->histogram_window_launches;   // launches of its window kernels (option "cell_histogram_windows")
    if (n == "cell_histogram_windows") return ctx->histogram_windows;               // ... and that option's value
    if (n == "cell_histogram_groups_kernel_ns") return ctx->histogram_groups_kernel_ns;   // the last hmg_cell_histogram_groups: its group-sum kernel alone
    if (n == "comm_nranks") return ctx->comm ? ctx->comm_nranks : 0;    // as the RCCL communicator was created; 0: none
    return -1;
}

int hmg_ctx_release_memory(hmg_ctx *ctx)
{
    HMG_TRY
    need(ctx != nullptr, "null ctx");
    vec_pool_trim(ctx);
    HMG_END
}

int hmg_ctx_set_option(hmg_ctx *ctx, const char *name, int64_t value)
{
    HMG_TRY
    need(ctx && name, "null argument");
    std::string n(name);
    // a pending r-update that has its Ap still to rebuild rests on the kernel choice: formed under the options it was recorded with
    // (a copy: the list shrinks as the records close; a setter is not a reader; records that hold their Ap stay as they are)
    {
        LifetimeLock lock(lifetime_mutex());
        const std::vector<hmg_grid *> open = ctx->pend_grids;
        for (hmg_grid *g : open) settle_rebuild(g);
    }
    // the on / off options of the V-cycle's forms (what each one does: the members of hmg_ctx)
    static const std::pair<const char *, bool hmg_ctx::*> flags[] = {
        {"coarse_probe", &hmg_ctx::coarse_probe}, {"fuse_cg", &hmg_ctx::fuse_cg_default}, {"fold_x", &hmg_ctx::fold_x},
        {"swap_rp", &hmg_ctx::swap_rp}, {"fold_prolong", &hmg_ctx::fold_prolong}, {"zero_entry", &hmg_ctx::zero_entry},
        {"fold_restrict", &hmg_ctx::fold_restrict}, {"lazy_dead", &hmg_ctx::lazy_dead}, {"lazy_pre", &hmg_ctx::lazy_pre}, {"fold_coarse_x", &hmg_ctx::fold_coarse_x}, {"fold_faces", &hmg_ctx::fold_faces},
        {"lean_post", &hmg_ctx::lean_post}, {"lazy_post", &hmg_ctx::lazy_post}, {"lazy_r", &hmg_ctx::lazy_r}, {"lazy_ap", &hmg_ctx::lazy_ap}, {"lazy_x", &hmg_ctx::lazy_x}, {"prolong_in_image", &hmg_ctx::prolong_in_image},
        {"comm_rehearsal", &hmg_ctx::comm_rehearsal}};
    for (const auto &f : flags)
        if (n == f.first) {
            ctx->*f.second = value != 0;
            return 0;
        }
    if (n == "apply_threads")
        ctx->L.apply_threads = (int)value;
    else if (n == "apply_wg512")
        ctx->L.apply_wg512 = value != 0;
    else if (n == "apply_pack")            // 1 = default; 0: level 2 one cell per wave like levels 3-4 (A/B knob)
        ctx->L.apply_pack = value != 0;
    else if (n == "apply_small")           // 1 = default; 0: levels 2-4 keep k_apply<3,64,*> (A/B knob)
        ctx->L.apply_small = value != 0;
    else if (n == "weight_cache")          // 1 = default; 0: level 6 combines its class weights per cell (A/B knob)
        ctx->L.weight_cache = value != 0;
    else if (n == "weight_cache_classes")  // most distinct coefficient rows that still get a cache at the next operator (0 = default: no limit)
        ctx->wc_max_classes = std::max<int64_t>(0, value);
    else if (n == "apply_slab2")           // 1 = default; 0: cells larger than the LDS keep k_apply_slab (A/B knob)
        ctx->L.apply_slab2 = value != 0;
    else if (n == "restrict_slab2")        // 1 = default; 0: the stand-alone restriction keeps k_apply_slab (A/B knob)
        ctx->L.restrict_slab2 = value != 0;
    else if (n == "slab2_force")           // experiment: level 6 through the window kernel (needs HMG_SLAB_LDS_KB <= 30 at grid creation)
        ctx->L.slab2_force = value != 0;
    else if (n == "slab2_grid")            // its persistent workgroups (0 = default: one per CU; tests: fewer, many cells each)
        ctx->L.slab2_grid = std::max<int64_t>(0, value);
    else if (n == "apply_wave")            // 1 = default; 0: level 5 keeps the 256-thread kernel (A/B knob)
        ctx->L.apply_wave = value != 0;
    else if (n == "wave_grid")             // persistent waves per CU of the one-wave apply (default 16: what the LDS holds)
        ctx->L.wave_grid = std::max<int64_t>(1, value) * (int64_t)ctx->L.num_cu;
    else if (n == "wave_grid_total")       // ... as an absolute number of waves (tests: fewer waves than cells)
        ctx->L.wave_grid = std::max<int64_t>(1, value);
    else if (n == "cell_order")            // 1 = default: XCD-aware cell order of the register-blocked full-grid apply launches
        ctx->L.cell_order = value != 0;
    else if (n == "cell_moments_windows") {   // 0 = default: per-cell moments refuse cells larger than the LDS; 1: those take the window
        if (value < 0 || value > 2)           // kernels; 2: every level the window kernels can address does (test and A/B knob)
            throw std::runtime_error("option cell_moments_windows: 0, 1 or 2");
        ctx->moments_windows = (int)value;
    }
    else if (n == "cell_extrema_windows") {   // the same for hmg_cell_extrema (hmg_extrema_window.hip): 0 = default, 1, 2
        if (value < 0 || value > 2)
            throw std::runtime_error("option cell_extrema_windows: 0, 1 or 2");
        ctx->extrema_windows = (int)value;
    }
    else if (n == "cell_histogram_windows") {   // the same for hmg_cell_histogram (hmg_histogram_window.hip): 0 = default, 1, 2
        if (value < 0 || value > 2)
            throw std::runtime_error("option cell_histogram_windows: 0, 1 or 2");
        ctx->histogram_windows = (int)value;
    }
    else if (n == "cell_histogram_variant") {   // how hmg_cell_histogram's counts reach the LDS histogram: 0 one add per element,
        if (value < 0 || value > 2)             // 1 = default: a node's elements combined first, 2: and the wave's first bin summed
            throw std::runtime_error("option cell_histogram_variant: 0, 1 or 2");   // across lanes (A/B knob: the same ints from each)
        ctx->histogram_variant = (int)value;
    }
    else if (n == "coarse_poly")           // Chebyshev iterates per preconditioner application of the level-1 PCG (1 = Jacobi)
        ctx->coarse_poly = std::max<int>(1, std::min<int>(16, (int)value));
    else if (n == "coarse_maxit")
        ctx->coarse_maxit = (int)value;
    else if (n == "coarse_check")
        ctx->coarse_check = std::max<int>(1, (int)value);
    else if (n == "lazy_top")
        ctx->lazy_top = (int)value;
    else if (n == "overlap_min_doubles")
        ctx->overlap_min_doubles = value;
    else if (n == "vec_pool") {
        ctx->vec_pool_on = value != 0;
        if (!ctx->vec_pool_on) vec_pool_trim(ctx);
    }
    else if (n == "time_apply") {   // value = minimum level to time, 0 = off; resets the counters
        ctx->timer.on = value > 0;
        ctx->timer.min_level = (int)value;
        ctx->timer.used = 0;
        ctx->timer.ev_level.clear();
        ctx->timer.ev_bytes.clear();
    }
    else
        throw std::runtime_error("unknown option: " + n);
    HMG_END
}

int hmg_ctx_set_option_f64(hmg_ctx *ctx, const char *name, double value)
{
    HMG_TRY
    need(ctx && name, "null argument");
    std::string n(name);
    if (n == "coarse_rtol")
        ctx->coarse_rtol = value;
    else if (n == "coarse_poly_ratio")     // lmax / lmin of the interval the level-1 PCG's Chebyshev preconditioner is built for
        ctx->coarse_poly_ratio = value;
    else
        throw std::runtime_error("unknown option: " + n);
    HMG_END
}

void *hmg_ctx_scalar_bank(hmg_ctx *ctx) { return ctx ? (void *)ctx->L.scal : nullptr; }

/* Replace the library's scalar bank (16 device doubles) by caller-owned device memory, e.g. a torch
 * tensor that torch.distributed can all-reduce in place. */
int hmg_ctx_set_scalar_bank(hmg_ctx *ctx, void *device_doubles16)
{
    HMG_TRY
    need(ctx != nullptr, "null argument");
    HIPCHK(hipStreamSynchronize(ctx->stream));
    double *to = device_doubles16 ? (double *)device_doubles16 : ctx->scal.p;   // NULL: back to the library's own bank
    if (to != ctx->L.scal) HIPCHK(hipMemcpy(to, ctx->L.scal, S_COUNT * sizeof(double), hipMemcpyDeviceToDevice));
    ctx->L.scal = to;
    HMG_END
}

// the timed operator applies of one level, or of every level, since option "time_apply" was last set
static int apply_timing(hmg_ctx *ctx, bool every, int level, int64_t *launches, double *total_ms, double *total_bytes)
{
    HMG_TRY
    need(ctx && launches && total_ms && total_bytes, "null argument");
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const ApplyTimer &tm = ctx->timer;
    double ms = 0.0, by = 0.0;
    int64_t n = 0;
    for (size_t i = 0; i < tm.used; ++i) {
        if (!every && tm.ev_level[i] != level) continue;
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, tm.pool[i].first, tm.pool[i].second));
        ms += t;
        by += tm.ev_bytes[i];
        n += 1;
    }
    *launches = n;
    *total_ms = ms;
    *total_bytes = by;
    HMG_END
}

int hmg_ctx_apply_timing(hmg_ctx *ctx, int64_t *launches, double *total_ms, double *total_bytes)
{
    return apply_timing(ctx, true, 0, launches, total_ms, total_bytes);
}

int hmg_ctx_apply_timing_level(hmg_ctx *ctx, int level, int64_t *launches, double *total_ms, double *total_bytes)
{
    return apply_timing(ctx, false, level, launches, total_ms, total_bytes);
}

void *hmg_ctx_stream(hmg_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int hmg_grid_destroy(hmg_grid *grid)
{
    HMG_TRY
    grid_unref(grid);
    HMG_END
}

// ---- vectors ----------------------------------------------------------------------------------
int hmg_vec_create(hmg_grid *g, int level, hmg_vec **out)
{
    HMG_TRY
    need(g && out, "null argument");
    const LevelDev &lv = lev(g, level);
    HIPCHK(hipSetDevice(g->ctx->device));
    std::unique_ptr<hmg_vec> v(new hmg_vec);
    v->g = g;
    v->level = level;
    v->own = true;
    v->alloc_cells = g->md.ncells;
    size_t bytes = sizeof(double) * (size_t)lv.ld * (size_t)g->md.ncells;
    ensure_reduce_scratch(g->ctx, (int64_t)lv.ld * g->md.ncells);
    v->d = vec_alloc(g->ctx, bytes);
    v->bytes = bytes;
    if (wants_top_spare(g, level)) (void)reserve_top_spare(g, false);
    {
        LifetimeLock lock(lifetime_mutex());
        g->refs += 1;
    }
    *out = v.release();
    HMG_END
}

int hmg_vec_wrap(hmg_grid *g, int level, void *device_ptr, hmg_vec **out)
{
    HMG_TRY
    need(g && out && device_ptr, "null argument");
    // (the streaming kernels read and write the storage as double2, hmg_kernels.hip; checked before anything is allocated)
    need(((uintptr_t)device_ptr & 15u) == 0, "hmg_vec_wrap: device_ptr must be 16-byte aligned (the vector kernels move pairs of doubles)");
    ensure_reduce_scratch(g->ctx, (int64_t)lev(g, level).ld * g->md.ncells);
    std::unique_ptr<hmg_vec> v(new hmg_vec);
    v->g = g;
    v->level = level;
    v->own = false;
    v->alloc_cells = g->md.ncells;
    v->d = (double *)device_ptr;
    if (wants_top_spare(g, level)) (void)reserve_top_spare(g, false);
    {
        LifetimeLock lock(lifetime_mutex());
        g->refs += 1;
    }
    *out = v.release();
    HMG_END
}

int hmg_vec_destroy(hmg_vec *v)
{
    HMG_TRY
    if (v) {
        LifetimeLock lock(lifetime_mutex());
        if (!pending_keeps(v)) release_vec(v);
    }
    HMG_END
}

// From here on the memory can be read behind the library's back: a pending r-update on the vector is formed now, and V-cycles on it
// take the eager tail.
void *hmg_vec_device_ptr(hmg_vec *v)
{
    if (!v) return nullptr;
    try {
        settle(v);
    } catch (const std::exception &e) {
        (void)fail(e);
        return nullptr;
    }
    v->exposed = true;
    return (void *)v->d;
}

}  // extern "C"

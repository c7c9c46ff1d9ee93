// hmg_fcg_*: flexible CG with one retained direction (Notay's FCG(1)) on the top level, preconditioned by one hmg_vcycle.
//
// Storage forms: x, z and p are consistent (every copy of a shared node holds the same value), b, R and q = A_loc p are loads
// (the copies add up to the global value; A_loc = the cell-local apply with the Dirichlet mask, without the interface sum).
// The plain dot product over the storage of a consistent vector with a load is the global inner product, so the outer
// iteration has no interface sum and no cut exchange of its own -- only the V-cycle inside it communicates, plus two small
// sums over the ranks per step.
//
//   start   R = b - A_loc x (Dirichlet rows zero)
//   step    z = V(0, R);  first step p = z, later beta = -(z.q) / (p.q)_prev, p = z + beta p;  q = A_loc p;
//           alpha = (p.R) / (p.q);  x += alpha p;  R -= alpha q
//
// Everything a step does is enqueued on the context's stream; alpha and beta are formed on the device.
#include "../../include/hmg.h"
#include "hmg_fcg.hpp"
#include "hmg_objects.hpp"

// (the handle crosses the C ABI as void *)
struct hmg_fcg {
    int refs = 1;
    hmg_grid *g = nullptr;
    hmg_ctx *ctx = nullptr;
    int level = 0, steps = 0, steps_coarse = 0;
    hmg_vec *p = nullptr, *q = nullptr, *R = nullptr;    // setup memory: three vectors of the top level's size
    double *scratch = nullptr;                           // F_COUNT scalars | 512 folded partials | block partials
    int64_t nb_cap = 0;                                  // blocks the partials hold
    int64_t vec_bytes = 0;
    bool started = false, have_dir = false;
    uint64_t epoch = 0;                                  // the grid's operator count at the last start
};

namespace {

// a call of the C ABI from inside: its message is already in hmg_last_error
void ok(int rc)
{
    if (rc != 0) throw std::runtime_error(last_error());
}

FcgLaunch launch_of(hmg_fcg *f)
{
    FcgLaunch F{};
    F.stream = f->ctx->stream;
    F.fs = f->scratch;
    F.fold = f->scratch + F_COUNT;
    F.part = f->scratch + F_COUNT + 512;
    F.bank = f->ctx->L.scal;                             // (read per call: hmg_ctx_set_scalar_bank may have moved it)
    need(F.bank != nullptr, "the context has no scalar bank");
    return F;
}

void release(hmg_fcg *f)
{
    if (f->p) (void)hmg_vec_destroy(f->p);
    if (f->q) (void)hmg_vec_destroy(f->q);
    if (f->R) (void)hmg_vec_destroy(f->R);
    if (f->scratch) {                                    // (set after the context, as vec_bytes is)
        LifetimeLock lock(lifetime_mutex());
        (void)hipStreamSynchronize(f->ctx->stream);
        (void)hipFree(f->scratch);
        f->ctx->fcg_bytes -= 3 * f->vec_bytes;
    }
    delete f;
}

void check_states(hmg_fcg *f, hmg_vec **states)
{
    need(states != nullptr, "null states");
    for (int l = 1; l <= f->level; ++l)
        for (int k = 0; k < 5; ++k)   // (a pending r-update of the last V-cycle: settled or dropped by whoever touches r or Ap next)
            check_vec(f->g, l, states[5 * (l - 1) + k], "states[]", /*settle_pending=*/false);
}

void need_current(hmg_fcg *f, const char *what)
{
    if (!f->started) throw std::runtime_error(std::string(what) + ": hmg_fcg_start has not been called");
    if (f->epoch != f->g->op_epoch)
        throw std::runtime_error(std::string(what) + ": the grid was shrunk or its operator, lambda or smoother changed since hmg_fcg_start; "
                                 "the residual and the direction belong to the old operator -- call hmg_fcg_start again");
}

}  // namespace

extern "C" {

int hmg_fcg_create(hmg_grid *grid, int top_level, int steps, int steps_coarse, void **out)
{
    HMG_TRY
    need(grid && out, "null argument");
    need(top_level >= 1 && top_level <= hmg_grid_nlevels(grid), "top_level out of range");
    need(steps >= 0 && steps_coarse >= 0, "negative number of smoothing steps");
    hmg_fcg *f = new hmg_fcg;
    f->g = grid;
    f->level = top_level;
    f->steps = steps;
    f->steps_coarse = steps_coarse;
    try {
        const int64_t n = (int64_t)lev(grid, top_level).ld * grid->md.ncells;     // (lev: a host-only grid has no compute path)
        f->ctx = grid->ctx;
        // p, q, R: from the context's pool of level-vector memory; a vector that does not fit is an error, there is no
        // form of the iteration without them
        ok(hmg_vec_create(grid, top_level, &f->p));
        ok(hmg_vec_create(grid, top_level, &f->q));
        ok(hmg_vec_create(grid, top_level, &f->R));
        f->nb_cap = fcg_blocks(n);
        const size_t sbytes = sizeof(double) * (size_t)(F_COUNT + 512 + 2 * f->nb_cap);
        HIPCHK(hipSetDevice(f->ctx->device));
        hipError_t e = device_malloc((void **)&f->scratch, sbytes);
        if (e != hipSuccess)
            throw std::runtime_error(std::string("hipMalloc of the reduction scratch (") + std::to_string(sbytes >> 10) +
                                     " KiB) failed: " + hipGetErrorString(e));
        HIPCHK(hipMemsetAsync(f->scratch, 0, sbytes, f->ctx->stream));
        f->vec_bytes = (int64_t)sizeof(double) * n;
        LifetimeLock lock(lifetime_mutex());
        f->ctx->fcg_bytes += 3 * f->vec_bytes;
    } catch (const std::exception &e) {
        const std::string why = e.what();
        release(f);
        throw std::runtime_error("hmg_fcg_create: " + why);
    }
    *out = f;
    HMG_END
}

int hmg_fcg_destroy(void *handle)
{
    HMG_TRY
    hmg_fcg *fcg = (hmg_fcg *)handle;
    if (fcg && --fcg->refs <= 0) release(fcg);
    HMG_END
}

int hmg_fcg_start(void *handle, hmg_vec *x, hmg_vec *b, hmg_vec **states)
{
    HMG_TRY
    hmg_fcg *f = (hmg_fcg *)handle;
    need(f && x && b, "null argument");
    check_states(f, states);
    const int64_t n = vec_len(f->R);
    need(fcg_blocks(n) <= f->nb_cap, "the grid has grown since hmg_fcg_create");
    hmg_vec **top = states + 5 * (f->level - 1);
    for (int k = 0; k < 5; ++k)
        need(x != top[k], "x must not be one of the top level's state vectors: the V-cycle inside a step overwrites them");
    f->started = false;
    ensure_smoother_diag(f->g, f->level, states);
    ok(hmg_apply_ex(f->g, f->level, -1.0, x, b, f->R, 1));      // R = b - A_loc x, Dirichlet rows zeroed
    f->have_dir = false;
    f->epoch = f->g->op_epoch;
    f->started = true;
    HMG_END
}

int hmg_fcg_step(void *handle, hmg_vec *x, hmg_vec **states)
{
    HMG_TRY
    hmg_fcg *f = (hmg_fcg *)handle;
    need(f && x, "null argument");
    need_current(f, "hmg_fcg_step");
    check_states(f, states);
    const int64_t n = vec_len(f->R);
    check_vec(f->g, f->level, x, "x");
    hmg_vec **top = states + 5 * (f->level - 1);
    for (int k = 0; k < 5; ++k) need(x != top[k], "x must not be one of the top level's state vectors");
    check_vec(f->g, f->level, f->p, "p");
    check_vec(f->g, f->level, f->q, "q");
    check_vec(f->g, f->level, f->R, "R");
    ensure_smoother_diag(f->g, f->level, states);
    double *xd = x->d, *pd = f->p->d, *qd = f->q->d, *Rd = f->R->d;
    // z = V(0, R): the V-cycle takes R where the top level's b stands (the handle, not a copy) and leaves z in the top level's x
    hmg_vec *b_keep = top[1];
    top[1] = f->R;
    try {
        // (with a direction to combine with, the first reader of z is the pass that forms z.q: it can take z's last updates)
        vcycle(f->g, f->level, f->steps, f->steps_coarse, states, /*top=*/true, /*zero_guess=*/true, /*lazy_x=*/f->have_dir);
    } catch (...) {
        top[1] = b_keep;
        throw;
    }
    top[1] = b_keep;
    const double *zd = top[0]->d;                        // (read after the V-cycle, which exchanges device pointers of handles)
    const FcgLaunch F = launch_of(f);
    if (f->have_dir) {
        const PendingX px = take_pending_x(f->g, top[0]);
        if (px.form)
            // z = x lacks its last two or three CG updates (option lazy_x): formed where z.q reads it, 48 B/DOF instead of 40 + 16
            launch_fcg_dot_zq_x(F, top[0]->d, saved_updates(f->g, px), qd, n);
        else
            launch_fcg_dot_zq(F, zd, qd, n);
        scalar_sum(f->g, FB_ZQ, 1);
    }
    launch_fcg_direction(F, pd, zd, n, f->have_dir ? 0 : 1);
    f->have_dir = true;
    ok(hmg_apply_ex(f->g, f->level, 1.0, f->p, nullptr, f->q, 1));          // q = A_loc p, Dirichlet rows zeroed
    launch_fcg_dots_pq_pr(F, pd, qd, Rd, n);
    scalar_sum(f->g, FB_PQ, 2);
    launch_fcg_update(F, xd, Rd, pd, qd, n);
    HMG_END
}

int hmg_fcg_residual_norm(void *handle, hmg_vec **states, double *norm)
{
    HMG_TRY
    hmg_fcg *f = (hmg_fcg *)handle;
    need(f && norm, "null argument");
    need_current(f, "hmg_fcg_residual_norm");
    check_states(f, states);
    hmg_vec *r = states[5 * (f->level - 1) + 2];          // the top level's r: scratch between two V-cycles
    ok(hmg_vec_copy(r, f->R));
    ok(hmg_interface_sum(f->g, f->level, r));
    ok(hmg_vec_norm_unique(r, norm));
    HMG_END
}

int hmg_fcg_scalars(void *handle, double *out)
{
    HMG_TRY
    hmg_fcg *f = (hmg_fcg *)handle;
    need(f && out, "null argument");
    double h[F_COUNT];
    if (hipMemcpyAsync(h, f->scratch, sizeof(h), hipMemcpyDeviceToHost, f->ctx->stream) != hipSuccess)
        throw std::runtime_error("hmg_fcg_scalars: copy from the device failed");
    ok(hmg_ctx_sync(f->ctx));
    out[0] = h[F_ALPHA];
    out[1] = h[F_BETA];
    out[2] = h[F_PQ];
    out[3] = h[F_PR];
    HMG_END
}

hmg_vec *hmg_fcg_vec(void *handle, int which)
{
    hmg_fcg *f = (hmg_fcg *)handle;
    if (!f) return nullptr;
    return which == 0 ? f->p : which == 1 ? f->q : which == 2 ? f->R : nullptr;
}

}  // extern "C"

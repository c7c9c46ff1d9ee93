// The level-1 system: assembly to the device, its PCG with the Chebyshev preconditioner, the probes that budgeted solves
// leave behind and their verdicts; with the entry points that front them (hmg_coarse_*).
#include "../../include/hmg.h"
#include "hmg_objects.hpp"

#include <algorithm>
#include <cmath>

namespace hmg {

void probe_unlist(hmg_grid *g)
{
    if (!g->ctx) return;
    auto &v = g->ctx->probe_grids;
    v.erase(std::remove(v.begin(), v.end(), g), v.end());
}

namespace {

// Iterations a later solve enqueues blindly, from the count the last judged solve needed.  Plain Jacobi-PCG: 1.5 x + 16 (the
// count moves by 10-20 % from one right-hand side to the next; a no-op iteration costs two launches of ~3 us).  With the
// polynomial preconditioner an iteration is k + 1 launches and takes the residual down by a larger, steadier factor (config 3:
// 27 iterations where plain PCG needs 99): 1.25 x + 4 -- at 1.5 x + 16 the no-op tail was a third of the solve.
int coarse_budget_for(const hmg_ctx *c, int last_it)
{
    return c->coarse_poly > 1 ? last_it + last_it / 4 + 4 : last_it + last_it / 2 + 16;
}

// A new level-1 matrix is about to replace the one the pending probe belongs to: wait for it, count a miss, drop it.
void coarse_probe_drop(hmg_grid *g)
{
    if (!g->probe || !g->probe->pending) return;
    CoarseProbe &pr = *g->probe;
    (void)hipEventSynchronize(pr.ev);
    pr.pending = false;
    probe_unlist(g);
    if (pr.h[0] == 0.0 && pr.h[3] > 0.0) g->coarse_misses += 1;
}

// Blocks until the probe of the last budgeted solve has landed and judges it.  A solve that ran out of its budget is an
// error (its unconverged x has already been prolonged): the budget is reset, so the caller may simply repeat the V-cycle
// -- the next solve counts its iterations the slow way.
void coarse_probe_wait(hmg_grid *g)
{
    if (!g->probe || !g->probe->pending) return;
    CoarseProbe &pr = *g->probe;
    HIPCHK(hipEventSynchronize(pr.ev));
    pr.pending = false;
    probe_unlist(g);
    if (pr.generation != g->coarse_generation) return;      // (a solve on a matrix that is gone: coarse_probe_drop counts those)
    const double done = pr.h[0], rr = pr.h[2], bb = pr.h[3];
    g->coarse_last_it = (int)pr.h[1];
    if (!std::isfinite(rr) || !std::isfinite(bb)) throw std::runtime_error("coarse PCG diverged (non-finite residual)");
    if (done == 0.0 && bb > 0.0) {
        g->coarse_budget = 0;                      // next solve: find the count the slow way again
        g->coarse_misses += 1;
        throw std::runtime_error("coarse PCG: the last level-1 solve did not reach coarse_rtol within the " +
                                 std::to_string(pr.budget) + " iterations enqueued for it (relative residual " +
                                 std::to_string(std::sqrt(rr / bb)) + "); the V-cycle that used it is inexact -- repeat it, "
                                 "the next solve counts its iterations again");
    }
    g->coarse_budget = std::max(g->coarse_budget, std::min(g->ctx->coarse_maxit, coarse_budget_for(g->ctx, g->coarse_last_it)));
}

void coarse_setup(hmg_grid *g)
{
    need(g->has_op, "hmg_grid_set_operator must be called first");
    const MeshTables &M = g->part ? g->part->global : g->cur();
    // (the constants are in the kernel: solved on their complement where the grid says so, hmg_grid_set_mean_free)
    g->coarse_singular = g->lambda == 0.0 && std::find(M.node_on_boundary.begin(), M.node_on_boundary.end(), (uint8_t)1) == M.node_on_boundary.end();
    if (g->coarse_singular && !g->mean_free)
        throw std::runtime_error("hmg_coarse_setup: no node is constrained (hmg_grid_set_dirichlet_faces with an empty set) and "
                                 "lambda = 0: the level-1 matrix is singular");
    assemble_coarse_matrix(M, g->part ? g->sigma_global.data() : g->sigma.data(), g->sig_n, g->lambda, g->cm);
    DryUploads dry_scope(!g->ctx, &g->upload_hash);
    hipStream_t s = g->ctx ? g->ctx->stream : nullptr;
    g->c_rowptr.upload(g->cm.rowptr, s);
    g->c_colidx.upload(g->cm.colidx, s);
    g->c_val.upload(g->cm.val, s);
    g->c_diag.upload(g->cm.diag, s);
    g->c_interior.upload(g->cm.interior, s);
    size_t n = (size_t)std::max<int64_t>(g->cm.n, 1);
    g->c_b.alloc(n);
    g->c_x.alloc(n);
    g->c_r.alloc(n);
    g->c_z.alloc(n);
    g->c_p.alloc(n);
    g->c_q.alloc(n);
    g->c_z2.alloc(n);
    g->c_d.alloc(n);
    {
        // lmax(D^-1 A) <= max_i sum_j |a_ij| / a_ii: an upper bound that HOLDS (the Chebyshev polynomial of the preconditioner must
        // stay positive on the whole spectrum)
        double lmax = 0.0;
        for (int64_t i = 0; i < g->cm.n; ++i) {
            double sabs = 0.0;
            for (int32_t k = g->cm.rowptr[(size_t)i]; k < g->cm.rowptr[(size_t)i + 1]; ++k) sabs += std::fabs(g->cm.val[(size_t)k]);
            if (g->cm.diag[(size_t)i] > 0.0) lmax = std::max(lmax, sabs / g->cm.diag[(size_t)i]);
        }
        g->c_lmax = lmax > 0.0 ? lmax : 2.0;
    }
    g->c_u.alloc((size_t)M.nnodes);
    g->cd.n = g->cm.n;
    g->cd.rowptr = g->c_rowptr.p;
    g->cd.colidx = g->c_colidx.p;
    g->cd.val = g->c_val.p;
    g->cd.diag = g->c_diag.p;
    g->cd.interior = g->c_interior.p;
    if (!g->ctx) return;                           // (host-only grid: the matrix is assembled and checksummed, there is nothing to solve on)
    if (!g->probe->h) {
        HIPCHK(hipHostMalloc((void **)&g->probe->h, 4 * sizeof(double), hipHostMallocDefault));
        HIPCHK(hipEventCreateWithFlags(&g->probe->ev, hipEventDisableTiming));
        device_allocs() += 1;
    }
    g->coarse_ready = true;
    // New matrix: the first solve counts its iterations again.  A probe the previous matrix's last solve left behind is
    // waited for and dropped here -- judged by coarse_pcg() it would put the old matrix's count back into the budget
    // (max), and the first solve on the new, possibly harder, system would be enqueued blindly with it.
    coarse_probe_drop(g);
    g->coarse_generation += 1;
    g->coarse_budget = 0;
}

void coarse_pcg(hmg_grid *g)
{
    // CG (preconditioner: coarse_poly Chebyshev iterates of the Jacobi-scaled operator; 1 = plain Jacobi) on (lambda M + K_sigma)[interior, interior] x = b to a relative residual of
    // coarse_rtol; stands in for the reference's CHOLMOD solve (src/multigrid.jl:84).
    // Convergence is decided on the device: k_coarse_pupdate sets a flag once r.r <= rtol^2 b.b and every kernel of
    // the later iterations returns at once, so a fixed number of iterations can be enqueued without a host round trip.
    // The first solve after a (re)assembly finds that number the slow way (a look every coarse_check iterations);
    // later solves enqueue the budget coarse_budget_for() gives, leave a probe (flag, count, r.r) behind in pinned
    // memory and return; the probe is checked at the next solve (or when the iteration count is asked for).
    hmg_ctx *c = g->ctx;
    const Launch &L = c->L;
    const CoarseDev &A = g->cd;
    if (A.n == 0) {
        g->coarse_last_it = 0;
        return;
    }
    coarse_probe_wait(g);                          // the previous solve's verdict (throws if it did not converge)
    CoarseProbe &pr = *g->probe;
    need(pr.h != nullptr, "level-1 solve without a level-1 system (coarse_setup)");
    const double rtol2 = c->coarse_rtol * c->coarse_rtol;
    // Polynomial preconditioner (round 4): z = p_{k-1}(D^-1 A) D^-1 r by k - 1 Chebyshev steps behind the init / update kernel (each
    // one sparse product, no reduction) -- an outer iteration is k + 1 launches for k products instead of two launches and two
    // grid-wide sums per product; about a third fewer launches to the same residual at config 3, half the time at 64^3 cubes.
    const int kpoly = std::max(1, c->coarse_poly);
    const double lmax = 1.02 * g->c_lmax, lmin = lmax / std::max(2.0, c->coarse_poly_ratio);
    const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin), sigma1 = theta / delta;
    double *dch = kpoly > 1 ? g->c_d.p : nullptr;
    const double zscale = 1.0 / theta;
    const double *zfinal = g->c_z.p;
    auto cheb_steps = [&]() {            // z_1 (in c_z, d in c_d) -> z_k; returns where it is
        double rho = 1.0 / sigma1;
        const double *zin = g->c_z.p;
        double *zout = g->c_z2.p;
        for (int j = 1; j < kpoly; ++j) {
            const double rho_n = 1.0 / (2.0 * sigma1 - rho);
            launch_coarse_cheb(L, A, g->c_r.p, zin, zout, g->c_d.p, rho_n * rho, 2.0 * rho_n / delta, j == kpoly - 1 ? 1 : 0);
            rho = rho_n;
            const double *t = zin;
            zin = zout;
            zout = const_cast<double *>(t);
        }
        zfinal = zin;
    };
    launch_coarse_init(L, A, g->c_b.p, g->c_x.p, g->c_r.p, g->c_z.p, g->c_p.p, zscale, dch);
    if (kpoly > 1) {
        cheb_steps();
        launch_coarse_rz_from_cheb(L, A);       // r.z of the first iteration
    }
    int slot_old = S_C0, slot_new = S_C3;          // r.z of the current / next iteration
    // One iteration = two launches (k_coarse_direction, k_coarse_update; three until round 3).  The direction launch of
    // iteration j does the bookkeeping of update j-1 (beta, convergence flag, count); a batch ends with a bookkeeping-only
    // launch so that the flag and the count the host (or the probe) reads are those of its last update.
    bool first = true, counted = true;
    auto iterate = [&](int count) {
        for (int q = 0; q < count; ++q) {
            if (first)
                launch_coarse_direction(L, A, g->c_p.p, g->c_q.p, zfinal, slot_old, slot_new, rtol2, 1, 0, kpoly > 1);
            else {
                launch_coarse_direction(L, A, g->c_p.p, g->c_q.p, zfinal, slot_old, slot_new, rtol2, 0, counted ? 0 : 1, kpoly > 1);
                std::swap(slot_old, slot_new);     // (the launch has published the new r.z in the other slot)
            }
            first = false;
            launch_coarse_update(L, A, g->c_x.p, g->c_r.p, g->c_z.p, g->c_p.p, g->c_q.p, slot_old, zscale, dch);
            if (kpoly > 1) cheb_steps();
            counted = false;
        }
        // bookkeeping of the batch's last update (leaves the slots alone: the next regular launch publishes the same value again)
        launch_coarse_direction(L, A, g->c_p.p, g->c_q.p, zfinal, slot_old, slot_new, rtol2, 2, 1, kpoly > 1);
        counted = true;
    };
    auto probe = [&]() {
        HIPCHK(hipMemcpyAsync(pr.h, L.scal + S_DONE, 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(pr.h + 3, L.scal + S_C2, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipEventRecord(pr.ev, c->stream));
        pr.pending = true;
        pr.generation = g->coarse_generation;
        if (std::find(c->probe_grids.begin(), c->probe_grids.end(), g) == c->probe_grids.end()) c->probe_grids.push_back(g);
    };
    if (g->coarse_budget > 0) {
        iterate(g->coarse_budget);
        pr.budget = g->coarse_budget;
        if (c->coarse_probe) probe();
        return;
    }
    int it = 0;
    while (it < c->coarse_maxit) {
        const int chunk = std::min(c->coarse_check, c->coarse_maxit - it);
        iterate(chunk);
        it += chunk;
        pr.budget = it;
        probe();
        HIPCHK(hipEventSynchronize(pr.ev));
        pr.pending = false;                        // judged right here
        probe_unlist(g);
        const double done = pr.h[0], rr = pr.h[2], bb = pr.h[3];
        if (!std::isfinite(rr) || !std::isfinite(bb)) throw std::runtime_error("coarse PCG diverged (non-finite residual)");
        if (done != 0.0 || !(bb > 0.0)) break;
        if (it >= c->coarse_maxit)
            throw std::runtime_error("coarse PCG: no convergence to coarse_rtol within coarse_maxit iterations");
    }
    g->coarse_last_it = (int)pr.h[1];
    // (b = 0: every kernel returned at once and the count is 0, which says nothing about the next right-hand side -- a budget
    // from it, four iterations, made the next solve a miss; that one counts its iterations instead)
    if (pr.h[3] > 0.0) g->coarse_budget = std::min(c->coarse_maxit, coarse_budget_for(c, g->coarse_last_it));
}

// The solve on the range of a matrix with the constants in its kernel: the mean leaves the right-hand side in front of the PCG --
// whose b.b, and with it the stopping rule, is then that of the projected right-hand side -- and the solution behind it.  Both in
// the stream: the blind iterations and the probe between them are what they are for a regular matrix.
void coarse_pcg_on_range(hmg_grid *g)
{
    if (!g->coarse_singular) return coarse_pcg(g);
    launch_coarse_remove_mean(g->ctx->L, g->cd, g->c_b.p);
    coarse_pcg(g);
    launch_coarse_remove_mean(g->ctx->L, g->cd, g->c_x.p);
}

}  // namespace

// Called wherever the API has just synchronised the context's stream: probes that have landed by then are judged at once,
// so an unconverged budgeted solve is reported by the call that follows its V-cycle (the driver's integrals / residual
// norm), not by the next V-cycle -- and the last V-cycle of a run is judged as well.
void judge_probes(hmg_ctx *c)
{
    while (!c->probe_grids.empty()) {
        hmg_grid *g = c->probe_grids.back();
        c->probe_grids.pop_back();                 // first: the verdict may throw, and a listed grid need not be pending
        coarse_probe_wait(g);
    }
}

void coarse_solve(hmg_grid *g, hmg_vec *b1, hmg_vec *x1)
{
    // ref: src/multigrid.jl:74-93
    if (!g->coarse_ready) coarse_setup(g);
    const LevelDev &lv = lev(g, 1);
    const Launch &L = g->ctx->L;
    interface_sum(g, lv, b1->d);
    if (g->part) {
        // Replicated coarse solve: every rank contributes the nodes it owns to a global nodal vector
        // (one sum over ranks), solves the whole level-1 system, and scatters to its own cells.
        need(g->exchange != nullptr, "partitioned grid: hmg_grid_set_exchange must be called before a coarse solve");
        const int64_t ng = g->part->global.nnodes;
        need(ng <= g->ex_cap, "exchange buffer too small for the coarse gather");
        launch_fill(L, g->ex_buf, ng, 0.0);
        launch_gather_owned(L, g->md, g->d_nodes_g.p, g->d_owned.p, lv.ld, b1->d, g->ex_buf);
        if (g->exchange(g->ex_user, g->ex_buf, ng) != 0) throw std::runtime_error("exchange callback failed");
        launch_coarse_gather_rhs(L, g->cd, g->ex_buf, g->c_b.p);
        coarse_pcg_on_range(g);
        launch_coarse_scatter_sol(L, g->cd, ng, g->c_x.p, g->c_u.p);
        launch_scatter_cells(L, g->d_cells_gnode.p, g->md.ncells, g->dim + 1, lv.ld, g->c_u.p, x1->d);
        return;
    }
    launch_gather_base(L, g->md, lv.ld, b1->d, g->c_u.p);
    launch_coarse_gather_rhs(L, g->cd, g->c_u.p, g->c_b.p);
    coarse_pcg_on_range(g);
    launch_coarse_scatter_sol(L, g->cd, g->md.nnodes, g->c_x.p, g->c_u.p);
    launch_scatter_base(L, g->md, lv.ld, g->c_u.p, x1->d);
}

}  // namespace hmg

extern "C" {

int hmg_coarse_setup(hmg_grid *g)
{
    HMG_TRY
    need(g != nullptr, "null grid");
    coarse_setup(g);
    HMG_END
}

int hmg_coarse_solve(hmg_grid *g, hmg_vec *b1, hmg_vec *x1)
{
    HMG_TRY
    need(g && g->has_op, "operator not set");
    check_vec(g, 1, b1, "b1");
    check_vec(g, 1, x1, "x1");
    coarse_solve(g, b1, x1);
    HMG_END
}

int hmg_coarse_last_iterations(const hmg_grid *g)
{
    if (!g) return -1;
    try {
        coarse_probe_wait(const_cast<hmg_grid *>(g));
    } catch (const std::exception &e) {
        last_error() = e.what();
        return -1;
    }
    return g->coarse_last_it;
}

int64_t hmg_coarse_misses(const hmg_grid *g) { return g ? g->coarse_misses : -1; }

}  // extern "C"

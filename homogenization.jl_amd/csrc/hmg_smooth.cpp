// The operator apply with its interface sums and reductions, the CG smoother in the form its caller's reads allow, the V-cycle
// and the placement tuner, on one HIP stream with device-resident CG scalars; with the entry points that front them
// (hmg_smooth, hmg_vcycle*, hmg_level_tune_placement, hmg_grid_reserve_spare).
#include "../../include/hmg.h"
#include "hmg_objects.hpp"
#include "hmg_cheb.hpp"
#include "hmg_pcg.hpp"

#include <algorithm>
#include <cmath>

namespace hmg {

void set_slab(hmg_grid *g, const LevelDev &lv)
{
    const LevelBufs &B = *g->lb[lv.level - 1];
    g->md.slab.head = B.slab_head.p;
    g->md.slab.ld_word = B.slab_ld_word.p;
    g->md.slab.cp_word = B.slab_cp_word.p;
    g->md.slab.cp_slot = B.slab_cp_slot.p;
    g->md.slab.nslab = B.nslab;
    g->md.slab.lds_nodes = B.slab_lds_nodes;
    g->md.slab.max_surf = B.slab_max_surf;
    g->md.slab.max_int = B.slab_max_int;
}

namespace {

struct TimedRegion {   // HIP-event bracket of an operator apply (bench.py roofline): every apply goes through one
    hmg_ctx *c;
    bool timed;
    int level;
    double bytes;          // algorithmic HBM bytes of the launch
    TimedRegion(hmg_grid *g, const LevelDev &lv, double bytes_) : c(g->ctx), level(lv.level), bytes(bytes_)
    {
        ApplyTimer &t = c->timer;
        timed = t.on && lv.level >= t.min_level;
        if (!timed) return;
        if (t.used == t.pool.size()) {
            hipEvent_t a, b;
            HIPCHK(hipEventCreate(&a));
            HIPCHK(hipEventCreate(&b));
            t.pool.emplace_back(a, b);
        }
        HIPCHK(hipEventRecord(t.pool[t.used].first, c->stream));
    }
    void stop()
    {
        if (!timed) return;
        ApplyTimer &t = c->timer;
        HIPCHK(hipEventRecord(t.pool[t.used].second, c->stream));
        t.used += 1;
        t.ev_level.push_back(level);
        t.ev_bytes.push_back(bytes);
        timed = false;
    }
};

}  // namespace

// every operator apply goes through here: optional HIP-event bracketing for bench.py's roofline
void apply(hmg_grid *g, const LevelDev &lv, double alpha, const double *x, const double *src, double *out, int mask)
{
    TimedRegion tr(g, lv, 8.0 * (double)lv.nf * (double)g->md.ncells * (src ? 3.0 : 2.0));
    set_slab(g, lv);
    ensure_weight_cache(g);
    launch_apply(g->ctx->L, lv, g->md, alpha, g->lambda, x, src, out, mask);
    tr.stop();
}

void restrict_level(hmg_grid *g, int level_fine, const double *rf, double *bc)
{
    // ref: src/interpolation.jl:52-62
    const LevelDev &fine = lev(g, level_fine), &coarse = lev(g, level_fine - 1);
    const LevelBufs &B = *g->lb[level_fine - 1];
    if (B.slab_rs_head.p) {
        LevelDev fr = fine;
        fr.ctab = B.rtab.p;
        SlabTables st{};
        st.head = B.slab_rs_head.p;
        st.ld_word = B.slab_ld_word.p;
        st.cp_word = B.slab_rs_word.p;
        st.cp_slot = B.slab_rs_slot.p;
        st.nslab = B.nslab;
        st.lds_nodes = B.slab_lds_nodes;
        st.max_surf = B.slab_rs_max_surf;
        st.max_int = B.slab_rs_max_int;
        launch_restrict_slab(g->ctx->L, fr, g->md, st, coarse.ld, rf, bc);
        return;
    }
    launch_restrict(g->ctx->L, fine, coarse, g->md.ncells, rf, bc);
}

void interface_sum(hmg_grid *g, const LevelDev &lv, double *x, bool faces)
{
    launch_interface_sum(g->ctx->L, lv, g->md, x, 0, faces);
    if (has_exchange(g)) exchange_cut(g, lv, x);
}

void scalar_sum(hmg_grid *g, int slot, int count)
{
    if (g->scalar_sum) {
        if (g->scalar_sum(g->ex_user, g->ctx->L.scal + slot, count) != 0)
            throw std::runtime_error("scalar_sum callback failed");
    }
}

namespace {

// The size of the cut as EVERY rank sees it: per kind the number of cut entities of the whole partition.  A global analysis
// knows it (Partition::nglobal); a halo-only analysis knows the entities this rank shares -- each is counted by the lowest
// rank among its sharers (the segment's first member) and the counts are summed over the ranks through the scalar_sum
// callback, once per partition analysis (first apply on the partitioned grid, and again after a domain shrink).  Collective:
// every rank reaches it at the same point of the same call sequence.
void agree_on_cut(hmg_grid *g)
{
    if (g->cut_agreed_ready) return;
    const Partition &P = *g->part;
    hmg_ctx *c = g->ctx;
    if (P.global_ids) {
        for (int k = 0; k < 3; ++k) g->cut_agreed[k] = g->cut[k].nglobal;
    } else if (!g->scalar_sum) {
        for (int k = 0; k < 3; ++k) g->cut_agreed[k] = -1;        // nothing to agree with: the plain form on every rank
    } else {
        double lead[3] = {0.0, 0.0, 0.0};
        for (const Partition::Segment &S : P.segs)
            if (!S.members.empty() && S.members.front() == P.rank)
                for (int k = 0; k < 3; ++k) lead[k] += (double)S.count[k];
        double *d = c->L.scal + S_HOST;           // (the last slots of the scalar bank are not used by the kernels)
        HIPCHK(hipMemcpyAsync(d, lead, sizeof(lead), hipMemcpyHostToDevice, c->stream));
        scalar_sum(g, S_HOST, 3);
        HIPCHK(hipMemcpyAsync(lead, d, sizeof(lead), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int k = 0; k < 3; ++k) g->cut_agreed[k] = (int64_t)std::llround(lead[k]);
    }
    g->cut_agreed_ready = true;
}

}  // namespace

// out = (src ? src : 0) + alpha*A*xin with the Dirichlet constraint, followed by the interface sum of
// `out` (local + across ranks).  fused: the CG extras of k_apply<.., FUSED> (xin = x + beta*x2 written to
// xout, scal[slot_pap] = sum mult*xin*out, scal[slot_rr] = sum xin*xin), summed over ranks.
// On a partitioned grid the cells that own a copy of a cut entity go first; their cut DOFs are packed and
// the sum over ranks is started, then the remaining cells and interface entities are processed while it
// is in flight.
void apply_then_sum(hmg_grid *g, const LevelDev &lv, ApplyArgs a, bool fused, int slot_pap, int slot_rr, bool sum_out, bool faces)
{
    hmg_ctx *c = g->ctx;
    const Launch &L = c->L;
    set_slab(g, lv);
    ensure_weight_cache(g);
    // algorithmic HBM streams of this launch: x in, out, + src, + x2 (p_old), + xout (p), + xacc (x read and write)
    // (flags bit 7: x is a zero that is not read)
    const double streams = ((a.flags & 128) ? 0.0 : 1.0) + (a.out ? 1.0 : 0.0) + (a.src ? 1.0 : 0.0) + (a.x2 ? 1.0 : 0.0) + (a.xout ? 1.0 : 0.0) +
                           (a.xacc ? 2.0 : 0.0) + (a.x3 ? 1.0 : 0.0) + (a.x4 ? 1.0 : 0.0) + (a.xcoarse ? (double)lv.nf_coarse / (double)lv.nf : 0.0) +
                           (a.rcoarse ? (double)lv.nf_coarse / (double)lv.nf : 0.0) + (a.xc_p ? 2.0 * (double)lv.nf_coarse / (double)lv.nf : 0.0);
    TimedRegion tr(g, lv, 8.0 * (double)lv.nf * (double)g->md.ncells * streams);
    // (overlapping costs launches -- the apply in two parts, the interface sums in two parts: worth it where the exchange
    //  moves real data; on the small levels, launch-bound as they are, it only adds to the chain.  Rehearsal on one rank,
    //  profiles/r03_partitioned_overhead.txt: every level overlapped +3.6 ms per V-cycle, none +0.0.)
    // The decision must be the SAME ON EVERY RANK: the overlapped form issues the exchange before the scalar sums, the plain
    // form after them, and calls on one communicator have to come in one order everywhere.  So it looks at the global size of
    // the cut on this level (identical on all ranks), never at what this rank happens to own; a rank without cut cells walks
    // the overlapped form with empty lists.
    // (round 3 read CutKind::nglobal here, which counts only the cut entities THIS rank has a copy of once the partition is
    //  analysed on the rank's halo: ranks on either side of the threshold chose different forms -- ADVICE r3.  The counts are
    //  now summed over the ranks once per partition analysis, every entity counted by the lowest rank that shares it.)
    if (has_exchange(g) && g->part) agree_on_cut(g);
    const bool has_cut = has_exchange(g) && g->part && g->cut_agreed[0] >= 0 &&
                         g->cut_agreed[0] + g->cut_agreed[1] + g->cut_agreed[2] > 0;
    const int64_t global_cut = has_cut ? g->cut_agreed[0] * lv.nfi + g->cut_agreed[1] * lv.nei + g->cut_agreed[2] : 0;
    const bool overlap = has_cut && (g->sharers ? g->p2p_begin != nullptr : g->ex_begin != nullptr) && g->ex_end && g->overlap &&
                         global_cut >= std::max<int64_t>(1, c->overlap_min_doubles);
    auto launch = [&](const int32_t *list, int64_t n) {
        ApplyArgs b = a;
        b.cell_list = list;
        b.ncell_list = n;
        if (fused)
            launch_apply_fused_kernel(L, lv, g->md, b);
        else
            launch_apply_args(L, lv, g->md, b);
    };
    auto sums = [&]() {
        if (!fused || slot_pap < 0) return;
        launch_apply_fused_reduce(L, g->md, slot_pap, slot_rr);
        // (r.r and p.Ap of CG step 0 sit in neighbouring slots of the scalar bank: one sum over ranks for both)
        if (slot_rr >= 0 && (slot_rr == slot_pap + 1 || slot_rr + 1 == slot_pap))
            scalar_sum(g, std::min(slot_rr, slot_pap), 2);
        else {
            if (slot_rr >= 0) scalar_sum(g, slot_rr, 1);
            scalar_sum(g, slot_pap, 1);
        }
    };
    if (!a.out && a.rcoarse) {       // local residual restricted in the kernel's epilogue: nothing is stored, summed or reduced
        need(fused && !sum_out, "epilogue restriction belongs to the cell-local residual");
        launch(nullptr, 0);
        tr.stop();
        return;
    }
    if (!a.out) {                    // reductions only (dead-tail step of a pre-smoother): nothing to sum or exchange
        need(fused, "apply without an output vector");
        launch(nullptr, 0);
        tr.stop();
        sums();
        return;
    }
    if (!sum_out) {                  // cell-local result wanted (local residual before the restriction): no reductions
        launch(nullptr, 0);
        tr.stop();
        return;
    }
    if (!overlap) {
        launch(nullptr, 0);
        tr.stop();
        sums();
        interface_sum(g, lv, a.out, faces);
        return;
    }
    if (g->md.ncells_cut > 0) launch(g->md.cells_cut, g->md.ncells_cut);
    launch_interface_sum(L, lv, g->md, a.out, 1);        // local copies of the cut entities
    exchange_prepare(g, lv);
    cut_pack(g, lv, a.out, 0);
    exchange_run(g, lv, true);
    if (g->md.ncells_inner > 0)                           // (an empty list must not read as "all cells")
        launch(g->md.cells_inner, g->md.ncells_inner);    // overlaps the sum over ranks
    tr.stop();
    launch_interface_sum(L, lv, g->md, a.out, 2, faces);
    sums();
    exchange_finish(g, lv, true);
    cut_pack(g, lv, a.out, 1);
}

namespace {

// Who runs a smoother, and so what of its state is read afterwards: inside a V-cycle the reference overwrites part of it
// unread (src/multigrid.jl:46-50,100-115).  With option lean_post = 0 the post-smoothers leave what Plain leaves.
enum class Role {
    Plain,       // hmg_smooth: x, r, p and Ap as the reference leaves them
    Pre,         // vcycle_down: x only, and its last x-update(s) may be handed back (XUpdates)
    PostTop,     // vcycle_up on the finest level: x and r; p and Ap are scratch
    PostBelow,   // vcycle_up below the finest level: x only
};

// The form of the last CG step.  A dead step keeps only alpha = rs / p.Ap and x += alpha p: the interface sum of Ap,
// r -= alpha Ap, r.r and the last p-update (src/multigrid.jl:60-68) go, and the fused kernel does not store Ap.
enum class Tail {
    Full,        // regular step, then x += alpha p and the reference's last p-update
    ScratchP,    // ... without that p-update; Ap stays unsummed on the faces (option lean_post)
    Top2,        // p formed in LDS only, Ap written alone, both pending x-updates ride in the r-update (lazy_top = 1)
    Top3,        // ... and step steps - 2 writes its direction into the spare vector and leaves its x-update too (lazy_top = 2)
    DeadXp,      // dead step, then x += alpha p
    DeadDefer,   // dead step, x += alpha p left to the caller's local residual (fold_x)
    DeadDefer2,  // dead step that writes nothing (p formed in LDS only), both pending x-updates left to the caller (lazy_dead)
    DeadDefer3,  // ... and step steps - 2 writes its direction into the spare vector and leaves its x-update too: three pending (lazy_pre)
    DeadX2,      // dead step that writes nothing, then one pass does both x-updates (lazy_post)
};

struct SmoothForm {
    bool swap_rp = false;   // step 0 takes r_0 itself as p_0 by exchanging the handles' device pointers (an even number of
                            // times per V-cycle: wrapped buffers end up holding what their names say)
    bool ride = false;      // the face part of Ap's interface sum rides in the r-update (every step but a live last one)
    Tail tail = Tail::Full;
    bool hand_up = false;   // (set by the caller, tail DeadX2) both x-updates are left to the finer level's first residual (coarse_x_folds())
    bool x_zero = false;    // (set by the caller) x is a coarse level's zero initial guess that is not in memory
                            // (zero_entry_ok): the first residual is the constrained copy of b, b - A 0 to the last bit
    bool lazy_r = false;    // (set by the caller, tails Top2 / Top3) the last launch finishes x only and leaves the r-update
                            // pending on the grid (lazy_r_ok())
    bool lazy_x = false;    // (set by the caller, with lazy_r) ... and may leave x's updates pending as well (lazy_x_ok())
    XUpdates carry_x;       // (set by the caller, Role::Pre on the top level of hmg_vcycle) x lacks the last two / three updates of
                            // the V-cycle before, which ride in the first residual (PendingX, taken out of the grid by enter_top())
};

// What smooth() returns: the x-updates a pre-smoother leaves to its caller (tails DeadDefer, DeadDefer2 and DeadDefer3: one, two, three),
// or a post-smoother below the finest level to the level above (tail DeadX2 with hand_up: two).  Two host functions, and nothing else,
// turn an XUpdates into the arguments of an apply:

// ... of a load phase that finishes this level's x on the way (written back): x2 / x3 / x4 are p1 / r2 / p0
void finish_x_in_load(ApplyArgs &a, const XUpdates &u, double *x)
{
    a.xout = x;
    a.scal = u.scal;
    a.x2 = u.p1;
    if (u.count == 1) {
        a.s = u.last;
        return;
    }
    a.x3 = u.r2;
    a.a = u.prev;
    a.s = u.beta;
    a.c = u.last;
    if (u.count == 3) {
        a.x4 = u.p0;
        a.d = u.first;
    }
}

// ... of a first residual that finishes the coarser level's x where its column is staged (two updates)
void finish_coarse_x_staged(ApplyArgs &a, const XUpdates &u)
{
    a.xc_p = u.p1;
    a.xc_r = u.r2;
    a.a = u.prev;
    a.s = u.beta;
    a.c = u.last;
}

// Every context option that shapes the smoother is read here, before the first launch.
SmoothForm smooth_form(const hmg_grid *g, int level, int steps, Role role)
{
    const LevelDev &lv = lev(g, level);
    const hmg_ctx *c = g->ctx;
    const bool lean = c->lean_post && (role == Role::PostTop || role == Role::PostBelow);
    const bool dead = role == Role::Pre || (lean && role == Role::PostBelow);
    SmoothForm f;
    // (the Jacobi-preconditioned and the Chebyshev smoother have the tails of the unfused path and nothing else: no pointer
    //  exchange, no riding face sums, no deferred x-updates)
    if (!g->fuse_cg || g->smoother != 0) {
        f.tail = dead ? Tail::DeadXp : lean ? Tail::ScratchP : Tail::Full;
        return f;
    }
    const bool faces = c->fold_faces && lv.dim == 3 && lv.nfi > 0;
    f.swap_rp = role != Role::Plain && c->swap_rp && steps > 0;
    f.ride = faces;
    if (role == Role::Pre && c->fold_x) {
        f.tail = steps >= 2 && c->lazy_dead ? Tail::DeadDefer2 : Tail::DeadDefer;
        // (the local residual must be the launch that has the fourth stream: vcycle_down takes it under the same conditions)
        if (f.tail == Tail::DeadDefer2 && steps >= 3 && c->lazy_pre && faces && c->fold_restrict && apply_defers3(c->L, lv) &&
            g->top_spare.n >= (size_t)lv.ld * (size_t)g->md.ncells)
            f.tail = Tail::DeadDefer3;
    }
    else if (dead)
        f.tail = steps >= 2 && c->lazy_post ? Tail::DeadX2 : Tail::DeadXp;
    else if (lean && steps >= 2 && c->lazy_top > 0 && faces)
        f.tail = steps >= 3 && c->lazy_top > 1 && g->top_spare.n >= (size_t)lv.ld * (size_t)g->md.ncells ? Tail::Top3 : Tail::Top2;
    else if (lean)
        f.tail = Tail::ScratchP;
    return f;
}

}  // namespace

// The spare direction vector of the Top3 form is SETUP: reserved when the first vector of the finest level is created or
// wrapped (or by hmg_grid_reserve_spare), never inside a smoother.  Without it (reservation refused for lack of memory,
// option lazy_top < 2 at that time, hmg_grid_reserve_spare(grid, 0)) smooth_form() picks Top2 -- which form the last
// finest-level post-smoother took is reported by hmg_ctx_counter "lazy_top_form", the bytes held by "spare_bytes".
bool reserve_top_spare(hmg_grid *g, bool must)
{
    hmg_ctx *c = g->ctx;
    const LevelDev &lv = g->ld[(size_t)g->nlevels - 1];
    const size_t n = (size_t)lv.ld * (size_t)g->mesh_full.ncells;
    if (g->top_spare.n >= n && n > 0) return true;
    if (g->top_spare_refused && !must) return false;
    HIPCHK(hipSetDevice(c->device));
    void *q = nullptr;
    if (device_malloc(&q, n * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        g->top_spare_refused = true;
        if (must)
            throw std::runtime_error("the spare direction vector of the finest level (" + std::to_string((n * sizeof(double)) >> 20) +
                                     " MiB, option lazy_top = 2) does not fit the device memory; V-cycles take the two-update form");
        return false;
    }
    c->spare_bytes -= (int64_t)(g->top_spare.n * sizeof(double));
    g->top_spare.release();
    g->top_spare.p = (double *)q;
    g->top_spare.n = n;
    g->top_spare_refused = false;
    c->spare_bytes += (int64_t)(n * sizeof(double));
    return true;
}

void release_top_spare(hmg_grid *g)
{
    if (g->ctx) {
        if (g->top_spare.p) (void)hipStreamSynchronize(g->ctx->stream);
        g->ctx->spare_bytes -= (int64_t)(g->top_spare.n * sizeof(double));
    }
    g->top_spare.release();
}

// the three-update form applies to: 3D grids whose finest level has face interiors (smooth_form(): Top3)
bool wants_top_spare(const hmg_grid *g, int level)
{
    return g->ctx && g->smoother == 0 && g->ctx->lazy_top > 1 && level == g->nlevels && g->dim == 3 && g->ld[(size_t)level - 1].nfi > 0;
}

// The inverse diagonals of the Jacobi-preconditioned smoother, level by level: the cell-local diagonal, its interface sum (on a
// partitioned grid with the cut exchange -- every rank gets here in the same call), then the inversion off the constrained nodes.
// A grid with an interface exchange or a partition: the maximum over the grid would need a maximum over the ranks, and the exchange
// hooks only sum.
static bool cheb_needs_given(const hmg_grid *g) { return g->part || has_exchange(g) || g->scalar_sum; }

static bool cheb_all_given(const hmg_grid *g, const std::vector<double> &given)
{
    if (given.size() != (size_t)g->nlevels) return false;
    for (int level = 2; level <= g->nlevels; ++level)
        if (!(given[(size_t)level - 1] > 0.0)) return false;
    return true;
}

static const char *const CHEB_PARTITIONED =
    "Chebyshev smoother: on a partitioned grid (or one with an interface exchange) the bound of every level >= 2 must be given "
    "(hmg_grid_set_smoother_chebyshev, lambda_hi): forming it needs a maximum over the ranks, which the exchange hooks do not have";

// For kind 2 the level's bound lambda_hi is formed right behind its inverse diagonal, in the same scratch vector: the cell-local
// absolute row sums, their interface sum, the maximum of dinv o s (one host read per level and generation), times CHEB_SAFETY.
void ensure_smoother_diag(hmg_grid *g, int level, double *scratch)
{
    if (g->smoother == 0 || level < 2) return;
    need(g->has_op, "operator not set");
    need(g->dinv.size() == (size_t)g->nlevels && level <= g->nlevels, "Jacobi-preconditioned smoother: the inverse diagonals were not reserved");
    if (g->smoother == 2 && cheb_needs_given(g) && !cheb_all_given(g, g->cheb_given)) throw std::runtime_error(CHEB_PARTITIONED);
    if (!g->dinv_ready) {                        // a new generation: nothing formed, nothing counted
        g->dinv_level_ready.assign((size_t)g->nlevels, 0);
        g->dinv_build_counted = false;
        g->dinv_ready = true;
    }
    if (g->dinv_level_ready[(size_t)level - 1]) return;
    const LevelDev &lv = lev(g, level);
    double *d = g->dinv[(size_t)level - 1]->p;
    need(scratch != nullptr && scratch != d, "Jacobi-preconditioned smoother: no scratch vector to form the diagonal with");
    // (a rank without cells launches nothing and still takes part in the exchanges)
    for (int limb = diag_limbs() - 1; limb >= 0; --limb) {
        launch_operator_diag(g->ctx->L, lv, g->md, g->lambda, limb, scratch);
        interface_sum(g, lv, scratch);
        launch_diag_accum(g->ctx->L, lv, g->md, scratch, d, limb);
    }
    launch_dinv_finish(g->ctx->L, lv, g->md, d);
    if (g->smoother == 2) {
        g->cheb_hi.resize((size_t)g->nlevels, 0.0);
        const double given = g->cheb_given.size() == (size_t)g->nlevels ? g->cheb_given[(size_t)level - 1] : 0.0;
        double hi = given;
        if (!(given > 0.0)) {
            launch_operator_rowabs(g->ctx->L, lv, g->md, g->lambda, scratch);
            interface_sum(g, lv, scratch);
            launch_cheb_max(g->ctx->L, d, scratch, (int64_t)lv.ld * g->md.ncells, S_HOST);
            hi = CHEB_SAFETY * read_scalar(g->ctx, S_HOST);
            g->ctx->smoother_bound_builds += 1;
            need(g->md.ncells == 0 || (std::isfinite(hi) && hi > 0.0), "Chebyshev smoother: the bound of this level is not a positive number");
        }
        g->cheb_hi[(size_t)level - 1] = hi;
    }
    g->dinv_level_ready[(size_t)level - 1] = 1;
    if (!g->dinv_build_counted) {
        g->ctx->smoother_diag_builds += 1;
        g->dinv_build_counted = true;
    }
}

void ensure_smoother_diag(hmg_grid *g, int top, hmg_vec **states)
{
    if (g->smoother == 0) return;
    for (int level = 2; level <= top; ++level) ensure_smoother_diag(g, level, states[5 * (level - 1) + 4]->d);
}

void release_smoother_diag(hmg_grid *g)
{
    int64_t bytes = 0;
    for (const auto &d : g->dinv)
        if (d) bytes += (int64_t)(d->n * sizeof(double));
    if (g->ctx) {
        if (bytes > 0) (void)hipStreamSynchronize(g->ctx->stream);
        g->ctx->smoother_diag_bytes -= bytes;
    }
    g->dinv.clear();
    g->dinv_level_ready.clear();
    g->dinv_ready = false;
}

namespace {

// r = b - A x, constraint, interface sum (src/multigrid.jl:50): the first residual of both smoothers, with the forms its caller
// may ask for -- x a zero that is not in memory (f.x_zero), the coarse-grid correction riding in the load phase (xcoarse, cx)
void first_residual(hmg_grid *g, int level, hmg_vec *x, hmg_vec *b, hmg_vec *r, const SmoothForm &f, const hmg_vec *xcoarse,
                    const XUpdates *cx)
{
    const LevelDev &lv = lev(g, level);
    const Launch &L = g->ctx->L;
    const int64_t n = vec_len(x);
    {
        ApplyArgs a{};
        a.alpha = -1.0;
        a.lambda = g->lambda;
        a.x = x->d;
        a.src = b->d;
        a.out = r->d;
        a.flags = 1;
        if (f.x_zero) {
            need(!xcoarse, "zero initial guess with a coarse-grid correction");
            launch_copy(L, r->d, b->d, n);
            launch_mask(L, lv, g->md, r->d, 0);
            interface_sum(g, lv, r->d);
        } else if (xcoarse) {
            // (xcoarse: x += P xcoarse, the coarse-grid correction of src/multigrid.jl:113, rides in the load phase)
            a.xcoarse = xcoarse->d;
            a.ldc = lev(g, level - 1).ld;
            a.xout = x->d;
            // (cells that fill a third of the LDS: no room for the coarse column next to three resident images)
            if (g->ctx->prolong_in_image && apply_lds_bytes(lv) > 48 * 1024) a.flags |= 64;
            if (cx && cx->count) {
                // the coarse x still lacks its last two CG updates: done per coarse entry where the column is staged (24 instead of
                // 32 + 8 B per coarse DOF, one launch fewer)
                need(cx->count == 2 && cx->p1 && cx->r2 && (a.flags & 64), "pending coarse x-updates where the residual cannot carry them");
                finish_coarse_x_staged(a, *cx);
                g->ctx->coarse_x_folds += 1;
            }
            apply_then_sum(g, lv, a, true, -1, -1);
        } else if (f.carry_x.count) {
            // x still lacks the last CG updates of the V-cycle before this one (option lazy_x): formed in the load phase as the down
            // leg's local residual forms them, from p0 (three updates: the p handle), p1 (the spare vector / the p handle) and r2 (still
            // in r) with the ratios k_cg_x_save put aside (saved_updates()), and written back -- 56 B/DOF instead of 40 + 24.  r goes over
            // r2 in place: a workgroup reads its own cell's column of it alone, in the load phase, and stores behind the barrier after it.
            need(f.carry_x.count == 2 || g->top_spare.p != nullptr, "pending x-updates have lost the spare vector they rest on");
            finish_x_in_load(a, f.carry_x, x->d);
            apply_then_sum(g, lv, a, true, -1, -1);
        } else {
            apply_then_sum(g, lv, a, false, -1, -1);
        }
    }
}

// CG preconditioned by the inverse diagonal of the assembled operator (hmg_grid_set_smoother(grid, 1)), after first_residual():
//   z = dinv o r;  p = z;  rz = r.z
//   steps x { Ap = A p, constraint, interface sum;  alpha = rz / p.Ap;  x += alpha p;  r -= alpha Ap;
//             rz' = r.(dinv o r);  p = dinv o r + (rz'/rz) p;  rz = rz' }
// z is never stored; rz / rz' alternate between S_RS and S_RS2 as r.r does in smooth(), p.Ap is in S_PAP.  With fuse_cg the apply is
// the fused step-0 launch (no x2, no xout: 16 B/DOF, p.Ap formed in its epilogue), else the plain apply and a dot product.  Tails:
// those of the unfused path of smooth() (smooth_form()).
void smooth_pcg(hmg_grid *g, int level, int steps, hmg_vec *x, hmg_vec *r, hmg_vec *p, hmg_vec *Ap, const SmoothForm &f)
{
    const LevelDev &lv = lev(g, level);
    const Launch &L = g->ctx->L;
    const int64_t n = vec_len(x);
    need(g->dinv_ready && g->dinv.size() == (size_t)g->nlevels && g->dinv_level_ready[(size_t)level - 1] && g->dinv[(size_t)level - 1] &&
             (g->dinv[(size_t)level - 1]->p || n == 0),
         "Jacobi-preconditioned smoother: no inverse diagonal for this level");
    need(f.tail == Tail::Full || f.tail == Tail::ScratchP || f.tail == Tail::DeadXp, "Jacobi-preconditioned smoother: unknown tail");
    const double *dinv = g->dinv[(size_t)level - 1]->p;
    int cur = S_RS, other = S_RS2;
    launch_pcg_start(L, p->d, r->d, dinv, n, cur);                          // p = dinv o r; rz = r.p
    scalar_sum(g, cur, 1);
    for (int i = 0; i < steps; ++i) {
        if (g->fuse_cg) {
            ApplyArgs a{};                                                    // Ap = A p, constraint, interface sum; p.Ap
            a.alpha = 1.0;
            a.lambda = g->lambda;
            a.x = p->d;
            a.out = Ap->d;
            a.flags = 1;
            apply_then_sum(g, lv, a, true, S_PAP, -1);
        } else {
            apply(g, lv, 1.0, p->d, nullptr, Ap->d, 1);
            interface_sum(g, lv, Ap->d);
            launch_dot(L, p->d, Ap->d, n, S_PAP);
            scalar_sum(g, S_PAP, 1);
        }
        const bool last = i == steps - 1;
        if (last && f.tail != Tail::Full) {
            if (f.tail == Tail::ScratchP) {
                launch_pcg_rupdate(L, r->d, Ap->d, dinv, n, {cur, S_PAP}, other);   // alpha = rz / p.Ap
                scalar_sum(g, other, 1);
            }
            launch_cg_xp_update(L, x->d, p->d, r->d, n, {cur, S_PAP}, {cur, other}, 0);   // x += (rz / p.Ap) p
            return;
        }
        launch_pcg_rupdate(L, r->d, Ap->d, dinv, n, {cur, S_PAP}, other);     // alpha = rz / p.Ap; rz'
        scalar_sum(g, other, 1);
        launch_pcg_xp(L, x->d, p->d, r->d, dinv, n, {cur, S_PAP}, {other, cur});  // beta = rz' / rz
        std::swap(cur, other);
    }
}

// The Chebyshev polynomial in dinv o A on [hi / ratio, hi] (hmg_grid_set_smoother_chebyshev), after first_residual():
//   d = c0 dinv o r
//   steps x { x += d;  Ad = A d, constraint, interface sum;  r -= Ad;  d = c1[k] d + c2[k] dinv o r }
// The coefficients (ChebCoef, hmg_cheb.hpp) are host numbers formed here from the level's bound: no reduction, no sum over ranks, no
// host round trip.  p holds d, Ap holds Ad; the apply is the plain one with the constraint.  Tails (smooth_form()): Full as above;
// ScratchP ends with x += d, r -= Ad; DeadXp ends with x += d and launches no apply for its last step.
void smooth_cheb(hmg_grid *g, int level, int steps, hmg_vec *x, hmg_vec *r, hmg_vec *p, hmg_vec *Ap, const SmoothForm &f)
{
    const LevelDev &lv = lev(g, level);
    const Launch &L = g->ctx->L;
    const int64_t n = vec_len(x);
    need(g->dinv_ready && g->dinv.size() == (size_t)g->nlevels && g->dinv_level_ready[(size_t)level - 1] && g->dinv[(size_t)level - 1] &&
             (g->dinv[(size_t)level - 1]->p || n == 0) && g->cheb_hi.size() == (size_t)g->nlevels,
         "Chebyshev smoother: no inverse diagonal or no bound for this level");
    need(f.tail == Tail::Full || f.tail == Tail::ScratchP || f.tail == Tail::DeadXp, "Chebyshev smoother: unknown tail");
    const double *dinv = g->dinv[(size_t)level - 1]->p;
    const double hi = g->cheb_hi[(size_t)level - 1];
    ChebCoef c(hi / g->cheb_ratio, hi);
    launch_cheb_start(L, p->d, r->d, dinv, n, c.c0);
    if (steps > 0) g->ctx->cheb_smoothings += 1;
    for (int i = 0; i < steps; ++i) {
        const bool last = i == steps - 1;
        if (last && f.tail == Tail::DeadXp) {
            launch_cheb_tail(L, x->d, p->d, nullptr, nullptr, n);         // x += d: nothing else of this step is read
            return;
        }
        apply(g, lv, 1.0, p->d, nullptr, Ap->d, 1);                       // Ad = A d, constraint
        interface_sum(g, lv, Ap->d);
        g->ctx->cheb_applies += 1;
        if (last && f.tail == Tail::ScratchP) {
            launch_cheb_tail(L, x->d, p->d, r->d, Ap->d, n);
            return;
        }
        double c1, c2;
        c.next(c1, c2);
        launch_cheb_step(L, x->d, p->d, r->d, Ap->d, dinv, n, c1, c2);
    }
}

XUpdates smooth(hmg_grid *g, int level, int steps, hmg_vec *x, hmg_vec *b, hmg_vec *r, hmg_vec *p, hmg_vec *Ap, const SmoothForm &f,
                const hmg_vec *xcoarse = nullptr, const XUpdates *cx = nullptr)
{
    // ref: src/multigrid.jl:46-71
    const LevelDev &lv = lev(g, level);
    const Launch &L = g->ctx->L;
    const int64_t n = vec_len(x);
    // (a record without a stored Ap rests on the spare vector, which these two tails write: on other vectors than the record's --
    //  hmg_vcycle_down / _up next to a V-cycle's states -- nothing else has settled it)
    if (f.tail == Tail::Top3 || f.tail == Tail::DeadDefer3) settle_rebuild(g);
    need(!f.carry_x.count || (!f.x_zero && !xcoarse), "pending x-updates where the first residual cannot carry them");
    first_residual(g, level, x, b, r, f, xcoarse, cx);
    if (g->smoother == 1) {
        smooth_pcg(g, level, steps, x, r, p, Ap, f);
        return {};
    }
    if (g->smoother == 2) {
        smooth_cheb(g, level, steps, x, r, p, Ap, f);
        return {};
    }
    int cur = S_RS, other = S_RS2;
    if (!g->fuse_cg || steps <= 0) {
        launch_copy_dot(L, p->d, r->d, n, cur);                          // p = r; rs = r.r
        scalar_sum(g, cur, 1);
        for (int i = 0; i < steps; ++i) {
            apply(g, lv, 1.0, p->d, nullptr, Ap->d, 1);                        // Ap = A p, constraint
            interface_sum(g, lv, Ap->d);
            launch_dot(L, p->d, Ap->d, n, S_PAP);
            scalar_sum(g, S_PAP, 1);
            const bool last = i == steps - 1;
            if (last && f.tail == Tail::DeadXp) {
                launch_cg_xp_update(L, x->d, p->d, r->d, n, {cur, S_PAP}, {cur, other}, 0);   // x += (rs / p.Ap) p
                return {};
            }
            launch_cg_update(L, x->d, r->d, p->d, Ap->d, n, {cur, S_PAP}, other);   // alpha = rs/pAp
            scalar_sum(g, other, 1);
            if (last && f.tail == Tail::ScratchP) return {};
            launch_cg_pupdate(L, p->d, r->d, n, {other, cur});                 // beta = rs'/rs
            std::swap(cur, other);
        }
        return {};
    }
    // Fused path: the p-update and both reductions ride along with the operator apply (see k_apply<.., FUSED>).
    // Per step:  fused apply  [x += alpha_prev p_old;  p = r + beta p_old;  Ap = A p;  p.Ap (, r.r)]
    //            interface sum of Ap
    //            r -= alpha Ap;  r.r'
    // The x-update of step i rides with the fused apply of step i+1 (which reads p anyway); the tail decides the last one.
    // (The kernels read the previous p.Ap from S_PAP; the reduction that overwrites it is enqueued behind them.)
    auto args = [&](int i) {
        ApplyArgs a{};
        a.alpha = 1.0;
        a.lambda = g->lambda;
        a.x = r->d;
        a.x2 = i == 0 ? nullptr : p->d;                                   // p = r  /  p = r + beta p, beta = rs'/rs
        a.xout = i == 0 && f.swap_rp ? nullptr : p->d;                   // (swap_rp: r_0 itself becomes p_0)
        a.xacc = i == 0 ? nullptr : x->d;                                 // x += alpha_{i-1} p_{i-1}
        a.a = {other, S_PAP};                                             // rs_{i-1} (after the swap below) / p_{i-1}.Ap_{i-1}: still the old value here
        a.out = Ap->d;
        a.s = {cur, other};
        a.flags = 1;
        return a;
    };
    auto exchange_rp = [&]() {                                            // p now names r_0, r the spare buffer
        std::swap(r->d, p->d);
        std::swap(r->own, p->own);
        std::swap(r->alloc_cells, p->alloc_cells);
        std::swap(r->bytes, p->bytes);
    };
    auto step = [&](int i, bool ride) {
        apply_then_sum(g, lv, args(i), true, S_PAP, i == 0 ? cur : -1, true, !ride);
        const double *r_in = r->d;
        if (i == 0 && f.swap_rp) {
            exchange_rp();
            r_in = p->d;
        }
        if (ride)
            launch_cg_rupdate_faces(L, lv, g->md, r_in, r->d, Ap->d, n, {cur, S_PAP}, other);
        else
            launch_cg_rupdate(L, r_in, r->d, Ap->d, n, {cur, S_PAP}, other);   // alpha = rs / p.Ap
        scalar_sum(g, other, 1);
        std::swap(cur, other);
    };
    const int last = steps - 1;
    for (int i = 0; i < last; ++i) {
        if ((f.tail == Tail::Top3 || f.tail == Tail::DeadDefer3) && i == last - 1) {
            // slots: rs_{i-1} in `other`, p.Ap_{i-1} in S_PAP (both kept for the deferred x-update), rs_i in `cur`;
            // this step's p.Ap goes to S_PAP2 and its r.r to S_RS3
            ApplyArgs a = args(i);
            a.xout = g->top_spare.p;
            a.xacc = nullptr;
            apply_then_sum(g, lv, a, true, S_PAP2, -1, true, false);
            launch_cg_rupdate_faces(L, lv, g->md, r->d, r->d, Ap->d, n, {cur, S_PAP2}, S_RS3);
            scalar_sum(g, S_RS3, 1);
            continue;
        }
        step(i, f.ride);
    }
    if (f.tail == Tail::Top2 || f.tail == Tail::Top3) g->ctx->last_top_form = f.tail == Tail::Top3 ? 2 : 1;
    // The x-updates a tail leaves undone, as the scalar bank and the vectors stand behind its last apply.  One or two: rs_{i-1} in `other`,
    // rs_i in `cur`, p.Ap_{i-1} in S_PAP, p.Ap_i in S_PAP2 (two; S_PAP with one), p_{i-1} in p.  Three: rs_{i-2} in `other`, rs_{i-1} in
    // `cur`, rs_i in S_RS3, p.Ap_{i-2} in S_PAP, p.Ap_{i-1} in S_PAP2, p.Ap_i in S_PAP3, p_{i-2} in p, p_{i-1} in the spare vector.
    auto pending = [&](int count) {
        XUpdates u;
        u.count = count;
        u.r2 = r->d;
        u.p1 = count == 3 ? g->top_spare.p : p->d;
        if (count == 1) u.last = {cur, S_PAP};
        if (count == 2) {
            u.prev = {other, S_PAP};       // alpha_{i-1}
            u.beta = {cur, other};         // beta_i
            u.last = {cur, S_PAP2};        // alpha_i
        }
        if (count == 3) {
            u.p0 = p->d;
            u.first = {other, S_PAP};      // alpha_{i-2}
            u.prev = {cur, S_PAP2};
            u.beta = {S_RS3, cur};
            u.last = {S_RS3, S_PAP3};
        }
        return u;
    };
    // The end of the finest level's tails Top2 / Top3, behind the last apply: the updates u of x and the r-update, in one launch, or x
    // alone and the r-update left pending (lazy_r), or the ratios of u put aside and both left pending (lazy_x)
    auto top_tail = [&](const XUpdates &u, bool ap_stored) {
        if (f.lazy_r && !g->r_reader) {
            if (f.lazy_x && !g->x_reader)
                launch_cg_x_save(L, u, g->pend_alpha());
            else
                launch_cg_x_tail(L, x->d, n, u, g->pend_alpha());
            open_pending(g, level, r, Ap, other, false, ap_stored);
            if (f.lazy_x) open_pending_x(g, level, x, p, r, g->x_reader ? 0 : u.count);
            return;
        }
        launch_cg_rupdate_faces_x(L, lv, g->md, r->d, Ap->d, n, other, x->d, u);
        scalar_sum(g, other, 1);
        if (f.lazy_r) open_pending(g, level, r, Ap, other, true);
    };
    ApplyArgs a = args(last);
    switch (f.tail) {
    case Tail::Full:
    case Tail::ScratchP:
        step(last, f.ride && f.tail == Tail::ScratchP);
        // x += alpha_last p (alpha_last = rs_{s-1} / p.Ap: `other` holds rs_{s-1} after the swap) and, Full only, the
        // reference's last p-update p = r + (rs_s / rs_{s-1}) p
        launch_cg_xp_update(L, x->d, p->d, r->d, n, {other, S_PAP}, {cur, other}, f.tail == Tail::Full ? 1 : 0);
        return {};
    case Tail::DeadXp:
    case Tail::DeadDefer:
        a.out = nullptr;
        apply_then_sum(g, lv, a, true, S_PAP, last == 0 ? cur : -1, true, true);
        if (last == 0 && f.swap_rp) exchange_rp();
        if (f.tail == Tail::DeadDefer) return pending(1);
        launch_cg_xp_update(L, x->d, p->d, r->d, n, {cur, S_PAP}, {cur, other}, 0);   // x += (rs / p.Ap) p
        return {};
    case Tail::DeadDefer2:
    case Tail::DeadX2: {
        // p_i is formed in LDS only, for the apply and the p.Ap reduction: neither p nor x nor Ap is written.  p.Ap of this
        // step goes to its own slot: S_PAP still holds the previous step's, which the first of the two x-updates needs.
        a.out = a.xout = a.xacc = nullptr;
        apply_then_sum(g, lv, a, true, S_PAP2, -1);
        const XUpdates u = pending(2);
        if (f.tail == Tail::DeadX2 && !f.hand_up) {
            launch_cg_x2_update(L, x->d, n, u);
            return {};
        }
        return u;                          // to the local residual (DeadDefer2) or the level above (hand_up)
    }
    case Tail::DeadDefer3: {
        // the dead step after a step that wrote its direction into the spare vector: reads r and the spare, writes nothing;
        // x += alpha_{i-2} p_{i-2}, x += alpha_{i-1} p_{i-1} and x += alpha_i (r_i + beta_i p_{i-1}) are the caller's
        const XUpdates u = pending(3);
        a.x2 = u.p1;
        a.out = a.xout = a.xacc = nullptr;
        a.s = u.beta;
        apply_then_sum(g, lv, a, true, S_PAP3, -1);
        return u;
    }
    case Tail::Top2:
        // (p.Ap of this step to its own slot: S_PAP keeps the previous step's for the first of the two x-updates)
        a.xout = a.xacc = nullptr;
        apply_then_sum(g, lv, a, true, S_PAP2, -1, true, false);
        top_tail(pending(2), true);
        return {};
    case Tail::Top3: {
        const XUpdates u = pending(3);
        a.x2 = u.p1;
        a.xout = a.xacc = nullptr;
        a.s = u.beta;
        // A p_2 has one reader, the r-update: where that stays pending the step delivers p_2.Ap_2 alone -- the pre-smoother's dead launch
        // (16 instead of 24 B/DOF, no interface sum) -- and the record forms Ap again if somebody reads r (materialize_r())
        const bool ap_stored = !(f.lazy_r && lazy_ap_ok(g));
        if (!ap_stored) a.out = nullptr;
        apply_then_sum(g, lv, a, true, S_PAP3, -1, true, /*faces=*/!ap_stored);
        top_tail(u, ap_stored);
        return {};
    }
    }
    return {};
}

// Down leg of one level of the V-cycle (src/multigrid.jl:100-106): pre-smoother, local residual, restriction,
// zero initial guess on the coarser level.  Inside the library the pre-smoother's dead tail is dropped and its pending
// x-update(s) ride in the load phase of the local residual (Role::Pre); x, the local residual in r and the
// coarse right-hand side are what the reference leaves, p and Ap are scratch.
// Can level k be entered with a zero initial guess that is never written to memory?  Level 1: the scatter of the coarse
// solution overwrites every entry of x.  Levels above: with two CG steps and the tail DeadDefer2 the pre-smoother never
// touches x, and the local residual that carries both pending x-updates writes it (flags bit 7: x is not read).
bool zero_entry_ok(const hmg_grid *g, int k, int steps)
{
    if (!g->ctx->zero_entry) return false;
    if (k == 1) return true;
    if (g->smoother != 0) return false;          // (their zero guesses are written)
    if (steps != 2 || smooth_form(g, k, steps, Role::Pre).tail != Tail::DeadDefer2) return false;
    // (register-blocked levels take that residual through the instantiation that also restricts in its epilogue -- the only one
    //  of theirs the zero-input form is compiled into)
    const LevelDev &lv = g->ld[k - 1];
    if (lv.blk_R > 0) return g->ctx->fold_restrict && apply_restricts(g->ctx->L, lv);
    return true;
}

// Returns the number of x-updates the pre-smoother left to the local residual (hmg_ctx_counter "lazy_pre_form").
int vcycle_down(hmg_grid *g, int k, int steps, hmg_vec **st, bool inside = false, bool x_zero = false, int steps_next = -1,
                const XUpdates &carry_x = {})
{
    // carry_x: this level's x lacks the last x-updates of the V-cycle before (enter_top()): the pre-smoother's first residual has them
    // x_zero: this level's x is a zero nobody has written (see zero_entry_ok); steps_next: the CG steps the next coarser
    // level will take (inside hmg_vcycle; decides whether ITS zero initial guess has to be written)
    // inside (hmg_vcycle): nobody can read this level's r before the post-smoother's first residual overwrites it
    // (src/multigrid.jl:104-113), so where the apply kernel can restrict in its epilogue the cell-local residual is
    // never stored -- the coarse right-hand side is the same to the last bit (option fold_restrict)
    hmg_vec **cur = st + 5 * (k - 1);
    hmg_vec **nxt = st + 5 * (k - 2);
    const Launch &L = g->ctx->L;
    SmoothForm form = smooth_form(g, k, steps, Role::Pre);
    need(!x_zero || form.tail == Tail::DeadDefer2, "zero initial guess: the pre-smoother does not defer both x-updates");
    form.x_zero = x_zero;
    form.carry_x = carry_x;
    const XUpdates dx = smooth(g, k, steps, cur[0], cur[1], cur[2], cur[3], cur[4], form);
    const int deferred = dx.count;
    const bool skip_fill = inside && steps_next >= 0 && zero_entry_ok(g, k - 1, steps_next);
    if (deferred) {
        // local residual with the pre-smoother's pending x-update(s) folded into its load phase (x written back),
        // r = b - A x: 40 B/DOF instead of 24 + 24; in the lazy form the dead step wrote neither x nor p (16 B/DOF
        // instead of 40) and this pass reads r as well (48 B/DOF)
        ApplyArgs a{};
        a.alpha = -1.0;
        a.lambda = g->lambda;
        a.x = cur[0]->d;
        if (deferred == 3)             // (49 B/DOF: x, p0, p1, r and b in, x and the restricted column out)
            need(g->ctx->fold_restrict && apply_defers3(L, lev(g, k)), "three pending x-updates where the local residual cannot carry them");
        finish_x_in_load(a, dx, cur[0]->d);
        a.src = cur[1]->d;
        a.out = cur[2]->d;
        a.flags = 1 | (x_zero ? 128 : 0);
        if (g->ctx->fold_restrict && apply_restricts(L, lev(g, k))) {
            if (inside) a.out = nullptr;          // (hmg_vcycle_down hands r back: there it is stored as well)
            a.rcoarse = nxt[1]->d;
            a.ldrc = lev(g, k - 1).ld;
            apply_then_sum(g, lev(g, k), a, true, -1, -1, /*sum_out=*/false);
            if (!skip_fill) launch_fill(L, nxt[0]->d, vec_len(nxt[0]), 0.0);
            return deferred;
        }
        apply_then_sum(g, lev(g, k), a, true, -1, -1, /*sum_out=*/false);
    } else {
        apply(g, lev(g, k), -1.0, cur[0]->d, cur[1]->d, cur[2]->d, 1);                        // local residual
    }
    restrict_level(g, k, cur[2]->d, nxt[1]->d);
    if (!skip_fill) launch_fill(L, nxt[0]->d, vec_len(nxt[0]), 0.0);
    return deferred;
}

// Up leg (src/multigrid.jl:112-115): coarse-grid correction x_k += P x_{k-1}, post-smoother (role PostTop on the finest
// level, PostBelow below it).
// cx: what level k - 1's post-smoother left of its x (hand_up); hand_up: may this level's post-smoother leave its own in turn?
// lazy_r: the caller is hmg_vcycle / hmg_fcg_step on its top level and has settled the grid's pending record
XUpdates vcycle_up(hmg_grid *g, int k, int steps, hmg_vec **st, Role role, const XUpdates *cx = nullptr, bool hand_up = false,
                   bool lazy_r = false, bool lazy_x = false)
{
    hmg_vec **cur = st + 5 * (k - 1);
    hmg_vec **nxt = st + 5 * (k - 2);
    const Launch &L = g->ctx->L;
    // coarse-grid correction: folded into the post-smoother's first residual where the fused kernel can hold the
    // coarse column in LDS next to the lattice image (two workgroups per CU must still fit), else a separate pass
    const bool fold_p = g->ctx->fold_prolong && g->fuse_cg && apply_lds_bytes(lev(g, k)) <= 160 * 1024 &&
                        apply_lds_bytes(lev(g, k)) + sizeof(double) * (size_t)lev(g, k - 1).nf <= 80 * 1024;
    need(!(cx && cx->count) || fold_p, "pending coarse x-updates without the folded prolongation");
    if (!fold_p) launch_prolong_add(L, lev(g, k), lev(g, k - 1), g->md.ncells, nxt[0]->d, cur[0]->d);
    SmoothForm form = smooth_form(g, k, steps, role);
    form.hand_up = hand_up && form.tail == Tail::DeadX2;
    form.lazy_r = lazy_r && (form.tail == Tail::Top2 || form.tail == Tail::Top3) && lazy_r_ok(g, cur[2], cur[3], cur[4]);
    form.lazy_x = lazy_x && form.lazy_r && lazy_x_ok(g, k, form.tail == Tail::Top3 ? 3 : 2, cur[0], cur[2], cur[3], cur[4]);
    return smooth(g, k, steps, cur[0], cur[1], cur[2], cur[3], cur[4], form, fold_p ? nxt[0] : nullptr, cx);
}

// Does level k's post-smoother take the coarse x with its last two updates pending?  Its first residual must be the launch that
// stages the coarse column in the lattice image (the conditions of vcycle_up() and smooth(), and the kernel's own), and the level
// below must end in the one-pass form (DeadX2) that is handed up instead.  Nothing else reads that x: the next V-cycle's down leg
// enters the level with a zero guess (src/multigrid.jl:106).  Inside hmg_vcycle only -- hmg_vcycle_up takes a caller's coarse x.
bool coarse_x_folds(const hmg_grid *g, int k, int steps_below)
{
    const hmg_ctx *c = g->ctx;
    if (k < 3 || g->smoother != 0 || !c->fold_coarse_x || !c->lazy_post || !c->fold_prolong || !c->lean_post || !g->fuse_cg || !c->prolong_in_image) return false;
    const LevelDev &lv = g->ld[(size_t)k - 1];
    if (!(apply_lds_bytes(lv) > 48 * 1024 && apply_lds_bytes(lv) <= 160 * 1024 &&
          apply_lds_bytes(lv) + sizeof(double) * (size_t)g->ld[(size_t)k - 2].nf <= 80 * 1024))
        return false;
    return apply_folds_coarse_x(c->L, lv) && smooth_form(g, k - 1, steps_below, Role::PostBelow).tail == Tail::DeadX2;
}

// hand_up: the level above finishes this level's x in its first residual (coarse_x_folds()); returns what is left to it
XUpdates vcycle_level(hmg_grid *g, int k, int steps, int steps_coarse, hmg_vec **st, bool top, bool zero_guess, bool hand_up,
                      const XUpdates &carry_x = {}, bool lazy_x = false)
{
    // ref: src/multigrid.jl:73-119
    if (k == 1) {                                  // (the scatter of the level-1 solution overwrites every entry of x)
        hmg_vec **cur = st;
        coarse_solve(g, cur[1], cur[0]);
        return {};
    }
    // (below the top level x is the zero initial guess the level above left -- written only if this level needs it in memory;
    //  a zero guess on the top level (hmg_fcg_step) is written here on the same condition)
    const bool x_zero = (zero_guess || !top) && zero_entry_ok(g, k, steps);
    if (top && zero_guess && !x_zero) launch_fill(g->ctx->L, st[5 * (k - 1)]->d, vec_len(st[5 * (k - 1)]), 0.0);
    const int deferred = vcycle_down(g, k, steps, st, /*inside=*/true, x_zero, steps_coarse, carry_x);
    if (top) g->ctx->last_pre_form = deferred;
    const XUpdates cx = vcycle_level(g, k - 1, steps_coarse, steps_coarse, st, false, false, coarse_x_folds(g, k, steps_coarse));
    if (top) g->ctx->last_top_form = g->ctx->last_r_form = g->ctx->last_ap_form = g->ctx->last_x_form = 0;
    return vcycle_up(g, k, steps, st, top ? Role::PostTop : Role::PostBelow, &cx, hand_up, /*lazy_r=*/top, /*lazy_x=*/top && lazy_x);
}

}  // namespace

void vcycle(hmg_grid *g, int k, int steps, int steps_coarse, hmg_vec **st, bool top, bool zero_guess, bool lazy_x)
{
    const XUpdates carry_x = top ? enter_top(g, k, st, zero_guess) : XUpdates{};
    (void)vcycle_level(g, k, steps, steps_coarse, st, top, zero_guess, /*hand_up=*/false, carry_x, lazy_x);
}

}  // namespace hmg

extern "C" {

int hmg_grid_reserve_spare(hmg_grid *g, int enable)
{
    HMG_TRY
    need(g != nullptr, "null grid");
    need(g->ctx != nullptr, "this grid was created without a device context (host tables only)");
    if (enable) {
        (void)reserve_top_spare(g, true);
    } else {
        materialize_r(g);                        // (x is finished; a record without a stored Ap rebuilds it from the spare vector)
        release_top_spare(g);
        g->top_spare_refused = true;             // ... and the first vector of the finest level does not bring it back
    }
    HMG_END
}

// The smoother of a grid: 0 = the reference's CG (default), 1 = CG preconditioned by the inverse diagonal of the assembled operator.
// Kind 1 reserves one vector per level >= 2 here (setup memory; formed at the next call that smooths); kind 0 hands them back.
// one vector per level >= 2 for the inverse diagonals of kinds 1 and 2, unless the grid holds them already
static void reserve_smoother_diag(hmg_grid *g, const char *who)
{
    if (g->dinv.size() == (size_t)g->nlevels) return;
    release_smoother_diag(g);
    std::vector<std::unique_ptr<DevBuf<double>>> bufs((size_t)g->nlevels);
    int64_t bytes = 0;
    for (int level = 2; level <= g->nlevels; ++level) {
        const size_t n = (size_t)g->ld[(size_t)level - 1].ld * (size_t)g->mesh_full.ncells;
        bufs[(size_t)level - 1].reset(new DevBuf<double>);
        try {
            bufs[(size_t)level - 1]->alloc(n);
        } catch (const std::exception &) {
            (void)hipGetLastError();
            throw std::runtime_error(std::string(who) + ": the inverse diagonal of level " + std::to_string(level) + " (" +
                                     std::to_string((n * sizeof(double)) >> 20) + " MiB) does not fit the device memory; the smoother is unchanged");
        }
        bytes += (int64_t)(n * sizeof(double));
    }
    g->dinv = std::move(bufs);
    g->ctx->smoother_diag_bytes += bytes;
}

int hmg_grid_set_smoother(hmg_grid *g, int kind)
{
    HMG_TRY
    need(g != nullptr, "null grid");
    need(g->ctx != nullptr, "this grid was created without a device context (host tables only)");
    need(kind == 0 || kind == 1, "smoother kind must be 0 (CG) or 1 (Jacobi-preconditioned CG); kind 2, the Chebyshev-Jacobi smoother, "
                                 "takes its parameters through hmg_grid_set_smoother_chebyshev");
    HIPCHK(hipSetDevice(g->ctx->device));
    materialize_r(g);                            // (the Jacobi smoother forms its diagonal in the Ap of the next call)
    if (kind == 1) reserve_smoother_diag(g, "hmg_grid_set_smoother");
    if (kind == 0) {
        release_smoother_diag(g);
        // (a vector of the finest level created from now on brings the spare direction vector of the CG forms as it always did)
    }
    g->smoother = kind;
    g->cheb_ratio = 0.0;
    g->cheb_given.clear();
    g->cheb_hi.clear();
    g->dinv_ready = false;
    g->op_epoch += 1;                            // an hmg_fcg object's direction belongs to the old preconditioner
    HMG_END
}

// Kind 2: the Chebyshev polynomial in dinv o A on [lambda_hi / ratio, lambda_hi].  Reserves the inverse diagonals as kind 1 does; the
// bounds that are not given are formed with them (ensure_smoother_diag).
int hmg_grid_set_smoother_chebyshev(hmg_grid *g, double ratio, const double *lambda_hi)
{
    HMG_TRY
    need(g != nullptr, "null grid");
    need(g->ctx != nullptr, "this grid was created without a device context (host tables only)");
    need(std::isfinite(ratio) && (ratio <= 0.0 || ratio > 1.0), "hmg_grid_set_smoother_chebyshev: ratio must be a finite number > 1 (<= 0: the default)");
    std::vector<double> given;
    if (lambda_hi) {
        given.assign(lambda_hi, lambda_hi + g->nlevels);
        for (double &v : given) {
            need(!std::isnan(v) && v < HUGE_VAL, "hmg_grid_set_smoother_chebyshev: lambda_hi must hold finite numbers (<= 0: the bound is formed)");
            if (!(v > 0.0)) v = 0.0;
        }
    }
    if (cheb_needs_given(g) && !cheb_all_given(g, given)) throw std::runtime_error(CHEB_PARTITIONED);   // (before anything changes)
    HIPCHK(hipSetDevice(g->ctx->device));
    materialize_r(g);                            // (the diagonal and the bound are formed in the Ap of the next call)
    reserve_smoother_diag(g, "hmg_grid_set_smoother_chebyshev");
    g->smoother = 2;
    g->cheb_ratio = ratio > 1.0 ? ratio : CHEB_DEFAULT_RATIO;
    g->cheb_given = std::move(given);
    g->cheb_hi.clear();
    g->dinv_ready = false;
    g->op_epoch += 1;                            // an hmg_fcg object's direction belongs to the old preconditioner
    HMG_END
}

// lambda_lo and lambda_hi of a level as the Chebyshev smoother uses them; forms the inverse diagonal and the bound first where they are
// stale, with a scratch vector from the context's pool.  Synchronises: not for the inside of a V-cycle.
int hmg_grid_smoother_bounds(hmg_grid *g, int level, double *lambda_lo, double *lambda_hi)
{
    HMG_TRY
    need(g != nullptr, "null grid");
    need(g->ctx != nullptr, "this grid was created without a device context (host tables only)");
    need(g->smoother == 2, "hmg_grid_smoother_bounds: the grid's smoother has no bounds (hmg_grid_set_smoother_chebyshev)");
    need(level >= 2 && level <= g->nlevels, "level out of range (2..nlevels: level 1 has no smoother)");
    hmg_ctx *c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    if (!(g->dinv_ready && g->dinv_level_ready[(size_t)level - 1])) {
        materialize_r(g);
        const size_t bytes = sizeof(double) * (size_t)g->ld[(size_t)level - 1].ld * (size_t)std::max<int64_t>(g->mesh_full.ncells, 1);
        ensure_reduce_scratch(c, (int64_t)(bytes / sizeof(double)));   // (no vector of this level need exist yet)
        double *scratch = vec_alloc(c, bytes);
        try {
            ensure_smoother_diag(g, level, scratch);
            HIPCHK(hipStreamSynchronize(c->stream));
        } catch (...) {
            (void)hipStreamSynchronize(c->stream);
            vec_release(c, scratch, bytes);
            throw;
        }
        vec_release(c, scratch, bytes);
    }
    const double hi = g->cheb_hi[(size_t)level - 1];
    if (lambda_hi) *lambda_hi = hi;
    if (lambda_lo) *lambda_lo = hi / g->cheb_ratio;
    HMG_END
}

int hmg_grid_smoother(const hmg_grid *g) { return g ? g->smoother : -1; }

int hmg_grid_smoother_diag(hmg_grid *g, int level, hmg_vec *out)
{
    HMG_TRY
    need(g != nullptr, "null grid");
    need(g->smoother != 0, "hmg_grid_smoother_diag: the grid's smoother has no diagonal (hmg_grid_set_smoother(grid, 1), hmg_grid_set_smoother_chebyshev)");
    need(level >= 2 && level <= g->nlevels, "level out of range (2..nlevels: level 1 has no smoother)");
    check_vec(g, level, out, "out");
    ensure_smoother_diag(g, level, out->d);
    launch_copy(g->ctx->L, out->d, g->dinv[(size_t)level - 1]->p, vec_len(out));
    HMG_END
}

// ---- fused fast path ----------------------------------------------------------------------------
int hmg_smooth(hmg_grid *g, int level, int steps, hmg_vec *x, hmg_vec *b, hmg_vec *r, hmg_vec *p, hmg_vec *Ap)
{
    HMG_TRY
    need(g && g->has_op, "operator not set");
    check_vec(g, level, x, "x");
    check_vec(g, level, b, "b");
    check_vec(g, level, r, "r");
    check_vec(g, level, p, "p");
    check_vec(g, level, Ap, "Ap");
    ensure_smoother_diag(g, level, Ap->d);
    smooth(g, level, steps, x, b, r, p, Ap, smooth_form(g, level, steps, Role::Plain));
    HMG_END
}

// Where the five vectors of a level lie in HBM relative to each other moves the passes that stream five or six of them
// at once by up to 8 % (tools/dev/placement_pick.py: three smoothing steps at config 3 take 61.2 ... 66.5 ms depending on
// which of ten equal allocations plays which role; moving a vector INSIDE its allocation changes nothing, no rule in the
// virtual addresses, another process on the same box draws another table -- the physical pages decide).  So the choice is
// made by measurement, FFTW style: time this level's share of a V-cycle (the down and the up half, src/multigrid.jl:100-115,
// with the pointer exchanges and folds the real cycle uses) for `trials` assignments of the 5 + `extra` blocks to the roles
// x, b, r, p, Ap and keep the fastest.
int hmg_level_tune_placement(hmg_grid *g, int level, int steps, hmg_vec **states, int extra, int trials, double *ms_out)
{
    HMG_TRY
    need(g && g->has_op && states, "null argument or operator not set");
    need(level >= 2 && level <= g->nlevels, "level must be 2..nlevels (level 1 has no smoother)");
    need(steps >= 1, "steps must be positive");
    need(extra >= 0 && extra <= 8, "extra must be 0..8");
    need(trials >= 1 && trials <= 512, "trials must be 1..512");
    hmg_vec **state = states + 5 * (level - 1);
    hmg_vec **below = states + 5 * (level - 2);
    for (int q = 0; q < 5; ++q) {
        check_vec(g, level, state[q], "states[] (level)");
        check_vec(g, level - 1, below[q], "states[] (level - 1)");
        need(state[q]->own && state[q]->bytes == state[0]->bytes && state[q]->alloc_cells == state[0]->alloc_cells,
             "the five vectors of the level must be hmg_vec_create'd vectors");
        for (int p = 0; p < q; ++p) need(state[p] != state[q] && state[p]->d != state[q]->d, "the five vectors must be distinct");
    }
    hmg_ctx *c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    materialize_r(g);                            // (memory blocks change hands below)
    ensure_smoother_diag(g, level, state[4]->d);
    const size_t bytes = state[0]->bytes;
    const int64_t n = vec_len(state[0]);
    std::vector<double *> blk;
    for (int q = 0; q < 5; ++q) blk.push_back(state[q]->d);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    std::vector<int> first = {0, 1, 2, 3, 4}, best = first;
    auto assign = [&](const std::vector<int> &a) {
        for (int q = 0; q < 5; ++q) state[q]->d = blk[(size_t)a[q]];
    };
    auto cleanup = [&](const std::vector<int> &keep) {      // the blocks no handle refers to go back
        assign(keep);
        (void)hipStreamSynchronize(c->stream);
        for (size_t i = 0; i < blk.size(); ++i)
            if (std::find(keep.begin(), keep.end(), (int)i) == keep.end()) (void)hipFree(blk[i]);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    };
    double t_first = 0.0, t_best = 0.0;
    try {
        // Everything that can fail on ONE rank only (the spare blocks, the events) comes before the first collective, and on a
        // partitioned grid the ranks agree on the outcome: run() below holds exchanges, and a rank that threw here alone would
        // leave the others blocked in them.
        std::string local_failure;
        try {
            for (int e = 0; e < extra; ++e) blk.push_back(vec_alloc(c, bytes));
            HIPCHK(hipEventCreate(&e0));
            HIPCHK(hipEventCreate(&e1));
        } catch (const std::exception &ex) {
            local_failure = ex.what();
        }
        if (has_exchange(g) && g->part && g->scalar_sum) {
            double failed = local_failure.empty() ? 0.0 : 1.0;
            double *d = c->L.scal + S_HOST;
            HIPCHK(hipMemcpyAsync(d, &failed, sizeof(double), hipMemcpyHostToDevice, c->stream));
            scalar_sum(g, S_HOST, 1);
            HIPCHK(hipMemcpyAsync(&failed, d, sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            if (failed > 0.0 && local_failure.empty())
                local_failure = "placement tuning: another rank could not set it up (nothing was changed on this rank)";
        }
        if (!local_failure.empty()) throw std::runtime_error(local_failure);
        const int nb = (int)blk.size();
        auto run = [&](const std::vector<int> &a) {
            assign(a);
            launch_fill(c->L, state[0]->d, n, 0.5);       // (r, p, Ap are written before they are read)
            launch_fill(c->L, state[1]->d, n, 1.0);
            HIPCHK(hipEventRecord(e0, c->stream));
            // as hmg_vcycle runs them on its top level (each half exchanges the r and p pointers: restored by the pair; the
            // coarse x stays the zero it is)
            (void)vcycle_down(g, level, steps, states, /*inside=*/true, /*x_zero=*/false, /*steps_next=*/2);
            (void)vcycle_up(g, level, steps, states, Role::PostTop);
            HIPCHK(hipEventRecord(e1, c->stream));
            HIPCHK(hipEventSynchronize(e1));
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, e0, e1));
            return (double)ms;
        };
        (void)run(first);                                  // first touch of every kernel and table
        uint64_t rng = 0x9E3779B97F4A7C15ull;              // (the same sequence on every rank: the halves may hold collectives)
        auto next = [&]() {
            rng ^= rng << 13;
            rng ^= rng >> 7;
            rng ^= rng << 17;
            return rng;
        };
        t_best = 1e300;
        for (int t = 0; t < trials; ++t) {
            std::vector<int> a(nb);
            for (int i = 0; i < nb; ++i) a[i] = i;
            if (t > 0)
                for (int i = 0; i < 5; ++i) std::swap(a[i], a[i + (int)(next() % (uint64_t)(nb - i))]);
            a.resize(5);
            const double ms = run(a);
            if (t == 0) t_first = ms;
            if (ms < t_best) {
                t_best = ms;
                best = a;
            }
        }
        {   // a second look at both (always: every rank must issue the same number of calls): the handles keep what they
            // had unless the gain is real
            const double again_first = run(first), again_best = run(best);
            t_first = std::min(t_first, again_first);
            t_best = std::max(t_best, again_best);
            if (!(t_best < 0.995 * t_first)) {
                best = first;
                t_best = t_first;
            }
        }
    } catch (...) {
        cleanup(first);
        throw;
    }
    cleanup(best);
    for (int q = 0; q < 5; ++q) {
        HIPCHK(hipMemsetAsync(state[q]->d, 0, bytes, c->stream));
        HIPCHK(hipMemsetAsync(below[q]->d, 0, sizeof(double) * (size_t)vec_len(below[q]), c->stream));
    }
    if (ms_out) {
        ms_out[0] = t_first;
        ms_out[1] = t_best;
    }
    HMG_END
}

int hmg_vcycle(hmg_grid *g, int top_level, int steps, int steps_coarse, hmg_vec **states)
{
    HMG_TRY
    need(g && g->has_op && states, "null argument or operator not set");
    need(top_level >= 1 && top_level <= g->nlevels, "top_level out of range");
    for (int l = 1; l <= top_level; ++l)
        for (int q = 0; q < 5; ++q) check_vec(g, l, states[5 * (l - 1) + q], "states[]", /*settle_pending=*/false);   // (vcycle() does)
    ensure_smoother_diag(g, top_level, states);
    vcycle(g, top_level, steps, steps_coarse, states, /*top=*/true, /*zero_guess=*/false, /*lazy_x=*/true);
    HMG_END
}

static void check_two_levels(hmg_grid *g, int level, hmg_vec **states)
{
    need(g && g->has_op && states, "null argument or operator not set");
    need(level >= 2 && level <= g->nlevels, "level out of range (2..nlevels)");
    for (int l = level - 1; l <= level; ++l)
        for (int q = 0; q < 5; ++q) check_vec(g, l, states[5 * (l - 1) + q], "states[]");
}

int hmg_vcycle_down(hmg_grid *g, int level, int steps, hmg_vec **states)
{
    HMG_TRY
    check_two_levels(g, level, states);
    ensure_smoother_diag(g, level, states[5 * (level - 1) + 4]->d);
    g->ctx->last_pre_form = vcycle_down(g, level, steps, states);
    HMG_END
}

int hmg_vcycle_up(hmg_grid *g, int level, int steps, hmg_vec **states)
{
    HMG_TRY
    check_two_levels(g, level, states);
    ensure_smoother_diag(g, level, states[5 * (level - 1) + 4]->d);
    (void)vcycle_up(g, level, steps, states, Role::PostTop);   // as the finest level of hmg_vcycle
    HMG_END
}

}  // extern "C"

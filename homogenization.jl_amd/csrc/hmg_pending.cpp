// The records of work a V-cycle left undone on the finest level -- the last r-update (PendingR, options lazy_r / lazy_ap) and the last
// x-updates (PendingX, option lazy_x): when they may open, how they open, and every way they close -- formed by the launch the eager
// tail would have made, carried by the next V-cycle's first residual, handed to the flexible CG, or dropped unread.
#include "hmg_objects.hpp"

#include <algorithm>

namespace hmg {

// May the finest level's post-smoother inside hmg_vcycle leave its last r-update pending (option lazy_r)?  Not where the memory
// can be read behind the library's back (caller-owned vectors, pointers handed out -- p too: it changes places with r), and not on
// a partitioned grid, where the deferred sum over the ranks would be a collective at a place no rank can foresee.
bool lazy_r_ok(const hmg_grid *g, const hmg_vec *r, const hmg_vec *p, const hmg_vec *Ap)
{
    if (!g->ctx->lazy_r || g->smoother != 0 || g->part || has_exchange(g) || g->scalar_sum) return false;
    for (const hmg_vec *v : {r, p, Ap})
        if (!v->own || v->exposed) return false;
    return r != Ap && g->pend_alpha() != nullptr && vec_len(r) > 0;
}

// formed: the eager launch has run (the caller reads r after every cycle, hmg_grid::r_reader); the record only watches
// ap_stored = false: the last CG step ran in the dead form, Ap is rebuilt when the record is settled (option lazy_ap)
void open_pending(hmg_grid *g, int level, hmg_vec *r, hmg_vec *Ap, int slot, bool formed, bool ap_stored)
{
    LifetimeLock lock(lifetime_mutex());
    need(!g->pend.r, "a pending r-update was not settled before the next one");
    need(ap_stored || !formed, "a formed r-update without its Ap");
    g->pend.r = r;
    g->pend.Ap = Ap;
    g->pend.level = level;
    g->pend.slot = slot;
    g->pend.formed = formed;
    g->pend.ap_stored = ap_stored;
    g->ctx->last_r_form = formed ? 0 : 1;
    g->ctx->last_ap_form = ap_stored ? 0 : 1;
    auto &open = g->ctx->pend_grids;
    if (std::find(open.begin(), open.end(), g) == open.end()) open.push_back(g);
}

// Can the last step of the three-update form, where its r-update may stay pending (lazy_r_ok()), run without storing A p_2 (option
// lazy_ap)?  Where the record is opened unformed, and the dead launch is the one every fused apply family has (the pre-smoother's
// two-update tail takes it on every level: x, x2, no out, no xout, no xacc).
bool lazy_ap_ok(const hmg_grid *g) { return g->ctx->lazy_ap && !g->r_reader; }

// May that launch leave the x-updates pending as well (option lazy_x)?  Under lazy_r_ok()'s conditions with x and p added (the spare
// vector is the library's own), on a level whose first residual can carry them (apply_carries_x()).
// updates: how many the tail leaves, 2 or 3
bool lazy_x_ok(const hmg_grid *g, int level, int updates, const hmg_vec *x, const hmg_vec *r, const hmg_vec *p, const hmg_vec *Ap)
{
    if (!g->ctx->lazy_x || !g->fuse_cg) return false;
    for (const hmg_vec *v : {x, p})
        if (!v->own || v->exposed) return false;
    if (x == r || x == p || x == Ap || p == r || p == Ap) return false;
    return apply_carries_x(g->ctx->L, lev(g, level), g->md, g->lambda, updates);
}

// form 0: x is finished (its reader memory is set); the record watches whether it is read again
void open_pending_x(hmg_grid *g, int level, hmg_vec *x, hmg_vec *p, hmg_vec *r, int form)
{
    LifetimeLock lock(lifetime_mutex());
    need(!g->pendx.x, "pending x-updates were not settled before the next ones");
    g->pendx.x = x;
    g->pendx.p = form ? p : nullptr;
    g->pendx.r = form ? r : nullptr;
    g->pendx.level = level;
    g->pendx.form = form;
    g->ctx->last_x_form = form;
    if (form) g->ctx->x_deferred += 1;
}

namespace {

// the record is settled or dropped: an Ap it had to keep alive goes now
void close_pending(hmg_grid *g)
{
    hmg_vec *orphan = g->pend.orphan_Ap ? g->pend.Ap : nullptr;
    g->pend = PendingR{};
    if (g->ctx) {
        auto &open = g->ctx->pend_grids;
        open.erase(std::remove(open.begin(), open.end(), g), open.end());
    }
    if (orphan) release_vec(orphan);
}

void drop_pending(hmg_grid *g)
{
    settle_x(g);                                 // (pending x-updates read the r_2 that is about to go)
    if (!g->pend.formed) g->ctx->r_dropped += 1;
    g->r_reader = false;                         // nobody read it: the next V-cycle defers
    close_pending(g);
}

}  // namespace

// What a record with updates to form (form 2 or 3) says is pending, read from where it rests: p1 is the p handle's memory (form 2) or the
// grid's spare vector (form 3, where the p handle holds p0), r2 the r handle's, the ratios those of the saved block.
XUpdates saved_updates(const hmg_grid *g, const PendingX &q)
{
    need(g->pend_alpha() != nullptr && (q.form == 2 || (q.form == 3 && g->top_spare.p != nullptr)),
         "pending x-updates have lost the spare vector they rest on");
    XUpdates u;
    u.count = q.form;
    u.last = XS_LAST;
    u.prev = XS_PREV;
    u.beta = XS_BETA;
    u.first = XS_FIRST;
    u.p0 = q.form == 3 ? q.p->d : nullptr;
    u.p1 = q.form == 3 ? g->top_spare.p : q.p->d;
    u.r2 = q.r->d;
    u.scal = g->pend_alpha();
    return u;
}

// The eager launch of pending x-updates, now: k_cg_x_tail on (x, p1, p0, r2) with the ratios put aside as its scalars.  Before
// anything that forms or drops the pending r on the same vectors: the rebuild of Ap reads r_2 and the spare vector and writes Ap
// alone, the r-update then overwrites r_2 -- x first, and both see their inputs.
void settle_x(hmg_grid *g, bool read)
{
    LifetimeLock lock(lifetime_mutex());
    const PendingX q = g->pendx;
    if (!q.x) return;
    if (q.form) {
        HIPCHK(hipSetDevice(g->ctx->device));
        launch_cg_x_tail(g->ctx->L, q.x->d, vec_len(q.x), saved_updates(g, q), nullptr);
        g->ctx->x_settled += 1;
        if (read) g->ctx->x_settled_read += 1;
    }
    g->pendx = PendingX{};
    if (read) g->x_reader = true;                // (the next V-cycle finishes its x at once and watches again)
}

PendingX take_pending_x(hmg_grid *g, const hmg_vec *x)
{
    LifetimeLock lock(lifetime_mutex());
    const PendingX q = g->pendx;
    if (q.x == x && !q.form) {                   // (only watched: this reader costs nothing where the updates ride with it)
        g->pendx = PendingX{};
        g->x_reader = false;
        return PendingX{};
    }
    if (q.x != x) {
        settle_x(g);
        return PendingX{};
    }
    need(g->pend_alpha() != nullptr && (q.form == 2 || g->top_spare.p != nullptr), "pending x-updates have lost the spare vector they rest on");
    g->pendx = PendingX{};
    return q;
}

namespace {

// x is about to be overwritten unread, or goes: nothing is left to form
void drop_x(hmg_grid *g)
{
    g->pendx = PendingX{};
    g->x_reader = false;
}

// the x half of settle_overwritten() / pending_keeps(): x itself is dropped, a vector the updates rest on settles them
void release_x(hmg_grid *g, const hmg_vec *v)
{
    const PendingX &q = g->pendx;
    if (!q.x) return;
    if (v == q.x)
        drop_x(g);
    else if (v == q.p || v == q.r)
        settle_x(g);
}

}  // namespace

// The eager launch, now: launch_cg_rupdate_faces<0> on (r, r, Ap) with the stored step length (alpha / 1.0 is alpha) and its r.r
// into the slot the eager tail would have written.  (No sum over ranks: the record opens on unpartitioned grids only.)
void materialize_r(hmg_grid *g, bool read)
{
    LifetimeLock lock(lifetime_mutex());
    settle_x(g);
    const PendingR q = g->pend;
    if (!q.r) return;
    if (!q.formed) {
        HIPCHK(hipSetDevice(g->ctx->device));
        if (!q.ap_stored) {
            // the apply of the last CG step as the eager tail launches it: p_2 = r_2 + beta_2 p_1 formed in LDS, Ap = A p_2 with the
            // edge / node interface sum, p.Ap into S_PAP3 again -- beta_2 from the numbers the x-only tail saved behind the step length
            need(g->top_spare.p != nullptr && g->pend_alpha() != nullptr, "a pending r-update has lost the spare vector it rests on");
            const LevelDev &lv = lev(g, q.level);
            ApplyArgs a{};
            a.alpha = 1.0;
            a.lambda = g->lambda;
            a.x = q.r->d;
            a.x2 = g->top_spare.p;
            a.out = q.Ap->d;
            a.scal = g->pend_alpha();
            a.s = XS_BETA;
            a.flags = 1;
            apply_then_sum(g, lv, a, true, S_PAP3, -1, true, false);
            g->ctx->ap_rebuilt += 1;
        }
        launch_cg_rupdate_faces(g->ctx->L, lev(g, q.level), g->md, q.r->d, q.r->d, q.Ap->d, vec_len(q.r), XS_LAST, q.slot, g->pend_alpha());
        g->ctx->r_materialized += 1;
        if (read) g->ctx->r_materialized_read += 1;
    }
    close_pending(g);
    if (read) g->r_reader = true;                // (the next V-cycle forms its r at once and watches again)
}

void settle_overwritten(const hmg_vec *v)
{
    if (!v || !v->g || (!v->g->pend.r && !v->g->pendx.x)) return;
    LifetimeLock lock(lifetime_mutex());
    hmg_grid *g = v->g;
    release_x(g, v);
    if (!g->pend.r) return;
    if (v == g->pend.Ap)
        materialize_r(g);
    else if (v == g->pend.r)
        drop_pending(g);
}

bool pending_keeps(hmg_vec *v)
{
    hmg_grid *g = v->g;
    if (!g) return false;
    release_x(g, v);                             // (a vector pending x-updates rest on: they are formed now, the one launch a destroy makes)
    if (!g->pend.r) return false;
    if (v == g->pend.r)
        drop_pending(g);
    else if (v == g->pend.Ap) {
        if (!g->pend.formed) {
            g->pend.orphan_Ap = true;
            return true;
        }
        close_pending(g);                        // (a record that only watches needs no Ap)
    }
    return false;
}

// Entry of a V-cycle on the top level k: a record on the very r and Ap this cycle is about to overwrite (its first residual writes
// every entry of r, src/multigrid.jl:50; Ap is scratch) is dropped; any other is settled, the x-only tail needs the grid's
// step-length buffer for itself.
// Pending x-updates (option lazy_x) on this cycle's own x, p and r ride in its first residual: the record is taken out of the grid and
// what it says is pending returned (count 0: nothing to carry).  Any other are settled; with zero_guess x is not read at all and they are dropped.  A record
// that only watched x and is still open: nobody read x since, the reader memory goes.
XUpdates enter_top(hmg_grid *g, int k, hmg_vec **st, bool zero_guess)
{
    XUpdates carry;
    if (g->pendx.x) {
        LifetimeLock lock(lifetime_mutex());
        const PendingX px = g->pendx;
        bool same_x = k >= 2 && k == px.level;
        for (int i = 0; i < 5 * k && same_x; ++i) {
            const int at = i - 5 * (k - 1);
            same_x = (st[i] == px.x) == (at == 0) && (!px.form || ((st[i] == px.r) == (at == 2) && (st[i] == px.p) == (at == 3)));
        }
        if (!px.form) {
            if (same_x) g->x_reader = false;
            g->pendx = PendingX{};
        } else if (same_x && zero_guess)
            drop_x(g);
        else if (same_x && g->fuse_cg && g->smoother == 0 && g->ctx->lazy_x && px.r == g->pend.r && !g->pend.formed &&
                 apply_carries_x(g->ctx->L, lev(g, k), g->md, g->lambda, px.form)) {
            carry = saved_updates(g, px);
            g->pendx = PendingX{};               // (r_2 stays where it is: the pending r on the same states is dropped below, never formed)
        } else
            settle_x(g);
    }
    const PendingR &q = g->pend;
    if (!q.r) {
        need(!carry.count, "pending x-updates without the pending r they rest on");
        return carry;
    }
    bool same = k >= 2 && k == q.level;
    for (int i = 0; i < 5 * k && same; ++i) {
        const bool is_r = i == 5 * (k - 1) + 2, is_Ap = i == 5 * (k - 1) + 4;
        same = (st[i] == q.r) == is_r && (st[i] == q.Ap) == is_Ap;
    }
    if (same)
        settle_overwritten(q.r);
    else {
        if (carry.count) {                       // (cannot happen: the x record shares its r with this one and saw the same states)
            g->pendx = PendingX{st[5 * (k - 1)], st[5 * (k - 1) + 3], st[5 * (k - 1) + 2], k, carry.count};
            carry = XUpdates{};
        }
        materialize_r(g);
    }
    return carry;
}

}  // namespace hmg

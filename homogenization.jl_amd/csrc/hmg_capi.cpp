// C ABI (include/hmg.h), the entry points that front no module of their own: vector operations, the primitives, the driver's
// right-hand sides and integrals.  Each checks its arguments and calls the launchers or a module (hmg_objects.hpp).
#include "../../include/hmg.h"
#include "hmg_objects.hpp"

#include <algorithm>
#include <cmath>

extern "C" {

static const int64_t STAGE_DOUBLES = (int64_t)32 << 20;   // 256 MiB staging chunks

// host (Nf x Ne, hierarchical order) <-> level vector (entity-major, padded columns), through a staging buffer on the device
static void staged_copy(hmg_vec *v, double *host, bool upload)
{
    hmg_grid *g = v->g;
    const LevelDev &lv = lev(g, v->level);
    const int64_t ncells = g->md.ncells;
    int64_t cells_per = std::max<int64_t>(1, STAGE_DOUBLES / lv.nf);
    cells_per = std::min(cells_per, ncells);
    DevBuf<double> stage;
    stage.alloc((size_t)cells_per * lv.nf);
    for (int64_t c0 = 0; c0 < ncells; c0 += cells_per) {
        const int64_t nc = std::min(cells_per, ncells - c0);
        const size_t bytes = sizeof(double) * nc * lv.nf;
        if (upload) {
            HIPCHK(hipMemcpyAsync(stage.p, host + c0 * lv.nf, bytes, hipMemcpyHostToDevice, g->ctx->stream));
            launch_permute(g->ctx->L, lv, nc, stage.p, v->d + c0 * lv.ld, 1);
        } else {
            launch_permute(g->ctx->L, lv, nc, v->d + c0 * lv.ld, stage.p, 0);
            HIPCHK(hipMemcpyAsync(host + c0 * lv.nf, stage.p, bytes, hipMemcpyDeviceToHost, g->ctx->stream));
        }
        HIPCHK(hipStreamSynchronize(g->ctx->stream));
    }
}

int hmg_vec_upload(hmg_vec *v, const double *host)
{
    HMG_TRY
    need(v && host, "null argument");
    settle(v);
    staged_copy(v, const_cast<double *>(host), true);
    HMG_END
}

int hmg_vec_download(hmg_vec *v, double *host)
{
    HMG_TRY
    need(v && host, "null argument");
    settle(v);
    staged_copy(v, host, false);
    HMG_END
}

int hmg_vec_fill(hmg_vec *v, double value)
{
    HMG_TRY
    need(v != nullptr, "null vector");
    settle_overwritten(v);
    launch_fill(v->g->ctx->L, v->d, vec_len(v), value);
    HMG_END
}

int hmg_vec_fill_random(hmg_vec *v, uint64_t seed, int64_t cell_offset)
{
    HMG_TRY
    need(v != nullptr, "null vector");
    settle(v);
    launch_fill_random(v->g->ctx->L, lev(v->g, v->level), v->g->md.ncells, v->d, seed, cell_offset);
    HMG_END
}

int hmg_vec_copy(hmg_vec *dst, hmg_vec *src)
{
    HMG_TRY
    need(dst && src, "null vector");
    check_vec(dst->g, dst->level, src, "src");
    if (dst != src) settle_overwritten(dst);
    launch_copy(dst->g->ctx->L, dst->d, src->d, vec_len(dst));
    HMG_END
}

int hmg_vec_axpy(double alpha, hmg_vec *x, hmg_vec *y)
{
    HMG_TRY
    need(x && y, "null vector");
    check_vec(y->g, y->level, x, "x");
    settle(y);
    launch_axpy(y->g->ctx->L, alpha, x->d, y->d, vec_len(y));
    HMG_END
}

int hmg_vec_xpby(hmg_vec *r, double beta, hmg_vec *p)
{
    HMG_TRY
    need(r && p, "null vector");
    check_vec(p->g, p->level, r, "r");
    settle(p);
    launch_xpby(p->g->ctx->L, r->d, beta, p->d, vec_len(p));
    HMG_END
}

int hmg_vec_dot(hmg_vec *x, hmg_vec *y, double *out)
{
    HMG_TRY
    need(x && y && out, "null argument");
    check_vec(x->g, x->level, y, "y");
    settle(x);
    launch_dot(x->g->ctx->L, x->d, y->d, vec_len(x), S_TMP);
    scalar_sum(x->g, S_TMP, 1);
    *out = read_scalar(x->g->ctx, S_TMP);
    HMG_END
}

int hmg_vec_norm_unique(hmg_vec *r, double *out)
{
    HMG_TRY
    need(r && out, "null argument");
    settle(r);
    launch_norm2_unique(r->g->ctx->L, lev(r->g, r->level), r->g->md, r->d, S_TMP);
    scalar_sum(r->g, S_TMP, 1);
    *out = std::sqrt(read_scalar(r->g->ctx, S_TMP));
    HMG_END
}

// ---- primitives ---------------------------------------------------------------------------------
int hmg_apply(hmg_grid *g, int level, double alpha, hmg_vec *x, hmg_vec *y)
{
    HMG_TRY
    need(g && g->has_op, "operator not set");
    check_vec(g, level, x, "x");
    check_vec(g, level, y, "y");
    need(x->d != y->d, "x and y must not alias");
    apply(g, lev(g, level), alpha, x->d, y->d, y->d, 0);
    HMG_END
}

int hmg_apply_ex(hmg_grid *g, int level, double alpha, hmg_vec *x, hmg_vec *src, hmg_vec *out, int constrain)
{
    HMG_TRY
    need(g && g->has_op, "operator not set");
    check_vec(g, level, x, "x");
    check_vec(g, level, out, "out");
    if (src) check_vec(g, level, src, "src");
    need(x->d != out->d, "x and out must not alias");
    apply(g, lev(g, level), alpha, x->d, src ? src->d : nullptr, out->d, constrain ? 1 : 0);
    HMG_END
}

int hmg_residual(hmg_grid *g, int level, hmg_vec *x, hmg_vec *b, hmg_vec *r)
{
    HMG_TRY
    need(g && g->has_op, "operator not set");
    check_vec(g, level, x, "x");
    check_vec(g, level, b, "b");
    check_vec(g, level, r, "r");
    need(x->d != r->d, "x and r must not alias");
    apply(g, lev(g, level), -1.0, x->d, b->d, r->d, 1);
    HMG_END
}

int hmg_constraint(hmg_grid *g, int level, hmg_vec *x)
{
    HMG_TRY
    check_vec(g, level, x, "x");
    launch_mask(g->ctx->L, lev(g, level), g->md, x->d, 0);
    HMG_END
}

int hmg_interface_sum(hmg_grid *g, int level, hmg_vec *x)
{
    HMG_TRY
    check_vec(g, level, x, "x");
    interface_sum(g, lev(g, level), x->d);
    HMG_END
}

int hmg_zero_duplicates(hmg_grid *g, int level, hmg_vec *x)
{
    HMG_TRY
    check_vec(g, level, x, "x");
    launch_mask(g->ctx->L, lev(g, level), g->md, x->d, 1);
    HMG_END
}

int hmg_restrict(hmg_grid *g, int level_fine, hmg_vec *r_fine, hmg_vec *b_coarse)
{
    HMG_TRY
    need(g && level_fine >= 2, "restriction needs level_fine >= 2");
    check_vec(g, level_fine, r_fine, "r_fine");
    check_vec(g, level_fine - 1, b_coarse, "b_coarse");
    restrict_level(g, level_fine, r_fine->d, b_coarse->d);
    HMG_END
}

int hmg_prolong_add(hmg_grid *g, int level_fine, hmg_vec *x_coarse, hmg_vec *x_fine)
{
    HMG_TRY
    need(g && level_fine >= 2, "prolongation needs level_fine >= 2");
    check_vec(g, level_fine, x_fine, "x_fine");
    check_vec(g, level_fine - 1, x_coarse, "x_coarse");
    launch_prolong_add(g->ctx->L, lev(g, level_fine), lev(g, level_fine - 1), g->md.ncells, x_coarse->d, x_fine->d);
    HMG_END
}

int hmg_gather_base(hmg_grid *g, hmg_vec *v1, double *host_u)
{
    HMG_TRY
    need(g && host_u, "null argument");
    check_vec(g, 1, v1, "v1");
    DevBuf<double> u;
    u.alloc((size_t)g->md.nnodes);
    launch_gather_base(g->ctx->L, g->md, lev(g, 1).ld, v1->d, u.p);
    HIPCHK(hipMemcpyAsync(host_u, u.p, sizeof(double) * g->md.nnodes, hipMemcpyDeviceToHost, g->ctx->stream));
    HIPCHK(hipStreamSynchronize(g->ctx->stream));
    HMG_END
}

int hmg_scatter_base(hmg_grid *g, const double *host_u, hmg_vec *v1)
{
    HMG_TRY
    need(g && host_u, "null argument");
    check_vec(g, 1, v1, "v1");
    DevBuf<double> u;
    u.alloc((size_t)g->md.nnodes);
    HIPCHK(hipMemcpyAsync(u.p, host_u, sizeof(double) * g->md.nnodes, hipMemcpyHostToDevice, g->ctx->stream));
    launch_scatter_base(g->ctx->L, g->md, lev(g, 1).ld, u.p, v1->d);
    HIPCHK(hipStreamSynchronize(g->ctx->stream));
    HMG_END
}

// ---- driver right-hand sides -------------------------------------------------------
int hmg_rhs_axi_grad(hmg_grid *g, const double *xi, hmg_vec *b)
{
    HMG_TRY
    need(g && g->has_op && xi && b, "null argument or operator not set");
    check_vec(g, b->level, b, "b");
    const MeshTables &M = g->cur();
    const int dim = g->dim;
    // P = -detJ * (Jinv' * (sigma .* xi))   (ref: ...homogenized_coefficients.jl:468); a full tensor: sigma * xi
    const int sn = g->sig_n;
    std::vector<double> pv((size_t)M.ncells * 3, 0.0);
    for (int64_t c = 0; c < M.ncells; ++c) {
        const double *Ji = &M.jinv[(size_t)c * dim * dim];
        const double *sg = &g->sigma[(size_t)c * sn];
        double sx[3] = {0.0, 0.0, 0.0};
        if (sn != dim)
            for (int k = 0; k < dim; ++k)
                for (int l = 0; l < dim; ++l) sx[k] += sg[sym_index(dim, k, l)] * xi[l];
        for (int a = 0; a < dim; ++a) {
            double s = 0.0;
            for (int k = 0; k < dim; ++k) s += Ji[k + dim * a] * (sn != dim ? sx[k] : sg[k] * xi[k]);
            pv[(size_t)c * 3 + a] = -M.detj[c] * s;
        }
    }
    DevBuf<double> d;
    d.upload(pv, g->ctx->stream);
    launch_rhs_dphi(g->ctx->L, lev(g, b->level), M.ncells, d.p, b->d);
    HIPCHK(hipStreamSynchronize(g->ctx->stream));
    HMG_END
}

int hmg_local_rhs(hmg_grid *g, hmg_vec *b)
{
    HMG_TRY
    need(g && b, "null argument");
    check_vec(g, b->level, b, "b");
    const MeshTables &M = g->cur();
    LevelDev lv = lev(g, b->level);
    const LevelTables &T = g->lt[b->level - 1];
    // b[:, e] = (int phi over the refined reference simplex) * |det J_e|   (ref: src/implicit_fine_grid.jl:391-409);
    // evaluated by the d.p kernel of the other right-hand sides with d = (load, 0, 0), p = (|det J|, 0, 0)
    std::vector<double> tab((size_t)T.nf * 3, 0.0), pv((size_t)M.ncells * 3, 0.0);
    for (int t = 0; t < T.nf; ++t) tab[(size_t)t * 3] = T.load[t];
    for (int64_t c = 0; c < M.ncells; ++c) pv[(size_t)c * 3] = M.detj[c];
    DevBuf<double> dt, dp;
    dt.upload(tab, g->ctx->stream);
    dp.upload(pv, g->ctx->stream);
    lv.dphi = dt.p;
    launch_rhs_dphi(g->ctx->L, lv, M.ncells, dp.p, b->d);
    HIPCHK(hipStreamSynchronize(g->ctx->stream));
    HMG_END
}

int hmg_integrate(hmg_grid *g, int mode, hmg_vec *v, hmg_vec *vprev, int64_t ncells_subset, const double *xi, double *out)
{
    HMG_TRY
    need(g && g->has_op && v && out, "null argument or operator not set");
    // (partitioned grid: the subset counts LOCAL cells and the result is this rank's share; the host sums over ranks)
    check_vec(g, v->level, v, "v");
    need(ncells_subset >= 0 && ncells_subset <= g->md.ncells, "subset out of range");
    const MeshTables &M = g->cur();
    const int dim = g->dim;
    if (mode == 2) {   // integrate_area: sum(mass) * sum |J|   (ref: ...:673-689)
        const double m_total = dim == 3 ? 1.0 / 6.0 : 0.5;
        double area = 0.0;
        for (int64_t c = 0; c < ncells_subset; ++c) area += m_total * M.detj[c];
        *out = area;
        return 0;
    }
    need(mode == 0 || mode == 1 || mode == 3 || mode == 4,
         "mode must be 0 (first term), 1 (terms), 2 (area), 3 (mass pairing) or 4 (load pairing)");
    if (ncells_subset == 0) {
        *out = 0.0;
        return 0;
    }
    static const char *const need_second[5] = {
        "mode 0 needs the right-hand side rhs_a.xi.grad(v) (hmg_rhs_axi_grad) as second vector",
        "mode 1 needs the previous iterate as second vector", "",
        "mode 3 needs the second corrector as second vector (it may be v itself)",
        "mode 4 needs a load vector (such as hmg_rhs_axi_grad's) as second vector"};
    need(vprev != nullptr, need_second[mode]);
    check_vec(g, v->level, vprev, "second vector");
    // (modes 0 and 1 run with the second vector as the pass's source next to its input; 3 and 4 write nothing and read both)
    need(mode >= 3 || v->d != vprev->d, "the two vectors must not alias");
    (void)xi;   // (mode 0: the direction already sits in the right-hand side the caller passes)
    if (mode == 4) {
        launch_integrate_load(g->ctx->L, lev(g, v->level), g->md, ncells_subset, v->d, vprev->d, S_TMP);
    } else {
        set_slab(g, lev(g, v->level));
        launch_integrate(g->ctx->L, lev(g, v->level), g->md, mode, ncells_subset, v->d, vprev->d, S_TMP);
    }
    *out = read_scalar(g->ctx, S_TMP);
    HMG_END
}

int hmg_next_rhs(hmg_grid *g, hmg_vec *x, hmg_vec *b)
{
    HMG_TRY
    need(g && g->has_op && x && b, "null argument or operator not set");
    check_vec(g, x->level, b, "b");
    check_vec(g, x->level, x, "x");
    need(x->d != b->d, "x and b must not alias");
    // b = lambda*|J|*M*x  (ref: ...homogenized_coefficients.jl:695-713)
    g->ctx->L.apply_mass_only = 1;
    set_slab(g, lev(g, x->level));
    try {
        launch_apply(g->ctx->L, lev(g, x->level), g->md, 1.0, g->lambda, x->d, nullptr, b->d, 0);
    } catch (...) {
        g->ctx->L.apply_mass_only = 0;
        throw;
    }
    g->ctx->L.apply_mass_only = 0;
    HMG_END
}

}  // extern "C"

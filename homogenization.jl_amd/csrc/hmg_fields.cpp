// hmg_cell_moments: per coarse cell the mean gradient and the Gram tensor of the gradient of a level vector.
//
// Cell c has the affine map x = p0 + J x^; with Jinv = J^-T (MeshTables::jinv, column-major) d_k v = sum_a Jinv[k,a] d^_a v.  The
// kernel (hmg_fields.hip) leaves the reference sums of the cell's column,
//   l_a  = sum_i d_a[i] v_i             d_a[i]     = int_ref d^_a phi_i                   (LevelDev::dphi)
//   q_ab = sum_i v_i (A^(a,b) v_c)_i    A^(a,b)_ij = int_ref d^_a phi_i d^_b phi_j        (the class table's terms; an
//                                                                                          off-diagonal term is A^(a,b) + A^(b,a))
// and this module turns them into physical moments, |ref| = 1/2 (2D), 1/6 (3D), |c| = |J| |ref|:
//   m_v = Jinv l / |ref|                G_v = |J| Jinv q Jinv^T
//   m_u = xi + m_v                      G_u = |c| (xi xi^T + xi m_v^T + m_v xi^T) + G_v       for u = xi . x + v
//
// hmg_cell_pair_moments: the symmetrised cross moment of two vectors v, w of one level.  The same kernel leaves
//   q_ab = sum_i v_i (A^(a,b) w_c)_i  (an off-diagonal term: q_ab + q_ba), l^v_a, l^w_a
// and, with sym(A) = (A + A^T) / 2,
//   S_vw = |J| Jinv sym(q) Jinv^T       S_uz = S_vw + |c| sym(xi_v xi_w^T + xi_v m_w^T + m_v xi_w^T)
// for u = xi_v . x + v, z = xi_w . x + w.  S_vv = G_v.
// hmg_cell_moments is the pair of a vector with itself: one handle given twice is read once, and its rows hold one set of l.
// Cells larger than the LDS (3D level 7, 2D levels 9..11) are refused unless the context option "cell_moments_windows" routes them
// to the window kernels (hmg_fields_window.hip: 1 -- levels that do not fit only; 2 -- every level those kernels can address); the
// rows and the transforms below are the same on either path.
// Not on a V-cycle's path: both allocate (the raw sums, from the context's pool of level-vector memory) and synchronise.
#include "../../include/hmg.h"
#include "hmg_fields.hpp"
#include "hmg_objects.hpp"

#include <chrono>

namespace hmg {

// (declared in hmg_objects.hpp: hmg_extrema.cpp walks the same lists)
SlabTables slab_tables(const hmg_grid *g, const LevelDev &lv)
{
    const LevelBufs &B = *g->lb[lv.level - 1];
    SlabTables st{};
    st.head = B.slab_head.p;
    st.ld_word = B.slab_ld_word.p;
    st.cp_word = B.slab_cp_word.p;
    st.cp_slot = B.slab_cp_slot.p;
    st.nslab = B.nslab;
    st.lds_nodes = B.slab_lds_nodes;
    st.max_surf = B.slab_max_surf;
    st.max_int = B.slab_max_int;
    return st;
}

}  // namespace hmg

namespace {

// the raw sums of one kernel pass, downloaded: `launch` enqueues the kernel that fills `bytes` of device memory; the kernel's time
// (device events) and the download's (host clock) go to the two counters
template <class F>
void raw_sums(hmg_ctx *c, std::vector<double> &raw, F launch, int64_t &kernel_ns, int64_t &download_ns)
{
    const size_t bytes = sizeof(double) * raw.size();
    double *d = vec_alloc(c, bytes);
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    try {
        HIPCHK(hipEventCreate(&ev0));
        HIPCHK(hipEventCreate(&ev1));
        HIPCHK(hipEventRecord(ev0, c->stream));
        launch(d);
        HIPCHK(hipEventRecord(ev1, c->stream));
        HIPCHK(hipEventSynchronize(ev1));
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
        const auto t0 = std::chrono::steady_clock::now();
        HIPCHK(hipMemcpyAsync(raw.data(), d, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        kernel_ns = (int64_t)((double)ms * 1e6);
        download_ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    } catch (...) {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        vec_release(c, d, bytes);
        throw;
    }
    (void)hipEventDestroy(ev0);
    (void)hipEventDestroy(ev1);
    vec_release(c, d, bytes);
}

// does this call take the window kernels?  fits: the verdict of the LDS-resident kernel.  Throws the refusal where no kernel serves.
bool takes_window(const hmg_grid *g, const LevelDev &lv, const SlabTables &st, bool fits, const char *fn)
{
    const int mode = g->ctx->moments_windows;
    const bool can = mode != 0 && cell_moments_window_ok(lv, st);
    if (can && (mode == 2 || !fits)) return true;
    if (!fits)
        throw std::runtime_error(std::string(fn) + ": one cell of level " + std::to_string(lv.level) + " (" + std::to_string(lv.nf) +
                                 " nodes) does not fit the LDS; the per-cell moments serve " +
                                 (g->dim == 3 ? "3D levels up to 6" : "2D levels up to 8") +
                                 (mode == 0 && cell_moments_window_ok(lv, st)
                                      ? "; the context option \"cell_moments_windows\" = 1 takes larger cells through the window kernels"
                                      : ""));
    return false;
}

// the raw rows of one call (hmg_fields.hpp), downloaded: nraw sums per cell, one set of l where w is v
struct RawRows {
    int nraw = 0;
    bool same = false;
    std::vector<double> sums;
};

// What both entry points (fn) do before their transforms: the checks of v and w as level vectors of g, the choice of the kernel,
// its launch and the download.  pair: the times go to the counters "cell_pair_moments_*_ns", otherwise to "cell_moments_*_ns"
// (the last call's, hmg_ctx_counter).
RawRows cell_raw_rows(hmg_grid *g, hmg_vec *v, hmg_vec *w, bool pair, const char *fn)
{
    check_vec(g, v->level, v, "v");
    if (w != v) {
        need(w->g == g, "vector belongs to another grid: w");
        if (w->level != v->level)
            throw std::runtime_error(std::string(fn) + ": v (level " + std::to_string(v->level) + ") and w (level " +
                                     std::to_string(w->level) + ") are of different levels");
        check_vec(g, v->level, w, "w");
    }
    const LevelDev &lv = lev(g, v->level);
    const SlabTables st = slab_tables(g, lv);
    RawRows R;
    R.same = v->d == w->d;
    R.nraw = cell_moments_nraw(g->dim, R.same);
    const bool window = takes_window(g, lv, st, cell_moments_ok(lv, R.same), fn);
    const int64_t nc = g->md.ncells;
    if (nc == 0) return R;
    hmg_ctx *c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    R.sums.resize((size_t)R.nraw * (size_t)nc);
    raw_sums(c, R.sums, [&](double *d) {
        if (window) {
            launch_cell_pair_moments_window(c->L, lv, st, nc, v->d, w->d, d);
            c->moments_window_launches += 1;
        } else
            launch_cell_pair_moments(c->L, lv, nc, v->d, w->d, d);
    }, pair ? c->pair_moments_kernel_ns : c->moments_kernel_ns, pair ? c->pair_moments_download_ns : c->moments_download_ns);
    return R;
}

// sym(q) of a raw row: an off-diagonal term of the class table is q_ab + q_ba
void unpack_sym(int dim, const double *r, double q[3][3])
{
    for (int a = 0; a < dim; ++a)
        for (int b = a; b < dim; ++b) {
            const double t = r[sym_index(dim, a, b)];
            q[a][b] = q[b][a] = a == b ? t : 0.5 * t;
        }
}

// m = Jinv l / |ref|;  Jinv[k,a] = Ji[k + dim a]
void mean_gradient(int dim, const double *Ji, const double *l, double ref, double m[3])
{
    for (int k = 0; k < dim; ++k) {
        double s = 0.0;
        for (int a = 0; a < dim; ++a) s += Ji[k + dim * a] * l[a];
        m[k] = s / ref;
    }
}

// (|J| Jinv q Jinv^T)_kl
double physical_form(int dim, const double *Ji, double det, const double q[3][3], int k, int l)
{
    double s = 0.0;
    for (int a = 0; a < dim; ++a) {
        double qj = 0.0;
        for (int b = 0; b < dim; ++b) qj += q[a][b] * Ji[l + dim * b];
        s += Ji[k + dim * a] * qj;
    }
    return det * s;
}

}  // namespace

extern "C" {

int hmg_cell_moments_count(const hmg_grid *grid)
{
    if (!grid) {
        last_error() = "null grid";
        return -1;
    }
    return grid->dim + sym_ncomp(grid->dim);
}

int hmg_cell_moments(hmg_grid *g, hmg_vec *v, const double *xi, double *out)
{
    HMG_TRY
    need(g != nullptr, "null grid");
    need(out != nullptr, "hmg_cell_moments: null output array");
    need(g->ctx != nullptr, "hmg_cell_moments: this grid was created without a device context (host tables only): no compute path exists on the CPU");
    need(v != nullptr, "hmg_cell_moments: null vector");
    const RawRows R = cell_raw_rows(g, v, v, false, "hmg_cell_moments");
    const MeshTables &M = g->cur();
    const int dim = g->dim, nq = sym_ncomp(dim), nmom = dim + nq;
    const int64_t nc = g->md.ncells;
    const double ref = dim == 3 ? 1.0 / 6.0 : 0.5;
    for (int64_t e = 0; e < nc; ++e) {
        const double *r = &R.sums[(size_t)e * R.nraw];
        const double *Ji = &M.jinv[(size_t)e * dim * dim];
        const double det = M.detj[e], vol = det * ref;
        double q[3][3], mv[3];
        unpack_sym(dim, r, q);
        mean_gradient(dim, Ji, r + nq, ref, mv);
        double *o = out + (size_t)e * nmom;
        for (int k = 0; k < dim; ++k) o[k] = xi ? xi[k] + mv[k] : mv[k];
        for (int k = 0; k < dim; ++k)
            for (int l = k; l < dim; ++l) {
                double G = physical_form(dim, Ji, det, q, k, l);
                if (xi) G += vol * (xi[k] * xi[l] + xi[k] * mv[l] + mv[k] * xi[l]);
                o[dim + sym_index(dim, k, l)] = G;
            }
    }
    HMG_END
}

int hmg_cell_pair_moments_count(const hmg_grid *grid)
{
    if (!grid) {
        last_error() = "null grid";
        return -1;
    }
    return sym_ncomp(grid->dim);
}

int hmg_cell_pair_moments(hmg_grid *g, hmg_vec *v, hmg_vec *w, const double *xi_v, const double *xi_w, double *out)
{
    HMG_TRY
    need(g != nullptr, "null grid");
    need(out != nullptr, "hmg_cell_pair_moments: null output array");
    need(g->ctx != nullptr, "hmg_cell_pair_moments: this grid was created without a device context (host tables only): no compute path exists on the CPU");
    need(v != nullptr, "hmg_cell_pair_moments: null vector v");
    need(w != nullptr, "hmg_cell_pair_moments: null vector w");
    const RawRows R = cell_raw_rows(g, v, w, true, "hmg_cell_pair_moments");
    const MeshTables &M = g->cur();
    const int dim = g->dim, nq = sym_ncomp(dim);
    const int64_t nc = g->md.ncells;
    const double ref = dim == 3 ? 1.0 / 6.0 : 0.5;
    const bool with_xi = xi_v || xi_w;
    double xv[3] = {0.0, 0.0, 0.0}, xw[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < dim; ++k) {
        if (xi_v) xv[k] = xi_v[k];
        if (xi_w) xw[k] = xi_w[k];
    }
    for (int64_t e = 0; e < nc; ++e) {
        const double *r = &R.sums[(size_t)e * R.nraw];
        const double *Ji = &M.jinv[(size_t)e * dim * dim];
        const double det = M.detj[e], vol = det * ref;
        double q[3][3], mv[3], mw[3];
        unpack_sym(dim, r, q);
        mean_gradient(dim, Ji, r + nq, ref, mv);
        mean_gradient(dim, Ji, r + nq + (R.same ? 0 : dim), ref, mw);   // (w is v: one set of l, m_w = m_v)
        double *o = out + (size_t)e * nq;
        for (int k = 0; k < dim; ++k)
            for (int l = k; l < dim; ++l) {
                double S = physical_form(dim, Ji, det, q, k, l);
                if (with_xi)
                    S += vol * 0.5 * ((xv[k] * xw[l] + xv[l] * xw[k]) + (xv[k] * mw[l] + xv[l] * mw[k]) + (mv[k] * xw[l] + mv[l] * xw[k]));
                o[sym_index(dim, k, l)] = S;
            }
    }
    HMG_END
}

}  // extern "C"

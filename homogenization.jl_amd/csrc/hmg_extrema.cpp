// hmg_cell_extrema: per coarse cell the maximum and the minimum over the cell's fine elements of a quadratic form of the P1
// gradient of a level vector, and the number of elements on which the form exceeds each of a few thresholds.
//
// The pass over fine elements.  In the lattice coordinates of a level (slot_ijk, m = 2^(level-1) intervals per edge) every fine
// element is a Kuhn simplex {p, p + pi1, p + pi1 + pi2, p + s}: pi a permutation of a basis a, b, c (2D: a, b) of stencil
// directions, s = a + b + c, p the lexicographically lowest vertex.  build_element_tables finds the basis among the stencil's
// directions, marks per slot which of the 6 (2D: 2) simplices with p at that slot are elements of T.ref_cells, and checks the
// result against that list.  Along an element's path the successive differences of u are g . pi1, g . pi2, g . pi3: the components
// g~ = B^T g_lattice, B = [a b c], without a matrix per element.
//
// Cell c has the affine map x = p0 + J x^, x^ = lattice / m; with Jinv = J^-T (MeshTables::jinv, column-major)
//   grad u = Jinv m B^-T g~ = M_c g~            M_c = m Jinv B^-T
// so for u = xi . x + v and a symmetric Q_c
//   q_T = grad u . Q_c grad u = (xi~ + g~_T) . Q~_c (xi~ + g~_T)        Q~_c = M_c^T Q_c M_c,  xi~ = M_c^-1 xi
// and the kernel (hmg_extrema.hip) sees one row (Q~, xi~) per cell and never J.
// Cells larger than the LDS (3D level 7, 2D levels 9..11) are refused unless the context option "cell_extrema_windows" routes them
// to the window kernels (hmg_extrema_window.hip: 1 -- levels that do not fit only; 2 -- every level those kernels can address);
// mask, rows and results are the same on either path, and so are the bits on a level both serve.
// Not on a V-cycle's path: the call allocates (rows and results, from the context's pool of level-vector memory; the element
// mask of a level once, at its first call) and synchronises.
#include "../../include/hmg.h"
#include "hmg_extrema.hpp"
#include "hmg_fields.hpp"
#include "hmg_objects.hpp"

#include <array>
#include <cmath>

namespace hmg {

namespace {

using V3 = std::array<int, 3>;

V3 add(const V3 &x, const V3 &y) { return {x[0] + y[0], x[1] + y[1], x[2] + y[2]}; }
V3 sub(const V3 &x, const V3 &y) { return {x[0] - y[0], x[1] - y[1], x[2] - y[2]}; }

// inverse of a dim x dim matrix (row-major in 3 x 3 storage), Gauss-Jordan with partial pivoting; false: singular
bool invert(int dim, const double A[3][3], double inv[3][3])
{
    double w[3][6];
    for (int r = 0; r < dim; ++r)
        for (int c = 0; c < dim; ++c) {
            w[r][c] = A[r][c];
            w[r][dim + c] = r == c ? 1.0 : 0.0;
        }
    for (int k = 0; k < dim; ++k) {
        int p = k;
        for (int r = k + 1; r < dim; ++r)
            if (std::fabs(w[r][k]) > std::fabs(w[p][k])) p = r;
        if (w[p][k] == 0.0 || !std::isfinite(w[p][k])) return false;
        if (p != k)
            for (int c = 0; c < 2 * dim; ++c) std::swap(w[p][c], w[k][c]);
        const double d = w[k][k];
        for (int c = 0; c < 2 * dim; ++c) w[k][c] /= d;
        for (int r = 0; r < dim; ++r) {
            if (r == k) continue;
            const double f = w[r][k];
            for (int c = 0; c < 2 * dim; ++c) w[r][c] -= f * w[k][c];
        }
    }
    for (int r = 0; r < dim; ++r)
        for (int c = 0; c < dim; ++c) inv[r][c] = w[r][dim + c];
    return true;
}

// permutations of the basis in lexicographic order: bit k of the element mask
const int PERM3[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
const int PERM2[2][3] = {{0, 1, 0}, {1, 0, 0}};

}  // namespace

// Codes slot(p) * 8 + k -> the element's vertices p, p + pi1, p + pi1 + pi2, p + s as hierarchical node ids, pi the permutation
// bit k names (include/hmg.h: hmg_grid_element_vertices; the one decode of hmg_cell_extrema_where's kernel results too).
// The lattice -> slot table is formed per call from slot_ijk: (m + 1)^dim ints, next to nothing beside the call's own work.
void element_vertices(const LevelTables &T, const ElementTables &E, int64_t n, const int32_t *codes, int32_t *nodes, const char *who)
{
    const int dim = T.dim, nv = dim + 1, nperm = dim == 3 ? 6 : 2, m1 = T.m + 1;
    auto idx = [&](int i, int j, int k) { return ((size_t)k * m1 + j) * m1 + i; };
    std::vector<int32_t> slot_at((size_t)m1 * m1 * (dim == 3 ? m1 : 1), -1);
    for (int q = 0; q < T.nf; ++q) slot_at[idx(T.slot_ijk[3 * q], T.slot_ijk[3 * q + 1], T.slot_ijk[3 * q + 2])] = q;
    for (int64_t e = 0; e < n; ++e) {
        const int32_t code = codes[e];
        const int64_t slot = code >> 3;
        const int k = code & 7;
        if (code < 0 || slot >= T.nf)
            throw std::runtime_error(std::string(who) + ": code " + std::to_string(code) + " (entry " + std::to_string(e) +
                                     ") names slot " + std::to_string(slot) + "; level " + std::to_string(T.level) + " has slots 0 to " +
                                     std::to_string(T.nf - 1));
        if (k >= nperm || !((E.mask[slot] >> k) & 1u))
            throw std::runtime_error(std::string(who) + ": code " + std::to_string(code) + " (entry " + std::to_string(e) +
                                     ") names element " + std::to_string(k) + " of slot " + std::to_string(slot) +
                                     ", whose bit of \"elem_mask\" is clear: no fine element of level " + std::to_string(T.level));
        int x[3] = {T.slot_ijk[3 * slot], T.slot_ijk[3 * slot + 1], T.slot_ijk[3 * slot + 2]};
        nodes[e * nv] = T.slot2hier[slot];
        const int *pi = dim == 3 ? PERM3[k] : PERM2[k];
        for (int r = 0; r < dim; ++r) {
            for (int a = 0; a < dim; ++a) x[a] += E.dirs[(size_t)pi[r] * dim + a];
            nodes[e * nv + r + 1] = T.slot2hier[slot_at[idx(x[0], x[1], x[2])]];   // (inside the cell: build_element_tables checked)
        }
    }
}

ElementTables build_element_tables(const LevelTables &T)
{
    const int dim = T.dim, nv = dim + 1, nperm = dim == 3 ? 6 : 2;
    auto fail = [&](const char *what) {
        throw std::runtime_error("fine elements of level " + std::to_string(T.level) + ": " + what);
    };
    ElementTables E;
    E.dim = dim;

    // ---- the basis and its taps, from the stencil's direction list ----
    const int(*D)[3];
    const int ndir = stencil_dirs(dim, &D);
    auto tap_of = [&](const V3 &d) {
        for (int q = 1; q < ndir; ++q)
            if (D[q][0] == d[0] && D[q][1] == d[1] && D[q][2] == d[2]) return q;
        return -1;
    };
    std::vector<V3> pos;                                 // directions to lexicographically larger nodes
    for (int q = 1; q < ndir; ++q) {
        const V3 d{D[q][0], D[q][1], D[q][2]};
        if (d > V3{0, 0, 0}) pos.push_back(d);
    }
    if ((int)pos.size() != (dim == 3 ? 7 : 3)) fail("the stencil does not have 7 (2D: 3) positive directions");
    std::vector<V3> basis;                               // ... that are no sum of two others
    for (const V3 &d : pos) {
        bool sum = false;
        for (const V3 &x : pos)
            for (const V3 &y : pos) sum = sum || add(x, y) == d;
        if (!sum) basis.push_back(d);
    }
    std::sort(basis.begin(), basis.end());
    if ((int)basis.size() != dim) fail("the positive stencil directions have no basis of dim vectors");
    V3 s{0, 0, 0};
    for (const V3 &b : basis) s = add(s, b);
    for (const V3 &b : basis)
        for (int a = 0; a < dim; ++a) E.dirs.push_back(b[a]);
    if (dim == 3) {
        const V3 &a = basis[0], &b = basis[1], &c = basis[2];
        const int taps[7] = {tap_of(a), tap_of(b), tap_of(c), tap_of(add(a, b)), tap_of(add(a, c)), tap_of(add(b, c)), tap_of(s)};
        const int want[7] = {EX_TAP_A, EX_TAP_B, EX_TAP_C, EX_TAP_AB, EX_TAP_AC, EX_TAP_BC, EX_TAP_S};
        for (int q = 0; q < 7; ++q) {
            if (taps[q] != want[q]) fail("the taps of the lattice basis are not those the extrema kernel reads");
            E.taps[q] = taps[q];
        }
    } else {
        const int taps[3] = {tap_of(basis[0]), tap_of(basis[1]), tap_of(s)};
        const int want[3] = {EX2_TAP_A, EX2_TAP_B, EX2_TAP_S};
        for (int q = 0; q < 3; ++q) {
            if (taps[q] != want[q]) fail("the taps of the lattice basis are not those the extrema kernel reads");
            E.taps[q] = taps[q];
        }
    }
    auto perm = [&](int k) { return dim == 3 ? PERM3[k] : PERM2[k]; };

    // ---- the mask, from the element list ----
    const int m = T.m, m1 = m + 1;
    auto idx = [&](const V3 &x) { return (x[2] * m1 + x[1]) * m1 + x[0]; };
    auto inside = [&](const V3 &x) {
        return x[0] >= 0 && x[1] >= 0 && x[2] >= 0 && x[0] + x[1] + x[2] <= m && (dim == 3 || x[2] == 0);
    };
    std::vector<int32_t> slot_at((size_t)m1 * m1 * (dim == 3 ? m1 : 1), -1);
    auto ijk = [&](int s_) { return V3{T.slot_ijk[3 * s_], T.slot_ijk[3 * s_ + 1], T.slot_ijk[3 * s_ + 2]}; };
    for (int q = 0; q < T.nf; ++q) slot_at[idx(ijk(q))] = q;
    const size_t nel = T.ref_cells.size() / nv;
    E.mask.assign(T.nf, 0);
    using Key = std::array<int32_t, 4>;
    auto listed_key = [&](size_t e) {                   // an element of the list as sorted slots
        Key key{-1, -1, -1, -1};
        for (int q = 0; q < nv; ++q) {
            const int h = T.ref_cells[e * nv + q];
            if (h < 0 || h >= T.nf) fail("an element names a node that does not exist");
            key[q] = T.hier2slot[h];
        }
        std::sort(key.begin(), key.begin() + nv);
        return key;
    };
    std::vector<int32_t> owner((size_t)T.nf * nperm, -1);   // (slot, bit) -> the listed element that set it
    for (size_t e = 0; e < nel; ++e) {
        const Key key = listed_key(e);
        V3 X[4];
        for (int q = 0; q < nv; ++q) X[q] = ijk(key[q]);
        std::sort(X, X + nv);
        int which[3] = {-1, -1, -1};
        for (int q = 0; q < dim; ++q) {
            const V3 d = sub(X[q + 1], X[q]);
            for (int b = 0; b < dim; ++b)
                if (basis[b] == d) which[q] = b;
            if (which[q] < 0) fail("an element is no Kuhn simplex of the lattice basis");
        }
        int k = -1;
        for (int p = 0; p < nperm; ++p) {
            bool eq = true;
            for (int q = 0; q < dim; ++q) eq = eq && perm(p)[q] == which[q];
            if (eq) k = p;
        }
        if (k < 0) fail("an element's path is no permutation of the lattice basis");
        const int p0 = slot_at[idx(X[0])];
        if (E.mask[p0] & (1u << k)) fail("an element is listed twice");
        E.mask[p0] |= (uint8_t)(1u << k);
        owner[(size_t)p0 * nperm + k] = (int32_t)e;
    }
    // ---- back from (slot, bit) to elements: exactly the list.  Every listed element set a bit of its own (above), so the two
    // sets are equal if every set bit rebuilds the element that set it and the counts agree ----
    for (int q = 0; q < T.nf; ++q)
        for (int k = 0; k < nperm; ++k) {
            if (!(E.mask[q] & (1u << k))) continue;
            V3 x = ijk(q);
            Key key{-1, -1, -1, -1};
            key[0] = q;
            for (int r = 0; r < dim; ++r) {
                x = add(x, basis[perm(k)[r]]);
                if (!inside(x)) fail("a marked simplex leaves the cell");
                key[r + 1] = slot_at[idx(x)];
            }
            std::sort(key.begin(), key.begin() + nv);
            const int32_t e = owner[(size_t)q * nperm + k];
            if (e < 0 || key != listed_key((size_t)e)) fail("the elements rebuilt from the mask are not the element list");
            E.nelem += 1;
        }
    if (E.nelem != (int64_t)nel) fail("the elements rebuilt from the mask are not the element list");
    if (E.nelem != (int64_t)1 << (dim * (T.level - 1))) fail("the number of elements is not 2^(dim (level - 1))");
    return E;
}

// the device copy of a level's element mask, uploaded at the first call on that level
const uint8_t *device_element_mask(hmg_grid *g, int level)
{
    FieldState &F = g->fields;
    if (F.d_mask.size() != (size_t)g->nlevels) F.d_mask.resize(g->nlevels);
    auto &buf = F.d_mask[level - 1];
    if (!buf) {
        std::unique_ptr<DevBuf<uint8_t>> b(new DevBuf<uint8_t>);
        b->upload(F.elem[level - 1].mask, g->ctx->stream);
        buf = std::move(b);
    }
    return buf->p;
}

// One row per cell for the kernels of the pass over the fine elements (hmg_cell_extrema, hmg_cell_extrema_where,
// hmg_cell_histogram): Q~ = M^T Q M, then xi~ = M^-1 xi, M = m Jinv B^-T -- cell_extrema_nrow(dim) numbers per current cell.
// form: nq numbers per cell or null (the identity); xi: dim numbers or null (0); both checked by the caller.  One text of the
// arithmetic for every caller: the same rows, bit for bit.  `who` names the call in the messages.
std::vector<double> cell_form_rows(const std::string &who, const hmg_grid *g, int level, const double *xi, const double *form)
{
    auto need = [&](bool c, const char *msg) {
        if (!c) throw std::runtime_error(who + ": " + msg);
    };
    const LevelDev &lv = lev(g, level);
    const int dim = g->dim, nq = sym_ncomp(dim), nrow = cell_extrema_nrow(dim);
    const MeshTables &M = g->cur();
    const int64_t nc = g->md.ncells;
    const ElementTables &E = g->fields.elem.at(level - 1);
    double Bm[3][3] = {{0}}, Binv[3][3];
    for (int b = 0; b < dim; ++b)
        for (int a = 0; a < dim; ++a) Bm[a][b] = E.dirs[(size_t)b * dim + a];        // columns a, b, c
    need(invert(dim, Bm, Binv), "the lattice basis is singular");
    std::vector<double> rows((size_t)nc * nrow);
    const double scale = (double)lv.m;
    std::atomic<bool> singular{false};
    parallel_for(nc, [&](int64_t e0, int64_t e1) {
        for (int64_t e = e0; e < e1; ++e) {
            const double *Ji = &M.jinv[(size_t)e * dim * dim];
            double Mc[3][3], Mi[3][3], Q[3][3];
            for (int k = 0; k < dim; ++k)
                for (int c = 0; c < dim; ++c) {
                    double s = 0.0;
                    for (int a = 0; a < dim; ++a) s += Ji[k + dim * a] * Binv[c][a];   // (B^-T)[a][c] = Binv[c][a]
                    Mc[k][c] = scale * s;
                }
            for (int k = 0; k < dim; ++k)
                for (int l = 0; l < dim; ++l)
                    Q[k][l] = form ? form[(size_t)e * nq + sym_index(dim, k, l)] : (k == l ? 1.0 : 0.0);
            double *r = &rows[(size_t)e * nrow];
            for (int a = 0; a < dim; ++a)
                for (int b = a; b < dim; ++b) {
                    double s = 0.0;
                    for (int k = 0; k < dim; ++k) {
                        double qm = 0.0;
                        for (int l = 0; l < dim; ++l) qm += Q[k][l] * Mc[l][b];
                        s += Mc[k][a] * qm;
                    }
                    r[sym_index(dim, a, b)] = s;
                }
            for (int a = 0; a < dim; ++a) r[nq + a] = 0.0;
            if (xi) {
                if (!invert(dim, Mc, Mi)) {
                    singular = true;
                    continue;
                }
                for (int a = 0; a < dim; ++a) {
                    double s = 0.0;
                    for (int k = 0; k < dim; ++k) s += Mi[a][k] * xi[k];
                    r[nq + a] = s;
                }
            }
        }
    });
    need(!singular, "a cell's geometry is singular");
    return rows;
}

}  // namespace hmg

extern "C" {

int64_t hmg_grid_fine_elements(const hmg_grid *g, int level)
{
    if (!g || level < 1 || level > g->nlevels) return -1;
    return (int64_t)1 << (g->dim * (level - 1));
}

}  // extern "C"

namespace {

// hmg_cell_extrema (located = false) and hmg_cell_extrema_where: one text of the checks, the rows and the launch; `who` names the
// call in every message.  where: host, 2 (dim + 1) ints per cell.
void cell_extrema_call(const std::string &who, bool located, hmg_grid *g, hmg_vec *v, const double *xi, const double *form, int nthr,
                       const double *thresholds, double *out, int32_t *where)
{
    auto need = [&](bool c, const char *msg) {
        if (!c) throw std::runtime_error(who + ": " + msg);
    };
    hmg::need(g != nullptr, "null grid");
    need(out != nullptr, "null output array");
    need(!located || where != nullptr, "null where array");
    need(g->ctx != nullptr, "this grid was created without a device context (host tables only): no compute path exists on the CPU");
    need(v != nullptr, "null vector");
    need(v->g == g, "vector belongs to another grid");
    if (nthr < 0 || nthr > EX_MAX_THRESHOLDS)
        throw std::runtime_error(who + ": " + std::to_string(nthr) + " thresholds; 0 to 8 are served");
    need(nthr == 0 || thresholds != nullptr, "null thresholds");
    ExtremaThresholds thr;
    for (int j = 0; j < EX_MAX_THRESHOLDS; ++j) {
        thr.t[j] = j < nthr ? thresholds[j] : HUGE_VAL;
        if (j < nthr && !std::isfinite(thr.t[j])) throw std::runtime_error(who + ": threshold " + std::to_string(j) + " is not finite");
    }
    check_vec(g, v->level, v, "v");
    const LevelDev &lv = lev(g, v->level);
    const int dim = g->dim, nq = sym_ncomp(dim);
    // the kernel: k_cell_extrema where the cell fits the LDS, the window kernels by the option "cell_extrema_windows" (1: levels
    // that do not fit; 2: every level they address)
    const SlabTables st = slab_tables(g, lv);
    const bool fits = cell_extrema_ok(lv) && cell_moments_ok(lv, true), can = cell_extrema_window_ok(lv, st);
    const int mode = g->ctx->extrema_windows;
    const bool window = mode != 0 && can && (mode == 2 || !fits);
    if (!window && !fits)
        throw std::runtime_error(who + ": one cell of level " + std::to_string(lv.level) + " (" + std::to_string(lv.nf) +
                                 " nodes) does not fit the LDS; the per-cell extrema serve " +
                                 (dim == 3 ? "3D levels up to 6" : "2D levels up to 8") +
                                 (can ? "; the context option \"cell_extrema_windows\" = 1 takes larger cells through the window kernels"
                                      : "; no window kernel addresses this level"));
    const int64_t nc = g->md.ncells;
    if (form)
        for (int64_t q = 0; q < nc * nq; ++q)
            if (!std::isfinite(form[q]))
                throw std::runtime_error(who + ": the form of cell " + std::to_string(q / nq) + " is not finite");
    if (xi)
        for (int a = 0; a < dim; ++a) need(std::isfinite(xi[a]), "xi is not finite");
    if (nc == 0) return;
    const ElementTables &E = g->fields.elem.at(v->level - 1);
    const std::vector<double> rows = cell_form_rows(who, g, v->level, xi, form);

    hmg_ctx *c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    const uint8_t *d_mask = device_element_mask(g, v->level);
    const size_t nout = (size_t)(2 + nthr) * (size_t)nc;
    const size_t row_bytes = sizeof(double) * rows.size(), out_bytes = sizeof(double) * nout;
    const size_t code_bytes = sizeof(int32_t) * 2 * (size_t)nc;
    double *d_rows = vec_alloc(c, row_bytes), *d_out = nullptr;
    int32_t *d_codes = nullptr;
    std::vector<int32_t> codes(located ? 2 * (size_t)nc : 0);
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    try {
        d_out = vec_alloc(c, out_bytes);
        if (located) d_codes = (int32_t *)vec_alloc(c, code_bytes);
        HIPCHK(hipEventCreate(&ev0));
        HIPCHK(hipEventCreate(&ev1));
        HIPCHK(hipMemcpyAsync(d_rows, rows.data(), row_bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipEventRecord(ev0, c->stream));
        if (window) {
            launch_cell_extrema_window(c->L, lv, st, nc, v->d, d_mask, d_rows, thr, nthr, d_out, d_codes);
            c->extrema_window_launches += 1;
        } else
            launch_cell_extrema(c->L, lv, nc, v->d, d_mask, d_rows, thr, nthr, d_out, d_codes);
        if (located) c->extrema_where_launches += 1;
        HIPCHK(hipEventRecord(ev1, c->stream));
        HIPCHK(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
        if (located) HIPCHK(hipMemcpyAsync(codes.data(), d_codes, code_bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
        (located ? c->extrema_where_kernel_ns : c->extrema_kernel_ns) = (int64_t)((double)ms * 1e6);
    } catch (...) {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        (void)hipStreamSynchronize(c->stream);       // (the rows' host copy goes out of scope)
        vec_release(c, d_rows, row_bytes);
        if (d_out) vec_release(c, d_out, out_bytes);
        if (d_codes) vec_release(c, (double *)d_codes, code_bytes);
        throw;
    }
    (void)hipEventDestroy(ev0);
    (void)hipEventDestroy(ev1);
    vec_release(c, d_rows, row_bytes);
    vec_release(c, d_out, out_bytes);
    if (!located) return;
    vec_release(c, (double *)d_codes, code_bytes);
    // the kernel's codes -> vertices: -1 (the cell's extrema are NaN) stays -1 in all its entries, every other code is decoded
    const int nv = dim + 1;
    const LevelTables &T = g->lt.at(v->level - 1);
    std::vector<int32_t> valid, pos;
    for (size_t q = 0; q < codes.size(); ++q)
        if (codes[q] >= 0) {
            valid.push_back(codes[q]);
            pos.push_back((int32_t)q);
        }
    std::vector<int32_t> verts(valid.size() * nv);
    element_vertices(T, E, (int64_t)valid.size(), valid.data(), verts.data(), who.c_str());
    std::fill(where, where + codes.size() * nv, -1);
    for (size_t q = 0; q < pos.size(); ++q) std::copy(&verts[q * nv], &verts[q * nv] + nv, where + (size_t)pos[q] * nv);
}

}  // namespace

extern "C" {

int hmg_cell_extrema(hmg_grid *g, hmg_vec *v, const double *xi, const double *form, int nthr, const double *thresholds, double *out)
{
    HMG_TRY
    cell_extrema_call("hmg_cell_extrema", false, g, v, xi, form, nthr, thresholds, out, nullptr);
    HMG_END
}

int hmg_cell_extrema_where(hmg_grid *g, hmg_vec *v, const double *xi, const double *form, int nthr, const double *thresholds,
                           double *out, int32_t *where)
{
    HMG_TRY
    cell_extrema_call("hmg_cell_extrema_where", true, g, v, xi, form, nthr, thresholds, out, where);
    HMG_END
}

int hmg_grid_element_vertices(const hmg_grid *g, int level, int64_t n, const int32_t *codes, int32_t *nodes)
{
    HMG_TRY
    need(g != nullptr, "null grid");
    if (level < 1 || level > g->nlevels)
        throw std::runtime_error("hmg_grid_element_vertices: level " + std::to_string(level) + " out of range 1 to " + std::to_string(g->nlevels));
    need(n >= 0, "hmg_grid_element_vertices: a negative number of codes");
    if (n == 0) return 0;
    need(codes != nullptr && nodes != nullptr, "hmg_grid_element_vertices: null array");
    element_vertices(g->lt.at(level - 1), g->fields.elem.at(level - 1), n, codes, nodes, "hmg_grid_element_vertices");
    HMG_END
}

}  // extern "C"

// hmg_grid_locate, hmg_sample, hmg_sample_raster: a level vector's value, gradient and coarse cell at points of physical space and
// on the pixels of raster slices, without moving the vector off the device.
//
// The inverse direction of everything else in the library: physical point -> coarse cell -> fine element -> dim + 1 storage slots
// with P1 weights.  The evaluation is one __host__ __device__ text (hmg_sample_device.hpp: inside test, Kuhn decomposition, tie and
// zero-weight rules); hmg_grid_locate runs it in a host loop, k_sample (hmg_sample.hip) on the device.  This module builds what
// that text reads and fronts the three entry points.
//
// Locator (build_locator): a uniform bin grid over the bounding box of the current cells, grown by the slack of the inside test.
// A bin's edge is 0.61 of the edge of a cube that dim! cells would fill -- not commensurate with a mesh of split cubes, so that a
// bin does not sit on the cubes' faces and pick up both sides.  A bin lists, ascending, the cells whose bounding box (grown by the
// slack) meets it and which no face plane separates from it: over the bin's box the largest value of every barycentric
// coordinate of the cell must not be below -1e-9, three orders above the slack and the rounding of the test.  The lists are
// conservative (a listed cell may miss the bin), never short: a point's bin comes from the same floating-point expression
// (sample_bin) that placed the cells' boxes, and that expression is monotone.
// Built lazily -- grid creation, its checksum and its allocations are what they were -- and again after hmg_grid_shrink.
//
// Lattice -> slot (ensure_level): 2D levels use rows_slot (hmg_device.hpp), checked here against slot_ijk on every level used; 3D
// levels get a table over the (m + 1)^3 lattice box from slot_ijk, built per level used (level 7: 1.1 MB).  The basis the device
// text hard-codes is compared with ElementTables::dirs first.
//
// Grids on a torus (hmg_grid_set_periodic_sampling; off by default, and then refused as before): the bin grid covers exactly the
// box [0, period) -- fixed by the period alone, not by where the node representatives are stored --, a cell's X0 is its first
// vertex reduced into the box, A comes from the unwrapped edges (cell_edge_vectors, the rule cell_geo reads), and a cell is
// listed in every bin that one of its images X0 + s P, s in {-1, 0, 1} per axis, meets: every edge is below half a period, so
// the cell's box lies inside (-P / 2, 3 P / 2) and these images are all that reach the box.  Slack and face-plane pruning are
// applied to the image as they are to a cell of an ordinary grid.  The inside test takes x - X0 to its minimal image
// (sample_in_cell_torus), so the lists need no image code.
//
// Device memory: the locator's tables are one allocation of setup memory, a 3D level's table one more, both made by the first device
// call that needs them.  Points and results of a call are one block from the context's pool of level-vector memory, its size
// rounded up to 64 KiB so that calls of similar size reuse it.  The calls synchronise.  Not on a V-cycle's path.
#include "../../include/hmg.h"
#include "hmg_objects.hpp"
#include "hmg_sample.hpp"

#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>

namespace hmg {

namespace {

std::atomic<int64_t> locator_counters[3];

constexpr double BIN_EDGE = 0.61;            // of the edge of a cube that dim! cells would fill
constexpr double SLACK_PHYS = 0x1p-36;       // of a cell's largest extent: what a point may lie outside its cell, with room
constexpr double PLANE_MARGIN = 1e-9;        // a cell whose barycentric coordinate stays below -this over a bin is not listed there
constexpr int64_t MAX_BINS = (int64_t)1 << 24;
constexpr int64_t MAX_POINTS = 0x7fffffffll;

SampleLocator host_locator(const SampleState &S)
{
    SampleLocator L{};
    for (int a = 0; a < 3; ++a) {
        L.nb[a] = S.nb[a];
        L.lo[a] = S.lo[a];
        L.hi[a] = S.hi[a];
        L.inv_h[a] = S.inv_h[a];
    }
    L.bin_ptr = S.bin_ptr.data();
    L.bin_cell = S.bin_cell.data();
    L.geo = S.geo.data();
    return L;
}

// A = J^-1 (row-major), J's columns X_k - X_0: formed and inverted in long double and rounded once.  MeshTables::jinv carries the
// rounding of a double inverse, eps times the cell's condition number; on a flat cell of an unstructured mesh that alone is
// above the 16 (dim + 1) eps m / h_min a sampled gradient is held to (tests/_sample_form.py).
bool invert_jacobian(int dim, const long double (&J)[3][3], double *A)
{
    long double C[3][3];                                  // cofactors (a 2D cell: J[2][2] = 1 and the rest of row / column 2 zero)
    for (int r = 0; r < 3; ++r)
        for (int s = 0; s < 3; ++s) {
            const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, s1 = (s + 1) % 3, s2 = (s + 2) % 3;
            C[r][s] = J[r1][s1] * J[r2][s2] - J[r1][s2] * J[r2][s1];
        }
    const long double det = J[0][0] * C[0][0] + J[0][1] * C[0][1] + J[0][2] * C[0][2];
    if (!(det != 0.0L) || !std::isfinite((double)det)) return false;
    for (int b = 0; b < dim; ++b)
        for (int a = 0; a < dim; ++a) A[b * dim + a] = (double)(C[a][b] / det);      // (J^-1)[b][a] = C[a][b] / det
    return true;
}

bool inverse_jacobian(int dim, const double *coords, const int32_t *el, double *A)
{
    long double J[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int col = 0; col < dim; ++col)
        for (int a = 0; a < dim; ++a)
            J[a][col] = (long double)coords[(size_t)el[col + 1] * dim + a] - (long double)coords[(size_t)el[0] * dim + a];
    return invert_jacobian(dim, J, A);
}

// the same from a cell's unwrapped edge vectors (cell_edge_vectors: a grid on a torus)
bool inverse_jacobian(int dim, const double (&d)[4][3], double *A)
{
    long double J[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int col = 0; col < dim; ++col)
        for (int a = 0; a < dim; ++a) J[a][col] = (long double)d[col + 1][a];
    return invert_jacobian(dim, J, A);
}

void build_locator(hmg_grid *g)
{
    SampleState &S = g->sample;
    const MeshTables &M = g->cur();
    const int dim = g->dim, N = dim + 1, ng = dim + dim * dim;
    const int64_t nc = M.ncells;
    const bool torus = M.periodic();
    need(nc >= 1, "sampling: the grid has no cells");
    S.ready = false;
    S.on_device = false;
    S.geo.assign((size_t)nc * ng, 0.0);
    std::vector<double> box((size_t)nc * 6), slack(nc);
    for (int64_t c = 0; c < nc; ++c) {
        const int32_t *el = &M.cells[c * N];
        double *G = &S.geo[(size_t)c * ng];
        if (torus) {
            // X0 reduced into the box, A and the cell's box from the unwrapped edges
            double d[4][3];
            cell_edge_vectors(M, c, d);
            if (!inverse_jacobian(dim, d, G + dim)) throw std::runtime_error("sampling: degenerate cell " + std::to_string(c));
            double *B = &box[(size_t)c * 6];
            double ext = 0.0;
            for (int a = 0; a < dim; ++a) {
                const double P = M.period[a], x = M.coords[(size_t)el[0] * dim + a];
                need(std::isfinite(x), "sampling: a node coordinate of the base mesh is not finite");
                double x0 = x - P * std::floor(x / P);
                if (x0 < 0.0) x0 += P;
                if (x0 >= P) x0 -= P;
                G[a] = x0;
                double mn = 0.0, mx = 0.0;
                for (int q = 1; q < N; ++q) {
                    mn = std::min(mn, d[q][a]);
                    mx = std::max(mx, d[q][a]);
                }
                need(std::isfinite(mn) && std::isfinite(mx), "sampling: a node coordinate of the base mesh is not finite");
                B[a] = x0 + mn;
                B[3 + a] = x0 + mx;
                ext = std::max(ext, mx - mn);
            }
            slack[c] = SLACK_PHYS * ext;
            continue;
        }
        for (int a = 0; a < dim; ++a) G[a] = M.coords[(size_t)el[0] * dim + a];
        if (!inverse_jacobian(dim, M.coords.data(), el, G + dim)) throw std::runtime_error("sampling: degenerate cell " + std::to_string(c));
        double *B = &box[(size_t)c * 6];
        double ext = 0.0;
        for (int a = 0; a < dim; ++a) {
            double mn = HUGE_VAL, mx = -HUGE_VAL;
            for (int q = 0; q < N; ++q) {
                const double x = M.coords[(size_t)el[q] * dim + a];
                mn = std::min(mn, x);
                mx = std::max(mx, x);
            }
            need(std::isfinite(mn) && std::isfinite(mx), "sampling: a node coordinate of the base mesh is not finite");
            B[a] = mn;
            B[3 + a] = mx;
            ext = std::max(ext, mx - mn);
        }
        slack[c] = SLACK_PHYS * ext;
    }
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, gext = 0.0, smax = 0.0, vol = 1.0;
    for (int a = 0; a < dim; ++a) {
        lo[a] = HUGE_VAL;
        hi[a] = -HUGE_VAL;
        for (int64_t c = 0; c < nc; ++c) {
            lo[a] = std::min(lo[a], box[(size_t)c * 6 + a]);
            hi[a] = std::max(hi[a], box[(size_t)c * 6 + 3 + a]);
        }
        if (torus) {                             // the box is the period's, whatever the cells' boxes reach
            lo[a] = 0.0;
            hi[a] = M.period[a];
        }
        gext = std::max(gext, hi[a] - lo[a]);
        vol *= hi[a] - lo[a];
    }
    for (int64_t c = 0; c < nc; ++c) smax = std::max(smax, slack[c]);
    const double grow = smax + 1e-12 * gext;     // (the second term: roundings of a bin's edges, which scale with the whole box)
    double fact = 1.0;
    for (int a = 2; a <= dim; ++a) fact *= a;
    const double h = BIN_EDGE * std::pow(vol * fact / (double)nc, 1.0 / dim);
    int64_t nbins = 1;
    for (int a = 0; a < 3; ++a) {
        S.nb[a] = 1;
        S.lo[a] = S.hi[a] = 0.0;
        S.inv_h[a] = 0.0;
        if (a >= dim) continue;
        S.lo[a] = torus ? lo[a] : lo[a] - grow;      // (a torus: the bins cover exactly the box)
        S.hi[a] = torus ? hi[a] : hi[a] + grow;
        const double n = std::ceil((hi[a] - lo[a]) / h);
        S.nb[a] = (int)std::max(1.0, std::min(4096.0, n));
        nbins *= S.nb[a];
    }
    while (nbins > MAX_BINS) {                   // (a very elongated box: halve the finest axis)
        int a = 0;
        for (int b = 1; b < dim; ++b)
            if (S.nb[b] > S.nb[a]) a = b;
        nbins /= S.nb[a];
        S.nb[a] = (S.nb[a] + 1) / 2;
        nbins *= S.nb[a];
    }
    for (int a = 0; a < dim; ++a) S.inv_h[a] = (double)S.nb[a] / (S.hi[a] - S.lo[a]);
    SampleLocator L = host_locator(S);

    // f(bin) for every bin that cell c, moved by `move`, is listed in (an ordinary grid: move = 0, the cell as it stands)
    auto visit_image = [&](int64_t c, const double *move, auto &&f) {
        const double *G0 = &S.geo[(size_t)c * ng];
        double B[6], G[3] = {0, 0, 0};
        for (int a = 0; a < dim; ++a) {
            B[a] = box[(size_t)c * 6 + a] + move[a];
            B[3 + a] = box[(size_t)c * 6 + 3 + a] + move[a];
            G[a] = G0[a] + move[a];
        }
        const double s = slack[c] + 1e-12 * gext;
        int b0[3] = {0, 0, 0}, b1[3] = {0, 0, 0};
        for (int a = 0; a < dim; ++a) {
            if (B[3 + a] + s < S.lo[a] || B[a] - s > S.hi[a]) return;      // (an image that does not reach the box)
            b0[a] = sample_bin(L, a, std::max(B[a] - s, S.lo[a]));
            b1[a] = sample_bin(L, a, std::min(B[3 + a] + s, S.hi[a]));
        }
        for (int bz = b0[2]; bz <= b1[2]; ++bz)
            for (int by = b0[1]; by <= b1[1]; ++by)
                for (int bx = b0[0]; bx <= b1[0]; ++bx) {
                    const int bb[3] = {bx, by, bz};
                    double ctr[3], half[3];
                    for (int a = 0; a < dim; ++a) {
                        const double e0 = S.lo[a] + (double)bb[a] / S.inv_h[a], e1 = S.lo[a] + (double)(bb[a] + 1) / S.inv_h[a];
                        ctr[a] = 0.5 * (e0 + e1) - G[a];
                        half[a] = 0.5 * (e1 - e0) + s;
                    }
                    bool keep = true;
                    double l0c = 1.0, l0h = 0.0;                 // lambda_0 = 1 - sum of the others
                    for (int b = 0; b < dim && keep; ++b) {
                        double v = 0.0, r = 0.0;
                        for (int a = 0; a < dim; ++a) {
                            v += G0[dim + b * dim + a] * ctr[a];
                            r += std::fabs(G0[dim + b * dim + a]) * half[a];
                        }
                        keep = v + r >= -PLANE_MARGIN;
                        l0c -= v;
                    }
                    if (keep) {
                        for (int a = 0; a < dim; ++a) {
                            double col = 0.0;
                            for (int b = 0; b < dim; ++b) col += G0[dim + b * dim + a];
                            l0h += std::fabs(col) * half[a];
                        }
                        keep = l0c + l0h >= -PLANE_MARGIN;
                    }
                    if (keep) f(((int64_t)bz * S.nb[1] + by) * S.nb[0] + bx);
                }
    };
    // f(bin) for every bin cell c is listed in, each bin once.  On a torus: the bins of its images X0 + s P, s in {-1, 0, 1}
    // per axis, ascending (two images of a cell can meet one bin where an axis has few bins)
    auto visit = [&](int64_t c, auto &&f) {
        const double still[3] = {0.0, 0.0, 0.0};
        if (!torus) {
            visit_image(c, still, f);
            return;
        }
        std::vector<int64_t> bins;
        for (int sz = (dim == 3 ? -1 : 0); sz <= (dim == 3 ? 1 : 0); ++sz)
            for (int sy = -1; sy <= 1; ++sy)
                for (int sx = -1; sx <= 1; ++sx) {
                    const double move[3] = {sx * M.period[0], sy * M.period[1], sz * M.period[2]};
                    visit_image(c, move, [&](int64_t bin) { bins.push_back(bin); });
                }
        std::sort(bins.begin(), bins.end());
        bins.erase(std::unique(bins.begin(), bins.end()), bins.end());
        for (int64_t bin : bins) f(bin);
    };
    std::vector<int64_t> first(nc + 1, 0);
    parallel_for(nc, [&](int64_t c0, int64_t c1) {
        for (int64_t c = c0; c < c1; ++c) {
            int64_t n = 0;
            visit(c, [&](int64_t) { n += 1; });
            first[c + 1] = n;
        }
    });
    for (int64_t c = 0; c < nc; ++c) first[c + 1] += first[c];
    if (first[nc] > (int64_t)std::numeric_limits<int32_t>::max()) throw std::runtime_error("sampling: the locator's lists do not fit 32-bit offsets");
    std::vector<int32_t> pair_bin((size_t)first[nc]);
    parallel_for(nc, [&](int64_t c0, int64_t c1) {
        for (int64_t c = c0; c < c1; ++c) {
            int64_t q = first[c];
            visit(c, [&](int64_t bin) { pair_bin[(size_t)q++] = (int32_t)bin; });
        }
    });
    S.bin_ptr.assign((size_t)nbins + 1, 0);
    for (int32_t b : pair_bin) S.bin_ptr[(size_t)b + 1] += 1;
    int64_t longest = 0;
    for (int64_t b = 0; b < nbins; ++b) {
        longest = std::max<int64_t>(longest, S.bin_ptr[(size_t)b + 1]);
        S.bin_ptr[(size_t)b + 1] += S.bin_ptr[(size_t)b];
    }
    S.bin_cell.assign(pair_bin.size(), 0);
    {
        std::vector<int32_t> fill(S.bin_ptr.begin(), S.bin_ptr.end() - 1);
        for (int64_t c = 0; c < nc; ++c)                         // (cells ascending: so is every list)
            for (int64_t q = first[c]; q < first[c + 1]; ++q) S.bin_cell[(size_t)fill[(size_t)pair_bin[(size_t)q]]++] = (int32_t)c;
    }
    S.ready = true;
    locator_counters[0] += 1;
    locator_counters[1] = (int64_t)(S.geo.size() * sizeof(double) + (S.bin_ptr.size() + S.bin_cell.size()) * sizeof(int32_t));
    locator_counters[2] = longest;
}

void ensure_level(hmg_grid *g, int level)
{
    SampleState &S = g->sample;
    if (S.level_ready.size() != (size_t)g->nlevels) {
        S.level_ready.assign(g->nlevels, 0);
        S.slot_of.assign(g->nlevels, {});
        S.d_slot_of.resize(g->nlevels);
    }
    if (S.level_ready[level - 1]) return;
    const int dim = g->dim;
    const LevelTables &T = g->lt[level - 1];
    static const int32_t B3[9] = {0, 0, 1, 0, 1, -1, 1, -1, 0}, B2[4] = {0, 1, 1, -1};
    const std::vector<int32_t> &dirs = g->fields.elem.at(level - 1).dirs;
    need(dirs.size() == (size_t)dim * dim && std::equal(dirs.begin(), dirs.end(), dim == 3 ? B3 : B2),
         "sampling: the lattice basis of the fine elements is not the one the evaluation was written for");
    const int m = T.m, m1 = m + 1;
    if (dim == 2) {
        for (int q = 0; q < T.nf; ++q) {
            int cls;
            need(rows_slot(m, T.slot_ijk[3 * q], T.slot_ijk[3 * q + 1], T.nei, T.off_int, cls) == q,
                 "sampling: the storage order of this 2D level is not the one rows_slot derives");
        }
    } else {
        std::vector<int32_t> &tab = S.slot_of[level - 1];
        tab.assign((size_t)m1 * m1 * m1, -1);
        for (int q = 0; q < T.nf; ++q) tab[((size_t)T.slot_ijk[3 * q + 2] * m1 + T.slot_ijk[3 * q + 1]) * m1 + T.slot_ijk[3 * q]] = q;
        for (int k = 0; k <= m; ++k)
            for (int j = 0; j + k <= m; ++j)
                for (int i = 0; i + j + k <= m; ++i)
                    need(tab[((size_t)k * m1 + j) * m1 + i] >= 0, "sampling: a lattice node of the cell has no storage slot");
    }
    S.level_ready[level - 1] = 1;
}

SampleLevel host_level(const hmg_grid *g, int level)
{
    const LevelTables &T = g->lt[level - 1];
    SampleLevel lv{};
    lv.m = T.m;
    lv.nf = T.nf;
    lv.ld = T.ld;
    lv.nei = T.nei;
    lv.off_int = T.off_int;
    lv.slot_of = g->dim == 3 ? g->sample.slot_of[level - 1].data() : nullptr;
    return lv;
}

// what all three entry points refuse, and the host tables they need
void prepare(hmg_grid *g, int level, const char *call)
{
    need(g != nullptr, "null grid");
    if (g->part) throw std::runtime_error(std::string(call) + ": partitioned grids are not served (sample on an unpartitioned grid)");
    // (on a torus the nodes of a cell may sit on opposite sides of the box: served once hmg_grid_set_periodic_sampling says so)
    if (g->cur().periodic() && !g->sample.torus) throw std::runtime_error(std::string(call) + ": periodic grids are not served (point location on a torus is not built)");
    if (level < 1 || level > g->nlevels)
        throw std::runtime_error(std::string(call) + ": level " + std::to_string(level) + " out of range (1 to " + std::to_string(g->nlevels) + ")");
}

void ensure_host_tables(hmg_grid *g, int level)
{
    ensure_level(g, level);
    if (!g->sample.ready) build_locator(g);
}

template <int DIM>
void locate_points(const SampleLocator &L, const double *period, const SampleLevel &lv, const LevelTables &T, int64_t n,
                   const double *points, int32_t *cell, int32_t *nodes, double *weights, double *gweights)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    parallel_for(n, [&](int64_t p0, int64_t p1) {
        for (int64_t p = p0; p < p1; ++p) {
            const double *x = points + p * DIM;
            double xh[DIM], xr[DIM];
            const int c = !period                       ? sample_find_cell<DIM>(L, x, xh)
                          : sample_wrap<DIM>(period, x, xr) ? sample_find_cell_torus<DIM>(L, period, xr, xh)
                                                            : -1;
            if (cell) cell[p] = c;
            if (c < 0) {
                for (int q = 0; q <= DIM; ++q) {
                    if (nodes) nodes[p * (DIM + 1) + q] = -1;
                    if (weights) weights[p * (DIM + 1) + q] = nan;
                    if (gweights)
                        for (int a = 0; a < DIM; ++a) gweights[(p * (DIM + 1) + q) * DIM + a] = nan;
                }
                continue;
            }
            SampleElement<DIM> E;
            sample_element<DIM>(lv, xh, E);
            for (int q = 0; q <= DIM; ++q) {
                // (a vertex without a weight is reported as the element's first vertex)
                if (nodes) nodes[p * (DIM + 1) + q] = T.slot2hier[E.slot[E.w[q] != 0.0 ? q : 0]];
                if (weights) weights[p * (DIM + 1) + q] = E.w[q];
                if (gweights) {
                    double unit[DIM + 1] = {0.0};
                    unit[q] = 1.0;
                    sample_gradient<DIM>(lv, E, L.geo + (size_t)c * (DIM + DIM * DIM), unit, nullptr, &gweights[(p * (DIM + 1) + q) * DIM]);
                }
            }
        }
    });
}

// device_column must be device memory of this context's device with ld * ncells doubles inside one allocation
void check_column(hmg_grid *g, int level, const void *p, const char *call)
{
    const std::string who(call);
    if (!p) throw std::runtime_error(who + ": null device column");
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof at);
    hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        throw std::runtime_error(who + ": the column is not device memory (" + hipGetErrorString(e) + ")");
    }
    if (at.type != hipMemoryTypeDevice) throw std::runtime_error(who + ": the column is not device memory");
    if (at.device != g->ctx->device) throw std::runtime_error(who + ": the column lives on another device than the grid's context");
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    e = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        throw std::runtime_error(who + ": no allocation is known around the column (" + hipGetErrorString(e) + ")");
    }
    const size_t want = sizeof(double) * (size_t)g->lt[level - 1].ld * (size_t)g->md.ncells;
    const char *b = (const char *)base, *q = (const char *)p;
    if (q < b || (size_t)(q - b) > size || size - (size_t)(q - b) < want)
        throw std::runtime_error(who + ": a vector of level " + std::to_string(level) + " needs " + std::to_string(want) +
                                 " bytes from the column's address, its allocation has " + std::to_string(q < b ? 0 : size - (size_t)(q - b)) +
                                 " (wrong level, or a pointer into the middle of a vector)");
}

// locator and level tables on the device
void ensure_device_tables(hmg_grid *g, int level)
{
    SampleState &S = g->sample;
    hipStream_t s = g->ctx->stream;
    if (!S.on_device) {
        const size_t nint = S.bin_ptr.size() + S.bin_cell.size();
        std::vector<double> blob(S.geo.size() + (nint + 1) / 2, 0.0);
        std::memcpy(blob.data(), S.geo.data(), S.geo.size() * sizeof(double));
        int32_t *ip = (int32_t *)(blob.data() + S.geo.size());
        std::memcpy(ip, S.bin_ptr.data(), S.bin_ptr.size() * sizeof(int32_t));
        std::memcpy(ip + S.bin_ptr.size(), S.bin_cell.data(), S.bin_cell.size() * sizeof(int32_t));
        S.d_tables.upload(blob, s);
        S.on_device = true;
    }
    if (g->dim == 3 && !S.d_slot_of[level - 1]) {
        std::unique_ptr<DevBuf<int32_t>> b(new DevBuf<int32_t>);
        b->upload(S.slot_of[level - 1], s);
        S.d_slot_of[level - 1] = std::move(b);
    }
}

size_t round_up(size_t n, size_t to) { return (n + to - 1) / to * to; }

// the common part of hmg_sample and hmg_sample_raster: points != null -- a list; else the raster of origin, du, dv
void sample(hmg_grid *g, int level, const void *column, const double *xi, int64_t n, const double *points, const double *origin,
            const double *du, const double *dv, int64_t nu, int64_t nv, double *values, double *gradients, int32_t *cell, const char *call)
{
    const int dim = g->dim;
    hmg_ctx *c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    check_column(g, level, column, call);
    ensure_host_tables(g, level);
    ensure_device_tables(g, level);
    SampleState &S = g->sample;

    // one pool block: points | values | gradients | cell
    const size_t b_pts = points ? round_up(sizeof(double) * (size_t)n * dim, 256) : 0;
    const size_t b_val = values ? round_up(sizeof(double) * (size_t)n, 256) : 0;
    const size_t b_grd = gradients ? round_up(sizeof(double) * (size_t)n * dim, 256) : 0;
    const size_t b_cel = cell ? round_up(sizeof(int32_t) * (size_t)n, 256) : 0;
    const size_t bytes = round_up(b_pts + b_val + b_grd + b_cel, (size_t)64 << 10);
    char *blk = (char *)vec_alloc(c, bytes);

    SampleArgs a{};
    a.loc = host_locator(S);
    a.loc.geo = S.d_tables.p;
    a.loc.bin_ptr = (const int32_t *)(S.d_tables.p + S.geo.size());
    a.loc.bin_cell = a.loc.bin_ptr + S.bin_ptr.size();
    a.lev = host_level(g, level);
    a.lev.slot_of = dim == 3 ? S.d_slot_of[level - 1]->p : nullptr;
    a.column = (const double *)column;
    a.has_xi = xi != nullptr;
    for (int k = 0; k < dim; ++k) {
        a.xi[k] = xi ? xi[k] : 0.0;
        a.origin[k] = origin ? origin[k] : 0.0;
        a.du[k] = du ? du[k] : 0.0;
        a.dv[k] = dv ? dv[k] : 0.0;
    }
    a.npoints = n;
    a.nu = nu;
    a.nv = nv;
    a.points = points ? (const double *)blk : nullptr;
    a.values = values ? (double *)(blk + b_pts) : nullptr;
    a.gradients = gradients ? (double *)(blk + b_pts + b_val) : nullptr;
    a.cell = cell ? (int32_t *)(blk + b_pts + b_val + b_grd) : nullptr;

    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    try {
        HIPCHK(hipEventCreate(&ev0));
        HIPCHK(hipEventCreate(&ev1));
        if (points) HIPCHK(hipMemcpyAsync(blk, points, sizeof(double) * (size_t)n * dim, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipEventRecord(ev0, c->stream));
        launch_sample(c->stream, dim, points == nullptr, a, g->cur().periodic() ? g->cur().period : nullptr);
        c->sample_launches += 1;
        HIPCHK(hipEventRecord(ev1, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        const auto t0 = std::chrono::steady_clock::now();
        if (values) HIPCHK(hipMemcpyAsync(values, a.values, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        if (gradients) HIPCHK(hipMemcpyAsync(gradients, a.gradients, sizeof(double) * (size_t)n * dim, hipMemcpyDeviceToHost, c->stream));
        if (cell) HIPCHK(hipMemcpyAsync(cell, a.cell, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->sample_download_ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
        c->sample_kernel_ns = (int64_t)((double)ms * 1e6);
    } catch (...) {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        (void)hipStreamSynchronize(c->stream);       // (the caller's arrays are in flight)
        vec_release(c, blk, bytes);
        throw;
    }
    (void)hipEventDestroy(ev0);
    (void)hipEventDestroy(ev1);
    vec_release(c, blk, bytes);
}

}  // namespace

int64_t sample_locator_counter(int which) { return which >= 0 && which < 3 ? locator_counters[which].load() : -1; }

}  // namespace hmg

extern "C" {

int hmg_grid_locate(hmg_grid *g, int level, int64_t npoints, const double *points, int32_t *cell, int32_t *nodes, double *weights,
                    double *gweights)
{
    HMG_TRY
    prepare(g, level, "hmg_grid_locate");
    need(npoints >= 0 && npoints <= MAX_POINTS, "hmg_grid_locate: the number of points must be 0 to 2^31 - 1");
    need(cell || nodes || weights || gweights, "hmg_grid_locate: every output array is null");
    if (npoints == 0) return 0;
    need(points != nullptr, "hmg_grid_locate: null points");
    ensure_host_tables(g, level);
    const SampleLocator L = host_locator(g->sample);
    const SampleLevel lv = host_level(g, level);
    const LevelTables &T = g->lt[level - 1];
    const double *period = g->cur().periodic() ? g->cur().period : nullptr;
    if (g->dim == 3)
        locate_points<3>(L, period, lv, T, npoints, points, cell, nodes, weights, gweights);
    else
        locate_points<2>(L, period, lv, T, npoints, points, cell, nodes, weights, gweights);
    HMG_END
}

int hmg_grid_set_periodic_sampling(hmg_grid *g, int on)
{
    HMG_TRY
    need(g != nullptr, "null grid");
    need(g->cur().periodic(), "hmg_grid_set_periodic_sampling: the grid is not periodic (an ordinary grid is sampled as it is)");
    need(on == 0 || on == 1, "hmg_grid_set_periodic_sampling: on must be 0 or 1");
    SampleState &S = g->sample;
    S.torus = on == 1;
    S.ready = S.on_device = false;               // (the locator goes; the next call that is served builds it)
    HMG_END
}

int hmg_grid_periodic_sampling(hmg_grid *g, int *on)
{
    HMG_TRY
    need(g != nullptr, "null grid");
    need(on != nullptr, "hmg_grid_periodic_sampling: null result");
    *on = g->sample.torus ? 1 : 0;
    HMG_END
}

int hmg_sample(hmg_grid *g, int level, const void *device_column, const double *xi, int64_t npoints, const double *points,
               double *values, double *gradients, int32_t *cell)
{
    HMG_TRY
    prepare(g, level, "hmg_sample");
    need(g->ctx != nullptr, "hmg_sample: this grid was created without a device context (host tables only): hmg_grid_locate is the host's part");
    need(npoints >= 0 && npoints <= MAX_POINTS, "hmg_sample: the number of points must be 0 to 2^31 - 1");
    need(values || gradients || cell, "hmg_sample: every output array is null");
    if (npoints == 0) return 0;
    need(points != nullptr, "hmg_sample: null points");
    sample(g, level, device_column, xi, npoints, points, nullptr, nullptr, nullptr, 0, 0, values, gradients, cell, "hmg_sample");
    HMG_END
}

int hmg_sample_raster(hmg_grid *g, int level, const void *device_column, const double *xi, const double *origin, const double *du,
                      const double *dv, int64_t nu, int64_t nv, double *values, double *gradients, int32_t *cell)
{
    HMG_TRY
    prepare(g, level, "hmg_sample_raster");
    need(g->ctx != nullptr, "hmg_sample_raster: this grid was created without a device context (host tables only): hmg_grid_locate is the host's part");
    need(nu >= 0 && nv >= 0 && (nv == 0 || nu <= MAX_POINTS / nv), "hmg_sample_raster: nu * nv must be 0 to 2^31 - 1");
    need(values || gradients || cell, "hmg_sample_raster: every output array is null");
    if (nu * nv == 0) return 0;
    need(origin && du && dv, "hmg_sample_raster: null origin, du or dv");
    sample(g, level, device_column, xi, nu * nv, nullptr, origin, du, dv, nu, nv, values, gradients, cell, "hmg_sample_raster");
    HMG_END
}

}  // extern "C"

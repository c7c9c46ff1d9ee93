// hmg_cell_histogram: per coarse cell the histogram, over the cell's fine elements, of the quadratic form of hmg_cell_extrema --
// and the binning rule's host side: hmg_histogram_nbins, hmg_histogram_edges, hmg_histogram_bin.
//
// The rule is one text for host and kernel (hmg_histogram_device.hpp): floating-point buckets, found by integer arithmetic on the
// value's high word.  The pass is hmg_cell_extrema's (hmg_extrema.cpp): the same element mask, the same row (Q~, xi~) per cell from
// the same function, the same values from the kernel (hmg_histogram.hip); what comes back is nbins 32-bit counts per cell, widened
// here.  Cells larger than the LDS (3D level 7, 2D levels 9..11) are refused unless the context option "cell_histogram_windows" sends
// them through the window kernels (hmg_histogram_window.hip).  hmg_cell_histogram_groups runs the same pass, leaves the rows on the
// device and sums them per group of cells there (k_histogram_groups): ngroups * nbins numbers come down instead of ncells * nbins.
// Not on a V-cycle's path: the call allocates (rows and counts, from the context's pool of level-vector memory; the element mask
// of a level once, at its first call) and synchronises.
#include "../../include/hmg.h"
#include "hmg_extrema.hpp"
#include "hmg_fields.hpp"
#include "hmg_histogram.hpp"
#include "hmg_objects.hpp"

#include <cmath>
#include <cstring>

namespace {

// throws, naming the call and the parameter, where (emin, emax, sub_bits) are outside the rule -- and, for the call that keeps the
// histogram in LDS (device), where they ask for more regular bins than it serves
void check_rule(const char *who, int emin, int emax, int sub_bits, bool device = false)
{
    const std::string w = std::string(who) + ": ";
    const int bad = histogram_rule_check(emin, emax, sub_bits);
    if (bad == 0) {
        const int64_t nreg = (int64_t)(emax - emin) << sub_bits;
        if (device && nreg > HIST_MAX_REGULAR)
            throw std::runtime_error(w + std::to_string(nreg) + " regular bins ((emax - emin) 2^sub_bits = " + std::to_string(emax - emin) +
                                     " * " + std::to_string(1 << sub_bits) + "); at most " + std::to_string(HIST_MAX_REGULAR) +
                                     " fit the LDS next to a cell");
        return;
    }
    if (bad == 4) throw std::runtime_error(w + "sub_bits = " + std::to_string(sub_bits) + "; 0 to 5 are served");
    if (bad == 1) throw std::runtime_error(w + "emin = " + std::to_string(emin) + " is outside -1022 to 1023");
    if (bad == 2) throw std::runtime_error(w + "emax = " + std::to_string(emax) + " is outside -1022 to 1023");
    throw std::runtime_error(w + "emin = " + std::to_string(emin) + " is not below emax = " + std::to_string(emax));
}

// The pass of hmg_cell_histogram and hmg_cell_histogram_groups: one text of the checks, the rows, the kernel choice and the launch;
// `who` names the call in every message.  The per-cell rows (int32, nbins per cell) stay in the context's pool: `then(ctx, d_out,
// ncells, nbins)` runs behind the launch, on the context's stream, and is done with them when it returns (it synchronises).
// false: the grid has no cells and nothing ran.
template <class Then>
bool cell_histogram_pass(const std::string &who, hmg_grid *g, hmg_vec *v, const double *xi, const double *form, int emin, int emax,
                         int sub_bits, Then &&then)
{
    auto need = [&](bool c, const char *msg) {
        if (!c) throw std::runtime_error(who + ": " + msg);
    };
    need(g->ctx != nullptr, "this grid was created without a device context (host tables only): no compute path exists on the CPU");
    need(v != nullptr, "null vector");
    need(v->g == g, "vector belongs to another grid");
    check_rule(who.c_str(), emin, emax, sub_bits, /*device=*/true);
    const HistogramRule rule = histogram_rule(emin, emax, sub_bits);
    const int nbins = rule.nreg + 3;
    check_vec(g, v->level, v, "v");
    const LevelDev &lv = lev(g, v->level);
    const int dim = g->dim, nq = sym_ncomp(dim);
    // the kernel: k_cell_histogram where the cell fits the LDS together with its histogram, the window kernels by the option
    // "cell_histogram_windows" (1: levels that do not fit; 2: every level they address) -- the selection of hmg_cell_extrema
    const SlabTables st = slab_tables(g, lv);
    const bool fits = cell_histogram_ok(lv) && cell_extrema_ok(lv) && cell_moments_ok(lv, true), can = cell_histogram_window_ok(lv, st);
    const int mode = g->ctx->histogram_windows;
    const bool window = mode != 0 && can && (mode == 2 || !fits);
    if (!window && !fits)
        throw std::runtime_error(who + ": one cell of level " + std::to_string(lv.level) + " (" + std::to_string(lv.nf) +
                                 " nodes) does not fit the LDS together with its histogram; the per-cell histograms serve " +
                                 (dim == 3 ? "3D levels up to 6" : "2D levels up to 8") +
                                 (can ? "; the context option \"cell_histogram_windows\" = 1 takes larger cells through the window kernels"
                                      : "; no window kernel addresses this level"));
    const int64_t nc = g->md.ncells;
    if (form)
        for (int64_t q = 0; q < nc * nq; ++q)
            if (!std::isfinite(form[q]))
                throw std::runtime_error(who + ": the form of cell " + std::to_string(q / nq) + " is not finite");
    if (xi)
        for (int a = 0; a < dim; ++a) need(std::isfinite(xi[a]), "xi is not finite");
    if (nc == 0) return false;
    const std::vector<double> rows = cell_form_rows(who, g, v->level, xi, form);

    hmg_ctx *c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    const uint8_t *d_mask = device_element_mask(g, v->level);
    const size_t nout = (size_t)nbins * (size_t)nc;
    const size_t row_bytes = sizeof(double) * rows.size(), out_bytes = sizeof(int32_t) * nout;
    double *d_rows = vec_alloc(c, row_bytes);
    int32_t *d_out = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    try {
        d_out = (int32_t *)vec_alloc(c, out_bytes);
        HIPCHK(hipEventCreate(&ev0));
        HIPCHK(hipEventCreate(&ev1));
        HIPCHK(hipMemcpyAsync(d_rows, rows.data(), row_bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipEventRecord(ev0, c->stream));
        if (window) {
            launch_cell_histogram_window(c->L, lv, st, nc, v->d, d_mask, d_rows, rule, d_out);
            c->histogram_window_launches += 1;
        } else
            launch_cell_histogram(c->L, lv, nc, v->d, d_mask, d_rows, rule, c->histogram_variant, d_out);
        c->histogram_launches += 1;
        HIPCHK(hipEventRecord(ev1, c->stream));
        then(c, (const int32_t *)d_out, nc, nbins);
        HIPCHK(hipStreamSynchronize(c->stream));
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
        c->histogram_kernel_ns = (int64_t)((double)ms * 1e6);
    } catch (...) {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        (void)hipStreamSynchronize(c->stream);       // (the rows' host copy goes out of scope)
        vec_release(c, d_rows, row_bytes);
        if (d_out) vec_release(c, d_out, out_bytes);
        throw;
    }
    (void)hipEventDestroy(ev0);
    (void)hipEventDestroy(ev1);
    vec_release(c, d_rows, row_bytes);
    vec_release(c, d_out, out_bytes);
    return true;
}

}  // namespace

extern "C" {

int64_t hmg_histogram_nbins(int emin, int emax, int sub_bits)
{
    try {
        check_rule("hmg_histogram_nbins", emin, emax, sub_bits);
    } catch (const std::exception &e) {
        (void)fail(e);
        return -1;
    }
    return (int64_t)histogram_rule(emin, emax, sub_bits).nreg + 3;
}

int hmg_histogram_edges(int emin, int emax, int sub_bits, double *edges)
{
    HMG_TRY
    check_rule("hmg_histogram_edges", emin, emax, sub_bits);
    need(edges != nullptr, "hmg_histogram_edges: null edges array");
    const int nreg = histogram_rule(emin, emax, sub_bits).nreg;
    for (int i = 0; i <= nreg; ++i) {
        const uint64_t bits = histogram_edge_bits(i, emin, sub_bits);
        std::memcpy(&edges[i], &bits, sizeof(double));
    }
    HMG_END
}

int hmg_histogram_bin(int64_t n, const double *q, int emin, int emax, int sub_bits, int32_t *bins)
{
    HMG_TRY
    check_rule("hmg_histogram_bin", emin, emax, sub_bits);
    need(n >= 0, "hmg_histogram_bin: a negative number of values");
    if (n == 0) return 0;
    need(q != nullptr && bins != nullptr, "hmg_histogram_bin: null array");
    const HistogramRule rule = histogram_rule(emin, emax, sub_bits);
    for (int64_t i = 0; i < n; ++i) {
        uint64_t bits;
        std::memcpy(&bits, &q[i], sizeof(double));
        bins[i] = histogram_bin((uint32_t)(bits >> 32), (uint32_t)bits, rule);
    }
    HMG_END
}

int hmg_cell_histogram(hmg_grid *g, hmg_vec *v, const double *xi, const double *form, int emin, int emax, int sub_bits, int64_t *counts)
{
    HMG_TRY
    const std::string who = "hmg_cell_histogram";
    hmg::need(g != nullptr, "null grid");
    if (!counts) throw std::runtime_error(who + ": null counts array");
    std::vector<int32_t> got;
    const bool ran = cell_histogram_pass(who, g, v, xi, form, emin, emax, sub_bits, [&](hmg_ctx *c, const int32_t *d_out, int64_t nc, int nbins) {
        got.resize((size_t)nbins * (size_t)nc);
        HIPCHK(hipMemcpyAsync(got.data(), d_out, sizeof(int32_t) * got.size(), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    });
    if (ran)
        for (size_t q = 0; q < got.size(); ++q) counts[q] = got[q];
    HMG_END
}

int hmg_cell_histogram_groups(hmg_grid *g, hmg_vec *v, const double *xi, const double *form, int emin, int emax, int sub_bits,
                              int ngroups, const int32_t *group_of_cell, const double *weights, int64_t *counts, double *volume)
{
    HMG_TRY
    const std::string who = "hmg_cell_histogram_groups";
    auto need = [&](bool c, const std::string &msg) {
        if (!c) throw std::runtime_error(who + ": " + msg);
    };
    hmg::need(g != nullptr, "null grid");
    // the groups' own arguments, before anything touches the device
    need(ngroups >= 1, "ngroups = " + std::to_string(ngroups) + "; at least one group");
    need(ngroups <= HIST_MAX_GROUPS, "ngroups = " + std::to_string(ngroups) + "; at most " + std::to_string(HIST_MAX_GROUPS) + " are served");
    need(counts != nullptr, "null counts array");
    need((weights == nullptr) == (volume == nullptr),
         weights ? "weights are given and volume is null (both or neither)" : "volume is given and weights are null (both or neither)");
    const int64_t nc = g->md.ncells;
    need(nc == 0 || group_of_cell != nullptr, "null group_of_cell array");
    for (int64_t e = 0; e < nc; ++e) {
        if (group_of_cell[e] < -1 || group_of_cell[e] >= ngroups)
            throw std::runtime_error(who + ": group_of_cell[" + std::to_string(e) + "] = " + std::to_string(group_of_cell[e]) +
                                     " is outside -1 to " + std::to_string(ngroups - 1));
        if (weights && !std::isfinite(weights[e])) throw std::runtime_error(who + ": the weight of cell " + std::to_string(e) + " is not finite");
    }
    // the cells of each group, ascending: the order of the FP64 sums
    std::vector<int32_t> ptr((size_t)ngroups + 1, 0), cells;
    for (int64_t e = 0; e < nc; ++e)
        if (group_of_cell[e] >= 0) ptr[(size_t)group_of_cell[e] + 1] += 1;
    for (int k = 0; k < ngroups; ++k) ptr[k + 1] += ptr[k];
    cells.resize((size_t)ptr[ngroups] + 1, 0);                       // (+ 1: never an empty upload)
    {
        std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
        for (int64_t e = 0; e < nc; ++e)
            if (group_of_cell[e] >= 0) cells[(size_t)fill[group_of_cell[e]]++] = (int32_t)e;
    }
    const bool ran = cell_histogram_pass(who, g, v, xi, form, emin, emax, sub_bits, [&](hmg_ctx *c, const int32_t *d_out, int64_t ncells, int nbins) {
        const size_t nsum = (size_t)ngroups * (size_t)nbins;
        const size_t ptr_bytes = sizeof(int32_t) * ptr.size(), cell_bytes = sizeof(int32_t) * cells.size();
        const size_t w_bytes = weights ? sizeof(double) * (size_t)ncells : 0, sum_bytes = sizeof(int64_t) * nsum;
        double *d_ptr = nullptr, *d_cells = nullptr, *d_w = nullptr, *d_cnt = nullptr, *d_vol = nullptr;
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        auto release = [&]() {
            if (ev0) (void)hipEventDestroy(ev0);
            if (ev1) (void)hipEventDestroy(ev1);
            if (d_ptr) vec_release(c, d_ptr, ptr_bytes);
            if (d_cells) vec_release(c, d_cells, cell_bytes);
            if (d_w) vec_release(c, d_w, w_bytes);
            if (d_cnt) vec_release(c, d_cnt, sum_bytes);
            if (d_vol) vec_release(c, d_vol, sum_bytes);
        };
        try {
            d_ptr = vec_alloc(c, ptr_bytes);
            d_cells = vec_alloc(c, cell_bytes);
            if (weights) d_w = vec_alloc(c, w_bytes);
            d_cnt = vec_alloc(c, sum_bytes);
            if (weights) d_vol = vec_alloc(c, sum_bytes);
            HIPCHK(hipEventCreate(&ev0));
            HIPCHK(hipEventCreate(&ev1));
            HIPCHK(hipMemcpyAsync(d_ptr, ptr.data(), ptr_bytes, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(d_cells, cells.data(), cell_bytes, hipMemcpyHostToDevice, c->stream));
            if (weights) HIPCHK(hipMemcpyAsync(d_w, weights, w_bytes, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipEventRecord(ev0, c->stream));
            launch_histogram_groups(c->L, nbins, ngroups, d_out, (const int *)d_ptr, (const int *)d_cells, d_w, (long long *)d_cnt, d_vol);
            HIPCHK(hipEventRecord(ev1, c->stream));
            HIPCHK(hipMemcpyAsync(counts, d_cnt, sum_bytes, hipMemcpyDeviceToHost, c->stream));
            if (weights) HIPCHK(hipMemcpyAsync(volume, d_vol, sum_bytes, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            float ms = 0.0f;
            HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
            c->histogram_groups_kernel_ns = (int64_t)((double)ms * 1e6);
        } catch (...) {
            (void)hipStreamSynchronize(c->stream);   // (the host copies of the lists go out of scope)
            release();
            throw;
        }
        release();
    });
    if (!ran) {                                       // a grid without cells: every group is empty
        const int64_t nb = hmg_histogram_nbins(emin, emax, sub_bits);
        for (int64_t q = 0; q < (int64_t)ngroups * nb; ++q) {
            counts[q] = 0;
            if (volume) volume[q] = 0.0;
        }
    }
    HMG_END
}

}  // extern "C"

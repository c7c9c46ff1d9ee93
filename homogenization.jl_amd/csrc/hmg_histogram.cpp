// hmg_cell_histogram: per coarse cell the histogram, over the cell's fine elements, of the quadratic form of hmg_cell_extrema --
// and the binning rule's host side: hmg_histogram_nbins, hmg_histogram_edges, hmg_histogram_bin.
//
// The rule is one text for host and kernel (hmg_histogram_device.hpp): floating-point buckets, found by integer arithmetic on the
// value's high word.  The pass is hmg_cell_extrema's (hmg_extrema.cpp): the same element mask, the same row (Q~, xi~) per cell from
// the same function, the same values from the kernel (hmg_histogram.hip); what comes back is nbins 32-bit counts per cell, widened
// here.  Cells larger than the LDS (3D level 7, 2D levels 9..11) are refused: there is no window form of this kernel.
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
    auto need = [&](bool c, const char *msg) {
        if (!c) throw std::runtime_error(who + ": " + msg);
    };
    hmg::need(g != nullptr, "null grid");
    need(counts != nullptr, "null counts array");
    need(g->ctx != nullptr, "this grid was created without a device context (host tables only): no compute path exists on the CPU");
    need(v != nullptr, "null vector");
    need(v->g == g, "vector belongs to another grid");
    check_rule(who.c_str(), emin, emax, sub_bits, /*device=*/true);
    const HistogramRule rule = histogram_rule(emin, emax, sub_bits);
    const int nbins = rule.nreg + 3;
    check_vec(g, v->level, v, "v");
    const LevelDev &lv = lev(g, v->level);
    const int dim = g->dim, nq = sym_ncomp(dim);
    if (!(cell_histogram_ok(lv) && cell_extrema_ok(lv) && cell_moments_ok(lv, true)))
        throw std::runtime_error(who + ": one cell of level " + std::to_string(lv.level) + " (" + std::to_string(lv.nf) +
                                 " nodes) does not fit the LDS together with its histogram; the per-cell histograms serve " +
                                 (dim == 3 ? "3D levels up to 6" : "2D levels up to 8") + " and have no window kernels");
    const int64_t nc = g->md.ncells;
    if (form)
        for (int64_t q = 0; q < nc * nq; ++q)
            if (!std::isfinite(form[q]))
                throw std::runtime_error(who + ": the form of cell " + std::to_string(q / nq) + " is not finite");
    if (xi)
        for (int a = 0; a < dim; ++a) need(std::isfinite(xi[a]), "xi is not finite");
    if (nc == 0) return 0;
    const std::vector<double> rows = cell_form_rows(who, g, v->level, xi, form);

    hmg_ctx *c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    const uint8_t *d_mask = device_element_mask(g, v->level);
    const size_t nout = (size_t)nbins * (size_t)nc;
    const size_t row_bytes = sizeof(double) * rows.size(), out_bytes = sizeof(int32_t) * nout;
    std::vector<int32_t> got(nout);
    double *d_rows = vec_alloc(c, row_bytes);
    int32_t *d_out = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    try {
        d_out = (int32_t *)vec_alloc(c, out_bytes);
        HIPCHK(hipEventCreate(&ev0));
        HIPCHK(hipEventCreate(&ev1));
        HIPCHK(hipMemcpyAsync(d_rows, rows.data(), row_bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipEventRecord(ev0, c->stream));
        launch_cell_histogram(c->L, lv, nc, v->d, d_mask, d_rows, rule, c->histogram_variant, d_out);
        c->histogram_launches += 1;
        HIPCHK(hipEventRecord(ev1, c->stream));
        HIPCHK(hipMemcpyAsync(got.data(), d_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
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
    for (size_t q = 0; q < nout; ++q) counts[q] = got[q];
    HMG_END
}

}  // extern "C"

/*
 * host_locate.c -- the host side of point sampling (hmg_grid_locate: locator build, lattice tables, the shared evaluation text) on
 * a grid without a context, for the AddressSanitizer / UBSan / ThreadSanitizer builds of the library
 * (`make -C homogenization.jl_amd/csrc asan tsan`; tests/test_sample_sanitizers.py).  No GPU is touched.
 *
 * Points: a lattice over a box larger than the domain (so: inside, on faces, edges and nodes of coarse and fine cells, outside),
 * then NaN and inf; again after a shrink.  Prints a checksum of everything hmg_grid_locate returned: the same for every thread
 * count and every fill byte of fresh heap memory.
 *
 *   host_locate [width = 4] [levels = 4] [points per axis = 37]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hmg.h"

#define CHECK(call)                                                            \
    do {                                                                       \
        if ((call) != 0) {                                                     \
            fprintf(stderr, "%s failed: %s\n", #call, hmg_last_error());       \
            return 1;                                                          \
        }                                                                      \
    } while (0)

static unsigned long long fold(unsigned long long h, const void *p, size_t n)
{
    const unsigned char *b = p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

int main(int argc, char **argv)
{
    const int w = argc > 1 ? atoi(argv[1]) : 4, levels = argc > 2 ? atoi(argv[2]) : 4, per = argc > 3 ? atoi(argv[3]) : 37;
    const int64_t shape[3] = {w, w, w};
    const double origin[3] = {-0.5 * w, -0.5 * w, -0.5 * w};
    int64_t nnodes = 0, ncells = 0;
    CHECK(hmg_checkerboard_mesh_size(3, shape, &nnodes, &ncells));
    double *coords = malloc(sizeof(double) * 3 * (size_t)nnodes);
    int64_t *cells = malloc(sizeof(int64_t) * 4 * (size_t)ncells);
    CHECK(hmg_checkerboard_mesh(3, shape, origin, 1, 1, coords, cells));
    hmg_grid *g = NULL;
    CHECK(hmg_grid_create(NULL, 3, levels, nnodes, coords, ncells, cells, &g));

    const int64_t n = (int64_t)per * per * per + 3;
    double *x = malloc(sizeof(double) * 3 * (size_t)n);
    const double lo = -0.5 * w - 0.25, step = (w + 0.5) / (per - 1);
    int64_t q = 0;
    for (int i = 0; i < per; ++i)
        for (int j = 0; j < per; ++j)
            for (int k = 0; k < per; ++k, ++q) {
                x[3 * q] = lo + i * step;
                x[3 * q + 1] = lo + j * step;
                x[3 * q + 2] = lo + k * step;
            }
    for (int e = 0; e < 3; ++e, ++q) {
        x[3 * q] = x[3 * q + 1] = x[3 * q + 2] = 0.0;
        x[3 * q + e] = e == 0 ? NAN : e == 1 ? INFINITY : -INFINITY;
    }
    int32_t *cell = malloc(sizeof(int32_t) * (size_t)n), *nodes = malloc(sizeof(int32_t) * 4 * (size_t)n);
    double *wts = malloc(sizeof(double) * 4 * (size_t)n), *gw = malloc(sizeof(double) * 12 * (size_t)n);
    printf("host_locate: %d^3 cubes, %lld cells, %d levels, %lld points\n", w, (long long)ncells, levels, (long long)n);
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1) {   /* the centred (w-2)^3 box: a prefix of the ordered mesh */
            const int v = w - 2, k = w - 1;
            if (v < 1) break;
            CHECK(hmg_grid_shrink(g, 6 * (int64_t)v * v * v, (int64_t)k * k * k));
        }
        for (int level = 1; level <= levels; ++level) {
            CHECK(hmg_grid_locate(g, level, n, x, cell, nodes, wts, gw));
            int64_t inside = 0;
            for (int64_t p = 0; p < n; ++p) inside += cell[p] >= 0;
            if (cell[n - 1] != -1 || cell[n - 2] != -1 || cell[n - 3] != -1) {
                fprintf(stderr, "a point that is not finite was located\n");
                return 1;
            }
            unsigned long long h = 1469598103934665603ull;
            h = fold(h, cell, sizeof(int32_t) * (size_t)n);
            h = fold(h, nodes, sizeof(int32_t) * 4 * (size_t)n);
            for (int64_t p = 0; p < n; ++p)
                if (cell[p] >= 0) {   /* (NaN payloads of the points without a cell are not part of the contract) */
                    h = fold(h, wts + 4 * p, sizeof(double) * 4);
                    h = fold(h, gw + 12 * p, sizeof(double) * 12);
                }
            printf("hash pass %d level %d inside %lld  %016llx\n", pass, level, (long long)inside, h);
        }
        /* one output at a time, and none */
        CHECK(hmg_grid_locate(g, levels, n, x, cell, NULL, NULL, NULL));
        CHECK(hmg_grid_locate(g, levels, n, x, NULL, NULL, NULL, gw));
        if (hmg_grid_locate(g, levels, n, x, NULL, NULL, NULL, NULL) == 0 || hmg_grid_locate(g, levels + 1, n, x, cell, NULL, NULL, NULL) == 0) {
            fprintf(stderr, "a refusal did not refuse\n");
            return 1;
        }
    }
    printf("locator builds %lld, bytes %lld, longest list %lld\n", (long long)hmg_ctx_counter(NULL, "sample_locator_builds"),
           (long long)hmg_ctx_counter(NULL, "sample_locator_bytes"), (long long)hmg_ctx_counter(NULL, "sample_locator_max_candidates"));
    CHECK(hmg_grid_destroy(g));
    free(coords);
    free(cells);
    free(x);
    free(cell);
    free(nodes);
    free(wts);
    free(gw);
    printf("host_locate: done\n");
    return 0;
}

/*
 * host_tensor.c -- the HOST code paths of hmg_grid_set_operator_tensor, driven without a GPU (NULL context, as host_tables.c): a full
 * symmetric tensor per cell through the coefficient rows, the class table (a class of its own for every cell), the level-1
 * assembly, the refusal of an indefinite and of a non-finite tensor (the previous operator stays), the domain shrink, and a
 * partitioned grid's stored global field cut to its share, before and after a shrink.  Built against the AddressSanitizer / UBSan
 * build of the library by tests/test_sanitizers_tensor.py.
 *
 * Prints one "hash" line per step: the checksum of all tables a device grid would have uploaded.
 *
 *   host_tensor [width = 6] [levels = 3]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "hmg.h"

#define CHECK(call)                                                            \
    do {                                                                       \
        if ((call) != 0) {                                                     \
            fprintf(stderr, "%s failed: %s\n", #call, hmg_last_error());       \
            return 1;                                                          \
        }                                                                      \
    } while (0)

static int print_hash(const char *what, hmg_grid *g)
{
    int32_t h[2] = {0, 0};
    int64_t n = 0;
    CHECK(hmg_grid_table_i32(g, 1, "upload_hash", h, 2, &n));
    printf("hash %-28s cells %8lld  %08x%08x\n", what, (long long)hmg_grid_ncells(g), (unsigned)h[1], (unsigned)h[0]);
    return 0;
}

int main(int argc, char **argv)
{
    const int w = argc > 1 ? atoi(argv[1]) : 6, levels = argc > 2 ? atoi(argv[2]) : 3;
    const int64_t shape[3] = {w, w, w};
    const double origin[3] = {-0.5 * w, -0.5 * w, -0.5 * w};
    int64_t nnodes = 0, ncells = 0, n = 0;
    CHECK(hmg_checkerboard_mesh_size(3, shape, &nnodes, &ncells));
    double *coords = malloc(sizeof(double) * 3 * (size_t)nnodes);
    int64_t *cells = malloc(sizeof(int64_t) * 4 * (size_t)ncells);
    double *tensor = malloc(sizeof(double) * 6 * (size_t)ncells);
    int32_t *owner = malloc(sizeof(int32_t) * (size_t)ncells);
    int32_t *cls = malloc(sizeof(int32_t) * (size_t)ncells);
    CHECK(hmg_checkerboard_mesh(3, shape, origin, 1, 1, coords, cells));
    /* a two-valued diagonal plus off-diagonal entries that differ from cell to cell (diagonally dominant: positive definite) */
    unsigned s = 12345u;
    for (int64_t c = 0; c < ncells; ++c) {
        double d[3];
        for (int a = 0; a < 3; ++a) {
            s = s * 1664525u + 1013904223u;
            d[a] = (s >> 16) & 1u ? 100.0 : 1.0;
        }
        const double o = 0.25 * (double)(c + 1) / (double)ncells;
        const double t[6] = {d[0], o, -0.5 * o, d[1], 0.25 * o, d[2]};
        for (int q = 0; q < 6; ++q) tensor[6 * c + q] = t[q];
    }
    printf("host_tensor: %d^3 cubes, %lld cells, %d levels\n", w, (long long)ncells, levels);

    hmg_grid *g = NULL;
    CHECK(hmg_grid_create(NULL, 3, levels, nnodes, coords, ncells, cells, &g));
    CHECK(hmg_grid_set_operator_tensor(g, tensor, 1.0));
    CHECK(hmg_coarse_setup(g));
    if (print_hash("tensor grid + level 1", g)) return 1;
    CHECK(hmg_grid_table_i32(g, 1, "cell_class", cls, ncells, &n));
    if (levels >= 2 && n != ncells) {
        fprintf(stderr, "cell_class holds %lld entries, not %lld\n", (long long)n, (long long)ncells);
        return 1;
    }
    for (int64_t c = 0; c < n; ++c)
        if (cls[c] != (int32_t)c) {
            fprintf(stderr, "cell %lld has class %d: every row is distinct, classes are numbered by first use\n", (long long)c, cls[c]);
            return 1;
        }
    const int64_t last = ncells - 1;
    const double keep = tensor[6 * last + 1];
    tensor[6 * last + 1] = 1000.0;                                  /* second leading minor < 0 */
    if (hmg_grid_set_operator_tensor(g, tensor, 1.0) == 0) {
        fprintf(stderr, "an indefinite tensor was accepted\n");
        return 1;
    }
    printf("refused: %s\n", hmg_last_error());
    tensor[6 * last + 1] = NAN;
    if (hmg_grid_set_operator_tensor(g, tensor, 1.0) == 0) {
        fprintf(stderr, "a tensor that is not finite was accepted\n");
        return 1;
    }
    printf("refused: %s\n", hmg_last_error());
    tensor[6 * last + 1] = keep;
    CHECK(hmg_grid_set_lambda(g, 0.5));
    CHECK(hmg_coarse_setup(g));
    if (print_hash("  ... after two refusals", g)) return 1;
    if (w > 2) {
        const int64_t v = w - 2, k = v + 1;
        CHECK(hmg_grid_shrink(g, 6 * v * v * v, k * k * k));
        CHECK(hmg_coarse_setup(g));
        if (print_hash("tensor grid shrunk", g)) return 1;
    }
    CHECK(hmg_grid_destroy(g));

    /* two ranks (halves about the origin): the GLOBAL field, cut to each share; the last rank shrunk, then a new field */
    const int64_t blocks[3] = {2, 1, 1};
    CHECK(hmg_block_owner(3, nnodes, coords, ncells, cells, blocks, 0.5 * w, origin, owner));
    for (int r = 0; r < 2; ++r) {
        hmg_grid *p = NULL;
        char name[64];
        CHECK(hmg_grid_create_partition(NULL, 3, levels, nnodes, coords, ncells, cells, owner, r, 2, &p));
        CHECK(hmg_grid_set_operator_tensor(p, tensor, 1.0));
        CHECK(hmg_coarse_setup(p));
        snprintf(name, sizeof name, "rank %d of 2", r);
        if (print_hash(name, p)) return 1;
        if (w > 2 && r == 1) {
            const int64_t v = w - 2, k = v + 1;
            CHECK(hmg_grid_shrink(p, 6 * v * v * v, k * k * k));
            if (print_hash("  ... shrunk", p)) return 1;
            CHECK(hmg_grid_set_operator_tensor(p, tensor, 0.5));
            CHECK(hmg_coarse_setup(p));
            if (print_hash("  ... a new field", p)) return 1;
        }
        CHECK(hmg_grid_destroy(p));
    }
    free(cls);
    free(owner);
    free(tensor);
    free(cells);
    free(coords);
    printf("host_tensor: done\n");
    return 0;
}

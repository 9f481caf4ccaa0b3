/* the bin order of a ray dump (lucille_amd/csrc/lh_order.h) as a stand-alone program: tests/test_order_key.py feeds it rays and compares what it
 * writes with numpy.  lh_order_check IN OUT
 * IN:  uint64 n; uint32 bits, octant; float grid_lo[3], grid_step[3]; double org[3 n]; double dir[3 n]
 * OUT: uint32 nblocks, nbins, block, pad; uint32 key[n], dest[n]; uint32 counts[nblocks x nbins], offset[nblocks x nbins]; plan: uint64 x 15 */
#include <stdio.h>
#include <stdlib.h>
#include "../../lucille_amd/csrc/lh_order.h"

static void die(const char *what) { fprintf(stderr, "lh_order_check: %s\n", what); exit(2); }

int main(int argc, char **argv)
{
    uint64_t n; uint32_t hb[2], head[4]; float lo[3], step[3];
    if (argc != 3) die("usage: lh_order_check IN OUT");
    FILE *f = fopen(argv[1], "rb");
    if (!f) die("cannot open IN");
    if (fread(&n, sizeof(n), 1, f) != 1 || fread(hb, sizeof(hb), 1, f) != 1 || fread(lo, sizeof(lo), 1, f) != 1 || fread(step, sizeof(step), 1, f) != 1) die("short header");
    if (n == 0 || !lh_order_valid(hb[0], hb[1])) die("bad header");
    double *org = (double *)malloc(sizeof(double) * 3 * n), *dir = (double *)malloc(sizeof(double) * 3 * n);
    if (!org || !dir || fread(org, sizeof(double) * 3, n, f) != n || fread(dir, sizeof(double) * 3, n, f) != n) die("short rays");
    fclose(f);
    const lh_order_grid_t g = lh_order_grid(lo, step, hb[0], hb[1]);
    const lh_order_plan_t p = lh_order_plan(n, hb[0], hb[1], 1), pa = lh_order_plan(n, hb[0], hb[1], 0);
    const size_t table = (size_t)p.nblocks * p.nbins;
    uint32_t *key = (uint32_t *)malloc(sizeof(uint32_t) * n), *dest = (uint32_t *)malloc(sizeof(uint32_t) * n);
    uint32_t *counts = (uint32_t *)malloc(sizeof(uint32_t) * table), *offset = (uint32_t *)malloc(sizeof(uint32_t) * table);
    if (!key || !dest || !counts || !offset) die("out of memory");
    lh_order_host(n, org, dir, &g, key, counts, offset, dest);
    head[0] = p.nblocks; head[1] = p.nbins; head[2] = p.block; head[3] = 0;
    const uint64_t plan[15] = {p.org, p.dir, p.t, p.u, p.v, p.prim, p.dest, p.counts, p.offset, p.bintotal, p.binbase, p.bytes, pa.occ, pa.bytes, p.slot};
    f = fopen(argv[2], "wb");
    if (!f) die("cannot open OUT");
    if (fwrite(head, sizeof(head), 1, f) != 1 || fwrite(key, sizeof(uint32_t), n, f) != n || fwrite(dest, sizeof(uint32_t), n, f) != n ||
        fwrite(counts, sizeof(uint32_t), table, f) != table || fwrite(offset, sizeof(uint32_t), table, f) != table || fwrite(plan, sizeof(plan), 1, f) != 1) die("short write");
    fclose(f);
    free(org); free(dir); free(key); free(dest); free(counts); free(offset);
    return 0;
}

/* the rule of area lights (lucille_amd/csrc/lh_area.h) as a stand-alone program: tests/test_area_rule.py feeds it hits with their lights, emitter
 * triangles, uniforms and any-hit bytes and compares what it writes, bit for bit, with its own restatement in numpy.  lh_area_check IN OUT
 * IN:  uint64 count; per case: head_t, ntab x 9 doubles (triangles), use_uni ? 3 L S doubles : nothing, L S bytes padded to a multiple of 8
 *      (mode 1: the acceptance helpers alone -- no triangles, uniforms or bytes follow; the table's count is `claim`)
 *      (mode 2: lh_area_pick alone -- x0 in P[0], ntris in `claim`)
 * OUT: per case: tail_t; mode 0 then: ntab x 16 doubles (records), L S x item_t */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../lucille_amd/csrc/lh_area.h"

typedef struct { double P[3], Ns[3], eps, bound; uint32_t L, S, ntab, use_uni; uint64_t key, seed, claim; uint32_t mode, reserved;
                 lh_area_light_t lights[LH_AREA_LIGHTS_MAX]; } head_t;
typedef struct { double O[3]; uint32_t mask, closed, ok, pad; float value[3]; int32_t pick; } tail_t;
typedef struct { double x[3], dir[3], w, tmax; } item_t;

static void die(const char *what) { fprintf(stderr, "lh_area_check: %s\n", what); exit(2); }
static void rd(void *p, size_t n, FILE *f) { if (n && fread(p, 1, n, f) != n) die("short input"); }
static void wr(const void *p, size_t n, FILE *f) { if (n && fwrite(p, 1, n, f) != n) die("short write"); }

int main(int argc, char **argv)
{
    uint64_t count;
    if (argc != 3) die("usage: lh_area_check IN OUT");
    if (sizeof(lh_area_light_t) != 40 || sizeof(lh_area_params_t) != 24 || sizeof(lh_emitter_t) != 128) die("struct sizes");
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) die("cannot open IN or OUT");
    rd(&count, sizeof(count), f);
    for (uint64_t k = 0; k < count; k++) {
        head_t h;
        tail_t t;
        rd(&h, sizeof(h), f);
        memset(&t, 0, sizeof(t));
        const lh_area_params_t prm = {h.eps, h.bound, (int32_t)h.S, h.reserved};
        if (h.mode == 2) { t.pick = lh_area_pick(h.P[0], (uint32_t)h.claim); wr(&t, sizeof(t), g); continue; }
        t.ok = (uint32_t)lh_area_lights_ok(h.lights, (int)h.L, &prm, h.mode == 1 ? h.claim : h.ntab);
        if (h.mode == 1) { wr(&t, sizeof(t), g); continue; }
        if (h.L < 1 || h.L > LH_AREA_LIGHTS_MAX || h.S < 1 || h.S > LH_AREA_SAMPLES_MAX || h.ntab < 1) die("bad case");
        const size_t LS = (size_t)h.L * h.S, nb = (LS + 7) & ~(size_t)7;
        double *tri = (double *)malloc(sizeof(double) * 9 * h.ntab), *uni = h.use_uni ? (double *)malloc(sizeof(double) * 3 * LS) : NULL;
        lh_emitter_t *rec = (lh_emitter_t *)malloc(sizeof(lh_emitter_t) * h.ntab);
        uint8_t *occ = (uint8_t *)malloc(nb);
        item_t *it = (item_t *)calloc(LS, sizeof(item_t));
        if (!tri || !rec || !occ || !it || (h.use_uni && !uni)) die("out of memory");
        rd(tri, sizeof(double) * 9 * h.ntab, f);
        if (uni) rd(uni, sizeof(double) * 3 * LS, f);
        rd(occ, nb, f);
        for (uint32_t j = 0; j < h.ntab; j++) lh_area_emitter(tri + 9 * j, rec + j);
        t.O[0] = h.P[0] + h.Ns[0] * h.eps; t.O[1] = h.P[1] + h.Ns[1] * h.eps; t.O[2] = h.P[2] + h.Ns[2] * h.eps;
        for (uint32_t l = 0; l < h.L; l++) {
            if ((uint64_t)h.lights[l].first_tri + h.lights[l].ntris > h.ntab || h.lights[l].ntris < 1) die("a run leaves the table");
            for (uint32_t s = 0; s < h.S; s++) {
                item_t *o = it + (size_t)l * h.S + s;
                lh_area_item_uniforms(uni, h.key, h.seed, (int)h.L, (int)h.S, (int)l, (int)s, o->x);
                o->tmax = lh_area_item(t.O, h.Ns, h.lights + l, rec, o->x, h.bound, o->dir, &o->w);
            }
        }
        t.mask = lh_area_value(t.O, h.Ns, h.lights, (int)h.L, (int)h.S, rec, h.bound, uni, h.key, h.seed, occ, t.value, &t.closed);
        wr(&t, sizeof(t), g); wr(rec, sizeof(lh_emitter_t) * h.ntab, g); wr(it, sizeof(item_t) * LS, g);
        free(tri); free(uni); free(rec); free(occ); free(it);
    }
    fclose(f);
    if (fclose(g) != 0) die("short write");
    return 0;
}

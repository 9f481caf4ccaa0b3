/* the rule of direct light (lucille_amd/csrc/lh_lights.h) as a stand-alone program: tests/test_lights_rule.py feeds it a table of hits with their
 * lights and any-hit bytes and compares what it writes, bit for bit, with its own restatement in numpy.  lh_lights_check IN OUT
 * IN:  uint64 count; count x case_t
 * OUT: count x out_t */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../lucille_amd/csrc/lh_lights.h"

typedef struct { double P[3], Ns[3], eps; uint32_t L, pad; lh_light_t lights[LH_LIGHTS_MAX]; uint8_t occ[32]; } case_t;
typedef struct { double O[3]; double dir[LH_LIGHTS_MAX][3]; double tmax_ray[LH_LIGHTS_MAX], w[LH_LIGHTS_MAX], tmax_item[LH_LIGHTS_MAX];
                 uint32_t mask, ok; float value[3]; uint32_t pad; } out_t;

static void die(const char *what) { fprintf(stderr, "lh_lights_check: %s\n", what); exit(2); }

int main(int argc, char **argv)
{
    uint64_t count;
    if (argc != 3) die("usage: lh_lights_check IN OUT");
    if (sizeof(lh_light_t) != 56 || sizeof(lh_light_tab_t) != 56 * LH_LIGHTS_MAX || sizeof(lh_lights_params_t) != 8) die("struct sizes");
    FILE *f = fopen(argv[1], "rb");
    if (!f) die("cannot open IN");
    if (fread(&count, sizeof(count), 1, f) != 1 || count == 0) die("bad header");
    case_t *in = (case_t *)malloc(sizeof(case_t) * count);
    out_t *out = (out_t *)calloc(count, sizeof(out_t));
    if (!in || !out || fread(in, sizeof(case_t), count, f) != count) die("short table");
    fclose(f);
    for (uint64_t k = 0; k < count; k++) {
        const case_t *c = &in[k];
        out_t *o = &out[k];
        if (c->L < 1 || c->L > LH_LIGHTS_MAX) die("bad L");
        lh_light_origin(c->P, c->Ns, c->eps, o->O);
        for (uint32_t l = 0; l < c->L; l++) {
            double d2[3], w2;
            o->tmax_ray[l] = lh_light_ray(o->O, &c->lights[l], o->dir[l]);
            o->w[l] = lh_light_weight(c->Ns, o->dir[l], c->lights[l].flags);
            o->tmax_item[l] = lh_light_item(o->O, c->Ns, &c->lights[l], d2, &w2);
            if (memcmp(d2, o->dir[l], sizeof(d2)) != 0 || memcmp(&w2, &o->w[l], sizeof(w2)) != 0) die("lh_light_item disagrees with its parts");
        }
        o->mask = lh_lights_value(o->O, c->Ns, c->lights, (int)c->L, c->occ, o->value);
        o->ok = (uint32_t)lh_lights_ok(c->lights, (int)c->L, c->eps);
    }
    f = fopen(argv[2], "wb");
    if (!f) die("cannot open OUT");
    if (fwrite(out, sizeof(out_t), count, f) != count) die("short write");
    fclose(f);
    free(in); free(out);
    return 0;
}

/* the gather stage's plan (lucille_amd/csrc/lh_gather.h) as a stand-alone program: tests/test_gather_plan.py feeds it a table of stages and compares
 * the plans it writes with its own restatement of the two expressions the plan replaced.  lh_gather_check IN OUT
 * IN:  uint64 count; count x case_t
 * OUT: count x out_t */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "../../lucille_amd/csrc/lh_gather.h"

typedef struct { uint32_t kind, where, ao_fused, uniforms, ao_group, sun, sync, pad; uint64_t entries, N; } case_t;
typedef struct { uint32_t fused, late; } out_t;

static void die(const char *what) { fprintf(stderr, "lh_gather_check: %s\n", what); exit(2); }

int main(int argc, char **argv)
{
    uint64_t count;
    if (argc != 3) die("usage: lh_gather_check IN OUT");
    FILE *f = fopen(argv[1], "rb");
    if (!f) die("cannot open IN");
    if (fread(&count, sizeof(count), 1, f) != 1 || count == 0) die("bad header");
    case_t *in = (case_t *)malloc(sizeof(case_t) * count);
    out_t *out = (out_t *)malloc(sizeof(out_t) * count);
    if (!in || !out || fread(in, sizeof(case_t), count, f) != count) die("short table");
    fclose(f);
    for (uint64_t k = 0; k < count; k++) {
        const case_t *c = &in[k];
        const lh_gather_plan_t p = lh_gather_plan((int)c->kind, (int)c->where, (size_t)c->entries, (size_t)c->N, (int)c->ao_fused, (int)c->uniforms,
                                                  (int)c->ao_group, (int)c->sun, (int)c->sync);
        out[k].fused = (uint32_t)p.fused; out[k].late = (uint32_t)p.late;
    }
    f = fopen(argv[2], "wb");
    if (!f) die("cannot open OUT");
    if (fwrite(out, sizeof(out_t), count, f) != count) die("short write");
    fclose(f);
    free(in); free(out);
    return 0;
}

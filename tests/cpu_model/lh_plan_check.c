/* the launch geometry (lucille_amd/csrc/lh_plan.h) as a stand-alone program: tests/test_launch_plan.py feeds it a table of scenes and launches and
 * compares the plans it writes with its own restatement of the rules.  lh_plan_check IN OUT
 * IN:  uint64 count; count x case_t
 * OUT: count x out_t -- the plan, then what sizes the grid: lh_plan_trace_rows and the workgroups per CU of those rows */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../lucille_amd/csrc/lh_plan.h"

typedef struct { uint32_t q4_stack, q4_depth, stack_cap, top_nodes, nq4nodes, q8_depth, prefer_q8, max_depth, ray_chunk, ray_budget, n_dev, kind, variant, have_queue;
                 int32_t grid_blocks; uint32_t pad; uint64_t n; } case_t;
typedef struct { uint32_t walk, rows, guard, top_nodes, lds_bytes, wgs_per_cu, ray_chunk, coop, ray_budget, coop_rows, coop_lds_bytes, err, trace_rows, grid_wgs; } out_t;

static void die(const char *what) { fprintf(stderr, "lh_plan_check: %s\n", what); exit(2); }

int main(int argc, char **argv)
{
    uint64_t count;
    static const uint32_t on_device = 0;          /* a launch whose ray count lives on the device names its address; the plan looks at whether it does */
    static const char some_nodes[128];
    if (argc != 3) die("usage: lh_plan_check IN OUT");
    FILE *f = fopen(argv[1], "rb");
    if (!f) die("cannot open IN");
    if (fread(&count, sizeof(count), 1, f) != 1 || count == 0) die("bad header");
    case_t *in = (case_t *)malloc(sizeof(case_t) * count);
    out_t *out = (out_t *)malloc(sizeof(out_t) * count);
    if (!in || !out || fread(in, sizeof(case_t), count, f) != count) die("short table");
    fclose(f);
    for (uint64_t k = 0; k < count; k++) {
        const case_t *c = &in[k];
        lh_dev_scene_t sc;
        memset(&sc, 0, sizeof(sc));
        sc.q4_stack = c->q4_stack; sc.q4_depth = c->q4_depth; sc.stack_cap = c->stack_cap; sc.top_nodes = c->top_nodes; sc.nq4nodes = c->nq4nodes;
        sc.q8_depth = c->q8_depth; sc.prefer_q8 = (int)c->prefer_q8; sc.q8nodes = c->prefer_q8 ? some_nodes : NULL; sc.max_depth = c->max_depth;
        sc.ray_chunk = c->ray_chunk; sc.ray_budget = c->ray_budget; sc.n_dev = c->n_dev ? &on_device : NULL;
        const lh_plan_t p = lh_plan_launch(&sc, (size_t)c->n, (int)c->kind, (int)c->variant, c->grid_blocks, (int)c->have_queue);
        out_t *o = &out[k];
        o->walk = (uint32_t)p.walk; o->rows = p.rows; o->guard = (uint32_t)p.guard; o->top_nodes = p.top_nodes; o->lds_bytes = (uint32_t)p.lds_bytes;
        o->wgs_per_cu = p.wgs_per_cu; o->ray_chunk = p.ray_chunk; o->coop = (uint32_t)p.coop; o->ray_budget = p.ray_budget; o->coop_rows = p.coop_rows;
        o->coop_lds_bytes = (uint32_t)p.coop_lds_bytes; o->err = (uint32_t)p.err;
        o->trace_rows = lh_plan_trace_rows(&sc); o->grid_wgs = lh_plan_wgs_per_cu(o->trace_rows);
    }
    f = fopen(argv[2], "wb");
    if (!f) die("cannot open OUT");
    if (fwrite(out, sizeof(out_t), count, f) != count) die("short write");
    fclose(f);
    free(in); free(out);
    return 0;
}

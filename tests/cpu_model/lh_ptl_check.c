/* lh_ptl.h on the CPU (tests/test_ptl_rule.py): a table of cases in, the header's answers out.
 *   lh_ptl_check in.bin out.bin          in: uint64 n, then n cases; out: n answers
 * Built with -ffp-contract=off, as the header asks. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../lucille_amd/csrc/lh_ptl.h"

typedef struct { float G[3], kd[3], col[3], value[3]; double c[9], w, u, v; } case_t;          /* c: three corners' colours, corner-major */
typedef struct { float r[3], colour[3]; } out_t;

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    uint64_t n = 0;
    if (fread(&n, sizeof(n), 1, f) != 1) return 4;
    case_t *in = (case_t *)malloc(sizeof(case_t) * (n ? n : 1));
    out_t *out = (out_t *)malloc(sizeof(out_t) * (n ? n : 1));
    if (!in || !out || fread(in, sizeof(case_t), n, f) != n) return 5;
    fclose(f);
    for (uint64_t i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) {
            out[i].r[k] = lh_ptl_direct(in[i].G[k], in[i].kd[k], in[i].col[k], in[i].value[k]);
            out[i].colour[k] = lh_ptl_colour(in[i].c[k], in[i].c[3 + k], in[i].c[6 + k], in[i].w, in[i].u, in[i].v);
        }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out, sizeof(out_t), n, f) != n) return 6;
    fclose(f);
    free(in); free(out);
    return 0;
}

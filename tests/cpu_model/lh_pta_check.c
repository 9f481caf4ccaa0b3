/* the area-light functions of lh_ptl.h on the CPU (tests/test_pta_rule.py): a table of cases in, the header's answers out.
 *   lh_pta_check in.bin out.bin          in: uint64 n, then n cases; out: n answers
 * Built with -ffp-contract=off, as the header asks. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../lucille_amd/csrc/lh_ptl.h"

typedef struct { int32_t px, py, width, height, spp_total, spp_begin, s, d; uint64_t seed; float delta[3], area[3]; } case_t;          /* 64 bytes */
typedef struct { uint64_t key, seed; float value[3]; uint32_t ok; } out_t;                                                             /* 32 bytes */

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
    for (uint64_t i = 0; i < n; i++) {
        out[i].key = lh_ptl_area_key(in[i].px, in[i].py, in[i].width, in[i].spp_total, in[i].spp_begin, in[i].s);
        out[i].seed = lh_ptl_area_seed(in[i].seed, in[i].d);
        for (int k = 0; k < 3; k++) out[i].value[k] = lh_ptl_value(in[i].delta[k], in[i].area[k]);
        out[i].ok = (uint32_t)lh_ptl_area_keys_ok(in[i].width, in[i].height, in[i].spp_total);
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out, sizeof(out_t), n, f) != n) return 6;
    fclose(f);
    free(in); free(out);
    return 0;
}

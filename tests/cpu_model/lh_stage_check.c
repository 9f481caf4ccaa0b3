/* the layout of a host form's staging block (lucille_amd/csrc/lh_stage.h) as a stand-alone program: tests/test_host_stage.py feeds it a table of field
 * lists and checks what it writes.  lh_stage_check IN OUT
 * IN:  uint64 count; count x case_t -- nf fields of bytes[k] bytes, made by the constructor kind[k] names (KIND_*: with the caller's array there or NULL)
 * OUT: count x out_t -- lh_stage_layout's answer and total, each field's bytes and offset as laid out, and its device pointer's distance from the
 *      block's base (ABSENT for NULL).  Every case is laid out twice, from fresh fields: answers that differ end the program */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../lucille_amd/csrc/lh_stage.h"

#define MAXF 12
#define ABSENT UINT64_MAX
enum { KIND_SCRATCH = 0, KIND_UP, KIND_UP_NULL, KIND_DOWN, KIND_DOWN_NULL, KIND_BOTH, KIND_BOTH_NULL };

typedef struct { uint32_t nf; uint8_t kind[MAXF]; uint64_t bytes[MAXF]; } case_t;
typedef struct { int32_t rc; uint32_t pad; uint64_t total, bytes[MAXF], off[MAXF], dev[MAXF]; } out_t;

static void die(const char *what) { fprintf(stderr, "lh_stage_check: %s\n", what); exit(2); }

static void lay_out(const case_t *c, out_t *o)
{
    static char caller[16];          /* the caller's array: looked at for being there, never read */
    char *const base = (char *)(uintptr_t)0x7000000000ull;          /* a block's address: places are computed from it, nothing is stored there */
    lh_field_t f[MAXF];
    memset(o, 0, sizeof(*o));
    for (uint32_t k = 0; k < c->nf; k++) {
        const size_t b = (size_t)c->bytes[k];
        switch (c->kind[k]) {
        case KIND_SCRATCH:   f[k] = lh_field_scratch(b); break;
        case KIND_UP:        f[k] = lh_field_up(caller, b); break;
        case KIND_UP_NULL:   f[k] = lh_field_up(NULL, b); break;
        case KIND_DOWN:      f[k] = lh_field_down(caller, b); break;
        case KIND_DOWN_NULL: f[k] = lh_field_down(NULL, b); break;
        case KIND_BOTH:      f[k] = lh_field_both(caller, b); break;
        case KIND_BOTH_NULL: f[k] = lh_field_both(NULL, b); break;
        default: die("unknown field kind");
        }
    }
    size_t total = 0;
    o->rc = lh_stage_layout(f, (int)c->nf, &total);
    if (o->rc != 0) return;
    lh_stage_place(f, (int)c->nf, base);
    o->total = total;
    for (uint32_t k = 0; k < c->nf; k++) {
        o->bytes[k] = f[k].bytes; o->off[k] = f[k].off;
        o->dev[k] = f[k].dev ? (uint64_t)((uintptr_t)f[k].dev - (uintptr_t)base) : ABSENT;
    }
}

int main(int argc, char **argv)
{
    uint64_t count;
    if (sizeof(size_t) != 8) die("a 64-bit size_t is assumed by the table's format");
    if (argc != 3) die("usage: lh_stage_check IN OUT");
    FILE *f = fopen(argv[1], "rb");
    if (!f) die("cannot open IN");
    if (fread(&count, sizeof(count), 1, f) != 1 || count == 0) die("bad header");
    case_t *in = (case_t *)malloc(sizeof(case_t) * count);
    out_t *out = (out_t *)malloc(sizeof(out_t) * count);
    if (!in || !out || fread(in, sizeof(case_t), count, f) != count) die("short table");
    fclose(f);
    for (uint64_t k = 0; k < count; k++) {
        out_t again;
        if (in[k].nf < 1 || in[k].nf > MAXF) die("bad field count");
        lay_out(&in[k], &out[k]);
        lay_out(&in[k], &again);
        if (memcmp(&out[k], &again, sizeof(again)) != 0) die("the same fields were laid out differently the second time");
    }
    f = fopen(argv[2], "wb");
    if (!f) die("cannot open OUT");
    if (fwrite(out, sizeof(out_t), count, f) != count) die("short write");
    fclose(f);
    free(in); free(out);
    return 0;
}

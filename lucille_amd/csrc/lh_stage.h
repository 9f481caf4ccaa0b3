/*
 * lh_stage.h -- the layout of a host form's staging block, stated once.  An entry point that takes HOST arrays (lh_accel_*_host, lh_render_ao_tile_host,
 * ...) lists its arrays as fields; this rule gives every field its place in ONE device block; lh_stage_up / lh_stage_down (lh_internal.h) grow the
 * block, copy up, and copy down around the device form.  Plain C without HIP: the entry points and a stand-alone checker
 * (tests/cpu_model/lh_stage_check.c, tests/test_host_stage.py) read the same rule.
 *
 *   - every present field starts on an LH_STAGE_ALIGN boundary (no array relies on what stands before it for its alignment);
 *   - the fields keep their order;
 *   - a field of zero bytes takes no room and gets no device pointer: an optional array the caller left NULL is a zero-byte field;
 *   - a total that does not fit size_t is refused.
 */
#ifndef LH_STAGE_H
#define LH_STAGE_H

#include <stddef.h>
#include <stdint.h>

#define LH_STAGE_ALIGN 16u

typedef struct lh_field {
    const void *up;           /* the caller's array to copy up from before the device form runs, or NULL */
    void       *down;         /* the caller's array to copy down to after it, or NULL; both: what the device form leaves alone stays the caller's */
    size_t      bytes;        /* 0: the field is absent */
    size_t      off;          /* lh_stage_layout: where it starts in the block (an absent field: where the next present one does) */
    void       *dev;          /* lh_stage_place: its device pointer, NULL for an absent field */
} lh_field_t;

/* the four kinds of field; an array the caller left NULL makes an absent field of the first three */
static inline lh_field_t lh_field_up(const void *src, size_t bytes) { lh_field_t f = {src, NULL, src ? bytes : 0, 0, NULL}; return f; }
static inline lh_field_t lh_field_down(void *dst, size_t bytes) { lh_field_t f = {NULL, dst, dst ? bytes : 0, 0, NULL}; return f; }
static inline lh_field_t lh_field_both(void *arr, size_t bytes) { lh_field_t f = {arr, arr, arr ? bytes : 0, 0, NULL}; return f; }
static inline lh_field_t lh_field_scratch(size_t bytes) { lh_field_t f = {NULL, NULL, bytes, 0, NULL}; return f; }

/* offsets for f[0 .. nf) and the block's size (the last end rounded up to LH_STAGE_ALIGN); -1: the size does not fit size_t (nothing is written to *total) */
static inline int lh_stage_layout(lh_field_t *f, int nf, size_t *total)
{
    const size_t mask = LH_STAGE_ALIGN - 1u;
    size_t at = 0;
    for (int k = 0; k < nf; k++) {
        f[k].off = at;
        if (f[k].bytes > SIZE_MAX - mask || ((f[k].bytes + mask) & ~mask) > SIZE_MAX - at) return -1;
        at += (f[k].bytes + mask) & ~mask;
    }
    *total = at;
    return 0;
}

/* the device pointers of laid-out fields in a block at `base`: NULL for an absent field */
static inline void lh_stage_place(lh_field_t *f, int nf, void *base)
{
    for (int k = 0; k < nf; k++) f[k].dev = f[k].bytes ? (void *)((uintptr_t)base + f[k].off) : NULL;
}

#endif

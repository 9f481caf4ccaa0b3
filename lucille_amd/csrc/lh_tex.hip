/*
 * lh_tex.hip -- material textures on the accelerator (the rule: lh_tex.h; the kernels: lh_render.hip): the setters, the per-mesh
 * descriptor table the textured resolves read, and the fetch alone for a caller's batch of hit records.
 *
 * Reference: the texture multiply both occlusion transports end with (src/transport/ambientocclusion.c:393-401,
 * src/transport/dirtmap.c:273-281) over ri_texture_fetch (src/render/texture.c:86-235).
 *
 * A texture is a block of width x height RGBA fp32 texels the library owns.  The host setter works without a device (an
 * accelerator that is not committed yet): the block stays a host copy until the first call that reads it on the device
 * (lh_tex_sync).  A block that is replaced or removed is released behind a device-wide synchronise: every launch enqueued
 * earlier that may read it has finished.  Trees do not depend on textures: every setter is allowed before and after commit.
 */
#include <vector>

#include "lh_internal.h"

static uint32_t mesh_count(const lh_accel_t *a) { return a->committed ? a->hs->nmeshes : a->nmeshes + a->ndmeshes; }      /* host or device meshes, never both */

/* one reference less; the last one releases the block -- its device copy only after everything enqueued on the device has finished */
static void block_unref(lh_accel_t *a, lh_tex_block *b)
{
    if (!b || --b->refs > 0) return;
    if (b->dev || b->ev_live) {
        (void)hipSetDevice(a->device);
        (void)hipDeviceSynchronize();
        if (b->ev_live) (void)hipEventDestroy(b->ev);
        if (b->dev) (void)hipFree(b->dev);
    }
    free(b->host);
    free(b);
}

void lh_tex_release(lh_accel_t *a)
{
    for (uint32_t k = 0; k < a->ntex_slots; k++) { block_unref(a, a->tex[k]); a->tex[k] = NULL; }
    free(a->tex); a->tex = NULL; a->ntex_slots = a->ntex = 0;
    if (a->d_tex_table) { (void)hipSetDevice(a->device); (void)hipDeviceSynchronize(); (void)hipFree(a->d_tex_table); a->d_tex_table = NULL; }
    a->tex_table_n = 0;
}

/* what both setters refuse before they copy anything; *remove: the call takes the texture away */
static int setter_args(const char *who, const lh_accel_t *a, uint32_t mesh, const void *rgba, int width, int height, bool *remove)
{
    *remove = !rgba && width == 0 && height == 0;
    if (!*remove) {          /* the array and its size first: refused whatever the accelerator is */
        if (width < 1 || width > LH_TEX_MAX_SIZE || height < 1 || height > LH_TEX_MAX_SIZE)
            return fail("%s: bad texture size %d x %d (1 .. %d each)", who, width, height, LH_TEX_MAX_SIZE);
        if (!rgba) return fail("%s: NULL array", who);
        if (((uintptr_t)rgba % sizeof(float)) != 0) return fail("%s: texels not 4-byte aligned", who);
    }
    if (!a) return fail("%s: accel is NULL", who);
    if (mesh != LH_ALL_MESHES && mesh >= mesh_count(a)) return fail("%s: mesh %u out of range", who, mesh);
    return 0;
}

/* mesh (or every mesh) gets block b (NULL: none); b is released if no mesh took it */
static int assign(lh_accel_t *a, uint32_t mesh, lh_tex_block *b)
{
    const uint32_t nm = mesh_count(a);
    if (a->ntex_slots < nm) {
        lh_tex_block **nt = (lh_tex_block **)realloc(a->tex, sizeof(lh_tex_block *) * nm);
        if (!nt) { if (b) { b->refs = 1; block_unref(a, b); } return fail("out of memory"); }
        for (uint32_t k = a->ntex_slots; k < nm; k++) nt[k] = NULL;
        a->tex = nt; a->ntex_slots = nm;
    }
    if (b) b->refs = 1;          /* this function's own, dropped below */
    for (uint32_t k = 0; k < nm; k++)
        if (mesh == LH_ALL_MESHES || mesh == k) {
            if (b) b->refs++;
            block_unref(a, a->tex[k]);
            a->tex[k] = b;
        }
    block_unref(a, b);
    a->ntex = 0;
    for (uint32_t k = 0; k < a->ntex_slots; k++) if (a->tex[k]) a->ntex++;
    a->tex_dirty = 1;
    return 0;
}

extern "C" int lh_accel_set_texture(lh_accel_t *a, uint32_t mesh, const float *rgba, int width, int height)
{
    lh_guard guard(a);
    bool remove = false;
    if (setter_args("lh_accel_set_texture", a, mesh, rgba, width, height, &remove) != 0) return -1;
    if (remove) return assign(a, mesh, NULL);
    const size_t bytes = sizeof(float) * 4 * (size_t)width * (size_t)height;
    lh_tex_block *b = (lh_tex_block *)calloc(1, sizeof(*b));
    float *copy = (float *)malloc(bytes);
    if (!b || !copy) { free(b); free(copy); return fail("out of memory"); }
    memcpy(copy, rgba, bytes);
    b->width = width; b->height = height; b->host = copy;
    return assign(a, mesh, b);
}

extern "C" int lh_accel_set_texture_device(lh_accel_t *a, uint32_t mesh, const void *d_rgba, int width, int height, void *stream)
{
    lh_guard guard(a);
    const char *who = "lh_accel_set_texture_device";
    bool remove = false;
    if (setter_args(who, a, mesh, d_rgba, width, height, &remove) != 0) return -1;
    if (remove) return assign(a, mesh, NULL);
    const size_t bytes = sizeof(float) * 4 * (size_t)width * (size_t)height;
    HIPCHK(hipSetDevice(a->device));
    if (lh_device_array_ok(a, d_rgba, bytes, who, "the texel array") != 0) return -1;
    lh_tex_block *b = (lh_tex_block *)calloc(1, sizeof(*b));
    if (!b) return fail("out of memory");
    b->width = width; b->height = height;
    hipStream_t s = (hipStream_t)stream;
    /* the library's own copy, in the caller's stream order: the caller's array is free again once it has run */
    hipError_t e = hipMalloc(&b->dev, bytes);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&b->ev, hipEventDisableTiming);
    if (e == hipSuccess) b->ev_live = 1;
    if (e == hipSuccess) e = hipMemcpyAsync(b->dev, d_rgba, bytes, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipEventRecord(b->ev, s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        b->refs = 1; block_unref(a, b);
        return fail("%s: copying the texture failed: %s", who, hipGetErrorString(e));
    }
    return assign(a, mesh, b);
}

int lh_tex_sync(lh_accel_t *a)
{
    for (uint32_t k = 0; k < a->ntex_slots; k++) {
        lh_tex_block *b = a->tex[k];
        if (!b) continue;
        if (!b->dev) {          /* a host setter's block, first use */
            const size_t bytes = sizeof(float) * 4 * (size_t)b->width * (size_t)b->height;
            HIPCHK(hipMalloc(&b->dev, bytes));
            HIPCHK(hipMemcpy(b->dev, b->host, bytes, hipMemcpyHostToDevice));
            free(b->host); b->host = NULL;
        }
        if (b->ev_live) {       /* a device setter's copy on the caller's stream: launches on any stream come after it */
            HIPCHK(hipEventSynchronize(b->ev));
            (void)hipEventDestroy(b->ev); b->ev_live = 0;
        }
    }
    const uint32_t nm = a->hs->nmeshes ? a->hs->nmeshes : 1;
    if (a->tex_dirty || !a->d_tex_table || a->tex_table_n != nm) {
        std::vector<lh_tex_desc_t> table(nm, lh_tex_desc_t{NULL, 0, 0});
        for (uint32_t k = 0; k < a->ntex_slots && k < nm; k++)
            if (a->tex[k]) table[k] = lh_tex_desc_t{(const float *)a->tex[k]->dev, a->tex[k]->width, a->tex[k]->height};
        HIPCHK(hipDeviceSynchronize());          /* a launch enqueued earlier may still read the table */
        if (a->tex_table_n != nm && a->d_tex_table) { (void)hipFree(a->d_tex_table); a->d_tex_table = NULL; }
        if (!a->d_tex_table) HIPCHK(hipMalloc(&a->d_tex_table, sizeof(lh_tex_desc_t) * nm));
        a->tex_table_n = nm;
        HIPCHK(hipMemcpy(a->d_tex_table, table.data(), sizeof(lh_tex_desc_t) * nm, hipMemcpyHostToDevice));
        a->tex_dirty = 0;
    }
    return lh_ensure_prim_mesh(a);
}

/* ------------------------------------------------------------------------ */
/* the fetch alone for a caller's batch of hit records                       */
/* ------------------------------------------------------------------------ */

extern "C" int lh_accel_texture_device(lh_accel_t *a, size_t n_rays, const void *d_prim, const void *d_u, const void *d_v,
                                       const void *d_index, size_t n_index, const void *d_count, void *d_rgba_out, void *stream)
{
    lh_guard guard(a);
    const char *what = "lh_accel_texture_device";
    if (n_rays >= ((size_t)1 << 31)) return fail("%s: 2^31 - 1 rays at most in one batch (%zu given)", what, n_rays);
    if (n_index > ((size_t)1 << 30)) return fail("%s: a list holds 2^30 entries at most (%zu given)", what, n_index);
    if ((((uintptr_t)d_index | (uintptr_t)d_count | (uintptr_t)d_prim) & 3u) != 0)
        return fail("%s: the list, its count and the primitive ids are 32-bit words: a pointer is not 4-byte aligned", what);
    if ((((uintptr_t)d_u | (uintptr_t)d_v | (uintptr_t)d_rgba_out) & 7u) != 0) return fail("%s: u, v and the output are doubles: a pointer is not 8-byte aligned", what);
    if (!a || !a->committed) return fail("%s: accel not committed", what);
    if (n_rays == 0) return 0;
    if (!d_prim || !d_u || !d_v) return fail("%s: NULL record array", what);
    if (!d_rgba_out) return fail("%s: the output is NULL", what);
    const size_t L = (d_index || d_count || n_index) ? n_index : n_rays;          /* list entries; all NULL / 0: every ray */
    if (L == 0) return 0;
    HIPCHK(hipSetDevice(a->device));
    if (lh_tex_sync(a) != 0) return -1;
    const uint32_t ntris = a->hs->bvh.ntris;          /* an empty scene: every traced ray is a miss, no record array is read */
    const lh_tex_args_t tex = {ntris ? (const uint32_t *)d_prim : NULL, (const double *)d_u, (const double *)d_v, (const double *)a->d_st6,
                               (const uint32_t *)a->d_prim_mesh, (const lh_tex_desc_t *)a->d_tex_table};
    if (lh_render_launch_tex_batch(L, n_rays, (const uint32_t *)d_index, (const uint32_t *)d_count, &tex, ntris, (double *)d_rgba_out, stream) != 0)
        return fail("%s: kernel launch failed: %s", what, hipGetErrorString(hipGetLastError()));
    return 0;
}

extern "C" int lh_accel_texture_host(lh_accel_t *a, size_t n_rays, const uint32_t *prim, const double *u, const double *v, double *rgba_out)
{
    lh_guard guard(a);
    const char *what = "lh_accel_texture_host";
    if (n_rays >= ((size_t)1 << 31)) return fail("%s: 2^31 - 1 rays at most in one batch (%zu given)", what, n_rays);
    if (!a || !a->committed) return fail("%s: accel not committed", what);
    if (n_rays == 0) return 0;
    if (!prim || !u || !v) return fail("%s: NULL record array", what);
    if (!rgba_out) return fail("%s: the output is NULL", what);
    HIPCHK(hipSetDevice(a->device));
    const size_t n = n_rays, b_d = sizeof(double) * n;
    lh_field_t f[] = {lh_field_down(rgba_out, 4 * b_d), lh_field_up(u, b_d), lh_field_up(v, b_d), lh_field_up(prim, sizeof(uint32_t) * n)};
    if (lh_stage_up(a, f, 4) != 0) return -1;
    return lh_stage_down(a, f, 4, lh_accel_texture_device(a, n, f[3].dev, f[1].dev, f[2].dev, NULL, 0, NULL, f[0].dev, a->stream));
}

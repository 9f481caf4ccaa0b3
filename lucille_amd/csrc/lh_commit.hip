/*
 * lh_commit.hip -- lifetime of an accelerator behind the C ABI (include/lucille_hip.h): staging of the meshes, the host or
 * device build, the device replica of the scene, parameters.  Reference: accel_build_func / accel_free_func
 * (src/render/accel.h:24-28), ri_bvh_build (src/render/bvh.c:276-379), ri_bvh_free (bvh.c:381-387).
 */
#include <assert.h>
#include <thread>
#include <vector>

#include "lh_internal.h"
#include "lh_danger.h"
#include "lh_plan.h"
#include "lh_recommit.h"
#include "lh_route.h"

static thread_local char g_err[512] = "";

extern "C" void lh_set_error(const char *msg) { snprintf(g_err, sizeof(g_err), "%s", msg ? msg : ""); }

int lh_fail(const char *fmt, ...)
{
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
    return -1;
}

pthread_mutex_t g_scene_mu = PTHREAD_MUTEX_INITIALIZER;

extern "C" const char *lh_last_error(void) { return g_err; }

extern "C" int lh_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int lh_accel_create(lh_accel_t **out, int device)
{
    if (!out) return fail("lh_accel_create: out is NULL");
    int n = lh_device_count();
    if (n <= 0) return fail("lh_accel_create: no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= n) return fail("lh_accel_create: device %d out of range [0,%d)", device, n);
    lh_accel_t *a = (lh_accel_t *)calloc(1, sizeof(*a));
    if (!a) return fail("out of memory");
    a->hs = (lh_host_scene *)calloc(1, sizeof(lh_host_scene));
    if (!a->hs) { free(a); return fail("out of memory"); }
    a->hs->refs = 1;
    a->device = device;
    {
        pthread_mutexattr_t at; pthread_mutexattr_init(&at); pthread_mutexattr_settype(&at, PTHREAD_MUTEX_RECURSIVE);
        pthread_mutex_init(&a->mu, &at); pthread_mutexattr_destroy(&at);
    }
    a->default_variant = LH_VARIANT_SPEC;
    a->combine = 1;
    { const char *e = getenv("LH_COMBINE"); if (e) a->combine = atoi(e) != 0; }
    a->host_walk = 1;
    { const char *e = getenv("LH_HOST_WALK"); if (e) a->host_walk = atoi(e) != 0; }
    a->ao_fused = 1;
    a->wide8 = -1;
    a->build_depth_cap = LH_BUILD_DEPTH_MAX;
    { const char *e = getenv("LH_WIDE8"); if (e) a->wide8 = atoi(e); }
    { const char *e = getenv("LH_AO_FUSED"); if (e) a->ao_fused = atoi(e) != 0; }
    { const char *e = getenv("LH_FAST_START"); if (e) a->fast_start = atoi(e) != 0; }
    { const char *e = getenv("LH_POISON_OUTPUTS"); a->poison_outputs = e && atoi(e) != 0; }
    const char *env;
    a->min_active = 24;         /* the tile pipelines' regroup threshold (tools/experiments/knob_sweep6.py, r05: config 4 108.9 -> 107.4 ms, config 5 47.95 -> 47.67 ms against 32); ray dumps: LH_DUMP*_MIN_ACTIVE */
    a->tri_batch = 12;          /* parked leaves a triangle pass waits for (tools/experiments/knob_sweep2.py, r03: S-soup-1M 2119 -> 2142 Mrays/s, config-5 AO frame 87.0 -> 85.8 ms against 8) */
    env = getenv("LH_TRI_BATCH");
    if (env && atoi(env) > 0 && atoi(env) <= 64) { a->tri_batch = atoi(env); a->knobs_user = 1; }
    env = getenv("LH_MIN_ACTIVE");
    if (env && atoi(env) > 0 && atoi(env) <= 64) { a->min_active = atoi(env); a->knobs_user = 1; }
    a->ray_chunk = 256;
    env = getenv("LH_RAY_CHUNK");
    if (env && atoi(env) > 0 && atoi(env) <= (1 << 20)) a->ray_chunk = (uint32_t)atoi(env);
    a->dev.ray_chunk = a->ray_chunk;
    a->dev.ray_budget = LH_RAY_BUDGET; a->dump_budget = LH_DUMP_BUDGET;
    a->ao_budget = LH_AO_BUDGET;
    env = getenv("LH_AO_BUDGET");
    if (env && atoi(env) > 0) { a->ao_budget = (uint32_t)atoi(env); a->ao_budget_user = 1; }
    env = getenv("LH_DUMP_BUDGET");
    if (env && atoi(env) > 0) a->dump_budget = (uint32_t)atoi(env);
    env = getenv("LH_RAY_BUDGET");
    if (env && atoi(env) > 0) a->dev.ray_budget = (uint32_t)atoi(env);
    /* ray dumps in bin order (lh_order.h): on from LH_DUMP_ORDER_MIN rays, LH_DUMP_ORDER_BITS cell bits per axis under the octant, no cap on the workspace */
    a->dump_order = 1; a->dump_order_min = LH_DUMP_ORDER_MIN; a->dump_order_bits = LH_DUMP_ORDER_BITS; a->dump_order_max_mb = 0;
    env = getenv("LH_DUMP_ORDER");
    if (env) a->dump_order = atoi(env) != 0;
    a->dev.top_nodes = LH_TOP_AUTO;
    a->dev.deg_dcap = INFINITY; a->dev.cap_srcs = 0u; a->dev.ndanger = LH_DANGER_ALL;
    a->dev.coop_patience = 0;
    a->dev.ao_group = 0;            /* measured: the grouped order is SLOWER on the config-5 frame (84.6 -> 95.1 ms, tools/ao_group_probe.py): a slot's own rays share their first levels */
    env = getenv("LH_AO_GROUP");
    if (env && atoi(env) >= 0 && atoi(env) <= 4096) a->dev.ao_group = (uint32_t)atoi(env);
    env = getenv("LH_TOP_NODES");
    if (env && atoi(env) >= 0 && atoi(env) <= (int)LH_TOP_NODES_MAX) a->dev.top_nodes = (uint32_t)atoi(env);
    *out = a;
    return 0;
}

extern "C" int lh_accel_add_mesh(lh_accel_t *a, uint32_t npos, const double *pos, size_t stride,
                                 uint32_t nidx, const uint32_t *idx)
{
    lh_guard guard(a);
    if (!a) return fail("lh_accel_add_mesh: accel is NULL");
    if (a->committed) return fail("lh_accel_add_mesh: accel already committed");
    if (a->ndmeshes || a->updatable) return fail("lh_accel_add_mesh: host meshes and device meshes cannot be mixed on one accelerator%s", a->updatable ? " (\"updatable\" is for device meshes)" : "");
    if ((npos && !pos) || (nidx && !idx)) return fail("lh_accel_add_mesh: NULL array");
    if (stride < 3 * sizeof(double) || (stride % sizeof(double)) != 0) return fail("lh_accel_add_mesh: bad stride %zu", stride);
    for (uint32_t i = 0; i < nidx - (nidx % 3); i++)
        if (idx[i] >= npos) return fail("lh_accel_add_mesh: index %u out of range (npositions %u)", idx[i], npos);
    lh_mesh_copy *nm = (lh_mesh_copy *)realloc(a->meshes, sizeof(lh_mesh_copy) * (a->nmeshes + 1));
    if (!nm) return fail("out of memory");
    a->meshes = nm;
    lh_mesh_copy *m = &a->meshes[a->nmeshes];
    m->npos = npos; m->nidx = nidx; m->nrm = NULL; m->two_side = 0;
    for (int k = 0; k < 5; k++) m->attr[k] = NULL;
    m->pos = (double *)malloc(sizeof(double) * 3 * (size_t)(npos ? npos : 1));
    m->idx = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(nidx ? nidx : 1));
    if (!m->pos || !m->idx) return fail("out of memory");
    for (uint32_t i = 0; i < npos; i++) {
        const double *p = (const double *)((const char *)pos + (size_t)i * stride);
        m->pos[3 * (size_t)i] = p[0]; m->pos[3 * (size_t)i + 1] = p[1]; m->pos[3 * (size_t)i + 2] = p[2];
    }
    memcpy(m->idx, idx, sizeof(uint32_t) * nidx);
    a->nmeshes++;
    return 0;
}

extern "C" int lh_accel_set_normals(lh_accel_t *a, uint32_t mesh, const double *nrm, size_t stride, int two_side)
{
    lh_guard guard(a);
    if (!a) return fail("lh_accel_set_normals: accel is NULL");
    if (a->committed) return fail("lh_accel_set_normals: accel already committed");
    if (a->ndmeshes) return fail("lh_accel_set_normals: host arrays are not taken for device meshes (lh_accel_set_normals_device takes device arrays)");
    if (mesh >= a->nmeshes) return fail("lh_accel_set_normals: mesh %u out of range", mesh);
    if (nrm && (stride < 3 * sizeof(double) || (stride % sizeof(double)) != 0)) return fail("lh_accel_set_normals: bad stride");
    lh_mesh_copy *m = &a->meshes[mesh];
    free(m->nrm); m->nrm = NULL; m->two_side = two_side;
    if (nrm) {
        m->nrm = (double *)malloc(sizeof(double) * 3 * (size_t)(m->npos ? m->npos : 1));
        if (!m->nrm) return fail("out of memory");
        for (uint32_t i = 0; i < m->npos; i++) {
            const double *p = (const double *)((const char *)nrm + (size_t)i * stride);
            m->nrm[3 * (size_t)i] = p[0]; m->nrm[3 * (size_t)i + 1] = p[1]; m->nrm[3 * (size_t)i + 2] = p[2];
        }
    }
    return 0;
}

extern "C" int lh_accel_set_attribute(lh_accel_t *a, uint32_t mesh, int kind, const double *data, size_t stride, uint32_t count)
{
    lh_guard guard(a);
    if (!a) return fail("lh_accel_set_attribute: accel is NULL");
    if (a->committed) return fail("lh_accel_set_attribute: accel already committed");
    if (a->ndmeshes) return fail("lh_accel_set_attribute: host arrays are not taken for device meshes (lh_accel_set_attribute_device takes device arrays)");
    if (mesh >= a->nmeshes) return fail("lh_accel_set_attribute: mesh %u out of range", mesh);
    if (kind < LH_ATTR_COLOR || kind > LH_ATTR_TEXCOORD_UNSHARED) return fail("lh_accel_set_attribute: unknown attribute kind %d", kind);
    lh_mesh_copy *m = &a->meshes[mesh];
    const int ncomp = kind <= LH_ATTR_BINORMAL ? 3 : 2;
    const uint32_t need = kind == LH_ATTR_TEXCOORD_UNSHARED ? m->nidx : m->npos;
    free(m->attr[kind]); m->attr[kind] = NULL;
    if (!data) return 0;
    if (count != need) return fail("lh_accel_set_attribute: %u values given, the mesh needs %u (one per %s)", count, need,
                                   kind == LH_ATTR_TEXCOORD_UNSHARED ? "index" : "vertex");
    if (stride < (size_t)ncomp * sizeof(double) || (stride % sizeof(double)) != 0) return fail("lh_accel_set_attribute: bad stride %zu", stride);
    m->attr[kind] = (double *)malloc(sizeof(double) * ncomp * (size_t)(need ? need : 1));
    if (!m->attr[kind]) return fail("out of memory");
    for (uint32_t i = 0; i < need; i++) {
        const double *q = (const double *)((const char *)data + (size_t)i * stride);
        for (int k = 0; k < ncomp; k++) m->attr[kind][(size_t)ncomp * i + k] = q[k];
    }
    return 0;
}

/* ---- meshes handed over as device arrays ----------------------------------------------------- */
static void free_dmeshes(lh_accel_t *a)
{
    for (uint32_t g = 0; g < a->ndmeshes; g++) {
        if (a->dmeshes[g].block) (void)hipFree(a->dmeshes[g].block);
        if (a->dmeshes[g].pos_own) (void)hipFree(a->dmeshes[g].pos_own);
        for (int k = 0; k < LH_DATTR_SLOTS; k++) if (a->dmeshes[g].attr[k].block) (void)hipFree(a->dmeshes[g].attr[k].block);
    }
    free(a->dmeshes); a->dmeshes = NULL; a->ndmeshes = 0;
    for (uint32_t k = 0; k < a->ndmesh_events; k++) (void)hipEventDestroy(a->dmesh_events[k].ev);
    free(a->dmesh_events); a->dmesh_events = NULL; a->ndmesh_events = 0;
}

/* `bytes` at p are device memory of the accelerator's device, as the runtime knows it: asked, never tried */
int lh_device_array_ok(const lh_accel_t *a, const void *p, size_t bytes, const char *who, const char *what)
{
    hipPointerAttribute_t at; memset(&at, 0, sizeof(at));
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return fail("%s: %s is not a device pointer", who, what); }
    if (at.type != hipMemoryTypeDevice || at.device != a->device)
        return fail("%s: %s is not a device pointer on device %d (the accelerator's)", who, what, a->device);
    void *base = NULL; size_t size = 0;
    if (hipMemGetAddressRange((hipDeviceptr_t *)&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return 0; }
    if ((const char *)p + bytes > (const char *)base + size) return fail("%s: %s extends past its allocation (%zu bytes needed)", who, what, bytes);
    return 0;
}

/* the event of caller stream s: recorded behind every copy the library enqueues there, waited for by the commit */
static lh_dmesh_event *dmesh_event_of(lh_accel_t *a, hipStream_t s)
{
    for (uint32_t k = 0; k < a->ndmesh_events; k++) if (a->dmesh_events[k].stream == s) return &a->dmesh_events[k];
    lh_dmesh_event *ne = (lh_dmesh_event *)realloc(a->dmesh_events, sizeof(lh_dmesh_event) * (a->ndmesh_events + 1));
    if (!ne) { (void)fail("out of memory"); return NULL; }
    a->dmesh_events = ne;
    const hipError_t e = hipEventCreateWithFlags(&ne[a->ndmesh_events].ev, hipEventDisableTiming);
    if (e != hipSuccess) { (void)fail("hipEventCreateWithFlags failed: %s", hipGetErrorString(e)); return NULL; }
    ne[a->ndmesh_events].stream = s;
    return &ne[a->ndmesh_events++];
}

extern "C" int lh_accel_add_mesh_device(lh_accel_t *a, uint32_t npos, const void *d_pos, int fmt, size_t stride, uint32_t nidx,
                                        const void *d_idx, void *stream)
{
    lh_guard guard(a);
    if (!a) return fail("lh_accel_add_mesh_device: accel is NULL");
    if (a->committed || a->commit_failed) return fail("lh_accel_add_mesh_device: accel already committed");
    if (a->nmeshes) return fail("lh_accel_add_mesh_device: host meshes and device meshes cannot be mixed on one accelerator");
    if (fmt != LH_POS_F64 && fmt != LH_POS_F32) return fail("lh_accel_add_mesh_device: unknown position format %d", fmt);
    const size_t elem = fmt == LH_POS_F32 ? sizeof(float) : sizeof(double);
    if (stride < 3 * elem || (stride % elem) != 0) return fail("lh_accel_add_mesh_device: bad stride %zu", stride);
    if ((npos && !d_pos) || (nidx && !d_idx)) return fail("lh_accel_add_mesh_device: NULL array");
    if (((uintptr_t)d_pos % elem) != 0) return fail("lh_accel_add_mesh_device: positions not aligned to %zu bytes", elem);
    if (((uintptr_t)d_idx % sizeof(uint32_t)) != 0) return fail("lh_accel_add_mesh_device: indices not 4-byte aligned");
    const uint32_t ntris = nidx / 3;
    if (a->dmesh_tris + ntris >= (1ull << 29)) return fail("lh_accel_add_mesh_device: the scene would hold %llu triangles (the limit is 2^29 triangles)", a->dmesh_tris + ntris);
    if (ntris && npos == 0) return fail("lh_accel_add_mesh_device: index 0 out of range (npositions 0)");         /* every index is: known without reading one */
    /* what the flatten kernel will read: whole vertices up to the last one's z, whole triangles */
    const size_t pos_bytes = ntris ? (size_t)(npos - 1) * stride + 3 * elem : 0, idx_bytes = sizeof(uint32_t) * 3 * (size_t)ntris;
    HIPCHK(hipSetDevice(a->device));
    if (ntris && (lh_device_array_ok(a, d_pos, pos_bytes, "lh_accel_add_mesh_device", "positions") != 0 ||
                  lh_device_array_ok(a, d_idx, idx_bytes, "lh_accel_add_mesh_device", "indices") != 0)) return -1;
    lh_dmesh *nm = (lh_dmesh *)realloc(a->dmeshes, sizeof(lh_dmesh) * (a->ndmeshes + 1));
    if (!nm) return fail("out of memory");
    a->dmeshes = nm;
    lh_dmesh m; memset(&m, 0, sizeof(m));
    m.stride = stride; m.npos = npos; m.ntris = ntris; m.fmt = fmt; m.nidx = nidx;
    if (ntris) {
        hipStream_t s = (hipStream_t)stream;
        lh_dmesh_event *ev = dmesh_event_of(a, s);
        if (!ev) return -1;
        const size_t pos_room = (pos_bytes + 15) & ~(size_t)15;
        HIPCHK(hipMalloc(&m.block, pos_room + idx_bytes));
        m.pos = m.block; m.idx = (const uint32_t *)((char *)m.block + pos_room);
        /* the library's own copy, in the caller's stream order: the caller's arrays are free again once these two have run */
        if (hipMemcpyAsync(m.block, d_pos, pos_bytes, hipMemcpyDeviceToDevice, s) != hipSuccess ||
            hipMemcpyAsync((char *)m.block + pos_room, d_idx, idx_bytes, hipMemcpyDeviceToDevice, s) != hipSuccess ||
            hipEventRecord(ev->ev, s) != hipSuccess) {
            const char *why = hipGetErrorString(hipGetLastError());
            (void)hipStreamSynchronize(s); (void)hipFree(m.block);
            return fail("lh_accel_add_mesh_device: copying the mesh failed: %s", why);
        }
    }
    a->dmeshes[a->ndmeshes++] = m;
    a->dmesh_tris += ntris;
    return 0;
}

/* 1 if the accelerator holds, or was committed from, device meshes (lh_multi.hip asks) */
extern "C" int lh_accel_device_meshes(const lh_accel_t *a) { return a && (a->ndmeshes || a->hs->device_meshes) ? 1 : 0; }

/* lh_accel_set_normals_device / lh_accel_set_attribute_device: slot `slot` of staged device mesh `mesh` becomes the library's own
 * copy of `count` elements of `ncomp` components (the caller's format and stride), enqueued on `stream`; d == NULL removes it.
 * Every refusal comes before anything is enqueued or changed */
static int set_dmesh_attr(lh_accel_t *a, const char *who, uint32_t mesh, int slot, uint32_t count, const void *d, int fmt, size_t stride,
                          const int *two_side, void *stream)
{
    if (a->commit_failed || (a->committed && !(a->updatable && a->ndmeshes))) return fail("%s: accel already committed", who);      /* an updatable accelerator stages them for lh_accel_recommit */
    if (!a->ndmeshes) return fail("%s: for device meshes (lh_accel_add_mesh_device); host meshes take %s", who,
                                  slot == LH_DATTR_NORMAL ? "lh_accel_set_normals" : "lh_accel_set_attribute");
    if (mesh >= a->ndmeshes) return fail("%s: mesh %u out of range", who, mesh);
    if (!two_side && (slot < LH_ATTR_COLOR || slot > LH_ATTR_TEXCOORD_UNSHARED)) return fail("%s: unknown attribute kind %d", who, slot);      /* two_side: the normals' call */
    lh_dmesh *m = &a->dmeshes[mesh];
    const uint32_t ncomp = (slot == LH_ATTR_TEXCOORD || slot == LH_ATTR_TEXCOORD_UNSHARED) ? 2u : 3u;
    const uint32_t need = slot == LH_ATTR_TEXCOORD_UNSHARED ? m->nidx : m->npos;
    size_t bytes = 0;
    if (d || count) {
        if (fmt != LH_POS_F64 && fmt != LH_POS_F32) return fail("%s: unknown format %d", who, fmt);
        const size_t elem = fmt == LH_POS_F32 ? sizeof(float) : sizeof(double);
        if (stride < ncomp * elem || (stride % elem) != 0) return fail("%s: bad stride %zu", who, stride);
        if (((uintptr_t)d % elem) != 0) return fail("%s: array not aligned to %zu bytes", who, elem);
        if (!d) return fail("%s: NULL array", who);
        bytes = count ? (size_t)(count - 1) * stride + ncomp * elem : 0;
        HIPCHK(hipSetDevice(a->device));
        if (bytes && lh_device_array_ok(a, d, bytes, who, "the array") != 0) return -1;
        if (count != need) return fail("%s: %u values given, the mesh needs %u (one per %s)", who, count, need,
                                       slot == LH_ATTR_TEXCOORD_UNSHARED ? "index" : "vertex");
    }
    if (d && a->committed && m->attr[slot].block && m->attr[slot].fmt == fmt && m->attr[slot].stride == stride && bytes) {
        /* staged after the commit in the format and stride of the block that is there (count == need: the same bytes): copied over it, as
         * lh_accel_update_mesh_device does -- no allocation, and no hipFree, which waits for the device */
        hipStream_t s = (hipStream_t)stream;
        lh_dmesh_event *ev = dmesh_event_of(a, s);
        if (!ev) return -1;
        if (hipMemcpyAsync(m->attr[slot].block, d, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess || hipEventRecord(ev->ev, s) != hipSuccess) {
            const char *why = hipGetErrorString(hipGetLastError());
            (void)hipStreamSynchronize(s);
            return fail("%s: copying the array failed: %s", who, why);
        }
        if (two_side) m->two_side = *two_side;
        a->staged_attr = 1;
        return 0;
    }
    lh_dmesh_attr n; memset(&n, 0, sizeof(n));
    if (d) {
        n.has = 1; n.fmt = fmt; n.stride = stride;
        if (m->ntris && bytes) {                        /* a mesh without triangles is never read */
            hipStream_t s = (hipStream_t)stream;
            lh_dmesh_event *ev = dmesh_event_of(a, s);
            if (!ev) return -1;
            HIPCHK(hipMalloc(&n.block, bytes));
            /* the library's own copy, in the caller's stream order: the caller's array is free again once it has run */
            if (hipMemcpyAsync(n.block, d, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess || hipEventRecord(ev->ev, s) != hipSuccess) {
                const char *why = hipGetErrorString(hipGetLastError());
                (void)hipStreamSynchronize(s); (void)hipFree(n.block);
                return fail("%s: copying the array failed: %s", who, why);
            }
        }
    }
    if (m->attr[slot].block) { (void)hipSetDevice(a->device); (void)hipFree(m->attr[slot].block); }      /* replaced or removed */
    m->attr[slot] = n;
    if (two_side) m->two_side = *two_side;
    if (a->committed) a->staged_attr = 1;
    return 0;
}

extern "C" int lh_accel_set_normals_device(lh_accel_t *a, uint32_t mesh, uint32_t nnormals, const void *d_normals, int fmt, size_t stride,
                                           int two_side, void *stream)
{
    lh_guard guard(a);
    if (!a) return fail("lh_accel_set_normals_device: accel is NULL");
    return set_dmesh_attr(a, "lh_accel_set_normals_device", mesh, LH_DATTR_NORMAL, nnormals, d_normals, fmt, stride, &two_side, stream);
}

extern "C" int lh_accel_set_attribute_device(lh_accel_t *a, uint32_t mesh, int kind, uint32_t count, const void *d_data, int fmt, size_t stride,
                                             void *stream)
{
    lh_guard guard(a);
    if (!a) return fail("lh_accel_set_attribute_device: accel is NULL");
    return set_dmesh_attr(a, "lh_accel_set_attribute_device", mesh, kind, count, d_data, fmt, stride, NULL, stream);
}

/* running triangle counts of the staged device meshes: first[g] = primitive id of mesh g's triangle 0, first[n] = all */
static uint32_t *dmesh_first_prim(const lh_accel_t *a)
{
    uint32_t *first = (uint32_t *)malloc(sizeof(uint32_t) * ((size_t)a->ndmeshes + 1));
    if (!first) return NULL;
    first[0] = 0;
    for (uint32_t g = 0; g < a->ndmeshes; g++) first[g + 1] = first[g] + a->dmeshes[g].ntris;
    return first;
}

/* lh_accel_prim_lookup's tables (and the materials' mesh ordinals) from the triangle counts alone */
static int dmesh_prim_tables(lh_host_scene *hs, const uint32_t *first, uint32_t nmeshes)
{
    const uint32_t n = first[nmeshes];
    free(hs->bvh.prim_geom); free(hs->bvh.prim_index); hs->bvh.prim_geom = hs->bvh.prim_index = NULL;
    if (n == 0) return 0;
    hs->bvh.prim_geom = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)n); hs->bvh.prim_index = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)n);
    if (!hs->bvh.prim_geom || !hs->bvh.prim_index) return fail("out of memory");
    for (uint32_t g = 0; g < nmeshes; g++)
        for (uint32_t p = first[g]; p < first[g + 1]; p++) { hs->bvh.prim_geom[p] = g; hs->bvh.prim_index[p] = 3 * (p - first[g]); }
    return 0;
}

/* the staged device meshes -> an array of triangle records of its own, *d_tri64 (a side's: the caller's to free, whatever is
 * returned), on the accelerator's stream, behind the copies the adds enqueued (an event per caller stream; no device-wide
 * synchronise).  Returns once the kernel's status word is back: an index out of range fails the commit */
static int flatten_device_meshes(lh_accel_t *a, const uint32_t *first, void **d_tri64, const char *who)
{
    const uint32_t nm = a->ndmeshes, nt = first[nm];
    const double t0 = now_s();
    HIPCHK(hipMalloc(d_tri64, sizeof(lh_tri64_t) * (size_t)nt));
    for (uint32_t k = 0; k < a->ndmesh_events; k++) HIPCHK(hipStreamWaitEvent(a->stream, a->dmesh_events[k].ev, 0));
    /* one block: the descriptors, the first_prim table, the status words */
    const size_t desc_bytes = sizeof(lh_dmesh_desc_t) * (size_t)nm, first_bytes = (sizeof(uint32_t) * ((size_t)nm + 1) + 15) & ~(size_t)15;
    std::vector<char> h(desc_bytes + first_bytes + 16, 0);
    lh_dmesh_desc_t *hd = (lh_dmesh_desc_t *)h.data();
    for (uint32_t g = 0; g < nm; g++) { hd[g].pos = a->dmeshes[g].pos; hd[g].idx = a->dmeshes[g].idx; hd[g].stride = a->dmeshes[g].stride; hd[g].npos = a->dmeshes[g].npos; hd[g].fmt = (uint32_t)a->dmeshes[g].fmt; }
    memcpy(h.data() + desc_bytes, first, sizeof(uint32_t) * ((size_t)nm + 1));
    char *d_tab = NULL; uint32_t status[4] = {0, 0, 0, 0};
    HIPCHK(hipMalloc((void **)&d_tab, h.size()));
    int rc = 0;
    if (hipMemcpyAsync(d_tab, h.data(), h.size(), hipMemcpyHostToDevice, a->stream) != hipSuccess) rc = fail("%s: uploading the mesh table failed", who);
    if (rc == 0) rc = lh_flatten_launch(nt, nm, (const lh_dmesh_desc_t *)d_tab, (const uint32_t *)(d_tab + desc_bytes), *d_tri64, (uint32_t *)(d_tab + desc_bytes + first_bytes), a->stream);
    if (rc == 0 && hipMemcpyAsync(status, d_tab + desc_bytes + first_bytes, sizeof(status), hipMemcpyDeviceToHost, a->stream) != hipSuccess) rc = fail("%s: reading the flatten status failed", who);
    const hipError_t es = hipStreamSynchronize(a->stream);
    (void)hipFree(d_tab);
    if (rc == 0 && es != hipSuccess) rc = fail("%s: flattening the device meshes failed: %s", who, hipGetErrorString(es));
    if (rc == 0 && status[0]) rc = fail("%s: mesh %u: index %u out of range (npositions %u)", who, status[1], status[2], status[3]);
    if (rc == 0 && getenv("LH_BUILD_TIMING")) fprintf(stderr, "[lucille_hip] commit: device flatten (%u meshes, %.0f MB) %8.2f ms\n", nm, sizeof(lh_tri64_t) * (double)nt / 1e6, (now_s() - t0) * 1e3);
    return rc;
}

/* the per-vertex normals and attributes of the staged device meshes -> arrays of their own, *o (a side's: the caller's to free,
 * whatever is returned), laid out as the nrm9 / attr9[] / st6 / inside a host scene uploads (device_upload): one kernel on the
 * accelerator's stream.  Called behind flatten_device_meshes, which has waited for the callers' copies and found every index in
 * range; an array no mesh contributes to stays NULL, a scene without any costs nothing here */
static int gather_device_attributes(lh_accel_t *a, const uint32_t *first, lh_gather_out_t *o, const char *who)
{
    memset(o, 0, sizeof(*o));
    const uint32_t nm = a->ndmeshes, nt = first[nm];
    bool any[LH_DATTR_SLOTS] = {false, false, false, false, false, false}, any_two = false, work = false;
    for (uint32_t g = 0; g < nm; g++) {
        for (int k = 0; k < LH_DATTR_SLOTS; k++) any[k] = any[k] || a->dmeshes[g].attr[k].has;
        any_two = any_two || a->dmeshes[g].two_side;
    }
    for (int k = 0; k < LH_DATTR_SLOTS; k++) work = work || any[k];
    if (nt == 0 || !(work || any_two)) return 0;
    const double t0 = now_s();
    if (any[LH_DATTR_NORMAL]) HIPCHK(hipMalloc((void **)&o->nrm9, sizeof(double) * 9 * (size_t)nt));
    for (int k = 0; k < 3; k++) if (any[k]) HIPCHK(hipMalloc((void **)&o->attr9[k], sizeof(double) * 9 * (size_t)nt));
    if (any[LH_ATTR_TEXCOORD] || any[LH_ATTR_TEXCOORD_UNSHARED]) HIPCHK(hipMalloc((void **)&o->st6, sizeof(double) * 6 * (size_t)nt));
    if (any_two) HIPCHK(hipMalloc((void **)&o->inside, (size_t)nt));
    const lh_gather_out_t out = *o;
    /* one block: the index descriptors, the attribute descriptors, the first_prim table */
    const size_t desc_bytes = sizeof(lh_dmesh_desc_t) * (size_t)nm, attr_bytes = sizeof(lh_dmesh_attr_desc_t) * (size_t)nm;
    std::vector<char> h(desc_bytes + attr_bytes + sizeof(uint32_t) * ((size_t)nm + 1), 0);
    lh_dmesh_desc_t *hd = (lh_dmesh_desc_t *)h.data();
    lh_dmesh_attr_desc_t *ha = (lh_dmesh_attr_desc_t *)(h.data() + desc_bytes);
    for (uint32_t g = 0; g < nm; g++) {
        const lh_dmesh *m = &a->dmeshes[g];
        hd[g].pos = m->pos; hd[g].idx = m->idx; hd[g].stride = m->stride; hd[g].npos = m->npos; hd[g].fmt = (uint32_t)m->fmt;
        for (int k = 0; k < LH_DATTR_SLOTS; k++) {
            ha[g].data[k] = m->attr[k].block; ha[g].stride[k] = m->attr[k].stride;
            if (m->attr[k].fmt == LH_POS_F32) ha[g].f32_mask |= 1u << k;
        }
        ha[g].two_side = m->two_side ? 1u : 0u; ha[g].nidx = m->nidx;
    }
    memcpy(h.data() + desc_bytes + attr_bytes, first, sizeof(uint32_t) * ((size_t)nm + 1));
    char *d_tab = NULL;
    HIPCHK(hipMalloc((void **)&d_tab, h.size()));
    int rc = 0;
    if (hipMemcpyAsync(d_tab, h.data(), h.size(), hipMemcpyHostToDevice, a->stream) != hipSuccess) rc = fail("%s: uploading the attribute table failed", who);
    if (rc == 0) rc = lh_gather_launch(nt, nm, (const lh_dmesh_desc_t *)d_tab, (const lh_dmesh_attr_desc_t *)(d_tab + desc_bytes),
                                       (const uint32_t *)(d_tab + desc_bytes + attr_bytes), out, a->stream);
    const hipError_t es = hipStreamSynchronize(a->stream);         /* the table is the host vector's until here */
    (void)hipFree(d_tab);
    if (rc == 0 && es != hipSuccess) rc = fail("%s: gathering the device meshes' attributes failed: %s", who, hipGetErrorString(es));
    if (rc == 0 && getenv("LH_BUILD_TIMING")) fprintf(stderr, "[lucille_hip] commit: device attribute gather      %8.2f ms\n", (now_s() - t0) * 1e3);
    return rc;
}

void lh_free_buf(lh_buf *b) { if (b->p) (void)hipFree(b->p); b->p = NULL; b->cap = 0; }
#define free_buf lh_free_buf

int lh_ensure_buf(lh_buf *b, size_t bytes)
{
    if (b->cap >= bytes && b->p) return 0;
    if (b->p) { (void)hipFree(b->p); b->p = NULL; b->cap = 0; }
    if (bytes == 0) bytes = 16;
    HIPCHK(hipMalloc(&b->p, bytes));
    b->cap = bytes;
    return 0;
}

int lh_stage_carve(lh_buf *block, lh_field_t *f, int nf)
{
    size_t total = 0;
    if (lh_stage_layout(f, nf, &total) != 0) return fail("a staging block of %d fields does not fit size_t", nf);
    if (lh_ensure_buf(block, total) != 0) return -1;
    lh_stage_place(f, nf, block->p);
    return 0;
}

/* the copies of one direction; a failure is reported (the first one of the call: lh_stage_down passes a failed device form through) and waited behind */
static int stage_copies(lh_accel_t *a, const lh_field_t *f, int nf, bool up, int rc)
{
    for (int k = 0; k < nf && rc == 0; k++) {
        if (!f[k].bytes || !(up ? f[k].up != NULL : f[k].down != NULL)) continue;
        const hipError_t e = up ? hipMemcpyAsync(f[k].dev, f[k].up, f[k].bytes, hipMemcpyHostToDevice, a->stream)
                                : hipMemcpyAsync(f[k].down, f[k].dev, f[k].bytes, hipMemcpyDeviceToHost, a->stream);
        if (e != hipSuccess) rc = fail("staging copy %s of field %d (%zu bytes) failed: %s", up ? "up" : "down", k, f[k].bytes, hipGetErrorString(e));
    }
    if (up && rc == 0) return 0;
    const hipError_t e = hipStreamSynchronize(a->stream);
    if (rc == 0 && e != hipSuccess) rc = fail("hipStreamSynchronize(a->stream) failed: %s", hipGetErrorString(e));
    return rc;
}

int lh_stage_up(lh_accel_t *a, lh_field_t *f, int nf)
{
    if (lh_stage_carve(&a->stage, f, nf) != 0) return -1;
    return stage_copies(a, f, nf, true, 0);
}

int lh_stage_down(lh_accel_t *a, const lh_field_t *f, int nf, int rc) { return stage_copies(a, f, nf, false, rc); }

/* the scene's device arrays, a row each: the slot of the accelerator that owns the array, its size, and whether it is there
 * -- as the image's header h says (a receiver, before it has allocated), else as the slot says.  The first LH_IMAGE_ROWS rows,
 * in this order, are the scene image: a wire format between ranks (lh_dist.hip) */
struct scene_row { void **slot; size_t bytes; bool present; };
#define LH_SCENE_ROWS 15
#define LH_IMAGE_ROWS 14          /* the 2-wide fp32 nodes (the textbook walk of a host-built scene) are never sent */
static void scene_rows(lh_accel_t *a, const lh_scene_image_t *h, scene_row r[LH_SCENE_ROWS])
{
    const lh_bvh_t *b = &a->hs->bvh;
    const size_t nt = b->ntris, rn = a->dev.ref_nnodes;
    int n = 0;
#define LH_ROW(SLOT, BYTES, IN_IMAGE) do { r[n].slot = &(SLOT); r[n].bytes = (BYTES); r[n].present = h ? (nt && (IN_IMAGE)) : (SLOT) != NULL; n++; } while (0)
    LH_ROW(a->d_tri32, sizeof(lh_tri32_t) * nt + 64, true);          /* the unified walk reads 16 B past a record */
    LH_ROW(a->d_tri64, sizeof(lh_tri64_t) * nt, true);
    LH_ROW(a->d_q4nodes, sizeof(lh_q4node_t) * (size_t)b->nq4nodes, true);
    LH_ROW(a->d_q8nodes, sizeof(lh_q8node_t) * (size_t)b->nq8nodes, h->nq8);
    LH_ROW(a->d_ref_lca, sizeof(int) * 4 * rn, h->have_ref);
    LH_ROW(a->d_prim_leafpos, sizeof(uint32_t) * 2 * nt, h->have_ref);
    LH_ROW(a->d_ref_nodes, sizeof(lh_refnode_t) * rn, h->have_ref);
    LH_ROW(a->d_ref_leaf_prims, sizeof(uint32_t) * nt, h->have_ref);
    LH_ROW(a->d_nrm9, sizeof(double) * 9 * nt, h->has_nrm);
    for (int k = 0; k < 3; k++) LH_ROW(a->d_attr9[k], sizeof(double) * 9 * nt, h->has_attr[k]);
    LH_ROW(a->d_st6, sizeof(double) * 6 * nt, h->has_st);
    LH_ROW(a->d_inside, nt, h->has_inside);
    LH_ROW(a->d_nodes, sizeof(lh_node_t) * (size_t)b->nnodes, false);
#undef LH_ROW
}

/* the resident scene of a->dev and the accelerator's byte count: the arrays from their owners, the rest from the host scene's
 * header.  Every path that adds, replaces or frees an array ends here; nothing else writes these fields.  (The header of
 * lucille's own tree is this replica's: publish_ref.) */
static void publish_scene(lh_accel_t *a)
{
    const lh_bvh_t *b = &a->hs->bvh; lh_dev_scene_t *d = &a->dev;
    d->nodes = a->d_nodes; d->tri32 = a->d_tri32; d->tri64 = a->d_tri64; d->q4nodes = a->d_q4nodes; d->q8nodes = a->d_q8nodes;
    d->ref_lca = a->d_ref_lca; d->prim_leafpos = a->d_prim_leafpos; d->ref_nodes = a->d_ref_nodes; d->ref_leaf_prims = a->d_ref_leaf_prims;
    d->ntris = b->ntris; d->nnodes = b->nnodes; d->max_depth = b->max_depth;
    d->nq4nodes = b->nq4nodes; d->q4_depth = b->q4_depth; d->q4_stack = b->q4_stack;
    assert((uint64_t)b->nq4nodes * sizeof(lh_q4node_t) < (1ull << 32));      /* node_step4 (lh_kernels.hip) addresses a node by a 32-bit byte offset from q4nodes */
    d->nq8nodes = a->d_q8nodes ? b->nq8nodes : 0u; d->q8_depth = a->d_q8nodes ? b->q8_depth : 0u;       /* the host scene's may be another replica's */
    d->scene_r = 0.0f;
    for (int k = 0; k < 3; k++) {
        d->grid_lo[k] = b->grid_lo[k]; d->grid_step[k] = b->grid_step[k];
        d->scene_r = fmaxf(d->scene_r, fmaxf(fabsf(b->bmin[k]), fabsf(b->bmax[k])));
    }
    d->deg_dcap = lh_dcap_device(b->deg_dcap);          /* lh_danger.h: rounded toward zero, never above the double the host walk compares with */
    d->cap_srcs = lh_dcap_srcs(b->deg_dcap);
    /* lh_accel_info's device_bytes.  A received scene counts the 64 bytes behind its triangle records, an uploaded or
     * device-built one does not: kept as it was, the figure is compared across versions */
    scene_row r[LH_SCENE_ROWS];
    scene_rows(a, NULL, r);
    a->device_bytes = 0;
    for (int k = 0; k < LH_SCENE_ROWS; k++) if (r[k].present) a->device_bytes += r[k].bytes;
    if (a->d_tri32 && !a->hs->received) a->device_bytes -= 64;
}

/* lucille's own tree is in a->d_ref_*: the header of this replica's copy (built here, the host scene's, or an image's) */
static void publish_ref(lh_accel_t *a, uint32_t nnodes, int empty, const double bmin[3], const double bmax[3])
{
    a->dev.ref_nnodes = nnodes; a->dev.ref_empty = empty;
    for (int k = 0; k < 3; k++) { a->dev.ref_bmin[k] = bmin[k]; a->dev.ref_bmax[k] = bmax[k]; }
    publish_scene(a);
}

/* a host array becomes one of the scene's device arrays (pad: bytes allocated behind it) */
static int upload_array(lh_accel_t *a, void **slot, const void *src, size_t bytes, size_t pad = 0)
{
    HIPCHK(hipMalloc(slot, bytes + pad));
    HIPCHK(hipMemcpy(*slot, src, bytes, hipMemcpyHostToDevice));
    publish_scene(a);
    return 0;
}

static void release_device(lh_accel_t *a)
{
    lh_buf *bufs[] = {&a->r_org, &a->r_dir, &a->r_prim, &a->r_t, &a->r_u, &a->r_v, &a->stage, &a->diag_drop,
                      &a->p_org2, &a->p_dir2, &a->p_path, &a->p_path2, &a->p_thr, &a->p_thr2, &a->p_rad, &a->p_counts, &a->p_value,
                      &a->p_value2, &a->p_key};
    for (size_t i = 0; i < sizeof(bufs) / sizeof(bufs[0]); i++) free_buf(bufs[i]);
    /* the gather stage's scratch table: every entry is lh_buf after lh_buf */
    static_assert(sizeof(a->gather) == sizeof(lh_buf) * LH_GATHER_BUFS * LH_GATHER_KINDS * 2, "lh_gather_scratch holds lh_buf members only");
    for (size_t i = 0; i < sizeof(a->gather) / sizeof(lh_buf); i++) free_buf((lh_buf *)a->gather + i);
    for (lh_buf *b : {&a->w_chain, &a->w_counts, &a->w_tile}) free_buf(b);
    if (a->d_total) (void)hipFree(a->d_total);
    scene_row rows[LH_SCENE_ROWS];
    scene_rows(a, NULL, rows);
    for (int k = 0; k < LH_SCENE_ROWS; k++) { if (*rows[k].slot) (void)hipFree(*rows[k].slot); *rows[k].slot = NULL; }
    publish_scene(a);
    if (a->d_prim_mesh) (void)hipFree(a->d_prim_mesh);
    if (a->d_materials) (void)hipFree(a->d_materials);
    if (a->d_env_map) (void)hipFree(a->d_env_map);
    a->d_prim_mesh = a->d_materials = a->d_env_map = NULL;
    free_buf(&a->r_bands); free_buf(&a->r_diag);
    if (a->h_read) { (void)hipHostFree(a->h_read); a->h_read = NULL; }
    a->d_total = NULL;
    if (a->d_danger) (void)hipFree(a->d_danger);
    a->d_danger = NULL; a->dev.ndanger = LH_DANGER_ALL;
    if (a->d_cursor) (void)hipFree(a->d_cursor);
    if (a->d_counters) (void)hipFree(a->d_counters);
    for (int k = 0; k < LH_AOQ_SLOTS; k++) {
        lh_fixq_t *q = &a->aoq[k].q;
        if (q->queue) {
            (void)hipFree(q->queue); (void)hipFree(q->qcount);
            (void)hipStreamDestroy((hipStream_t)q->aux_stream); (void)hipEventDestroy((hipEvent_t)q->ev_ready); (void)hipEventDestroy((hipEvent_t)q->ev_done);
        }
        memset(q, 0, sizeof(*q)); a->aoq[k].used = 0;
        free_buf(&a->aoq[k].order_ws);
    }
    if (a->pipe.ready) {
        for (int b = 0; b < a->pipe.depth; b++) {
            (void)hipHostFree(a->pipe.h_in[b]); (void)hipHostFree(a->pipe.h_out[b]);
            (void)hipFree(a->pipe.d_in[b]); (void)hipFree(a->pipe.d_out[b]);
            (void)hipEventDestroy(a->pipe.in_done[b]); (void)hipEventDestroy(a->pipe.done[b]);
        }
        for (int b = 0; b < 3; b++) (void)hipStreamDestroy(a->pipe.s[b]);
        a->pipe.ready = 0;
    }
    if (a->stream) (void)hipStreamDestroy(a->stream);
    a->d_cursor = a->d_counters = NULL;
    a->stream = NULL;
}

static void free_trash(lh_host_scene *hs)
{
    if (!hs->trash) return;
    for (uint32_t k = 0; k < hs->ntrash; k++) free(hs->trash[k]);
    free(hs->trash); hs->trash = NULL; hs->ntrash = 0;
}

static void *ref_thread_main(void *arg)
{
    lh_host_scene *hs = (lh_host_scene *)arg;
    const double t0 = now_s();
    free_trash(hs);
    if (hs->ref_on_device) { __atomic_store_n(&hs->ref_state, 0, __ATOMIC_RELEASE); return NULL; }       /* only the mesh copies to return */
    const int rc = lh_refbvh_build(&hs->ref, hs->bvh.tri64, hs->bvh.ntris, hs->ref_threads);
    hs->ref_build_seconds = now_s() - t0;
    __atomic_store_n(&hs->ref_state, rc == 0 ? 2 : -1, __ATOMIC_RELEASE);
    return NULL;
}

/* lh_bvh_build_hook's callback on the host path: the triangles are flattened, start lucille's own tree */
static void start_ref_thread(void *arg)
{
    lh_host_scene *hs = (lh_host_scene *)arg;
    if (hs->bvh.ntris == 0) return;
    hs->ref_state = 1;
    if (pthread_create(&hs->ref_thread, NULL, ref_thread_main, hs) != 0) { hs->ref_state = 0; return; }
    hs->ref_thread_live = 1;
}

/* ---- host build (once per scene) ------------------------------------------------------------ */
static int host_build(lh_accel_t *a, int build_threads, bool on_device, bool keep_meshes)
{
    lh_host_scene *hs = a->hs;
    if (build_threads <= 0) {
        /* LH_BUILD_THREADS: how a multi-process launcher (one rank per GPU) keeps N ranks from
         * oversubscribing the host N times over (lucille_amd/shard.py sets cores / world) */
        const char *e = getenv("LH_BUILD_THREADS");
        long nc = (e && atoi(e) > 0) ? atoi(e) : sysconf(_SC_NPROCESSORS_ONLN);
        build_threads = nc > 0 ? (int)nc : 1;
    }
    lh_mesh_view_t *views = (lh_mesh_view_t *)calloc(a->nmeshes ? a->nmeshes : 1, sizeof(*views));
    if (!views) return fail("out of memory");
    for (uint32_t g = 0; g < a->nmeshes; g++) {
        views[g].npositions = a->meshes[g].npos; views[g].positions = a->meshes[g].pos;
        views[g].stride_bytes = 3 * sizeof(double);
        views[g].nindices = a->meshes[g].nidx; views[g].indices = a->meshes[g].idx;
    }
    /* host build: lucille's own tree (needs only the flattened triangles) is built next to the traversal tree */
    {
        const char *e = getenv("LH_REFTREE");
        hs->have_ref = !(e && atoi(e) == 0);
        hs->ref_threads = build_threads;
    }
    const double tf = now_s();
    int rc = on_device ? lh_bvh_flatten(&hs->bvh, views, a->nmeshes, build_threads)
                       : lh_bvh_build_hook(&hs->bvh, views, a->nmeshes, build_threads, hs->have_ref ? start_ref_thread : NULL, hs);
    free(views);
    if (on_device && getenv("LH_BUILD_TIMING")) fprintf(stderr, "[lucille_hip] commit: host flatten                 %8.2f ms\n", (now_s() - tf) * 1e3);
    if (!on_device && hs->ref_thread_live) {           /* the host path returns with both trees */
        pthread_join(hs->ref_thread, NULL); hs->ref_thread_live = 0;
        if (rc == 0 && hs->ref_state != 2) return fail("lh_accel_commit: reference-order tree build failed (out of memory)");
    }
    hs->device_built = on_device ? 1 : 0;
    if (rc == -2) return fail("lh_accel_commit: a vertex coordinate is NaN, infinite or beyond 1e30");
    if (rc != 0) return fail("lh_accel_commit: BVH build failed (bad input or out of memory)");
    /* the reference-order tree: exact-t tie winners, the reference walk for fragile hits, beam
     * visibility (LH_REFTREE=0 skips it: ties then fall back to "larger primitive id wins",
     * fragile hits are not re-traced and beam queries are refused) */
    {
        const double t0 = now_s();
        if (hs->have_ref && on_device && hs->bvh.ntris) {
            /* not in front of the first frame: a background thread builds it, launch() attaches it when it is ready.  It is
             * started by lh_accel_commit AFTER the device has its scene (start_ref_background): its first phase streams the
             * same 1.5 GB the upload reads and would take a third of the host's memory bandwidth from it */
            hs->ref_threads = build_threads; hs->ref_state = 1;
        } else if (hs->ref_state != 2) {
            /* not started next to the tree build (an empty scene, or the thread could not be created): now */
            if (hs->have_ref && lh_refbvh_build(&hs->ref, hs->bvh.tri64, hs->bvh.ntris, build_threads) != 0)
                return fail("lh_accel_commit: reference-order tree build failed (out of memory)");
            hs->ref_build_seconds = now_s() - t0;
            hs->ref_state = hs->have_ref ? 2 : 0;
        }
    }
    /* per-primitive normals in primitive-id order, if any mesh carries normals */
    {
        bool any = false;
        for (uint32_t g = 0; g < a->nmeshes; g++) any = any || a->meshes[g].nrm != NULL;
        if (any && hs->bvh.ntris) {
            hs->nrm9 = (double *)malloc(sizeof(double) * 9 * (size_t)hs->bvh.ntris);
            if (!hs->nrm9) return fail("out of memory");
            for (uint32_t p = 0; p < hs->bvh.ntris; p++) {
                const lh_mesh_copy *m = &a->meshes[hs->bvh.prim_geom[p]];
                double *o = hs->nrm9 + 9 * (size_t)p;
                if (!m->nrm) { for (int k = 0; k < 9; k++) o[k] = NAN; continue; }
                for (int c = 0; c < 3; c++) {
                    uint32_t vi = m->idx[hs->bvh.prim_index[p] + c];
                    for (int k = 0; k < 3; k++) o[3 * c + k] = m->nrm[3 * (size_t)vi + k];
                }
            }
        }
    }
    /* the packed mesh copies are no longer needed: the BVH holds tri64 */
    /* the other per-vertex attributes ri_intersection_state_build reads, flattened the same way */
    {
        const uint32_t n = hs->bvh.ntris;
        hs->nmeshes = a->nmeshes;
        for (int kind = 0; kind < 3 && n; kind++) {
            bool anyk = false;
            for (uint32_t g = 0; g < a->nmeshes; g++) anyk = anyk || a->meshes[g].attr[kind] != NULL;
            if (!anyk) continue;
            hs->attr9[kind] = (double *)malloc(sizeof(double) * 9 * (size_t)n);
            if (!hs->attr9[kind]) return fail("out of memory");
            for (uint32_t p = 0; p < n; p++) {
                const lh_mesh_copy *m = &a->meshes[hs->bvh.prim_geom[p]];
                double *o = hs->attr9[kind] + 9 * (size_t)p;
                if (!m->attr[kind]) { for (int k = 0; k < 9; k++) o[k] = NAN; continue; }
                for (int c = 0; c < 3; c++) {
                    const uint32_t vi = m->idx[hs->bvh.prim_index[p] + c];
                    for (int k = 0; k < 3; k++) o[3 * c + k] = m->attr[kind][3 * (size_t)vi + k];
                }
            }
        }
        bool any_st = false, any_two = false;
        for (uint32_t g = 0; g < a->nmeshes; g++) { any_st = any_st || a->meshes[g].attr[3] || a->meshes[g].attr[4]; any_two = any_two || a->meshes[g].two_side; }
        if (any_st && n) {
            hs->st6 = (double *)malloc(sizeof(double) * 6 * (size_t)n);
            if (!hs->st6) return fail("out of memory");
            for (uint32_t p = 0; p < n; p++) {
                const lh_mesh_copy *m = &a->meshes[hs->bvh.prim_geom[p]];
                double *o = hs->st6 + 6 * (size_t)p;
                const uint32_t first = hs->bvh.prim_index[p];
                if (m->attr[3]) {                 /* shared: geom->texcoords[2 * i_c] (intersection_state.c:210-216) */
                    for (int c = 0; c < 3; c++) { const uint32_t vi = m->idx[first + c]; o[2 * c] = m->attr[3][2 * (size_t)vi]; o[2 * c + 1] = m->attr[3][2 * (size_t)vi + 1]; }
                } else if (m->attr[4]) {          /* unshared: geom->texcoords_unshared[2 * (index + c)] (:218-224) */
                    for (int c = 0; c < 3; c++) { o[2 * c] = m->attr[4][2 * (size_t)(first + c)]; o[2 * c + 1] = m->attr[4][2 * (size_t)(first + c) + 1]; }
                } else for (int k = 0; k < 6; k++) o[k] = NAN;
            }
        }
        if (any_two && n) {
            hs->inside = (uint8_t *)calloc(n, 1);
            if (!hs->inside) return fail("out of memory");
            for (uint32_t p = 0; p < n; p++) {
                const lh_mesh_copy *m = &a->meshes[hs->bvh.prim_geom[p]];
                hs->inside[p] = (m->two_side && hs->bvh.prim_index[p] >= m->nidx / 2) ? 1 : 0;
            }
        }
    }
    if (!keep_meshes) {
        for (uint32_t g = 0; g < a->nmeshes; g++) {
            free(a->meshes[g].pos); free(a->meshes[g].idx); free(a->meshes[g].nrm);
            for (int k = 0; k < 5; k++) free(a->meshes[g].attr[k]);
        }
        free(a->meshes); a->meshes = NULL; a->nmeshes = 0;
    }
    return 0;
}

extern "C" int lh_device_build(uint32_t ntris, const double *d_tri64, void **d_q4nodes, uint32_t *nq4, uint32_t *q4_depth, uint32_t *q4_stack,
                               int want_q8, void **d_q8nodes, uint32_t *nq8, uint32_t *q8_depth,
                               void **d_tri32, float bmin[3], float bmax[3], float grid_lo[3], float grid_step[3],
                               uint32_t *nlive, double *deg_dcap, void *stream, char *err, size_t errlen);                /* lh_build.hip */

/* flag = 1 if the two word arrays differ anywhere */
__global__ void k_words_differ(size_t nwords, const uint32_t *__restrict__ x, const uint32_t *__restrict__ y, int *__restrict__ flag)
{
    bool diff = false;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += (size_t)gridDim.x * blockDim.x) diff |= x[i] != y[i];
    if (__ballot(diff) != 0ull && (threadIdx.x & 63) == 0) atomicExch(flag, 1);
}

/* *diff: the two arrays of nwords words differ somewhere (what: the comparison, for the error text) */
static int words_differ(lh_accel_t *a, const void *x, const void *y, size_t nwords, bool *diff, const char *what)
{
    int *flag = NULL, h_flag = 0;
    HIPCHK(hipMalloc((void **)&flag, sizeof(int)));
    int rc = 0;
    if (hipMemsetAsync(flag, 0, sizeof(int), a->stream) != hipSuccess) rc = fail("%s failed", what);
    if (rc == 0) {
        hipLaunchKernelGGL(k_words_differ, dim3(2048), dim3(256), 0, a->stream, nwords, (const uint32_t *)x, (const uint32_t *)y, flag);
        if (hipMemcpyAsync(&h_flag, flag, sizeof(int), hipMemcpyDeviceToHost, a->stream) != hipSuccess || hipStreamSynchronize(a->stream) != hipSuccess)
            rc = fail("%s failed: %s", what, hipGetErrorString(hipGetLastError()));
    }
    (void)hipFree(flag);
    *diff = h_flag != 0;
    return rc;
}

extern "C" int lh_device_ref_build(uint32_t ntris, const double *d_tri64, void **d_nodes, uint32_t *nnodes, uint32_t *max_depth,
                                   void **d_leaf_prims, void **d_lca, void **d_leafpos, double scene6[6], void *stream, char *err, size_t errlen);   /* lh_refbuild.hip */

/* ---- the leaves of lucille's own tree that hold a zero-area triangle (round 6; lh_bvh.h ndanger / danger, lh_walk.h danger_hit) ----
 * A numerically collinear triangle that stays in the traversal tree caps the directions the tree can vouch for at 1 / s2 (lh_bvh.c
 * tri_zero_area_s2) -- below 1 as soon as |e1|_1 |e2|_1 > 1, i.e. for ANY such sliver in a scene modelled in small units -- and every
 * ray beyond the cap used to take the single-lane reference walk: correct, and a hundred times slower.  The reference
 * can "hit" such a triangle only on rays that reach its leaf, so once lucille's own tree is on the device this scan lists the
 * boxes of those leaves (the child box the leaf's parent holds: what test_ray_node tests, bvh.c:938-1083); rays that miss them all
 * walk the traversal tree like any other.  More than LH_DANGER_MAX of them: every ray, as before. */
__global__ __launch_bounds__(256) void k_danger_scan(uint32_t n, const double *__restrict__ tri64, const uint2 *__restrict__ leafpos, const int4 *__restrict__ lca,
                                                     const lh_refnode_t *__restrict__ nodes, double s0, double s1, double s2_, double s3, double s4, double s5,
                                                     unsigned long long *__restrict__ count, double *__restrict__ boxes)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const double *t = tri64 + 9 * (size_t)p;
    /* tri_dead_class (lh_bvh.c): out of the traversal tree, never reported below LH_DEG_DCAP_ALL */
    if ((t[0] == t[3] && t[1] == t[4] && t[2] == t[5]) || (t[0] == t[6] && t[1] == t[7] && t[2] == t[8])) return;
    if (t[3] == t[6] && t[4] == t[7] && t[5] == t[8]) {
        const double sN = fabs(t[3] - t[0]) + fabs(t[4] - t[1]) + fabs(t[5] - t[2]);
        if (sN * sN * (1.0 + 1e-9) <= 1.0e-14 / (1.0e-15 * LH_DEG_DCAP_ALL)) return;
    }
    if (!(lh_zero_area_weight(t, t + 3, t + 6) > 0.0)) return;          /* lh_bvh.h: the triangles lh_bvh.c tri_zero_area_s2 / lh_build.hip k_prim_boxes bound deg_dcap with */
    const unsigned long long slot = atomicAdd(count, 1ull);
    if (slot >= LH_DANGER_MAX) return;
    const int leaf = (int)leafpos[p].x, parent = lca[leaf].x;
    double *o = boxes + 6 * slot;
    if (parent < 0) { o[0] = s0; o[1] = s1; o[2] = s2_; o[3] = s3; o[4] = s4; o[5] = s5; return; }       /* the root is the leaf: the scene box (bvh.c:325-340) */
    const int k = (lca[parent].w == leaf) ? 0 : 1;          /* children are allocated adjacently: child[1] = child[0] + 1 */
    for (int q = 0; q < 6; q++) o[q] = nodes[parent].box[k][q];
}

/* what a scan found: the list the one-ray host walk reads (nhost boxes; LH_DANGER_ALL: none, every ray beyond the cap) and the device's one box (ndev, words) */
struct lh_danger_found { uint32_t nhost, ndev, words[3]; double boxes[6 * LH_DANGER_MAX]; };

/* the scan over arrays that need not be the resident scene's (a re-commit's stand beside it): n triangle records, lucille's own tree over them and
 * its box, the cap and the 16-bit grid of the traversal tree built from the same records.  a->d_danger is its scratch; nothing of the scene is written */
static int danger_scan_arrays(lh_accel_t *a, uint32_t n, double deg_dcap, const void *tri64, const void *leafpos, const void *lca, const void *nodes,
                              const double rbmin[3], const double rbmax[3], const float grid_lo[3], const float grid_step[3], lh_danger_found *o)
{
    o->nhost = o->ndev = LH_DANGER_ALL;
    if (!nodes || !tri64 || n == 0) return 0;
    if (!(deg_dcap < LH_DEG_DCAP_ALL)) return 0;              /* no zero-area triangle in the tree caps the directions: nothing to list */
    if (getenv("LH_DANGER_BOXES") && atoi(getenv("LH_DANGER_BOXES")) == 0) return 0;       /* A/B: round 5's rule (every ray beyond the cap) */
    HIPCHK(hipSetDevice(a->device));
    if (!a->d_danger) HIPCHK(hipMalloc(&a->d_danger, sizeof(double) * (8 + 6 * LH_DANGER_MAX)));
    HIPCHK(hipMemsetAsync(a->d_danger, 0, sizeof(double) * (8 + 6 * LH_DANGER_MAX), a->stream));
    hipLaunchKernelGGL(k_danger_scan, dim3((n + 255u) / 256u), dim3(256), 0, a->stream, n, (const double *)tri64, (const uint2 *)leafpos,
                       (const int4 *)lca, (const lh_refnode_t *)nodes, rbmin[0], rbmin[1], rbmin[2],
                       rbmax[0], rbmax[1], rbmax[2], (unsigned long long *)a->d_danger, (double *)a->d_danger + 8);
    HIPCHK(hipGetLastError());
    double h[8 + 6 * LH_DANGER_MAX];
    HIPCHK(hipMemcpyAsync(h, a->d_danger, sizeof(h), hipMemcpyDeviceToHost, a->stream));
    HIPCHK(hipStreamSynchronize(a->stream));
    unsigned long long cnt; memcpy(&cnt, h, sizeof(cnt));
    if (cnt == 0 || cnt > LH_DANGER_MAX) return 0;                      /* none found (the cap came from somewhere else: keep round 5's rule) or too many */
    memcpy(o->boxes, h + 8, sizeof(double) * 6 * (size_t)cnt);
    o->nhost = (uint32_t)cnt;
    /* the union of the listed boxes on the scene's 16-bit grid, a cell wider on every side (the nodes' own boxes are rounded outward
     * the same way: lh_bvh.c).  A union that leaves the grid on any side (a leaf that also holds a triangle outside the traversal
     * tree's bounds, however little outside): round 5's rule (lh_danger.h lh_danger_pack) */
    double u[6] = {1.0e308, 1.0e308, 1.0e308, -1.0e308, -1.0e308, -1.0e308};
    for (unsigned long long i = 0; i < cnt; i++)
        for (int k = 0; k < 3; k++) { u[k] = fmin(u[k], h[8 + 6 * i + k]); u[3 + k] = fmax(u[3 + k], h[8 + 6 * i + 3 + k]); }
    if (!lh_danger_pack(u, grid_lo, grid_step, o->words)) return 0;
    o->ndev = (uint32_t)cnt;
    return 0;
}

/* a danger list becomes the accelerator's: the one a side brings (side_install), or -- none brought -- the one a scan of the resident scene finds
 * now that lucille's own tree has arrived from somewhere else: the host thread (attach_ref), another rank (lh_scene_image_finish).  The host list
 * is written only over LH_DANGER_ALL: the first replica of a shared host scene writes it, the others found the same one */
static int lh_danger_scan(lh_accel_t *a, const lh_danger_found *brought = NULL)
{
    lh_bvh_t *b = &a->hs->bvh; lh_danger_found f; int rc = 0;
    if (brought) f = *brought;          /* (a scan that fails finds LH_DANGER_ALL) */
    else rc = danger_scan_arrays(a, b->ntris, b->deg_dcap, a->d_tri64, a->d_prim_leafpos, a->d_ref_lca, a->d_ref_nodes, a->dev.ref_bmin, a->dev.ref_bmax, b->grid_lo, b->grid_step, &f);
    pthread_mutex_lock(&g_scene_mu);
    if (b->ndanger == LH_DANGER_ALL && f.nhost != LH_DANGER_ALL) {
        memcpy(b->danger, f.boxes, sizeof(double) * 6 * (size_t)f.nhost);
        __atomic_store_n(&b->ndanger, f.nhost, __ATOMIC_RELEASE);      /* the one-ray host walk reads it (lh_hostwalk.c) */
    }
    pthread_mutex_unlock(&g_scene_mu);
    a->dev.ndanger = f.ndev;
    for (int k = 0; k < 3; k++) a->dev.danger[k] = f.ndev != LH_DANGER_ALL ? f.words[k] : 0u;
    return rc;
}

/* a side: everything the device builders make of a scene, owned by nobody until side_install makes it the accelerator's -- the arrays of scene_rows
 * a device build fills and what goes into the headers for them.  A first commit's stands beside an empty scene, a re-commit's beside the resident one */
struct lh_side {
    void *tri64, *tri32, *q4, *q8, *ref_nodes, *ref_leaf_prims, *ref_lca, *leafpos;
    lh_gather_out_t attr; int gathered;          /* gathered: attr is what the meshes have now, its NULLs included */
    uint32_t nq4, d4, st4, nq8, d8, nlive, ref_nnodes; double dcap, sc6[6], build_seconds, ref_seconds;
    float bmin[3], bmax[3], glo[3], gst[3];
    lh_danger_found danger;
};

static void side_free(lh_side *s)
{
    void *p[] = {s->tri64, s->tri32, s->q4, s->q8, s->ref_nodes, s->ref_leaf_prims, s->ref_lca, s->leafpos,
                 s->attr.nrm9, s->attr.attr9[0], s->attr.attr9[1], s->attr.attr9[2], s->attr.st6, s->attr.inside};
    for (size_t k = 0; k < sizeof(p) / sizeof(p[0]); k++) if (p[k]) (void)hipFree(p[k]);
    memset(s, 0, sizeof(*s));
}

/* the one run of the device builders: from nt > 0 triangle records (the side's own, or resident ones) the traversal tree and tri32 (lh_build.hip), with
 * the 8-wide nodes if want_q8, then -- own_tree -- lucille's own tree (lh_refbuild.hip) and the danger list.  Nothing of the accelerator is written but
 * its scratch; whatever the outcome the side (zeroed by its owner: no danger list is LH_DANGER_ALL) owns what was allocated, and err says what a builder said (a failed scan: lh_last_error()).  What follows: lh_route.h */
static lh_side_outcome_t side_build(lh_accel_t *a, lh_side *s, const void *tri64, uint32_t nt, int want_q8, bool own_tree, char *err, size_t errlen)
{
    const double tb = now_s();
    const int rcb = lh_device_build(nt, (const double *)tri64, &s->q4, &s->nq4, &s->d4, &s->st4, want_q8, &s->q8, &s->nq8, &s->d8, &s->tri32, s->bmin, s->bmax, s->glo, s->gst,
                                    &s->nlive, &s->dcap, (void *)a->stream, err, errlen);
    if (rcb != 0) return rcb == -2 ? LH_SIDE_BAD_VERTEX : LH_SIDE_BUILDER_FAILED;
    s->build_seconds = now_s() - tb;
    /* deeper than k_overflow_fix's private stack (LH_BUILD_DEPTH_MAX: 3 d + 5 <= 264 rows; "build_depth_cap" lowers it) */
    if (s->d4 > (uint32_t)a->build_depth_cap) { snprintf(err, errlen, "a tree of %u levels, the walks' stacks take %d", s->d4, a->build_depth_cap); return LH_SIDE_TOO_DEEP; }
    if ((uint64_t)s->nq4 * sizeof(lh_q4node_t) >= (1ull << 32)) { snprintf(err, errlen, "more 4-wide nodes than a 32-bit byte offset addresses"); return LH_SIDE_TOO_MANY_NODES; }
    if (!own_tree) return LH_SIDE_BUILT;
    const double tr = now_s(); uint32_t rdepth = 0;
    if (lh_device_ref_build(nt, (const double *)tri64, &s->ref_nodes, &s->ref_nnodes, &rdepth, &s->ref_leaf_prims, &s->ref_lca, &s->leafpos, s->sc6,
                            (void *)a->stream, err, errlen) != 0) {
        s->ref_nodes = s->ref_leaf_prims = s->ref_lca = s->leafpos = NULL;          /* the builder freed them */
        return LH_SIDE_REF_FAILED;
    }
    s->ref_seconds = now_s() - tr;
    if (danger_scan_arrays(a, nt, s->dcap, tri64, s->leafpos, s->ref_lca, s->ref_nodes, s->sc6, s->sc6 + 3, s->glo, s->gst, &s->danger) != 0) return LH_SIDE_SCAN_FAILED;
    return LH_SIDE_BUILT;
}

/* the side becomes the scene: whichever of its parts it holds -- the triangle records; the trees (tri32, the 4-wide nodes, lucille's own tree and the
 * danger list, if they were built); the 8-wide nodes; the gathered attribute arrays -- change places with the accelerator's, their header fields are
 * written, the scene is published, and what was displaced is freed with the side.  Nothing else writes the header fields a device build produces.
 * The caller has made sure no launch reads what is displaced (a first commit displaces nothing) */
static void side_install(lh_accel_t *a, lh_side *s)
{
    lh_host_scene *hs = a->hs; lh_bvh_t *b = &hs->bvh;
    auto put = [](void **slot, void **p) { void *was = *slot; *slot = *p; *p = was; };
    const bool trees = s->q4 != NULL, own_tree = s->ref_nodes != NULL;
    if (s->tri64) put(&a->d_tri64, &s->tri64);
    pthread_mutex_lock(&g_scene_mu);
    if (trees) {
        b->nq4nodes = s->nq4; b->q4_depth = s->d4; b->q4_stack = s->st4; b->nnodes = s->nq4; b->max_depth = s->d4; b->build_seconds = s->build_seconds;
        b->nlive = s->nlive; b->deg_dcap = s->dcap;
        for (int k = 0; k < 3; k++) { b->bmin[k] = s->bmin[k]; b->bmax[k] = s->bmax[k]; b->grid_lo[k] = s->glo[k]; b->grid_step[k] = s->gst[k]; }
        put(&a->d_tri32, &s->tri32); put(&a->d_q4nodes, &s->q4);
        put(&a->d_ref_nodes, &s->ref_nodes); put(&a->d_ref_leaf_prims, &s->ref_leaf_prims); put(&a->d_ref_lca, &s->ref_lca); put(&a->d_prim_leafpos, &s->leafpos);
        a->hw_ns = 0.0; a->hw_gpu_left = 0;
    }
    if (s->q8 || (trees && a->d_q8nodes)) { b->nq8nodes = s->q8 ? s->nq8 : 0u; b->q8_depth = s->q8 ? s->d8 : 0u; }          /* none made, none displaced: the fields stay, the host scene's may be another replica's */
    if (own_tree) { hs->ref_on_device = 1; hs->ref_build_seconds = s->ref_seconds; }
    pthread_mutex_unlock(&g_scene_mu);
    if (trees) (void)lh_danger_scan(a, &s->danger);
    if (own_tree) publish_ref(a, s->ref_nnodes, 0, s->sc6, s->sc6 + 3);
    if (trees || s->q8) put(&a->d_q8nodes, &s->q8);
    if (s->gathered) {
        put(&a->d_nrm9, (void **)&s->attr.nrm9); put(&a->d_st6, (void **)&s->attr.st6); put(&a->d_inside, (void **)&s->attr.inside);
        for (int k = 0; k < 3; k++) put(&a->d_attr9[k], (void **)&s->attr.attr9[k]);
    }
    publish_scene(a);
    side_free(s);
}

/* the 8-wide nodes of a scene whose tree was built on this device without them: the build is run once more (it is
 * deterministic: stable sort, stable partitions, a layout of the top that does not depend on its threads) and only its 8-wide
 * collapse is kept.  The leaves of those nodes index the resident triangle records, so the second run's records must be the
 * resident ones word for word -- checked, not assumed */
static int device_rebuild_q8(lh_accel_t *a)
{
    lh_host_scene *hs = a->hs;
    char err[256] = "";
    lh_side s; memset(&s, 0, sizeof(s));
    const lh_side_outcome_t o = side_build(a, &s, a->d_tri64, hs->bvh.ntris, 1, false, err, sizeof(err));
    /* too deep: as deep as the resident tree, which a commit accepted ("build_depth_cap" may have been lowered since) */
    if (o != LH_SIDE_BUILT && o != LH_SIDE_TOO_DEEP) { side_free(&s); return fail("building the 8-wide nodes on the device failed: %s", err); }
    int rc = 0; bool diff = false;
    if (s.q8) {
        rc = words_differ(a, s.tri32, a->d_tri32, sizeof(lh_tri32_t) / 4 * (size_t)hs->bvh.ntris, &diff, "comparing the rebuilt triangle order");
        if (rc == 0 && (diff || s.nq4 != hs->bvh.nq4nodes))
            rc = fail("the device build did not repeat itself (%u nodes, then %u): the 8-wide nodes are not usable; set \"wide8\" = 1 before the commit", hs->bvh.nq4nodes, s.nq4);
    }
    (void)hipFree(s.q4); (void)hipFree(s.tri32); s.q4 = s.tri32 = NULL;          /* only the 8-wide nodes are kept */
    if (rc != 0) { side_free(&s); return -1; }
    side_install(a, &s);
    return 0;
}

int lh_ensure_formats(lh_accel_t *a, int mask)
{
    const lh_bvh_t *b = &a->hs->bvh;
    if ((mask & LH_FMT_Q8) && !a->d_q8nodes && a->hs->device_built && !a->hs->received && b->nq4nodes > 1 && device_rebuild_q8(a) != 0) return -1;
    if ((mask & LH_FMT_Q8) && !a->d_q8nodes && !a->hs->device_built) {
        /* the 8-wide 16-bit-grid nodes for ray dumps over scenes larger than the Infinity Cache: built on first use */
        pthread_mutex_lock(&g_scene_mu);
        const int rc8 = lh_bvh_ensure_q8(&a->hs->bvh);
        pthread_mutex_unlock(&g_scene_mu);
        if (rc8 != 0) return fail("building the 8-wide tree failed (out of memory)");
        if (upload_array(a, &a->d_q8nodes, b->q8nodes, sizeof(lh_q8node_t) * (size_t)b->nq8nodes) != 0) return -1;
    }
    if (a->hs->device_built) return 0;         /* the tree exists only as 4-wide nodes on the device */
    if ((mask & LH_FMT_F32) && !a->d_nodes && upload_array(a, &a->d_nodes, b->nodes, sizeof(lh_node_t) * (size_t)b->nnodes) != 0) return -1;
    if ((mask & LH_FMT_Q16X4) && !a->d_q4nodes && upload_array(a, &a->d_q4nodes, b->q4nodes, sizeof(lh_q4node_t) * (size_t)b->nq4nodes) != 0) return -1;
    return 0;
}

/* the reference-order tree of the host scene onto this replica's device (exact-t tie winners, the reference walk for
 * fragile hits, beams).  With a device-built traversal tree this happens when the background build has finished. */
static int attach_ref(lh_accel_t *a)
{
    lh_host_scene *hs = a->hs;
    if (a->d_ref_nodes || !hs->have_ref || hs->bvh.ntris == 0) return 0;
    {
        const uint32_t rn = hs->ref.nnodes;
        int *lca = (int *)malloc(sizeof(int) * 4 * (size_t)rn);
        uint32_t *lp = (uint32_t *)malloc(sizeof(uint32_t) * 2 * (size_t)hs->bvh.ntris);
        if (!lca || !lp) { free(lca); free(lp); return fail("out of memory"); }
        for (uint32_t i = 0; i < rn; i++) {
            lca[4 * i] = hs->ref.nodes[i].parent; lca[4 * i + 1] = hs->ref.nodes[i].depth;
            lca[4 * i + 2] = hs->ref.nodes[i].axis; lca[4 * i + 3] = hs->ref.nodes[i].child[0];
        }
        for (uint32_t p = 0; p < hs->bvh.ntris; p++) { lp[2 * p] = hs->ref.prim_leaf[p]; lp[2 * p + 1] = hs->ref.prim_pos[p]; }
        const size_t nt = hs->bvh.ntris;
        const bool ok = upload_array(a, &a->d_ref_lca, lca, sizeof(int) * 4 * (size_t)rn) == 0 && upload_array(a, &a->d_prim_leafpos, lp, sizeof(uint32_t) * 2 * nt) == 0 &&
                        upload_array(a, &a->d_ref_nodes, hs->ref.nodes, sizeof(lh_refnode_t) * (size_t)rn) == 0 && upload_array(a, &a->d_ref_leaf_prims, hs->ref.leaf_prims, sizeof(uint32_t) * nt) == 0;
        free(lca); free(lp);
        if (!ok) return fail("reference-order tree upload failed");
        publish_ref(a, rn, hs->ref.empty, hs->ref.bmin, hs->ref.bmax);
    }
    return lh_danger_scan(a);
}

/* the background build of the reference-order tree: attach it if it has finished (wait: block until it has) */
int lh_sync_ref(lh_accel_t *a, bool wait)
{
    lh_host_scene *hs = a->hs;
    if (!hs->have_ref || a->d_ref_nodes || hs->bvh.ntris == 0) return 0;
    if (wait) {
        pthread_mutex_lock(&g_scene_mu);
        if (hs->ref_thread_live) { pthread_join(hs->ref_thread, NULL); hs->ref_thread_live = 0; }
        pthread_mutex_unlock(&g_scene_mu);
    }
    const int st = __atomic_load_n(&hs->ref_state, __ATOMIC_ACQUIRE);
    if (st == -1) return fail("the reference-order tree build failed (out of memory)");
    if (st != 2) return 0;
    HIPCHK(hipSetDevice(a->device));
    return attach_ref(a);
}

/* persistent workgroups per launch: as many as the LDS stack rows of this scene let a CU hold -- at most 4: the walk's 128 VGPRs */
static int size_grid(lh_accel_t *a)
{
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, a->device));
    const int per_cu = (int)lh_plan_wgs_per_cu((uint32_t)lh_trace_rows(&a->dev));          /* lh_plan.h: what the top-of-tree copy counts on; at least 2 (64 rows at most) */
    a->grid_blocks = prop.multiProcessorCount * per_cu; a->ncus = prop.multiProcessorCount;
    const char *env = getenv("LH_GRID_BLOCKS");
    if (env && atoi(env) > 0) { a->grid_blocks = atoi(env); a->grid_user = 1; }
    return 0;
}

/* what an accelerator launches with whatever its scene came from: its stream, the cursor blocks, the counters */
static int device_begin(lh_accel_t *a)
{
    HIPCHK(hipSetDevice(a->device));
    HIPCHK(hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking));
    HIPCHK(hipMalloc((void **)&a->d_cursor, sizeof(uint32_t) * LH_CURSOR_WORDS * LH_NCURSOR));
    HIPCHK(hipMalloc((void **)&a->d_counters, sizeof(unsigned long long) * LH_CNT_DEV));
    HIPCHK(hipMalloc((void **)&a->d_total, sizeof(unsigned long long) * 72));      /* the hit count of a batch; then k_ao_resolve's 64 occlusion counters; [64]: the hit count kept for the fused AO stage and the batch's one read-back */
    return 0;
}

/* ---- device replica of the host scene (once per GPU) ---------------------------------------- */
static int dmesh_host_fallback(lh_accel_t *a, const uint32_t *first, uint32_t nm, lh_side *s);
/* LH_ROUTE_INSTALL: committed.  LH_ROUTE_HOST_BUILDERS: the device builders were given up and the caller builds from its host arrays; device
 * meshes (dmesh_first: their first_prim table) have none and take dmesh_host_fallback from here, with the side */
static lh_route_t device_upload(lh_accel_t *a, lh_side_builder_t who, const uint32_t *dmesh_first = NULL)
{
    lh_host_scene *hs = a->hs;
    const double t0 = now_s();
    if (device_begin(a) != 0) return LH_ROUTE_ERROR;
    const size_t nt = hs->bvh.ntris;
    if (hs->nrm9 && upload_array(a, &a->d_nrm9, hs->nrm9, sizeof(double) * 9 * nt) != 0) return LH_ROUTE_ERROR;
    for (int kind = 0; kind < 3; kind++)
        if (hs->attr9[kind] && upload_array(a, &a->d_attr9[kind], hs->attr9[kind], sizeof(double) * 9 * nt) != 0) return LH_ROUTE_ERROR;
    if (hs->st6 && upload_array(a, &a->d_st6, hs->st6, sizeof(double) * 6 * nt) != 0) return LH_ROUTE_ERROR;
    if (hs->inside && upload_array(a, &a->d_inside, hs->inside, nt) != 0) return LH_ROUTE_ERROR;
    if (hs->bvh.ntris) {
        lh_side s; memset(&s, 0, sizeof(s));          /* a device-built scene is made aside: installed whole, or freed */
        const bool timing = getenv("LH_BUILD_TIMING") != NULL;
        const size_t t64 = sizeof(lh_tri64_t) * nt;
        const double tu = now_s();
        lh_route_t r = LH_ROUTE_INSTALL;
        if (who == LH_FOR_DEVICE_MESHES) {          /* the records are made here, nothing crosses the link */
            if (flatten_device_meshes(a, dmesh_first, &s.tri64, "lh_accel_commit") != 0 || gather_device_attributes(a, dmesh_first, &s.attr, "lh_accel_commit") != 0) r = LH_ROUTE_ERROR;
            s.gathered = 1;
        } else if (upload_array(a, hs->device_built ? &s.tri64 : &a->d_tri64, hs->bvh.tri64, t64) != 0) r = LH_ROUTE_ERROR;
        else if (timing) fprintf(stderr, "[lucille_hip] commit: tri64 upload (%.0f MB)      %8.2f ms\n", t64 / 1e6, (now_s() - tu) * 1e3);
        if (r == LH_ROUTE_INSTALL && hs->device_built) {
            /* the trees are built here, on this device (lh_build.hip: LBVH -> the same 4-wide nodes).  "wide8" = 1: the 8-wide nodes of ray dumps are
             * collapsed from the same binary tree now.  Left to itself (-1) a scene gets them when its first dump asks (lh_ensure_formats: the build is
             * run again, ~40 ms per 10 M triangles) -- a renderer that re-commits every frame and never dumps does not pay for them.  Lucille's own tree
             * belongs to this build where its home is the device already (device meshes, a replica of such a scene) or the host thread is held back
             * for it (ref_state 1) -- unless LH_REF_BUILD=host leaves a tree that need not be here to that thread */
            const char *e = getenv("LH_REF_BUILD");
            const bool own_tree = hs->have_ref && (hs->ref_on_device || (hs->ref_state == 1 && !(e && strcmp(e, "host") == 0)));
            char err[256] = "";
            const lh_side_outcome_t o = side_build(a, &s, s.tri64, hs->bvh.ntris, a->wide8 == 1, own_tree, err, sizeof(err));
            const bool tree_failed = o == LH_SIDE_BUILDER_FAILED || o == LH_SIDE_TOO_MANY_NODES;
            r = lh_side_route(who, o, a->build_auto, hs->ref_on_device);
            if (r == LH_ROUTE_ERROR && o == LH_SIDE_BAD_VERTEX) (void)fail("lh_accel_commit: a vertex coordinate is NaN, infinite or beyond 1e30");
            if (r == LH_ROUTE_ERROR && tree_failed) (void)fail("device BVH build failed: %s", err);
            if (r == LH_ROUTE_ERROR && o == LH_SIDE_TOO_DEEP) (void)fail("lh_accel_commit_replica: the device-built tree is deeper than the traversal kernels' stacks (the source fell back to the host builder?)");
            if (r == LH_ROUTE_ERROR && o == LH_SIDE_REF_FAILED) (void)fail("building lucille's own tree on the device failed: %s", err);          /* (a failed scan has left its own text) */
            if (timing && r == LH_ROUTE_HOST_BUILDERS && tree_failed) fprintf(stderr, "[lucille_hip] commit: device build failed (%s): host builders\n", err);
            if (timing && r == LH_ROUTE_HOST_BUILDERS && o == LH_SIDE_REF_FAILED) fprintf(stderr, "[lucille_hip] commit: building lucille's own tree on the device failed: %s: host builders\n", err);
            if (timing && r == LH_ROUTE_HOST_BUILDERS && o == LH_SIDE_SCAN_FAILED) fprintf(stderr, "[lucille_hip] commit: %s: host builders\n", lh_last_error());
            if (timing && r == LH_ROUTE_REF_HOST_THREAD) fprintf(stderr, "[lucille_hip] commit: lucille's own tree not built on the device (%s): host thread\n", err);
            if (r == LH_ROUTE_INSTALL || r == LH_ROUTE_REF_HOST_THREAD) side_install(a, &s);          /* the latter: side_build has left the side without that tree */
        }
        const bool fell_back = r == LH_ROUTE_HOST_BUILDERS && who == LH_FOR_DEVICE_MESHES;          /* the fallback's own device_upload commits the scene */
        if (fell_back) r = dmesh_host_fallback(a, dmesh_first, a->ndmeshes, &s) == 0 ? LH_ROUTE_INSTALL : LH_ROUTE_ERROR;
        if (fell_back || r == LH_ROUTE_ERROR || r == LH_ROUTE_HOST_BUILDERS) { side_free(&s); return r; }
        if (!hs->device_built && upload_array(a, &a->d_tri32, hs->bvh.tri32, sizeof(lh_tri32_t) * nt, 64) != 0) return LH_ROUTE_ERROR;
        if (hs->have_ref && __atomic_load_n(&hs->ref_state, __ATOMIC_ACQUIRE) == 2 && attach_ref(a) != 0) return LH_ROUTE_ERROR;
        /* resident from the start: what the default kernel reads (everything else on first use) */
        if (lh_ensure_formats(a, LH_FMT_Q16X4) != 0) return LH_ROUTE_ERROR;
    }
    a->upload_seconds = now_s() - t0;
    if (size_grid(a) != 0) return LH_ROUTE_ERROR;
    a->committed = 1;
    return LH_ROUTE_INSTALL;
}

/* a device-mesh scene whose trees the device builders could not make (an LBVH deeper than the walks' stacks, memory): the one case
 * in which its triangles are copied to the host -- once, as flattened by the kernel -- and both trees are built there from that
 * copy, handed to the host builders as ONE mesh of 3 n vertices with the identity index list; the scene goes on as a host-built one */
static int dmesh_host_fallback(lh_accel_t *a, const uint32_t *first, uint32_t nm, lh_side *s)
{
    lh_host_scene *hs = a->hs;
    a->update_fellback = a->updatable;
    const size_t nt = first[nm];
    double *tri = (double *)malloc(sizeof(lh_tri64_t) * nt);
    uint32_t *ident = (uint32_t *)malloc(sizeof(uint32_t) * 3 * nt);
    lh_mesh_copy *mc = (lh_mesh_copy *)calloc(1, sizeof(lh_mesh_copy));
    if (!tri || !ident || !mc) { free(tri); free(ident); free(mc); return fail("out of memory"); }
    const double t0 = now_s();
    const hipError_t e = hipMemcpy(tri, s->tri64, sizeof(lh_tri64_t) * nt, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { free(tri); free(ident); free(mc); return fail("lh_accel_commit: copying the flattened triangles to the host failed: %s", hipGetErrorString(e)); }
    if (getenv("LH_BUILD_TIMING")) fprintf(stderr, "[lucille_hip] commit: tri64 to the host (%.0f MB)   %8.2f ms\n", sizeof(lh_tri64_t) * (double)nt / 1e6, (now_s() - t0) * 1e3);
    for (size_t i = 0; i < 3 * nt; i++) ident[i] = (uint32_t)i;
    /* the per-primitive attribute arrays the gather made cross the release with the triangles: into the host scene, in the layout
     * device_upload carries back (host_build below sees one mesh without attributes and leaves them alone) */
    struct { void *dev; void **host; size_t bytes; } carry[] = {
        {s->attr.nrm9, (void **)&hs->nrm9, sizeof(double) * 9 * nt}, {s->attr.attr9[0], (void **)&hs->attr9[0], sizeof(double) * 9 * nt},
        {s->attr.attr9[1], (void **)&hs->attr9[1], sizeof(double) * 9 * nt}, {s->attr.attr9[2], (void **)&hs->attr9[2], sizeof(double) * 9 * nt},
        {s->attr.st6, (void **)&hs->st6, sizeof(double) * 6 * nt}, {s->attr.inside, (void **)&hs->inside, nt}};
    for (size_t k = 0; k < sizeof(carry) / sizeof(carry[0]); k++) {
        if (!carry[k].dev) continue;
        free(*carry[k].host);
        *carry[k].host = malloc(carry[k].bytes);                /* the host scene's from here on: freed with it */
        const hipError_t ec = *carry[k].host ? hipMemcpy(*carry[k].host, carry[k].dev, carry[k].bytes, hipMemcpyDeviceToHost) : hipErrorOutOfMemory;
        if (ec != hipSuccess) { free(tri); free(ident); free(mc); return fail("lh_accel_commit: copying the gathered attributes to the host failed: %s", hipGetErrorString(ec)); }
    }
    free_dmeshes(a);
    side_free(s);
    release_device(a);
    lh_bvh_release(&hs->bvh); lh_refbvh_release(&hs->ref); hs->ref_state = 0; hs->ref_on_device = 0;
    mc->npos = mc->nidx = (uint32_t)(3 * nt); mc->pos = tri; mc->idx = ident;
    a->meshes = mc; a->nmeshes = 1;
    if (host_build(a, 0, false, false) != 0) return -1;
    hs->nmeshes = nm;
    if (dmesh_prim_tables(hs, first, nm) != 0) return -1;
    return device_upload(a, LH_FOR_HOST_MESHES) == LH_ROUTE_INSTALL ? 0 : -1;
}

/* lh_accel_commit of an accelerator that holds device meshes: always the device path, no host copy of the triangles */
static int commit_device_meshes(lh_accel_t *a)
{
    lh_host_scene *hs = a->hs;
    const double tc0 = now_s();
    HIPCHK(hipSetDevice(a->device));
    const uint32_t nm = a->ndmeshes;
    uint32_t *first = dmesh_first_prim(a);
    if (!first) return fail("out of memory");
    memset(&hs->bvh, 0, sizeof(hs->bvh));
    hs->bvh.deg_dcap = INFINITY; hs->bvh.ntris = hs->bvh.nlive = first[nm];
    { const char *e = getenv("LH_REFTREE"); hs->have_ref = !(e && atoi(e) == 0); }
    hs->nmeshes = nm; hs->device_meshes = 1; hs->device_built = 1; hs->ref_state = 0;
    hs->ref_on_device = 1;                      /* lucille's own tree is built on the device too: there are no host triangles for a host thread */
    a->build_auto = 0;
    int rc = dmesh_prim_tables(hs, first, nm);
    if (rc == 0) rc = device_upload(a, LH_FOR_DEVICE_MESHES, first) == LH_ROUTE_INSTALL ? 0 : -1;
    free(first);
    if (rc != 0 || !a->updatable || a->update_fellback) free_dmeshes(a);          /* an updatable accelerator keeps its blocks and events: freed by lh_accel_destroy */
    if (rc != 0) return -1;
    if (getenv("LH_BUILD_TIMING")) fprintf(stderr, "[lucille_hip] commit: device meshes, %.2f ms in all\n", (now_s() - tc0) * 1e3);
    a->commit_failed = 0;
    return 0;
}

extern "C" int lh_accel_commit(lh_accel_t *a, int build_threads)
{
    lh_guard guard(a);
    if (!a) return fail("lh_accel_commit: accel is NULL");
    if (a->committed) return fail("lh_accel_commit: already committed");
    if (a->commit_failed) return fail("lh_accel_commit: an earlier commit of this accelerator failed; create a new one");
    if (a->ndmeshes) {
        if (build_threads != 0 && build_threads != LH_BUILD_ON_DEVICE)
            return fail("lh_accel_commit: device meshes are built on the device (build_threads must be 0 or LH_BUILD_ON_DEVICE)");
        a->commit_failed = 1;
        return commit_device_meshes(a);
    }
    a->commit_failed = 1;                       /* cleared on success */
    /* where the trees are built: said by the caller (LH_BUILD_ON_DEVICE, LH_BUILD_ON_HOST, or a thread count = the host), by
     * LH_BUILD in the environment, or -- build_threads == 0 -- by the size of the scene: from LH_AUTO_DEVICE_TRIANGLES on the
     * device builders (0.3 s instead of 4 s for 21 M triangles, frames ~2 % slower, HISTORY.md 15), below it the host builders
     * (milliseconds either way, and the better tree).  An automatic device build that fails falls back to the host. */
    bool on_device = build_threads == LH_BUILD_ON_DEVICE;
    bool chosen = build_threads == LH_BUILD_ON_DEVICE || build_threads == LH_BUILD_ON_HOST || build_threads > 0;
    { const char *e = getenv("LH_BUILD"); if (e && strcmp(e, "device") == 0) { on_device = true; chosen = true; } if (e && strcmp(e, "host") == 0) { on_device = false; chosen = true; } }
    if (!chosen) {
        unsigned long long ntri = 0;
        for (uint32_t g = 0; g < a->nmeshes; g++) ntri += a->meshes[g].nidx / 3;
        unsigned long long at = LH_AUTO_DEVICE_TRIANGLES;
        { const char *e = getenv("LH_AUTO_DEVICE_TRIANGLES"); if (e && atoll(e) > 0) at = (unsigned long long)atoll(e); }
        on_device = ntri >= at;
    }
    a->build_auto = !chosen;
    if (build_threads < 0) build_threads = 0;
    if (on_device) {
        const bool timing = getenv("LH_BUILD_TIMING") != NULL;
        const double tc0 = now_s();
        if (host_build(a, build_threads, true, true) != 0) return -1;
        const double tc1 = now_s();
        const lh_route_t next = device_upload(a, LH_FOR_HOST_MESHES);
        if (timing) fprintf(stderr, "[lucille_hip] commit: host side %.2f ms, device side %.2f ms\n", (tc1 - tc0) * 1e3, (now_s() - tc1) * 1e3);
        {
            lh_host_scene *hs = a->hs;
            if (hs->ref_state == 1 && !hs->ref_thread_live && next != LH_ROUTE_INSTALL) hs->ref_state = 0;      /* the device side failed, or was given up for the host builders: no background
                                                                                                  * build of lucille's tree for a scene that is about to be rebuilt on the host, or dropped */
            if (hs->ref_state == 1 && !hs->ref_thread_live) {
                if (next == LH_ROUTE_INSTALL && a->nmeshes) {
                    /* the mesh copies are no longer needed: the background thread returns them to the system */
                    hs->trash = (void **)calloc((size_t)a->nmeshes * 8, sizeof(void *));
                    if (hs->trash) {
                        for (uint32_t g = 0; g < a->nmeshes; g++) {
                            hs->trash[hs->ntrash++] = a->meshes[g].pos; hs->trash[hs->ntrash++] = a->meshes[g].idx; hs->trash[hs->ntrash++] = a->meshes[g].nrm;
                            for (int k = 0; k < 5; k++) hs->trash[hs->ntrash++] = a->meshes[g].attr[k];
                            a->meshes[g].pos = NULL; a->meshes[g].idx = NULL; a->meshes[g].nrm = NULL;
                            for (int k = 0; k < 5; k++) a->meshes[g].attr[k] = NULL;
                        }
                    }
                }
                if (pthread_create(&hs->ref_thread, NULL, ref_thread_main, hs) != 0) { hs->ref_state = 0; free_trash(hs); return fail("lh_accel_commit: cannot start the reference-tree thread"); }
                hs->ref_thread_live = 1;
            }
        }
        if (next == LH_ROUTE_HOST_BUILDERS) {
            /* an LBVH deeper than the kernel's stack bound (degenerate distributions), or one nobody asked for that failed: build on the host after all */
            (void)hipSetDevice(a->device); release_device(a);
            lh_host_scene *hs = a->hs;
            pthread_mutex_lock(&g_scene_mu);
            if (hs->ref_thread_live) { pthread_join(hs->ref_thread, NULL); hs->ref_thread_live = 0; }
            pthread_mutex_unlock(&g_scene_mu);
            free(hs->nrm9); free(hs->attr9[0]); free(hs->attr9[1]); free(hs->attr9[2]); free(hs->st6); free(hs->inside);
            hs->nrm9 = NULL; hs->attr9[0] = hs->attr9[1] = hs->attr9[2] = NULL; hs->st6 = NULL; hs->inside = NULL;
            lh_bvh_release(&hs->bvh); lh_refbvh_release(&hs->ref); hs->ref_state = 0; hs->ref_on_device = 0;
            on_device = false;
        } else {
            for (uint32_t g = 0; g < a->nmeshes; g++) {
                free(a->meshes[g].pos); free(a->meshes[g].idx); free(a->meshes[g].nrm);
                for (int k = 0; k < 5; k++) free(a->meshes[g].attr[k]);
            }
            free(a->meshes); a->meshes = NULL; a->nmeshes = 0;
            if (next != LH_ROUTE_INSTALL) return -1;
            a->commit_failed = 0;
            return 0;
        }
    }
    if (host_build(a, build_threads, false, false) != 0) return -1;
    if (device_upload(a, LH_FOR_HOST_MESHES) != LH_ROUTE_INSTALL) return -1;
    a->commit_failed = 0;
    return 0;
}

/* ---- updatable device meshes: new vertices, then a re-commit in place (include/lucille_hip.h) ------------------ */
static int updatable_check(const lh_accel_t *a, const char *who)
{
    if (!a->committed) return fail("%s: accel not committed", who);
    if (!a->updatable) return fail("%s: accel not updatable (lh_accel_set_param \"updatable\" = 1 comes before the commit)", who);
    if (a->update_fellback) return fail("%s: accel not updatable: its commit fell back to the host builders, which keep no device meshes", who);
    return 0;
}

extern "C" int lh_accel_update_mesh_device(lh_accel_t *a, uint32_t mesh, uint32_t npos, const void *d_pos, int fmt, size_t stride, void *stream)
{
    const char *who = "lh_accel_update_mesh_device";
    lh_guard guard(a);
    if (!a) return fail("%s: accel is NULL", who);
    if (updatable_check(a, who) != 0) return -1;
    if (mesh >= a->ndmeshes) return fail("%s: mesh %u out of range", who, mesh);
    lh_dmesh *m = &a->dmeshes[mesh];
    if (npos != m->npos) return fail("%s: %u positions given, the mesh has %u", who, npos, m->npos);
    if (fmt != LH_POS_F64 && fmt != LH_POS_F32) return fail("%s: unknown position format %d", who, fmt);
    const size_t elem = fmt == LH_POS_F32 ? sizeof(float) : sizeof(double);
    if (stride < 3 * elem || (stride % elem) != 0) return fail("%s: bad stride %zu", who, stride);
    if (npos && !d_pos) return fail("%s: NULL array", who);
    if (((uintptr_t)d_pos % elem) != 0) return fail("%s: positions not aligned to %zu bytes", who, elem);
    if (!m->ntris) return 0;                            /* never read: nothing is kept of it */
    const size_t pos_bytes = (size_t)(npos - 1) * stride + 3 * elem;          /* ntris > 0: the add saw npos > 0 */
    HIPCHK(hipSetDevice(a->device));
    if (lh_device_array_ok(a, d_pos, pos_bytes, who, "positions") != 0) return -1;
    hipStream_t s = (hipStream_t)stream;
    lh_dmesh_event *ev = dmesh_event_of(a, s);
    if (!ev) return -1;
    /* into the library's own copy and nothing else.  The same format and stride as the copy's: in place; another: a block of its own, the one
     * before it freed (hipFree waits for a copy that may still be writing it) */
    const bool same = fmt == m->fmt && stride == m->stride;
    void *own = NULL;
    if (!same) HIPCHK(hipMalloc(&own, pos_bytes));
    void *dst = same ? (void *)m->pos : own;
    if (hipMemcpyAsync(dst, d_pos, pos_bytes, hipMemcpyDeviceToDevice, s) != hipSuccess || hipEventRecord(ev->ev, s) != hipSuccess) {
        const char *why = hipGetErrorString(hipGetLastError());
        (void)hipStreamSynchronize(s);
        if (own) (void)hipFree(own);
        return fail("%s: copying the positions failed: %s", who, why);
    }
    if (!same) {
        if (m->pos_own) (void)hipFree(m->pos_own);
        m->pos_own = own; m->pos = own; m->fmt = fmt; m->stride = stride;
    }
    a->staged_pos = 1;
    return 0;
}

extern "C" int lh_accel_recommit(lh_accel_t *a, lh_recommit_info_t *info)
{
    const char *who = "lh_accel_recommit";
    lh_guard guard(a);
    if (info) memset(info, 0, sizeof(*info));
    if (!a) return fail("%s: accel is NULL", who);
    if (updatable_check(a, who) != 0) return -1;
    if (!a->staged_pos && !a->staged_attr) return 0;
    lh_host_scene *hs = a->hs;
    const double t0 = now_s();
    const bool timing = getenv("LH_BUILD_TIMING") != NULL;
    HIPCHK(hipSetDevice(a->device));
    /* the staged copies, through their events (the flatten waits for them again: an attribute-only re-commit does not flatten) */
    for (uint32_t k = 0; k < a->ndmesh_events; k++) HIPCHK(hipStreamWaitEvent(a->stream, a->dmesh_events[k].ev, 0));
    uint32_t *first = dmesh_first_prim(a);
    if (!first) return fail("out of memory");
    const uint32_t nt = first[a->ndmeshes];
    const int had_q8 = a->d_q8nodes != NULL;
    lh_recommit_plan_t plan = lh_recommit_plan(a->staged_pos, a->staged_attr, 1, had_q8, a->wide8);
    lh_side s; memset(&s, 0, sizeof(s));
    int rc = 0;
    /* everything below is built aside: the accelerator's arrays and headers are read, never written, until the install */
    if (plan.flatten && nt) {
        bool changed = false;
        rc = flatten_device_meshes(a, first, &s.tri64, who);
        if (rc == 0 && plan.compare) rc = words_differ(a, s.tri64, a->d_tri64, sizeof(lh_tri64_t) / 4 * (size_t)nt, &changed, "lh_accel_recommit: comparing the triangle records");
        plan = lh_recommit_plan(a->staged_pos, a->staged_attr, changed, had_q8, a->wide8);
        if (rc == 0 && !plan.trees) { (void)hipFree(s.tri64); s.tri64 = NULL; }          /* the resident records word for word: the trees stand */
    } else
        plan = lh_recommit_plan(a->staged_pos, a->staged_attr, 0, had_q8, a->wide8);          /* no triangles: nothing to build from */
    const double t1 = now_s();
    if (rc == 0 && plan.trees) {
        char err[256] = "";
        const lh_side_outcome_t o = side_build(a, &s, s.tri64, nt, plan.q8, hs->have_ref != 0, err, sizeof(err));
        if (lh_side_route(LH_FOR_RECOMMIT, o, 0, hs->ref_on_device) != LH_ROUTE_INSTALL)
            rc = o == LH_SIDE_BAD_VERTEX ? fail("%s: a vertex coordinate is NaN, infinite or beyond 1e30", who) : o == LH_SIDE_SCAN_FAILED ? -1 /* the scan's own text */
                                         : fail("%s: the device builders cannot build the updated scene (%s): it needs a new accelerator", who, err);
    }
    const double t2 = now_s();
    if (rc == 0 && plan.gather) { rc = gather_device_attributes(a, first, &s.attr, who); s.gathered = 1; }
    const double tg = now_s();
    free(first);
    /* a launch a caller enqueued earlier, on any stream, may still read the old arrays through its own copy of the scene */
    if (rc == 0 && hipDeviceSynchronize() != hipSuccess) rc = fail("%s: waiting for the device failed: %s", who, hipGetErrorString(hipGetLastError()));
    if (rc != 0) { side_free(&s); return -1; }          /* still committed, still the old scene; what was staged stays staged */
    const double t3 = now_s();
    if (plan.trees) {          /* the danger list of the OLD geometry must not stay: an install writes the host list only over LH_DANGER_ALL */
        pthread_mutex_lock(&g_scene_mu); __atomic_store_n(&hs->bvh.ndanger, LH_DANGER_ALL, __ATOMIC_RELEASE); pthread_mutex_unlock(&g_scene_mu);
    }
    side_install(a, &s);
    if (plan.trees && !a->grid_user) (void)size_grid(a);          /* the new tree's stack rows (it asks the runtime for the device's CUs: the old grid stays a valid one) */
    a->staged_pos = a->staged_attr = 0;
    a->upload_seconds = now_s() - t0;
    if (info) { info->flattened = plan.flatten; info->rebuilt_trees = plan.trees; info->regathered = plan.gather; info->seconds = a->upload_seconds; }
    if (timing) fprintf(stderr, "[lucille_hip] recommit: flatten + compare %.2f ms, trees %.2f ms, gather %.2f ms, wait %.2f ms, swap %.2f ms: %.2f ms in all (%s)\n",
                        (t1 - t0) * 1e3, (t2 - t1) * 1e3, (tg - t2) * 1e3, (t3 - tg) * 1e3, (now_s() - t3) * 1e3, a->upload_seconds * 1e3, plan.trees ? "trees rebuilt" : "trees kept");
    return 0;
}

/* blocks until the reference-order tree of a device-built scene is attached: from then on exact-t ties and fragile
 * hits follow the reference's tree (before: ties fall back to "larger primitive id wins", as with LH_REFTREE=0) */
extern "C" int lh_accel_wait_exact(lh_accel_t *a)
{
    lh_guard guard(a);
    if (!a || !a->committed) return fail("lh_accel_wait_exact: accel not committed");
    return lh_sync_ref(a, true);
}

/* lh_multi.hip: `dst` (created, nothing added) becomes a replica of `src`'s committed scene on its own device */
extern "C" int lh_accel_commit_replica(lh_accel_t *dst, lh_accel_t *src)
{
    if (!dst || !src || !src->committed) return fail("lh_accel_commit_replica: source not committed");
    if (src->hs->received) return fail("lh_accel_commit_replica: the source scene was received from another rank (no host copy to replicate)");
    if (src->hs->device_meshes) return fail("lh_accel_commit_replica: the source scene was committed from device meshes (no host copy to replicate)");
    lh_guard guard(dst);
    if (dst->committed || dst->commit_failed || dst->nmeshes || dst->ndmeshes) return fail("lh_accel_commit_replica: destination is not a fresh accelerator");
    pthread_mutex_lock(&g_scene_mu);
    lh_host_scene *old = dst->hs;
    dst->hs = src->hs; dst->hs->refs++;
    pthread_mutex_unlock(&g_scene_mu);
    free(old);                                  /* a fresh accelerator's scene holds nothing */
    dst->commit_failed = 1;
    if (device_upload(dst, LH_FOR_REPLICA) != LH_ROUTE_INSTALL) return -1;              /* a device-built scene is built again on this replica's device */
    dst->commit_failed = 0;
    return 0;
}

extern "C" int lh_accel_ref_tree(lh_accel_t *a, uint32_t *nnodes, void *nodes_out, uint32_t *leaf_prims_out)
{
    lh_guard guard(a);
    if (!a || !a->committed) return fail("lh_accel_ref_tree: accel not committed");
    if (lh_sync_ref(a, true) != 0) return -1;
    if (!a->d_ref_nodes) return fail("lh_accel_ref_tree: the reference-order tree is not attached (empty scene or LH_REFTREE=0)");
    HIPCHK(hipSetDevice(a->device));
    if (nnodes) *nnodes = a->dev.ref_nnodes;
    if (nodes_out) HIPCHK(hipMemcpy(nodes_out, a->d_ref_nodes, sizeof(lh_refnode_t) * (size_t)a->dev.ref_nnodes, hipMemcpyDeviceToHost));
    if (leaf_prims_out) HIPCHK(hipMemcpy(leaf_prims_out, a->d_ref_leaf_prims, sizeof(uint32_t) * (size_t)a->hs->bvh.ntris, hipMemcpyDeviceToHost));
    return 0;
}

/* the resident traversal trees as the walks read them: the device arrays, and the figures of a->dev the launch plan and the rays' set-up are given */
extern "C" int lh_accel_tree_image(lh_accel_t *a, lh_tree_image_t *info, void *q4nodes, void *q8nodes, void *tri32, void *tri64)
{
    lh_guard guard(a);
    if (!a || !a->committed) return fail("lh_accel_tree_image: accel not committed");
    HIPCHK(hipSetDevice(a->device));
    const lh_bvh_t *b = &a->hs->bvh; const lh_dev_scene_t *d = &a->dev;
    const size_t nt = d->ntris, n4 = a->d_q4nodes ? d->nq4nodes : 0u, n8 = a->d_q8nodes ? d->nq8nodes : 0u;
    if (info) {
        memset(info, 0, sizeof(*info));
        info->ntris = d->ntris; info->nlive = nt ? b->nlive : 0u;
        info->nq4 = (uint32_t)n4; info->q4_depth = d->q4_depth; info->q4_stack = d->q4_stack;
        info->nq8 = (uint32_t)n8; info->q8_depth = n8 ? d->q8_depth : 0u;
        info->device_built = a->hs->device_built ? 1u : 0u;
        for (int k = 0; k < 3; k++) { info->bmin[k] = b->bmin[k]; info->bmax[k] = b->bmax[k]; info->grid_lo[k] = d->grid_lo[k]; info->grid_step[k] = d->grid_step[k]; }
        info->scene_r = d->scene_r;
    }
    HIPCHK(hipStreamSynchronize(a->stream));          /* 8-wide nodes made on first use are written on the accelerator's stream */
    if (q4nodes && n4) HIPCHK(hipMemcpy(q4nodes, a->d_q4nodes, sizeof(lh_q4node_t) * n4, hipMemcpyDeviceToHost));
    if (q8nodes && n8) HIPCHK(hipMemcpy(q8nodes, a->d_q8nodes, sizeof(lh_q8node_t) * n8, hipMemcpyDeviceToHost));
    if (tri32 && nt && a->d_tri32) HIPCHK(hipMemcpy(tri32, a->d_tri32, sizeof(lh_tri32_t) * nt, hipMemcpyDeviceToHost));
    if (tri64 && nt && a->d_tri64) HIPCHK(hipMemcpy(tri64, a->d_tri64, sizeof(lh_tri64_t) * nt, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int lh_accel_danger_list(const lh_accel_t *a, uint32_t *ndevice, uint32_t device_box[3], uint32_t *nhost, double *host_boxes)
{
    lh_guard guard(a);
    if (!a || !a->committed) return fail("lh_accel_danger_list: accel not committed");
    const uint32_t nd = a->dev.ndanger, nh = __atomic_load_n(&a->hs->bvh.ndanger, __ATOMIC_ACQUIRE);
    if (ndevice) *ndevice = nd;
    if (device_box) for (int k = 0; k < 3; k++) device_box[k] = nd != LH_DANGER_ALL ? a->dev.danger[k] : 0u;
    if (nhost) *nhost = nh;
    if (host_boxes && nh != LH_DANGER_ALL) memcpy(host_boxes, a->hs->bvh.danger, sizeof(double) * 6 * (size_t)nh);
    return 0;
}

extern "C" void lh_accel_destroy(lh_accel_t *a)
{
    if (!a) return;
    lh_tex_release(a);
    if (a->d_emitters) { (void)hipSetDevice(a->device); (void)hipDeviceSynchronize(); (void)hipFree(a->d_emitters); a->d_emitters = NULL; a->nemit = 0; }      /* lh_accel_set_emitters */
    if (a->committed || a->commit_failed) { (void)hipSetDevice(a->device); lh_comb_destroy(a); release_device(a); }
    if (a->ndmeshes || a->ndmesh_events) { (void)hipSetDevice(a->device); free_dmeshes(a); }
    for (uint32_t g = 0; g < a->nmeshes; g++) {
        free(a->meshes[g].pos); free(a->meshes[g].idx); free(a->meshes[g].nrm);
        for (int k = 0; k < 5; k++) free(a->meshes[g].attr[k]);
    }
    free(a->meshes);
    pthread_mutex_lock(&g_scene_mu);
    const int last = (--a->hs->refs == 0);
    pthread_mutex_unlock(&g_scene_mu);
    if (last) {
        if (a->hs->ref_thread_live) { pthread_join(a->hs->ref_thread, NULL); a->hs->ref_thread_live = 0; }
        free_trash(a->hs);
        free(a->hs->nrm9); free(a->hs->attr9[0]); free(a->hs->attr9[1]); free(a->hs->attr9[2]); free(a->hs->st6); free(a->hs->inside);
        lh_bvh_release(&a->hs->bvh);
        lh_refbvh_release(&a->hs->ref);
        free(a->hs);
    }
    pthread_mutex_destroy(&a->mu);
    free(a);
}

extern "C" int lh_accel_info(const lh_accel_t *a, lh_accel_info_t *o)
{
    if (!a || !o) return fail("lh_accel_info: NULL argument");
    if (!a->committed) return fail("lh_accel_info: accel not committed");
    o->ntriangles = a->hs->bvh.ntris; o->nnodes = a->hs->bvh.nnodes; o->nleaves = a->hs->bvh.nleaves;
    o->max_depth = a->hs->bvh.max_depth; o->device_bytes = a->device_bytes;
    o->build_seconds = a->hs->bvh.build_seconds; o->upload_seconds = a->upload_seconds;
    o->device = a->device;
    o->ref_build_seconds = a->hs->ref_build_seconds;
    o->nnodes_traversal = a->hs->bvh.nq4nodes;
    o->ntriangles_in_tree = a->hs->bvh.ntris ? a->hs->bvh.nlive : 0u;
    return 0;
}

extern "C" int lh_accel_prim_lookup(const lh_accel_t *a, uint32_t prim, uint32_t *mesh, uint32_t *index)
{
    if (!a || !a->committed) return fail("lh_accel_prim_lookup: accel not committed");
    if (prim >= a->hs->bvh.ntris) return fail("lh_accel_prim_lookup: prim %u out of range", prim);
    if (mesh) *mesh = a->hs->bvh.prim_geom[prim];
    if (index) *index = a->hs->bvh.prim_index[prim];
    return 0;
}

extern "C" int lh_accel_set_grid(lh_accel_t *a, int blocks)
{
    lh_guard guard(a);
    if (!a || blocks <= 0) return fail("lh_accel_set_grid: bad argument");
    a->grid_blocks = blocks;
    return 0;
}

/* tuning knobs of the traversal kernel (sweeps, tools/): "grid" persistent workgroups, "min_active" regroup threshold,
 * "tri_batch" parked leaves per triangle pass, "ray_chunk" rays per cursor atomic, "variant" default kernel variant,
 * "ao_fused", "wide8" (-1 auto / 0 / 1), "stack_cap" (tests of the overflow path),
 * "coop_patience" (10 ns ticks the pass beside a launch waits for progress; 0: half a second),
 * "dump_order" (1 / 0: large ray dumps are traced from a copy in bin order, lh_order.h), "dump_order_min" (rays of the smallest dump that is),
 * "dump_order_bits" (the key, 64 bins either way: 2 = the origin's cell at two bits per axis, 1 = one bit per axis under the direction octant), "dump_order_max_mb" (0: no cap; else a dump whose workspace would be larger is traced as given),
 * "build_depth_cap" (levels of a device-built traversal tree beyond which the device builders are given up: LH_BUILD_DEPTH_MAX, what the walks' stacks take, or
 * less -- tests of the host fallback and of a re-commit that cannot build),
 * "updatable" (0 / 1, before the commit, device meshes only: the commit keeps the meshes for lh_accel_update_mesh_device / lh_accel_recommit) */
extern "C" int lh_accel_set_param(lh_accel_t *a, const char *name, int value)
{
    lh_guard guard(a);
    if (!a || !name) return fail("lh_accel_set_param: NULL argument");
    if (!strcmp(name, "grid") && value > 0) { a->grid_blocks = value; a->grid_user = 1; }
    else if (!strcmp(name, "min_active") && value > 0 && value <= 64) { a->min_active = value; a->knobs_user = 1; }
    else if (!strcmp(name, "tri_batch") && value > 0 && value <= 64) { a->tri_batch = value; a->knobs_user = 1; }
    else if (!strcmp(name, "ray_chunk") && value > 0 && value <= (1 << 20)) { a->ray_chunk = (uint32_t)value; a->dev.ray_chunk = (uint32_t)value; }
    else if (!strcmp(name, "variant") && (value == LH_VARIANT_DIRECT || value == LH_VARIANT_SPEC)) a->default_variant = value;
    else if (!strcmp(name, "ray_budget") && value > 0) { a->dev.ray_budget = (uint32_t)value; a->dump_budget = (uint32_t)value; a->ao_budget = (uint32_t)value; a->ao_budget_user = 1; }
    else if (!strcmp(name, "dump_budget") && value > 0) a->dump_budget = (uint32_t)value;
    else if (!strcmp(name, "ao_budget") && value >= 0) { a->ao_budget = (uint32_t)value; a->ao_budget_user = 1; }
    else if (!strcmp(name, "coop_patience") && value >= 0) a->dev.coop_patience = (uint32_t)value;
    else if (!strcmp(name, "ao_fused")) a->ao_fused = value != 0;
    else if (!strcmp(name, "combine")) a->combine = value != 0;
    else if (!strcmp(name, "host_walk")) { a->host_walk = value != 0; a->hw_gpu_left = 0; a->hw_ns = 0.0; }
    else if (!strcmp(name, "ao_group") && value >= 0 && value <= 4096) a->dev.ao_group = (uint32_t)value;
    else if (!strcmp(name, "fast_start")) a->fast_start = value != 0;
    else if (!strcmp(name, "wide8") && value >= -1 && value <= 1) a->wide8 = value;
    else if (!strcmp(name, "top_nodes") && value >= -1 && value <= (int)LH_TOP_NODES_MAX) a->dev.top_nodes = value < 0 ? LH_TOP_AUTO : (uint32_t)value;
    else if (!strcmp(name, "dump_order")) a->dump_order = value != 0;
    else if (!strcmp(name, "dump_order_min") && value > 0) a->dump_order_min = (size_t)value;
    else if (!strcmp(name, "dump_order_bits") && (value == 1 || value == 2)) a->dump_order_bits = (uint32_t)value;
    else if (!strcmp(name, "dump_order_max_mb") && value >= 0) a->dump_order_max_mb = (size_t)value;
    else if (!strcmp(name, "build_depth_cap") && value >= 1 && value <= LH_BUILD_DEPTH_MAX) a->build_depth_cap = value;
    else if (!strcmp(name, "updatable") && (value == 0 || value == 1)) {
        if (a->committed || a->commit_failed) return fail("lh_accel_set_param: \"updatable\" is set before the commit");
        if (a->nmeshes) return fail("lh_accel_set_param: \"updatable\" is for device meshes: host meshes and device meshes cannot be mixed on one accelerator");
        a->updatable = value;
    }
    else if (!strcmp(name, "stack_cap") && (value == 0 || (value >= 8 && value <= 64 && value % 2 == 0))) a->dev.stack_cap = (uint32_t)value;
    else return fail("lh_accel_set_param: unknown parameter or bad value: %s = %d", name, value);
    return 0;
}

extern "C" int lh_accel_export(const lh_accel_t *a, void *nodes, void *tri32)
{
    if (!a || !a->committed) return fail("lh_accel_export: accel not committed");
    if (a->hs->device_meshes) return fail("lh_accel_export: the scene was committed from device meshes; there is no host copy");
    if (a->hs->device_built) return fail("lh_accel_export: the tree was built on the device; there is no host copy");
    if (nodes && a->hs->bvh.nnodes) memcpy(nodes, a->hs->bvh.nodes, sizeof(lh_node_t) * (size_t)a->hs->bvh.nnodes);
    if (tri32 && a->hs->bvh.ntris) memcpy(tri32, a->hs->bvh.tri32, sizeof(lh_tri32_t) * (size_t)a->hs->bvh.ntris);
    return 0;
}

/* ------------------------------------------------------------------------ */
/* the scene image: what one rank's commit hands the other ranks (lh_dist.hip) */
/* ------------------------------------------------------------------------ */
/* ONE host build, then a broadcast of the flattened arrays into every GPU's HBM.  The image is a header
 * (lh_scene_image_t), the device arrays in a fixed order (lh_scene_image_arrays) and two host arrays (primitive ->
 * mesh ordinal / index, for lh_accel_prim_lookup and the materials).  A receiver has no host tree and no host
 * triangles: it cannot spawn replicas or upload other node formats, everything else works. */
int lh_scene_image_header(lh_accel_t *a, lh_scene_image_t *h)
{
    if (!a || !a->committed) return fail("scene image: accel not committed");
    if (a->hs->device_meshes) return fail("scene image: a scene committed from device meshes is not broadcast");
    if (lh_sync_ref(a, true) != 0) return -1;           /* a device-built scene: lucille's own tree must be attached */
    /* a scene whose ray dumps walk the 8-wide nodes (hot set beyond the Infinity Cache) is sent WITH them: rank 0 builds them
     * lazily on its first dump, a receiver has no host tree to build them from and would walk the slower 4-wide nodes --
     * and the slowest rank sets the time of a sharded dump */
    if (lh_accel_dump_node_bytes(a) == (int)sizeof(lh_q8node_t) && !a->d_q8nodes && lh_ensure_formats(a, LH_FMT_Q8) != 0) return -1;
    const lh_host_scene *hs = a->hs;
    memset(h, 0, sizeof(*h));
    h->magic = 0x4C48494Du;
    h->ntris = hs->bvh.ntris; h->nnodes = hs->bvh.nnodes; h->max_depth = hs->bvh.max_depth; h->nleaves = hs->bvh.nleaves;
    h->nq4 = hs->bvh.nq4nodes; h->q4_depth = hs->bvh.q4_depth; h->q4_stack = hs->bvh.q4_stack;
    h->nq8 = a->d_q8nodes ? a->dev.nq8nodes : 0; h->q8_depth = a->d_q8nodes ? a->dev.q8_depth : 0;
    h->nmeshes = hs->nmeshes;
    h->have_ref = a->d_ref_nodes != NULL; h->ref_nnodes = a->dev.ref_nnodes; h->ref_empty = a->dev.ref_empty;
    h->has_nrm = a->d_nrm9 != NULL; h->has_st = a->d_st6 != NULL; h->has_inside = a->d_inside != NULL;
    for (int k = 0; k < 3; k++) {
        h->has_attr[k] = a->d_attr9[k] != NULL;
        h->bmin[k] = hs->bvh.bmin[k]; h->bmax[k] = hs->bvh.bmax[k]; h->grid_lo[k] = hs->bvh.grid_lo[k]; h->grid_step[k] = hs->bvh.grid_step[k];
        h->ref_bmin[k] = a->dev.ref_bmin[k]; h->ref_bmax[k] = a->dev.ref_bmax[k];
    }
    h->build_seconds = hs->bvh.build_seconds; h->ref_build_seconds = hs->ref_build_seconds;
    h->nlive = hs->bvh.nlive; h->deg_dcap = hs->bvh.deg_dcap;
    return 0;
}

/* the device arrays of the image, same order on the sender and on a receiver that ran lh_scene_image_alloc */
int lh_scene_image_arrays(lh_accel_t *a, const lh_scene_image_t *h, void **ptr, size_t *bytes, int cap)
{
    int n = 0;
    scene_row r[LH_SCENE_ROWS];
    scene_rows(a, h, r);
    for (int k = 0; k < LH_IMAGE_ROWS; k++) if (r[k].present) { if (n < cap) { ptr[n] = *r[k].slot; bytes[n] = r[k].bytes; } n++; }
    return n;
}

/* host side of the image: prim -> mesh ordinal, prim -> 3 * i (ntris uint32 each) */
uint32_t *lh_scene_image_prim_geom(lh_accel_t *a) { return a->hs->bvh.prim_geom; }
uint32_t *lh_scene_image_prim_index(lh_accel_t *a) { return a->hs->bvh.prim_index; }

/* a fresh accelerator becomes the receiving end: device arrays allocated as the header says */
int lh_scene_image_alloc(lh_accel_t *a, const lh_scene_image_t *h)
{
    if (!a || a->committed || a->commit_failed || a->nmeshes || a->ndmeshes) return fail("scene image: the receiver must be a fresh accelerator");
    if (h->magic != 0x4C48494Du) return fail("scene image: bad header");
    lh_guard guard(a);
    lh_host_scene *hs = a->hs;
    a->commit_failed = 1;
    if (device_begin(a) != 0) return -1;
    hs->received = 1; hs->device_built = 1;              /* no host tree: the walks over other node formats are not available */
    hs->bvh.ntris = h->ntris; hs->bvh.nnodes = h->nnodes; hs->bvh.max_depth = h->max_depth; hs->bvh.nleaves = h->nleaves;
    hs->bvh.nq4nodes = h->nq4; hs->bvh.q4_depth = h->q4_depth; hs->bvh.q4_stack = h->q4_stack; hs->nmeshes = h->nmeshes;
    hs->bvh.nq8nodes = h->nq8; hs->bvh.q8_depth = h->q8_depth;
    hs->bvh.build_seconds = h->build_seconds; hs->ref_build_seconds = h->ref_build_seconds;
    hs->bvh.nlive = h->nlive; hs->bvh.deg_dcap = h->deg_dcap;
    hs->have_ref = h->have_ref; hs->ref_state = h->have_ref ? 2 : 0;
    for (int k = 0; k < 3; k++) { hs->bvh.bmin[k] = h->bmin[k]; hs->bvh.bmax[k] = h->bmax[k]; hs->bvh.grid_lo[k] = h->grid_lo[k]; hs->bvh.grid_step[k] = h->grid_step[k]; }
    publish_ref(a, h->ref_nnodes, h->ref_empty, h->ref_bmin, h->ref_bmax);          /* the box of a tree that is no longer on any host: lh_danger_scan reads it */
    if (h->ntris) {
        hs->bvh.prim_geom = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)h->ntris); hs->bvh.prim_index = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)h->ntris);
        if (!hs->bvh.prim_geom || !hs->bvh.prim_index) return fail("out of memory");
        scene_row r[LH_SCENE_ROWS];
        scene_rows(a, h, r);
        for (int k = 0; k < LH_SCENE_ROWS; k++) if (r[k].present) HIPCHK(hipMalloc(r[k].slot, r[k].bytes));
        publish_scene(a);
    }
    return 0;
}

/* ... and, once the arrays have arrived, a committed replica */
int lh_scene_image_finish(lh_accel_t *a)
{
    if (!a || !a->hs->received || a->committed) return fail("scene image: not a receiving accelerator");
    HIPCHK(hipSetDevice(a->device));
    if (size_grid(a) != 0) return -1;
    if (lh_danger_scan(a) != 0) return -1;          /* the arrays have arrived: this replica lists its own boxes */
    a->upload_seconds = 0.0;
    a->committed = 1; a->commit_failed = 0;
    return 0;
}

extern "C" int lh_accel_add_rib_scene(lh_accel_t *a, const lh_rib_scene_t *scene)
{
    lh_guard guard(a);
    lh_rib_info_t info;
    if (!a || !scene) return fail("lh_accel_add_rib_scene: NULL argument");
    if (lh_rib_info(scene, &info) != 0) return fail("lh_accel_add_rib_scene: %s", lh_rib_last_error());
    for (uint32_t m = 0; m < info.nmeshes; m++) {
        uint32_t npos = 0, nidx = 0; const double *pos = NULL, *nrm = NULL; const uint32_t *idx = NULL; int two = 0;
        if (lh_rib_mesh(scene, m, &npos, &pos, &nidx, &idx, &nrm, &two) != 0) return fail("lh_accel_add_rib_scene: %s", lh_rib_last_error());
        const uint32_t ord = a->nmeshes;          /* add_mesh returns 0 / -1, not the ordinal */
        if (lh_accel_add_mesh(a, npos, pos, 4 * sizeof(double), nidx, idx) != 0) return -1;
        if (nrm && lh_accel_set_normals(a, ord, nrm, 4 * sizeof(double), two) != 0) return -1;
    }
    return 0;
}


/*
 * lh_whitted.hip -- the refraction chain on the device: the reference's Whitted transport (trace_whitted / ri_transport_whitted,
 * src/transport/whitted.c:32-151) for a caller's batch of hit records and for a tile.  The rule is lh_whitted.h; the hit epilogue's
 * P, Ns and I are k_state_build's (lh_shade.h state_core); the environment is env_lookup's.
 *
 * A wavefront loop that never reads a count back.  List d holds the chains that are alive after d rays: an id
 * column, the rays of depth d and -- once they are traced -- their closest-hit records, all compacted, entry j of each.  Per depth:
 *   k_whitted_bounce over list d:  a miss ends the chain in the environment, a hit at the limit cuts it -- both write the id's outputs
 *       where they happen -- and any other hit computes ray d + 1 and appends the chain to list d + 1 (one ballot and one atomic add
 *       per wave); list 0 is the caller's list, its rays and records the caller's arrays by ray id
 *   lh_launch over list d + 1:  closest hit, the identity list over the compacted arrays, the count on the device.
 * Nothing but rays (48 bytes), ids and records (28 bytes) goes through HBM; the order of a list's entries depends on scheduling and
 * shows in no output: every value of an entry is a function of its chain alone, and an id listed twice writes the same bytes twice.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/lucille_hip.h"
#include "lh_internal.h"
#include "lh_ao.h"
#include "lh_whitted.h"

#define ensure_buf lh_ensure_buf

namespace {

#include "lh_pt.h"
#include "lh_shade.h"

/* list d and what its entries index.  Depth 0 (by_id): the caller's list -- entry k is traced when k < min(*count, n_list) and its id
 * < n_rays (lh_accel_ao_device's semantics), rays and records are the caller's, by id.  Deeper: the chain's own, by entry */
struct ChainIn {
    const uint32_t *ids;        /* entry -> ray id; NULL: the identity */
    const uint32_t *count;      /* entries (clamped to n_list); NULL: all n_list */
    uint32_t n_list, n_rays;
    int by_id;
    const double *org, *dir;
    const uint32_t *prim;
    const double *t, *u, *v;
};
struct ChainOut { uint32_t *bounces; double *end_org, *end_dir; float *rgb; };          /* by ray id; any of them NULL */
struct ChainNext { uint32_t *count; uint32_t *ids; double *org, *dir; uint32_t cap; };    /* list d + 1 */
struct ChainScene { const void *tri64; const double *nrm9; uint32_t ntris; };

/* entry k of a list: traced or not, and its id */
__device__ __forceinline__ bool chain_entry(const ChainIn &in, uint32_t k, uint32_t &id)
{
    uint32_t lim = in.n_list;
    if (in.count) { const uint32_t c = *in.count; if (c < lim) lim = c; }
    if (k >= lim) return false;
    id = in.ids ? in.ids[k] : k;
    return id < in.n_rays;
}

/* the record at j is a hit of this scene (a primitive id the scene does not have counts as a miss: nothing outside its arrays is read) */
__device__ __forceinline__ bool chain_hit(const ChainIn &in, const ChainScene &sc, size_t j, uint32_t &p)
{
    p = in.prim[j];
    return p != LH_MISS_PRIM && p < sc.ntris;
}

/* the bounce of the hit at j: the subset of the epilogue it needs, then lh_whitted.h */
__device__ __forceinline__ void chain_bounce(const ChainIn &in, const ChainScene &sc, size_t j, uint32_t p, double eps, double eta, double o2[3], double d2[3])
{
    LH_NC
    const double org[3] = {in.org[3 * j], in.org[3 * j + 1], in.org[3 * j + 2]}, dir[3] = {in.dir[3 * j], in.dir[3 * j + 1], in.dir[3 * j + 2]};
    double P[3], Ng[3], Ns[3], I[3];
    state_core<false>(sc.tri64, sc.nrm9, p, org, dir, in.t[j], in.u[j], in.v[j], P, Ng, Ns, I);
    lh_whitted_bounce(P, Ns, I, eps, eta, o2, d2);
}

/* one thread per entry of list `depth`.  cam_miss (the tile, depth 0): a miss record is a camera miss and sees the environment in the
 * camera ray's direction; else a miss record of depth 0 gets LH_AO_NO_HIT and zeros */
__global__ __launch_bounds__(256) void k_whitted_bounce(const ChainIn in, const ChainOut out, const ChainNext nx, const ChainScene sc, const DevEnv env,
                                                        double eps, double eta, uint32_t depth, uint32_t max_depth, int cam_miss)
{
    LH_NC
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    uint32_t id = 0;
    const bool live = chain_entry(in, k, id);
    bool go = false;
    double o2[3] = {0.0, 0.0, 0.0}, d2[3] = {0.0, 0.0, 0.0};
    if (live) {
        const size_t j = in.by_id ? (size_t)id : (size_t)k;
        uint32_t p;
        if (!chain_hit(in, sc, j, p)) {
            float c[3] = {0.0f, 0.0f, 0.0f};
            if (depth > 0 || cam_miss) env_lookup(env, in.dir[3 * j], in.dir[3 * j + 1], in.dir[3 * j + 2], c);
            if (out.bounces) out.bounces[id] = depth > 0 ? depth : LH_AO_NO_HIT;
            if (out.rgb) { out.rgb[3 * (size_t)id] = c[0]; out.rgb[3 * (size_t)id + 1] = c[1]; out.rgb[3 * (size_t)id + 2] = c[2]; }
            if (depth > 0) for (int a = 0; a < 3; a++) {
                if (out.end_org) out.end_org[3 * (size_t)id + a] = in.org[3 * j + a];
                if (out.end_dir) out.end_dir[3 * (size_t)id + a] = in.dir[3 * j + a];
            }
        } else if (depth >= max_depth) {
            if (out.bounces) out.bounces[id] = depth | LH_WHITTED_CUT;
            if (out.rgb) { out.rgb[3 * (size_t)id] = 0.0f; out.rgb[3 * (size_t)id + 1] = 0.0f; out.rgb[3 * (size_t)id + 2] = 0.0f; }
            if (depth > 0) for (int a = 0; a < 3; a++) {
                if (out.end_org) out.end_org[3 * (size_t)id + a] = in.org[3 * j + a];
                if (out.end_dir) out.end_dir[3 * (size_t)id + a] = in.dir[3 * j + a];
            }
        } else {
            chain_bounce(in, sc, j, p, eps, eta, o2, d2);
            go = true;
        }
    }
    /* the append: the wave's survivors take consecutive entries of list depth + 1 */
    const unsigned long long m = __ballot(go);
    if (m == 0ull) return;
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(nx.count, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader);
    if (!go) return;
    const uint32_t slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (slot >= nx.cap) return;          /* cannot happen: an entry has one successor at most, and list d + 1 has room for list d */
    nx.ids[slot] = id;
    for (int a = 0; a < 3; a++) { nx.org[3 * (size_t)slot + a] = o2[a]; nx.dir[3 * (size_t)slot + a] = d2[a]; }
}

/* the bounce alone (lh_accel_whitted_rays_device): the next ray of every traced hit, by ray id */
__global__ __launch_bounds__(256) void k_whitted_rays(const ChainIn in, const ChainScene sc, double eps, double eta, double *org_out, double *dir_out)
{
    LH_NC
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    uint32_t id = 0, p;
    if (!chain_entry(in, k, id) || !chain_hit(in, sc, (size_t)id, p)) return;
    double o2[3], d2[3];
    chain_bounce(in, sc, (size_t)id, p, eps, eta, o2, d2);
    for (int a = 0; a < 3; a++) { org_out[3 * (size_t)id + a] = o2[a]; dir_out[3 * (size_t)id + a] = d2[a]; }
}

/* the tile's resolve, one thread per pixel: env_resolve's accumulation (lh_render.hip) over the samples' colours -- widened, added per
 * channel in sample order, scaled, converted, clamped at 0, written in image orientation (the tile's first line last) */
__global__ __launch_bounds__(256) void k_whitted_resolve(int w, int h, int spp, const float *__restrict__ sample_rgb, float *__restrict__ rgb)
{
    LH_NC
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (size_t)w * h) return;
    const int lx = (int)(pix % w), ly = (int)(pix / w);
    double accum[3] = {0.0, 0.0, 0.0};
    for (int s = 0; s < spp; s++)
        for (int c = 0; c < 3; c++) accum[c] = accum[c] + (double)sample_rgb[3 * (pix * spp + s) + c];
    for (int c = 0; c < 3; c++) {
        float f = (float)(accum[c] * ((double)1.0 / spp));
        if (f < 0.0f) f = 0.0f;
        rgb[3 * ((size_t)(h - 1 - ly) * w + lx) + c] = f;
    }
}

} /* namespace */

/* NULL: the defaults (whitted.c:24,38,46); else the caller's, if lh_whitted.h accepts them */
static int whitted_params(const char *what, const lh_whitted_params_t *params, lh_whitted_params_t *out)
{
    const lh_whitted_params_t def = LH_WHITTED_DEFAULTS;
    *out = params ? *params : def;
    if (!lh_whitted_params_ok(out->eps, out->eta, out->max_depth, out->reserved))
        return fail("%s: bad refraction parameters (eps %g, eta %g, max_depth %d, reserved %d: eps finite and >= 0, eta finite and > 0, 0 <= max_depth <= %d, reserved 0)",
                    what, out->eps, out->eta, out->max_depth, out->reserved, LH_WHITTED_DEPTH_MAX);
    return 0;
}

/* what the batch entry points refuse before they look at the accelerator's scene; 1: go on, 0: nothing to do (n_rays == 0).
 * out8_*: outputs that hold doubles; out4_*: 32-bit words */
static int whitted_args(const char *what, const lh_accel_t *a, size_t n_rays, const void *org, const void *dir, const void *prim, const void *t,
                        const void *u, const void *v, const void *index, size_t n_index, const void *count,
                        const void *out8_a, const void *out8_b, const void *out4_a, const void *out4_b)
{
    if (n_rays >= ((size_t)1 << 31)) return fail("%s: 2^31 - 1 rays at most in one batch (%zu given)", what, n_rays);
    if (n_index > ((size_t)1 << 30)) return fail("%s: a list holds 2^30 entries at most (%zu given)", what, n_index);
    if ((((uintptr_t)index | (uintptr_t)count) & 3u) != 0) return fail("%s: the list and its count are 32-bit words: a pointer is not 4-byte aligned", what);
    if ((((uintptr_t)org | (uintptr_t)dir | (uintptr_t)t | (uintptr_t)u | (uintptr_t)v) & 7u) != 0 || ((uintptr_t)prim & 3u) != 0)
        return fail("%s: rays and records are doubles (prim: 32-bit words): a pointer is not 8-byte aligned (prim: 4-byte)", what);
    if ((((uintptr_t)out8_a | (uintptr_t)out8_b) & 7u) != 0) return fail("%s: the ray outputs are doubles: a pointer is not 8-byte aligned", what);
    if ((((uintptr_t)out4_a | (uintptr_t)out4_b) & 3u) != 0) return fail("%s: the outputs are 32-bit words: a pointer is not 4-byte aligned", what);
    if (!a || !a->committed) return fail("%s: accel not committed", what);
    if (n_rays == 0) return 0;
    if (!(org && dir && prim && t && u && v)) return fail("%s: NULL ray or record array", what);
    return 1;
}

static ChainScene chain_scene(const lh_accel_t *a)
{
    ChainScene sc;
    sc.tri64 = a->dev.tri64; sc.nrm9 = (const double *)a->d_nrm9; sc.ntris = a->hs->bvh.ntris;
    return sc;
}

struct chain_totals { uint64_t rays, max_depth; };

/* the chain over the list (idx, cntp, L entries; rays and records by id in the caller's or the tile's arrays).  Enqueues everything on s and
 * ends with the loop's one read-back: the depths' counts, for `tot` and the statistics.  cnt: the counters of a counted launch or NULL (cleared
 * by the caller); extra_rays: rays the caller traced before the chain and counts with it */
static int whitted_chain(lh_accel_t *a, const char *what, const lh_whitted_params_t &p, size_t L, size_t n_rays, const uint32_t *idx, const uint32_t *cntp,
                         const void *d_org, const void *d_dir, const void *d_prim, const void *d_t, const void *d_u, const void *d_v,
                         const ChainOut &out, bool cam_miss, unsigned long long *cnt, uint64_t extra_rays, hipStream_t s, chain_totals *tot)
{
    const int D = p.max_depth;
    /* two sets of rays and ids, one of records: 132 bytes an entry; the counts of depths 1 .. D (word 0 stays 0: list 0 is the caller's) */
    if (D > 0 && ensure_buf(&a->w_chain, L * 132)) return -1;
    if (ensure_buf(&a->w_counts, sizeof(uint32_t) * (LH_WHITTED_DEPTH_MAX + 2))) return -1;
    if (!a->h_read) HIPCHK(hipHostMalloc(&a->h_read, 1024, hipHostMallocDefault));
    uint32_t *counts = (uint32_t *)a->w_counts.p, *h_counts = (uint32_t *)a->h_read;
    HIPCHK(hipMemsetAsync(counts, 0, sizeof(uint32_t) * (LH_WHITTED_DEPTH_MAX + 2), s));
    double *base = (double *)a->w_chain.p;
    double *org_a = base, *dir_a = base + 3 * L, *org_b = base + 6 * L, *dir_b = base + 9 * L, *r_t = base + 12 * L, *r_u = base + 13 * L, *r_v = base + 14 * L;
    uint32_t *r_prim = (uint32_t *)(base + 15 * L), *ids_a = r_prim + L, *ids_b = ids_a + L;
    const ChainScene sc = chain_scene(a);
    const lh_env_src_t esrc = lh_env_source(a);
    const unsigned nb = (unsigned)((L + 255) / 256);
    ChainIn in = {idx, cntp, (uint32_t)L, (uint32_t)n_rays, 1, (const double *)d_org, (const double *)d_dir, (const uint32_t *)d_prim,
                  (const double *)d_t, (const double *)d_u, (const double *)d_v};
    for (int d = 0; d <= D; d++) {
        const ChainNext nx = {counts + d + 1, ids_a, org_a, dir_a, (uint32_t)L};
        hipLaunchKernelGGL(k_whitted_bounce, dim3(nb), dim3(256), 0, s, in, out, nx, sc, env_of(esrc), p.eps, p.eta, (uint32_t)d, (uint32_t)D, cam_miss ? 1 : 0);
        { const hipError_t e = hipGetLastError(); if (e != hipSuccess) return fail("%s: bounce kernel launch failed: %s", what, hipGetErrorString(e)); }
        if (d == D) break;
        /* ray d + 1 of every chain of list d + 1: closest hit, the identity list over the compacted arrays, the count where the bounce left it */
        lh_launch_opt opt;
        opt.indexed = true; opt.index = NULL; opt.idx_nrays = (uint32_t)L; opt.n_dev = counts + d + 1;
        if (lh_launch(a, lh_batch_t{L, LH_MODE_CLOSEST, org_a, dir_a, r_prim, r_t, r_u, r_v, NULL, cnt}, LH_VARIANT_DEFAULT, s, true, opt) != 0) return -1;
        in = ChainIn{ids_a, counts + d + 1, (uint32_t)L, 0xFFFFFFFFu, 0, org_a, dir_a, r_prim, r_t, r_u, r_v};
        { double *x = org_a; org_a = org_b; org_b = x; x = dir_a; dir_a = dir_b; dir_b = x; uint32_t *y = ids_a; ids_a = ids_b; ids_b = y; }
    }
    HIPCHK(hipMemcpyAsync(h_counts, counts, sizeof(uint32_t) * (size_t)(D + 2), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    tot->rays = 0; tot->max_depth = 0;
    for (int d = 1; d <= D; d++) { tot->rays += h_counts[d]; if (h_counts[d]) tot->max_depth = (uint64_t)d; }
    if (cnt) {
        unsigned long long hc[LH_CNT_N];
        HIPCHK(hipMemcpy(hc, cnt, sizeof(hc), hipMemcpyDeviceToHost));
        lh_stat_add(a, hc, extra_rays + tot->rays, 0);
    }
    return 0;
}

extern "C" int lh_accel_whitted_rays_device(lh_accel_t *a, size_t n_rays, const void *d_org, const void *d_dir, const void *d_prim, const void *d_t,
                                            const void *d_u, const void *d_v, const lh_whitted_params_t *params, const void *d_index, size_t n_index,
                                            const void *d_count, void *d_org_out, void *d_dir_out, void *stream)
{
    lh_guard guard(a);
    const char *what = "lh_accel_whitted_rays_device";
    lh_whitted_params_t p;
    if (whitted_params(what, params, &p) != 0) return -1;
    const int go = whitted_args(what, a, n_rays, d_org, d_dir, d_prim, d_t, d_u, d_v, d_index, n_index, d_count, d_org_out, d_dir_out, NULL, NULL);
    if (go <= 0) return go;
    if (!d_org_out || !d_dir_out) return fail("%s: NULL output array", what);
    const size_t L = (d_index || d_count || n_index) ? n_index : n_rays;          /* list entries; all NULL / 0: every ray */
    if (L == 0) return 0;
    HIPCHK(hipSetDevice(a->device));
    const ChainIn in = {(const uint32_t *)d_index, (const uint32_t *)d_count, (uint32_t)L, (uint32_t)n_rays, 1, (const double *)d_org, (const double *)d_dir,
                        (const uint32_t *)d_prim, (const double *)d_t, (const double *)d_u, (const double *)d_v};
    hipLaunchKernelGGL(k_whitted_rays, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, chain_scene(a), p.eps, p.eta,
                       (double *)d_org_out, (double *)d_dir_out);
    { const hipError_t e = hipGetLastError(); if (e != hipSuccess) return fail("%s: kernel launch failed: %s", what, hipGetErrorString(e)); }
    return 0;
}

extern "C" int lh_accel_whitted_device(lh_accel_t *a, size_t n_rays, const void *d_org, const void *d_dir, const void *d_prim, const void *d_t,
                                       const void *d_u, const void *d_v, const lh_whitted_params_t *params, const void *d_index, size_t n_index,
                                       const void *d_count, void *d_bounces, void *d_end_org, void *d_end_dir, void *d_rgb, void *stream)
{
    lh_guard guard(a);
    const char *what = "lh_accel_whitted_device";
    lh_whitted_params_t p;
    if (whitted_params(what, params, &p) != 0) return -1;
    const int go = whitted_args(what, a, n_rays, d_org, d_dir, d_prim, d_t, d_u, d_v, d_index, n_index, d_count, d_end_org, d_end_dir, d_bounces, d_rgb);
    if (go <= 0) return go;
    const size_t L = (d_index || d_count || n_index) ? n_index : n_rays;
    if (L == 0) return 0;
    HIPCHK(hipSetDevice(a->device));
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *cnt = (a->stat_on && a->hs->bvh.ntris) ? a->d_counters : NULL;          /* lh_accel_trace_statistics */
    if (cnt) HIPCHK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * LH_CNT_DEV, s));
    const ChainOut out = {(uint32_t *)d_bounces, (double *)d_end_org, (double *)d_end_dir, (float *)d_rgb};
    chain_totals tot;
    return whitted_chain(a, what, p, L, n_rays, (const uint32_t *)d_index, (const uint32_t *)d_count, d_org, d_dir, d_prim, d_t, d_u, d_v, out, false, cnt, 0, s, &tot);
}

/* the same for HOST arrays: copies up (the end rays too: the slots the chain does not write stay the caller's), the device call, copies down */
extern "C" int lh_accel_whitted_host(lh_accel_t *a, size_t n_rays, const double *org, const double *dir, const uint32_t *prim, const double *t,
                                     const double *u, const double *v, const lh_whitted_params_t *params, uint32_t *bounces, double *end_org,
                                     double *end_dir, float *rgb)
{
    lh_guard guard(a);
    const char *what = "lh_accel_whitted_host";
    lh_whitted_params_t p;
    if (whitted_params(what, params, &p) != 0) return -1;
    const int go = whitted_args(what, a, n_rays, org, dir, prim, t, u, v, NULL, 0, NULL, end_org, end_dir, bounces, rgb);
    if (go <= 0) return go;
    HIPCHK(hipSetDevice(a->device));
    const size_t n = n_rays, b_ray = sizeof(double) * 3 * n, b_d = sizeof(double) * n, b_u32 = sizeof(uint32_t) * n;
    enum { ORG, DIR, END_ORG, END_DIR, T, U, V, PRIM, BOUNCES, RGB, NF };
    lh_field_t f[NF] = {lh_field_up(org, b_ray), lh_field_up(dir, b_ray), lh_field_both(end_org, b_ray), lh_field_both(end_dir, b_ray),
                        lh_field_up(t, b_d), lh_field_up(u, b_d), lh_field_up(v, b_d), lh_field_up(prim, b_u32),
                        lh_field_down(bounces, b_u32), lh_field_down(rgb, sizeof(float) * 3 * n)};
    if (lh_stage_up(a, f, NF) != 0) return -1;
    return lh_stage_down(a, f, NF, lh_accel_whitted_device(a, n, f[ORG].dev, f[DIR].dev, f[PRIM].dev, f[T].dev, f[U].dev, f[V].dev, &p, NULL, 0, NULL,
                                                           f[BOUNCES].dev, f[END_ORG].dev, f[END_DIR].dev, f[RGB].dev, a->stream));
}

/* ri_transport_whitted per camera sample: the camera rays of lh_render_primary_rays, their closest hits, the chain over every sample (a
 * camera miss ends at depth 0, in the environment), a resolve per pixel */
extern "C" int lh_render_whitted_tile(lh_accel_t *a, const lh_camera_t *cam, int x0, int y0, int w, int h, int ps, const lh_whitted_params_t *params,
                                      void *d_rgb, lh_pt_stats_t *stats, void *stream)
{
    lh_guard guard(a);
    const char *what = "lh_render_whitted_tile";
    lh_whitted_params_t p;
    if (whitted_params(what, params, &p) != 0) return -1;
    if (!a || !a->committed) return fail("%s: accel not committed", what);
    if (!cam || !d_rgb) return fail("%s: NULL argument", what);
    if (w <= 0 || h <= 0 || ps < 1) return fail("%s: bad tile/sample counts", what);
    if (((uintptr_t)d_rgb & 3u) != 0) return fail("%s: the tile holds floats: the pointer is not 4-byte aligned", what);
    const size_t S = (size_t)w * h * ps * ps;
    if (S > ((size_t)1 << 30)) return fail("%s: more than 2^30 samples in one tile (a list holds 2^30 entries); render the frame in tiles", what);
    HIPCHK(hipSetDevice(a->device));
    hipStream_t s = (hipStream_t)stream;
    /* camera rays, their records, the samples' colours: 88 bytes a sample */
    if (ensure_buf(&a->w_tile, S * 88)) return -1;
    double *r_org = (double *)a->w_tile.p, *r_dir = r_org + 3 * S, *r_t = r_dir + 3 * S, *r_u = r_t + S, *r_v = r_u + S;
    uint32_t *r_prim = (uint32_t *)(r_v + S); float *s_rgb = (float *)(r_prim + S);
    unsigned long long *cnt = (a->stat_on && a->hs->bvh.ntris) ? a->d_counters : NULL;
    if (cnt) HIPCHK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * LH_CNT_DEV, s));
    if (lh_render_launch_primary(cam, x0, y0, w, h, ps, ps, r_org, r_dir, s) != 0) return fail("%s: primary ray kernel launch failed", what);
    if (lh_launch(a, lh_batch_t{S, LH_MODE_CLOSEST, r_org, r_dir, r_prim, r_t, r_u, r_v, NULL, cnt}, LH_VARIANT_DEFAULT, s, false) != 0) return -1;
    const ChainOut out = {NULL, NULL, NULL, s_rgb};
    chain_totals tot;
    if (whitted_chain(a, what, p, S, S, NULL, NULL, r_org, r_dir, r_prim, r_t, r_u, r_v, out, true, cnt, S, s, &tot) != 0) return -1;
    hipLaunchKernelGGL(k_whitted_resolve, dim3((unsigned)(((size_t)w * h + 255) / 256)), dim3(256), 0, s, w, h, ps * ps, (const float *)s_rgb, (float *)d_rgb);
    { const hipError_t e = hipGetLastError(); if (e != hipSuccess) return fail("%s: resolve kernel launch failed: %s", what, hipGetErrorString(e)); }
    HIPCHK(hipStreamSynchronize(s));
    if (stats) { stats->paths = S; stats->rays = S + tot.rays; stats->max_depth_reached = tot.max_depth; }
    return 0;
}

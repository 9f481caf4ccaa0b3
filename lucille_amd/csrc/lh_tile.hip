/*
 * lh_tile.hip -- the callers on either side of the query, kept on the device: AO tiles / bands / frames (subsample,
 * render_bucket, bucket_write: src/render/render.c:715-823,1107-1166,919-983; ri_transport_ambientocclusion:
 * src/transport/ambientocclusion.c:42-151,332-415), the hit epilogue (ri_intersection_state_build,
 * src/render/intersection_state.c:99-248) and the wavefront path tracer's tile loop (src/transport/pathtrace.c:189-314,
 * 407-537).  The kernels are in lh_render.hip / lh_kernels.hip.
 */
#include <algorithm>
#include <thread>
#include <vector>

#include "lh_internal.h"
#include "lh_dirt.h"
#include "lh_env.h"
#include "lh_sky.h"
#include "lh_lights.h"
#include "lh_area.h"
#include "lh_ptl.h"

#define ensure_buf lh_ensure_buf


extern "C" int lh_render_primary_rays(lh_accel_t *a, const lh_camera_t *cam, int x0, int y0, int w, int h,
                                      int ps, void *d_org, void *d_dir, void *stream)
{
    lh_guard guard(a);
    if (!a || !a->committed) return fail("lh_render_primary_rays: accel not committed");
    if (!cam || !d_org || !d_dir) return fail("lh_render_primary_rays: NULL argument");
    if (w < 0 || h < 0 || ps < 1) return fail("lh_render_primary_rays: bad tile");
    HIPCHK(hipSetDevice(a->device));
    if (lh_render_launch_primary(cam, x0, y0, w, h, ps, ps, (double *)d_org, (double *)d_dir, stream) != 0)
        return fail("primary ray kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

/* the hemisphere's sample grid of a hit: nphi = ntheta = (int)sqrt(gather_nsamples), N = their product AO rays (ambientocclusion.c:378-380) */
struct ao_grid { int nphi, ntheta, N; };
static inline ao_grid ao_sample_grid(int gather_nsamples) { const int n = (int)sqrt((double)gather_nsamples); return ao_grid{n, n, n * n}; }

/* LH_STAGE_TIMING=1: HIP events between the stages of a batch, printed to stderr (tools/experiments/rank_breakdown.py); they go with the
 * scope, whichever way the batch returns */
struct stage_timer {
    hipEvent_t ev[6] = {NULL, NULL, NULL, NULL, NULL, NULL};
    ~stage_timer() { for (int k = 0; k < 6; k++) if (ev[k]) (void)hipEventDestroy(ev[k]); }
};

/* ... the report: the stages' times, and the percentiles of the clocks at which the persistent waves of the two launches (closest, AO)
 * started, found every cursor dry and left (clk: a->r_diag, [2][3][nwaves]) */
static int stage_report(const stage_timer &tm, const void *d_clk, size_t nwaves, size_t S, unsigned long long nhit, size_t nao)
{
    float ms[5] = {0, 0, 0, 0, 0};
    for (int k = 0; k < 5; k++) (void)hipEventElapsedTime(&ms[k], tm.ev[k], tm.ev[k + 1]);
    fprintf(stderr, "[lucille_hip] AO batch stages (ms): primary %.3f closest %.3f compact %.3f ao %.3f resolve %.3f | samples %zu hits %llu ao rays %zu\n",
            ms[0], ms[1], ms[2], ms[3], ms[4], S, nhit, nao);
    std::vector<unsigned long long> clk(6 * nwaves);
    HIPCHK(hipMemcpy(clk.data(), d_clk, sizeof(unsigned long long) * 6 * nwaves, hipMemcpyDeviceToHost));
    for (int launch = 0; launch < 2; launch++) {
        const unsigned long long *st = clk.data() + 3 * nwaves * launch, *ex = st + nwaves, *dry = ex + nwaves;
        unsigned long long t0 = ~0ull; std::vector<double> e;
        for (size_t w = 0; w < nwaves; w++) if (st[w] && st[w] < t0) t0 = st[w];
        for (size_t w = 0; w < nwaves; w++) if (ex[w]) e.push_back((double)(ex[w] - t0) * 1e-5);        /* 100 MHz -> ms */
        if (e.empty()) continue;
        std::sort(e.begin(), e.end());
        auto qq = [](std::vector<double> &v, double f) { return v[(size_t)(f * (v.size() - 1))]; };
        double last_start = 0; for (size_t w = 0; w < nwaves; w++) if (st[w]) last_start = fmax(last_start, (double)(st[w] - t0) * 1e-5);
        fprintf(stderr, "[lucille_hip]   %s kernel: %zu waves, last start %.3f ms; exits (ms) min %.3f p10 %.3f p50 %.3f p90 %.3f p99 %.3f max %.3f\n",
                launch ? "AO" : "closest", e.size(), last_start, e.front(), qq(e, 0.10), qq(e, 0.50), qq(e, 0.90), qq(e, 0.99), e.back());
        /* when a wave found every cursor dry, and how long it went on after that (its last range and its slowest last rays) */
        std::vector<double> d, g;
        for (size_t w = 0; w < nwaves; w++) if (dry[w] && ex[w]) { d.push_back((double)(dry[w] - t0) * 1e-5); g.push_back((double)(ex[w] - dry[w]) * 1e-5); }
        if (!d.empty()) {
            std::sort(d.begin(), d.end()); std::sort(g.begin(), g.end());
            fprintf(stderr, "[lucille_hip]     cursors found dry at (ms) min %.3f p50 %.3f p90 %.3f max %.3f; exit - dry (ms) min %.3f p10 %.3f p50 %.3f p90 %.3f p99 %.3f max %.3f (%zu waves)\n",
                    d.front(), qq(d, 0.5), qq(d, 0.9), d.back(), g.front(), qq(g, 0.1), qq(g, 0.5), qq(g, 0.9), qq(g, 0.99), g.back(), d.size());
        }
    }
    return 0;
}

/* ---- the gather stage: one description of its transport ------------------------------------------------------------------------------------
 * The kind (LH_GATHER_*, lh_gather.h) with its checked parameters, as the entry points hand it on: AO has none and offsets its rays by 1e-6 along Ns */
struct gather_params { int kind; double eps; lh_dirt_params_t dirt; lh_env_params_t env; const lh_light_t *lights; int nlights;          /* lights: LH_GATHER_LIGHT, the caller's HOST table (lh_lights.h) */
                       lh_area_tab_t area;             /* LH_GATHER_AREA: the caller's lights, the accelerator's emitter table, S, the bound (lh_area.h) */
                       ao_grid items; };               /* an item kind's grid (gather_check): LIGHT nphi = 1, ntheta = the lights; AREA r = l * S + s, "nphi" lights of "ntheta" samples */

/* what the code around the stage reads of a kind, one row per LH_GATHER_* -- a new kind is a row here, its case in gather_check and its resolve.
 * An item kind has one work item per (slot, light[, sample]) instead of a hemisphere sample: its ray kernel writes a bound per ray, the statistics count
 * its work items, traced or not, and its resolve fetches no texture */
struct gather_kind {
    const char *device_name, *prefix;          /* the device entry point (a host form's messages carry it), and the prefix of a batch stage's messages */
    const char *fused_name, *resolve_name;     /* in "... launch failed" */
    lh_buf lh_gather_scratch::*left;           /* what the stage leaves per hit slot: the buffer a fused stage sizes and its kernel fills ... */
    size_t slot_bytes, slot_bytes_n;           /* ... of slot_bytes + slot_bytes_n * N bytes per slot */
    bool bounded; int mode;                    /* materialised: bounded launches of LH_DIRT_CHUNK rays through the ray dumps' kernels, or one plain launch; closest or any hit */
    bool item;
    int uniforms_per_item, radiance_floats;    /* replayed uniforms per gather ray; floats of `radiance` per ray */
};
static const gather_kind gather_kinds[LH_GATHER_KINDS] = {
    {"lh_accel_ao_device", "lh_accel_ao_device: ", "fused AO", "resolve", &lh_gather_scratch::occcount, sizeof(unsigned int), 0, false, LH_MODE_ANY, false, 2, 1},          /* a count per slot */
    {"lh_accel_dirt_device", "lh_accel_dirt_device: ", "fused dirt", "dirt resolve", &lh_gather_scratch::t, 0, 8, true, LH_MODE_CLOSEST, false, 2, 1},                     /* a double per ray */
    {"lh_accel_env_device", "lh_accel_env_device: ", "fused environment-gather", "environment-gather resolve", &lh_gather_scratch::occ, 0, 1, false, LH_MODE_ANY, false, 2, 3},          /* a byte per ray */
    {"lh_accel_lights_device", "lh_accel_lights_device: ", "fused light", "light resolve", &lh_gather_scratch::occ, 0, 1, true, LH_MODE_ANY, true, 2, 3},                  /* a byte per shadow ray */
    {"lh_accel_area_lights_device", "lh_accel_area_lights_device: ", "fused area-light", "area-light resolve", &lh_gather_scratch::occ, 0, 1, true, LH_MODE_ANY, true, 3, 3},          /* the same, N = L x S */
};

/* the sample grid of a stage: the hemisphere's, or an item kind's own -- work item slot * N + r is item (slot, r) in every kernel and buffer the kinds share */
static inline ao_grid gather_grid(const gather_params &p, int gather_nsamples)
{
    return gather_kinds[p.kind].item ? p.items : ao_sample_grid(gather_nsamples);
}
/* ... and what ao_region / ao_batch_device make of it, once, at their top, for the stage and the resolves: the scratch entry of the kind and the caller
 * (lh_accel::gather), the light of an environment gather -- the accelerator's environment, or while a sky is set (lh_sky.h) the sun-and-sky light, with
 * LH_SKY_SUN the sun's direction: every hit then traces the sun's shadow ray -- the texture arguments of a tile's resolve (NULL: no mesh has a texture;
 * the sun-and-sky gather has no texture fetch: ambientocclusion.c:369-375), and the prefix of the stage's messages */
struct gather_desc {
    gather_params p;
    int where;                      /* LH_GATHER_TILE | LH_GATHER_BATCH */
    lh_gather_scratch *b;
    lh_env_src_t esrc; const lh_sky_src_t *sky; const double *sun_dir;
    lh_tex_args_t tex_store; const lh_tex_args_t *tex;
    const char *prefix;
};
static void gather_describe(lh_accel_t *a, const gather_params &p, int where, gather_desc *d)
{
    d->p = p; d->where = where;
    d->b = &a->gather[p.kind][where];
    d->esrc = lh_env_source(a);
    d->sky = (p.kind == LH_GATHER_ENV && a->sky_set) ? &a->sky : NULL;
    d->sun_dir = (d->sky && (d->sky->sky.flags & LH_SKY_SUN)) ? d->sky->sky.sun_dir : NULL;
    d->tex = NULL;
    d->prefix = where == LH_GATHER_TILE ? "" : gather_kinds[p.kind].prefix;
}

/* what the stage left, as the resolves take it (lh_gather_left_t, lh_internal.h).  fused: the stage ended fused -- AO counted per slot, the environment
 * gather has no direction in memory (the resolve makes them again); sun_occ: the sun's bytes (or NULL); total: the resolve's 64 counters */
static lh_gather_left_t gather_left(const gather_desc &d, ao_grid g, uint64_t seed, bool fused, const uint8_t *sun_occ, unsigned long long *total)
{
    const lh_gather_scratch *b = d.b;
    lh_gather_left_t l;
    l.kind = d.p.kind; l.ntheta = g.ntheta; l.nphi = g.nphi; l.seed = seed;
    l.occ_count = fused ? (const unsigned int *)b->occcount.p : NULL; l.occ = (const uint8_t *)b->occ.p; l.t = (const double *)b->t.p;
    l.hitrec = (const double *)b->hitrec.p; l.key = (const unsigned long long *)b->key.p; l.adir = fused ? NULL : (const double *)b->adir.p;
    l.near_clip = d.p.dirt.near_clip; l.far_clip = d.p.dirt.far_clip; l.scale = d.p.env.scale;
    l.env = &d.esrc; l.sky = d.sky; l.sun_occ = sun_occ; l.lights = d.p.lights; l.area = d.p.kind == LH_GATHER_AREA ? &d.p.area : NULL; l.total = total;
    return l;
}

/* The gather stage of the tile pipeline and of a caller's batch alike: from "the compaction has left hit records and keys (in d.b) and the hit count
 * (at d_nhit) on the device" to "totals, hit count and statistics words are on the host".  The hit records were built with the kind's origin (d.p.eps).
 * What the stage leaves for the caller's resolve depends on its kind alone -- fused and materialised differ only in who wrote it:
 *   AO    fused, the occluded rays of every slot counted in occcount; materialised, the any-hit byte of ray (slot, r) at element slot * N + r of occ;
 *   ENV   (lh_env.h) that byte either way: the resolve needs the answer of every RAY;
 *   DIRT  (lh_dirt.h) the t of every gather ray's bounded closest-hit record (lh_tmax.h, every bound far_clip), a double at element slot * N + r of t;
 *   LIGHT (lh_lights.h; N = the lights) the bounded any-hit byte of shadow ray (slot, l) at element slot * N + l of occ, 0 for an item that is not traced;
 *   AREA  (lh_area.h; N = lights x samples) the same byte for item (slot, l, s) at element slot * N + l * S + s.
 * The row of gather_kinds says which buffer that is and how a materialised stage launches.
 * plan.fused: the kernel generates ray (slot, r) in its refill (lh_ao.h; an item kind: the item) -- nothing per gather ray goes through HBM but what
 * is left (lh_launch_trace_gather).  Else, and as the second try of a fused launch whose fix-up queue overflowed, materialised: the kind's ray kernel
 * writes the gather rays to HBM (from d_uniforms if given: the parity replay; the area kind reads its own from d.p.area), then one any-hit batch -- or,
 * for a bounded kind, ONE bounded launch per LH_DIRT_CHUNK rays through the ray dumps' kernels: DIRT closest hit under a bound array filled with
 * far_clip, the records' t kept; an item kind any hit under the bound its ray kernel wrote beside every ray, a byte kept.
 * plan.late (with fused only): the count stays on the device -- the buffers are sized for the worst case (nmax slots: every sample / entry hits), the
 * kernels read it at d_nhit -- and the stage costs ONE host round trip, at its end (round 5: the two in the middle were ~0.25 ms of a rank's 8.9 ms
 * share of the config-5 frame).  Else the count is read first: it sizes the ray arrays and the launch.
 * d.sun_dir (or NULL): the sun's shadow ray of the sun-and-sky light -- one more ray per hit slot from the slot's origin along the light's direction,
 * written by k_sun_rays and answered by ONE plain any-hit launch, a ray dump as lh_accel_intersect_device traces it: no slot key, so no self-primitive
 * skip (a sun behind the surface is shadowed by the hit's own triangle).  It leaves a byte per slot, the same whether the N gather rays are then traced
 * fused or materialised, and runs BEFORE them: a launch resets the stream's fix-up queue, whose words a late stage reads at its end.  late: the slot
 * count is on the device, the launch is the identity list's with its count there (lh_launch_opt::n_dev).  Not counted: cnt and the totals stay the
 * gather rays'.
 * resolve(left) enqueues the caller's radiance kernel over what the stage left (gather_left), which adds its count -- occluded rays; DIRT: bounded
 * hits -- into the 64 counters at d_nocc.  cnt: the LH_CNT_DEV counters or NULL; tm: stage timing or NULL (events 3-5: count known, rays traced, resolved) */
struct ao_totals { unsigned long long nhit, nocc, cnt[LH_CNT_DEV]; bool fused; };      /* cnt: the words at `cnt`; fused: the stage ended fused (no gather ray in HBM) */
template <class Resolve>
static int ao_stage(lh_accel_t *a, const gather_desc &d, size_t nmax, ao_grid g, uint64_t seed, const void *d_uniforms,
                    const unsigned long long *d_nhit, unsigned long long *d_nocc, unsigned long long *cnt, const lh_launch_opt &opt,
                    stage_timer *tm, lh_gather_plan_t plan, Resolve resolve, hipStream_t s, ao_totals *out)
{
    const unsigned long long N = (unsigned long long)g.N;
    lh_gather_scratch *b = d.b;
    const char *prefix = d.prefix;
    bool fused = plan.fused != 0;
    const bool late = plan.late != 0;
    const gather_kind &K = gather_kinds[d.p.kind];
    lh_buf *left = &(b->*K.left);
    const size_t slot_bytes = K.slot_bytes + K.slot_bytes_n * (size_t)N;
    /* the stage's read-backs land in 1 KiB of pinned memory: 64 occlusion totals, the hit count, the queue's appends and overflow flag */
    if (!a->h_read) HIPCHK(hipHostMalloc(&a->h_read, 1024, hipHostMallocDefault));
    unsigned long long *h_nocc64 = (unsigned long long *)a->h_read, *h_nhit = h_nocc64 + 64; uint32_t *h_qc = (uint32_t *)(h_nocc64 + 65);
    unsigned long long nhit = 0;
    if (!late) {
        HIPCHK(hipMemcpyAsync(h_nhit, d_nhit, sizeof(*h_nhit), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        nhit = *h_nhit;
        /* the persistent kernel's ray index has 32 bits; nothing was hit: nothing to trace, the resolve sees misses only */
        if (nhit * N >= (1ull << 31) || nhit == 0) fused = false;
    }
    const uint8_t *sun_occ = NULL;
    if (d.sun_dir) {
        const size_t ns = late ? nmax : (size_t)nhit;
        if (ns) {
            if (ensure_buf(&b->sun, ns * 49)) return -1;          /* org | dir | occ */
            double *sorg = (double *)b->sun.p, *sdir = sorg + 3 * ns;
            uint8_t *socc = (uint8_t *)(sdir + 3 * ns);
            if (lh_render_launch_sun_rays(ns, late ? d_nhit : NULL, (const double *)b->hitrec.p, d.sun_dir, sorg, sdir, s) != 0)
                return fail("%ssun ray kernel launch failed", prefix);
            lh_launch_opt o;
            if (late) { o.indexed = true; o.index = NULL; o.idx_nrays = (uint32_t)ns; o.n_dev = (const uint32_t *)d_nhit; }          /* the count's low word: it is below 2^31 */
            if (lh_launch(a, lh_batch_t{ns, LH_MODE_ANY, sorg, sdir, NULL, NULL, NULL, NULL, socc, NULL}, LH_VARIANT_DEFAULT, s, true, o) != 0) return -1;
            sun_occ = socc;
        }
    }
    if (tm) HIPCHK(hipEventRecord(tm->ev[3], s));
    const bool fused_tried = fused;
    uint32_t budget = 0;
    int qslot = -1;
    /* the stream's wait behind a fused launch, with the queue's words (and the late count) behind what is enqueued */
    auto wait_queue = [&]() -> int {
        if (late) HIPCHK(hipMemcpyAsync(h_nhit, d_nhit, sizeof(*h_nhit), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h_qc, a->aoq[qslot].q.qcount, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        nhit = *h_nhit;
        if (tm) fprintf(stderr, "[lucille_hip]   fused AO stage: %u rays through the fix-up queue (budget %u)\n", h_qc[0], budget);
        return 0;
    };
    if (fused) {
        const size_t nslots = late ? nmax : (size_t)nhit;
        if (ensure_buf(left, nslots * slot_bytes)) return -1;
        qslot = lh_aoq_slot(a, s);
        if (qslot < 0) return -1;
        lh_dev_scene_t sc = a->dev;          /* the launch's own scene: its visit budget, its clocks */
        sc.diag_clock = opt.diag_clock;
        if (a->ao_budget) sc.ray_budget = a->ao_budget;
        /* the tail a budget costs a launch is fixed, the queue a low budget sends to the sweep grows with the launch: a launch of
         * 2^27 rays or more doubles the default (config 5: whole frame 57.6 -> 56.7 ms, half of it 30.8 -> 29.9; a quarter and an
         * eighth are best at 384 -- tools/ao_budget_probe.py).  With the count on the device the kernel picks between the two */
        const uint32_t big = (a->ao_budget && !a->ao_budget_user) ? 2u * a->ao_budget : 0u;
        if (!late && big && nhit * N >= (1ull << 27)) sc.ray_budget = big;
        budget = sc.ray_budget;
        const lh_gather_src_t src = {nslots, g.ntheta, g.nphi, seed, (const double *)b->hitrec.p, (const unsigned long long *)b->key.p,
                                     late ? d_nhit : NULL, late ? big : 0u, d.p.lights, d.p.kind == LH_GATHER_AREA ? &d.p.area : NULL};
        const lh_launch_ctx_t ctx = {lh_next_cursor(a), a->grid_blocks, a->min_active, a->tri_batch, &a->aoq[qslot].q, a->ncus, (void *)s};
        const lh_fused_out_t fo = {d.p.kind, left->p, d.p.dirt.far_clip};
        if (lh_launch_trace_gather(&sc, &src, &fo, cnt, &ctx) != 0)
            return fail("%s%s launch failed: %s", prefix, K.fused_name, hipGetErrorString(hipGetLastError()));
        if (!late) {
            if (wait_queue() != 0) return -1;
            fused = h_qc[1] == 0;             /* more than LH_AO_QCAP uncertain gather rays: redo the stage materialised */
        }
    }
    /* stages 4-5 with the gather rays in HBM */
    auto materialised = [&]() -> int {
        const size_t nao = (size_t)(nhit * N);
        if (!nao) return 0;
        const bool closest = K.mode == LH_MODE_CLOSEST;          /* the records' t kept; else a byte per ray */
        if (ensure_buf(&b->aorg, nao * 24) || ensure_buf(&b->adir, nao * 24) || (!closest && ensure_buf(&b->occ, nao)) ||
            (K.item && ensure_buf(&b->bound, nao * 8))) return -1;
        /* 4. gather rays; an item kind's kernel writes the bound of every ray beside it */
        switch (d.p.kind) {
        case LH_GATHER_LIGHT:
            if (lh_render_launch_light_rays((size_t)nhit, NULL, d.p.lights, d.p.nlights, (const double *)b->hitrec.p, (double *)b->aorg.p, (double *)b->adir.p,
                                            (double *)b->bound.p, s) != 0)
                return fail("%slight ray kernel launch failed", prefix);
            break;
        case LH_GATHER_AREA:
            if (lh_render_launch_area_rays((size_t)nhit, NULL, &d.p.area, seed, (const double *)b->hitrec.p, (const unsigned long long *)b->key.p,
                                           (double *)b->aorg.p, (double *)b->adir.p, (double *)b->bound.p, NULL, s) != 0)
                return fail("%sarea-light ray kernel launch failed", prefix);
            break;
        default:
            if (lh_render_launch_ao_rays((size_t)nhit, g.ntheta, g.nphi, seed, (const double *)b->hitrec.p, (const double *)d_uniforms,
                                         (const unsigned long long *)b->key.p, (double *)b->aorg.p, (double *)b->adir.p, s) != 0)
                return fail("%sAO ray kernel launch failed", prefix);
        }
        /* 5. the launch.  The abandoned fused pass is not counted (nor is what the caller counted before the stage) */
        if (cnt && fused_tried) HIPCHK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * LH_CNT_DEV, s));
        if (!K.bounded)
            return lh_launch(a, lh_batch_t{nao, LH_MODE_ANY, b->aorg.p, b->adir.p, NULL, NULL, NULL, NULL, b->occ.p, cnt}, LH_VARIANT_DEFAULT, s, false, opt);
        if (!K.item) {          /* the dirt stage: one bound array of far_clip serves every chunk, as do the records' other members */
            const size_t nb = nao < LH_DIRT_CHUNK ? nao : LH_DIRT_CHUNK;
            if (ensure_buf(&b->t, nao * 8) || ensure_buf(&b->bound, nb * 8) || ensure_buf(&b->prim, nb * 4) || ensure_buf(&b->uv, nb * 16)) return -1;
            if (lh_render_launch_dirt_bounds(nb, d.p.dirt.far_clip, (double *)b->bound.p, s) != 0) return fail("%sbound kernel launch failed", prefix);
        }
        for (size_t off = 0; off < nao; off += LH_DIRT_CHUNK) {
            const size_t m = nao - off < LH_DIRT_CHUNK ? nao - off : LH_DIRT_CHUNK;
            lh_launch_opt o = opt;
            o.indexed = true; o.idx_nrays = (uint32_t)m; o.tmax = (const double *)b->bound.p + (K.item ? off : 0);
            lh_batch_t rays = {m, K.mode, (const double *)b->aorg.p + 3 * off, (const double *)b->adir.p + 3 * off, NULL, NULL, NULL, NULL, NULL, cnt};
            if (closest) { rays.prim = b->prim.p; rays.t = (double *)b->t.p + off; rays.u = b->uv.p; rays.v = (double *)b->uv.p + m; }
            else rays.occ = (uint8_t *)b->occ.p + off;
            if (lh_launch(a, rays, LH_VARIANT_DEFAULT, s, true, o) != 0) return -1;
        }
        return 0;
    };
    /* 6. radiance, and its totals on their way to the host */
    auto resolved = [&](bool from_fused) -> int {
        HIPCHK(hipMemsetAsync(d_nocc, 0, sizeof(unsigned long long) * 64, s));
        if (resolve(gather_left(d, g, seed, from_fused, sun_occ, d_nocc)) != 0) return -1;
        HIPCHK(hipMemcpyAsync(h_nocc64, d_nocc, sizeof(unsigned long long) * 64, hipMemcpyDeviceToHost, s));
        return 0;
    };
    if (!fused && materialised() != 0) return -1;
    if (tm) HIPCHK(hipEventRecord(tm->ev[4], s));
    if (resolved(fused) != 0) return -1;
    if (tm) HIPCHK(hipEventRecord(tm->ev[5], s));
    if (late) {
        /* the stage's one round trip: hit count, totals, the queue's overflow flag */
        if (wait_queue() != 0) return -1;
        if (h_qc[1] != 0) {                           /* more than LH_AO_QCAP uncertain gather rays: the stage once more, materialised */
            fused = false;
            if (materialised() != 0 || resolved(false) != 0) return -1;
            HIPCHK(hipStreamSynchronize(s));
        }
    } else HIPCHK(hipStreamSynchronize(s));
    out->nhit = nhit; out->nocc = 0; out->fused = fused;
    for (int k = 0; k < 64; k++) out->nocc += h_nocc64[k];
    if (cnt) HIPCHK(hipMemcpy(out->cnt, cnt, sizeof(out->cnt), hipMemcpyDeviceToHost));
    return 0;
}

/* NULL: the defaults (dirtmap.c:98,110-111); else the caller's, if lh_dirt.h accepts them */
static int dirt_params(const char *what, const lh_dirt_params_t *params, lh_dirt_params_t *out)
{
    const lh_dirt_params_t def = LH_DIRT_DEFAULTS;
    *out = params ? *params : def;
    if (!lh_dirt_params_ok(out->near_clip, out->far_clip, out->eps))
        return fail("%s: bad dirt parameters (near_clip %g, far_clip %g, eps %g: all finite, 0 <= near_clip < far_clip <= 1e38, eps >= 0)", what,
                    out->near_clip, out->far_clip, out->eps);
    return 0;
}

/* NULL: the defaults (gather_sunsky's offset, ri_ibl_sample_cosweight's scale); else the caller's, if lh_env.h accepts them */
static int env_params(const char *what, const lh_env_params_t *params, lh_env_params_t *out)
{
    const lh_env_params_t def = LH_ENV_DEFAULTS;
    *out = params ? *params : def;
    if (!lh_env_params_ok(out->eps, out->scale))
        return fail("%s: bad environment-gather parameters (eps %g, scale %g: both finite, eps >= 0, scale >= 0)", what, out->eps, out->scale);
    return 0;
}

/* what the light stage's entry points hand to gather_check as `params`: the caller's list and its parameters (NULL: LH_LIGHTS_DEFAULTS) */
struct lights_in { const lh_light_t *lights; int nlights; const lh_lights_params_t *params; };

/* what the area-light stage's entry points hand to gather_check: the caller's list, its parameters (NULL: LH_AREA_DEFAULTS) and the accelerator whose
 * emitter table the runs must lie in (NULL, or no table: none does) */
struct area_in { const lh_area_light_t *lights; int nlights; const lh_area_params_t *params; const lh_accel_t *a; };

/* the kind of an entry point and its caller's parameters (NULL: the defaults; AO has none), checked */
static int gather_check(const char *what, int kind, const void *params, gather_params *p)
{
    const lh_env_params_t env_def = LH_ENV_DEFAULTS;
    *p = gather_params{kind, 1.0e-6, lh_dirt_params_t{0.0, 0.0, 0.0}, env_def, NULL, 0, {}, {}};
    if (kind == LH_GATHER_DIRT) {
        if (dirt_params(what, (const lh_dirt_params_t *)params, &p->dirt) != 0) return -1;
        p->eps = p->dirt.eps;
    }
    if (kind == LH_GATHER_ENV) {
        if (env_params(what, (const lh_env_params_t *)params, &p->env) != 0) return -1;
        p->eps = p->env.eps;
    }
    if (kind == LH_GATHER_LIGHT) {
        const lights_in *in = (const lights_in *)params;
        const lh_lights_params_t def = LH_LIGHTS_DEFAULTS;
        p->eps = in->params ? in->params->eps : def.eps;
        if (!lh_lights_ok(in->lights, in->nlights, p->eps))
            return fail("%s: bad lights (1 .. %d lights in host memory, every v and rgb finite, a directional v not zero, flags within POINT | COSINE | INVSQ, "
                        "INVSQ only with POINT, reserved 0; eps %g finite and >= 0)", what, LH_LIGHTS_MAX, p->eps);
        p->lights = in->lights; p->nlights = in->nlights;
        p->items = ao_grid{1, in->nlights, in->nlights};
    }
    if (kind == LH_GATHER_AREA) {
        const area_in *in = (const area_in *)params;
        const lh_area_params_t def = LH_AREA_DEFAULTS, prm = in->params ? *in->params : def;
        const uint64_t table = in->a ? in->a->nemit : 0;
        if (!lh_area_lights_ok(in->lights, in->nlights, &prm, table))
            return fail("%s: bad area lights (1 .. %d lights in host memory, every rgb finite, flags within COSINE | FACING | INVSQ | PDF, reserved 0, ntris >= 1 "
                        "and first_tri + ntris within the %llu triangles of lh_accel_set_emitters; eps %g finite and >= 0, 0 < bound %g <= 1, nsamples %d in "
                        "1 .. %d, reserved 0)", what, LH_AREA_LIGHTS_MAX, (unsigned long long)table, prm.eps, prm.bound, (int)prm.nsamples, LH_AREA_SAMPLES_MAX);
        p->eps = prm.eps;
        memset(&p->area, 0, sizeof(p->area));
        memcpy(p->area.l, in->lights, sizeof(lh_area_light_t) * (size_t)in->nlights);
        p->area.emitters = (const lh_emitter_t *)in->a->d_emitters; p->area.uniforms = NULL; p->area.bound = prm.bound;
        p->area.L = in->nlights; p->area.S = prm.nsamples;
        p->items = ao_grid{p->area.L, p->area.S, p->area.L * p->area.S};
    }
    return 0;
}

/* one device batch of the gather pipeline over a Region (lh_render.hip): a rectangle, or nbands full-width bands.  p: the transport -- every kind runs
 * the same pipeline with its own origin, stage and resolve, in scratch of its own */
static int ao_region(lh_accel_t *a, const gather_params &p, const lh_camera_t *cam, int x0, int w, int nbands, int band_rows, const int *d_band_y0, int y0,
                     uint64_t valid_pixels, int ps, int gather_nsamples, uint64_t seed, const void *d_uniforms, void *d_rgb,
                     lh_tile_stats_t *stats, void *stream)
{
    const int h = nbands * band_rows;              /* lines of the batch */
    HIPCHK(hipSetDevice(a->device));
    hipStream_t s = (hipStream_t)stream;
    const ao_grid g = gather_grid(p, gather_nsamples);
    const size_t S = (size_t)w * h * ps * ps;
    if ((unsigned long long)cam->width * (unsigned long long)cam->height * (unsigned long long)(ps * ps) >= (1ull << 34))
        return fail("AO pipeline: more than 2^34 samples in the frame (slot keys carry 34 bits)");
    if (S >= ((size_t)1 << 31)) return fail("AO pipeline: more than 2^31 samples in one batch; render the frame in tiles");     /* 32-bit sample indices on the device */
    const unsigned nb = (unsigned)((S + 255) / 256);
    gather_desc d;
    gather_describe(a, p, LH_GATHER_TILE, &d);
    lh_gather_scratch *b = d.b;
    void *r_org, *r_dir, *r_prim, *r_t, *r_u, *r_v;          /* camera rays and their closest-hit records */
    if (p.kind == LH_GATHER_AO) {          /* the AO tile's own buffers: what lh_render_scratch shows */
        if (ensure_buf(&a->r_org, S * 24) || ensure_buf(&a->r_dir, S * 24) || ensure_buf(&a->r_prim, S * 4) ||
            ensure_buf(&a->r_t, S * 8) || ensure_buf(&a->r_u, S * 8) || ensure_buf(&a->r_v, S * 8)) return -1;
        r_org = a->r_org.p; r_dir = a->r_dir.p; r_prim = a->r_prim.p; r_t = a->r_t.p; r_u = a->r_u.p; r_v = a->r_v.p;
    } else {          /* one block of the kind's own (org | dir | t | u | v | prim): lh_render_scratch keeps showing the last AO tile */
        if (ensure_buf(&b->rays, S * 76)) return -1;
        double *base = (double *)b->rays.p;
        r_org = base; r_dir = base + 3 * S; r_t = base + 6 * S; r_u = base + 7 * S; r_v = base + 8 * S; r_prim = base + 9 * S;
    }
    if (ensure_buf(&b->slot, S * 4) || ensure_buf(&b->blocks, (size_t)nb * 4)) return -1;
    /* material textures (lh_tex.h): with at least one set, the resolve multiplies; with none, tex is NULL and the launch is the one it always was */
    const gather_kind &K = gather_kinds[p.kind];
    const bool no_tex = d.sky || K.item;          /* neither the sun-and-sky gather nor direct light fetches a texture */
    if (a->ntex && !no_tex && lh_tex_sync(a) != 0) return -1;
    d.tex = no_tex ? NULL : lh_tex_args(a, r_prim, r_u, r_v, &d.tex_store);
    /* lh_accel_trace_statistics: the counting instantiations of the same kernels, accumulated over the batch */
    unsigned long long *cnt = (a->stat_on && a->hs->bvh.ntris) ? a->d_counters : NULL;
    if (cnt) HIPCHK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * LH_CNT_DEV, s));
    /* LH_STAGE_TIMING=1: events between the stages, and the wall clock at which every persistent wave starts and leaves (two launches: closest, AO) */
    stage_timer timer, *tm = getenv("LH_STAGE_TIMING") ? &timer : NULL;
    const size_t nwaves = (size_t)a->grid_blocks * (LH_BLOCK / 64);
    lh_launch_opt opt;
    if (tm) {
        for (int k = 0; k < 6; k++) HIPCHK(hipEventCreate(&tm->ev[k]));
        HIPCHK(hipEventRecord(tm->ev[0], s));
        if (ensure_buf(&a->r_diag, sizeof(unsigned long long) * 6 * nwaves)) return -1;
        HIPCHK(hipMemsetAsync(a->r_diag.p, 0, sizeof(unsigned long long) * 6 * nwaves, s));
        opt.diag_clock = (unsigned long long *)a->r_diag.p;
    }
    /* 1. camera rays */
    if (lh_render_launch_primary_region(cam, x0, w, nbands, band_rows, d_band_y0, y0, cam->height, ps, ps,
                                        (double *)r_org, (double *)r_dir, s) != 0)
        return fail("primary ray kernel launch failed");
    if (tm) HIPCHK(hipEventRecord(tm->ev[1], s));
    /* 2. closest hit */
    if (lh_launch(a, lh_batch_t{S, LH_MODE_CLOSEST, r_org, r_dir, r_prim, r_t, r_u, r_v, NULL, cnt},
                  LH_VARIANT_DEFAULT, s, false, opt) != 0) return -1;
    if (tm) { HIPCHK(hipEventRecord(tm->ev[2], s)); opt.diag_clock += 3 * nwaves; }
    unsigned long long *d_nhit = a->d_total + 64;          /* the compaction's total, kept clear of the resolve's 64 counters */
    /* 6. the samples' values into the pixels */
    const lh_resolve_tile_t to = {w, h, band_rows, ps, ps, (const uint32_t *)b->slot.p, (float *)d_rgb, d.tex};
    auto resolve = [&](const lh_gather_left_t &left) -> int {
        if (lh_render_launch_tile_resolve(&to, &left, s) != 0) return fail("%s kernel launch failed", d.sky ? "sun-and-sky resolve" : K.resolve_name);
        return 0;
    };
    ao_totals tot = {};
    if (a->hs->bvh.ntris) {
        /* 3. compaction (deterministic: hits in sample order) */
        if (ensure_buf(&b->hitrec, S * 96) || ensure_buf(&b->key, S * 8)) return -1;   /* worst case: every sample hits */
        if (lh_render_launch_compact(&a->dev, (const double *)a->d_nrm9, S, (const double *)r_org,
                                     (const double *)r_dir, (const uint32_t *)r_prim, (const double *)r_t,
                                     (const double *)r_u, (const double *)r_v, (uint32_t *)b->blocks.p,
                                     (uint32_t *)b->slot.p, (double *)b->hitrec.p, (unsigned long long *)b->key.p,
                                     x0, w, nbands, band_rows, d_band_y0, y0, ps * ps, cam->width, a->d_total, p.eps, s) != 0)
            return fail("compaction kernels failed: %s", hipGetErrorString(hipGetLastError()));
        HIPCHK(hipMemcpyAsync(d_nhit, a->d_total, sizeof(*d_nhit), hipMemcpyDeviceToDevice, s));
        /* 4-6.  Fused and late or not: lh_gather.h; LH_AO_SYNC is read per call */
        const lh_gather_plan_t plan = lh_gather_plan(p.kind, LH_GATHER_TILE, S, (size_t)g.N, a->ao_fused, d_uniforms != NULL, (int)a->dev.ao_group,
                                                     d.sun_dir != NULL, getenv("LH_AO_SYNC") != NULL);
        if (ao_stage(a, d, S, g, seed, d_uniforms, d_nhit, a->d_total, cnt, opt, tm, plan, resolve, s, &tot) != 0) return -1;
    } else {          /* an empty scene: every sample is a miss */
        HIPCHK(hipMemsetAsync(b->slot.p, 0xFF, S * 4, s));
        HIPCHK(hipMemsetAsync(d_nhit, 0, sizeof(*d_nhit), s));
        if (tm) { HIPCHK(hipEventRecord(tm->ev[3], s)); HIPCHK(hipEventRecord(tm->ev[4], s)); }
        HIPCHK(hipMemsetAsync(a->d_total, 0, sizeof(unsigned long long) * 64, s));
        if (resolve(gather_left(d, g, seed, false, NULL, a->d_total)) != 0) return -1;
        if (tm) HIPCHK(hipEventRecord(tm->ev[5], s));
        HIPCHK(hipStreamSynchronize(s));
    }
    const size_t nao = (size_t)tot.nhit * g.N;
    if (tm && stage_report(*tm, a->r_diag.p, nwaves, S, tot.nhit, nao) != 0) return -1;
    if (p.kind == LH_GATHER_AO) { a->r_nsamples = S; a->r_nslots = (size_t)tot.nhit; a->r_nao = tot.fused ? 0 : nao; }
    if (cnt) {
        /* (an item kind counts its work items, traced or not: the camera rays and hits x N) */
        lh_stat_add(a, tot.cnt, K.item ? (unsigned long long)S + nao : tot.cnt[LH_CNT_RAYS], tot.nhit + tot.nocc, true);
        if (getenv("LH_DEBUG_COUNTERS")) {
            fprintf(stderr, "[lucille_hip] AO batch: rays by node visits (bucket b: [2^(b-1), 2^b)):");
            for (int k = 0; k < 24; k++) fprintf(stderr, " %llu", tot.cnt[LH_CNT_HIST + k]);
            fprintf(stderr, "\n");
        }
    }
    if (stats) {
        stats->primary_rays = valid_pixels * (uint64_t)(ps * ps); stats->primary_hits = tot.nhit; stats->ao_rays = nao; stats->ao_occluded = tot.nocc;
    }
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

/* lh_render_ao_tile, lh_render_dirt_tile (ri_transport_dirtmap per camera sample, dirtmap.c:234-292: a miss gives 0, a hit its dirt value) and
 * lh_render_env_tile (the environment-lit gather per camera sample -- gather_sunsky's loop with ri_texture_ibl_fetch as its sky,
 * ambientocclusion.c:206-324,407-411: a miss gives 0, a hit the three floats of lh_env_value), each times the texture of the hit's mesh where it has
 * one: the refusals, in their order -- the parameters before the accelerator -- and the region of one rectangle */
static int gather_tile(const char *what, int kind, const void *params, lh_accel_t *a, const lh_camera_t *cam, int x0, int y0, int w, int h, int ps,
                       int gather_nsamples, uint64_t seed, const void *d_uniforms, void *d_rgb, lh_tile_stats_t *stats, void *stream)
{
    lh_guard guard(a);
    gather_params p;
    if (gather_check(what, kind, params, &p) != 0) return -1;
    if (!a || !a->committed) return fail("%s: accel not committed", what);
    if (!cam || !d_rgb) return fail("%s: NULL argument", what);
    if (w <= 0 || h <= 0 || ps < 1 || gather_nsamples < 1) return fail("%s: bad tile/sample counts", what);
    return ao_region(a, p, cam, x0, w, 1, h, NULL, y0, (uint64_t)w * h, ps, gather_nsamples, seed, d_uniforms, d_rgb, stats, stream);
}

extern "C" int lh_render_ao_tile(lh_accel_t *a, const lh_camera_t *cam, int x0, int y0, int w, int h, int ps,
                                 int gather_nsamples, uint64_t seed, const void *d_uniforms, void *d_rgb,
                                 lh_tile_stats_t *stats, void *stream)
{
    return gather_tile("lh_render_ao_tile", LH_GATHER_AO, NULL, a, cam, x0, y0, w, h, ps, gather_nsamples, seed, d_uniforms, d_rgb, stats, stream);
}

extern "C" int lh_render_dirt_tile(lh_accel_t *a, const lh_camera_t *cam, int x0, int y0, int w, int h, int ps, int gather_nsamples,
                                   const lh_dirt_params_t *params, uint64_t seed, const void *d_uniforms, void *d_rgb,
                                   lh_tile_stats_t *stats, void *stream)
{
    return gather_tile("lh_render_dirt_tile", LH_GATHER_DIRT, params, a, cam, x0, y0, w, h, ps, gather_nsamples, seed, d_uniforms, d_rgb, stats, stream);
}

extern "C" int lh_render_env_tile(lh_accel_t *a, const lh_camera_t *cam, int x0, int y0, int w, int h, int ps, int gather_nsamples,
                                  const lh_env_params_t *params, uint64_t seed, const void *d_uniforms, void *d_rgb,
                                  lh_tile_stats_t *stats, void *stream)
{
    return gather_tile("lh_render_env_tile", LH_GATHER_ENV, params, a, cam, x0, y0, w, h, ps, gather_nsamples, seed, d_uniforms, d_rgb, stats, stream);
}

/* nbands full-width bands of band_rows lines (band b = frame lines band_y0[b] ...; a band that runs past the frame is
 * clipped) as ONE device batch: how a rank renders all of its interleaved shards of a frame with one set of launches.
 * d_rgb: float[nbands][band_rows][width][3], every band in image orientation (top line first) like a tile. */
extern "C" int lh_render_ao_bands(lh_accel_t *a, const lh_camera_t *cam, int nbands, const int *band_y0, int band_rows, int ps,
                                  int gather_nsamples, uint64_t seed, void *d_rgb, lh_tile_stats_t *stats, void *stream)
{
    lh_guard guard(a);
    if (!a || !a->committed) return fail("lh_render_ao_bands: accel not committed");
    if (!cam || !d_rgb || (nbands > 0 && !band_y0)) return fail("lh_render_ao_bands: NULL argument");
    if (nbands < 0 || band_rows <= 0 || ps < 1 || gather_nsamples < 1) return fail("lh_render_ao_bands: bad band/sample counts");
    if (nbands == 0) { if (stats) memset(stats, 0, sizeof(*stats)); return 0; }
    HIPCHK(hipSetDevice(a->device));
    uint64_t valid = 0;
    for (int b = 0; b < nbands; b++) {
        if (band_y0[b] < 0 || band_y0[b] >= cam->height) return fail("lh_render_ao_bands: band %d starts at line %d outside the frame", b, band_y0[b]);
        const int rows = (band_y0[b] + band_rows <= cam->height) ? band_rows : cam->height - band_y0[b];
        valid += (uint64_t)rows * cam->width;
    }
    if (ensure_buf(&a->r_bands, sizeof(int) * (size_t)nbands)) return -1;
    HIPCHK(hipMemcpyAsync(a->r_bands.p, band_y0, sizeof(int) * (size_t)nbands, hipMemcpyHostToDevice, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));          /* band_y0 is the caller's memory */
    gather_params p;
    if (gather_check("lh_render_ao_bands", LH_GATHER_AO, NULL, &p) != 0) return -1;
    return ao_region(a, p, cam, 0, cam->width, nbands, band_rows, (const int *)a->r_bands.p, 0, valid, ps, gather_nsamples, seed, NULL,
                     d_rgb, stats, stream);
}

/* the same tile for a plain-C host program: uniforms (optional) come from and the tile goes to HOST memory */
extern "C" int lh_render_ao_tile_host(lh_accel_t *a, const lh_camera_t *cam, int x0, int y0, int w, int h, int ps,
                                      int gather_nsamples, uint64_t seed, const double *uniforms, size_t nuniforms,
                                      float *rgb, lh_tile_stats_t *stats)
{
    lh_guard guard(a);
    if (!a || !a->committed) return fail("lh_render_ao_tile_host: accel not committed");
    if (!cam || !rgb) return fail("lh_render_ao_tile_host: NULL argument");
    if (w <= 0 || h <= 0) return fail("lh_render_ao_tile_host: bad tile");
    HIPCHK(hipSetDevice(a->device));
    const size_t need = uniforms ? (size_t)2 * ao_sample_grid(gather_nsamples).N * w * h * ps * ps : 0;       /* worst case: every sample hits */
    if (nuniforms < need) return fail("lh_render_ao_tile_host: %zu uniforms given, the tile may consume %zu", nuniforms, need);
    lh_field_t f[] = {lh_field_up(uniforms, need * sizeof(double)), lh_field_down(rgb, (size_t)w * h * 3 * sizeof(float))};
    if (lh_stage_up(a, f, 2) != 0) return -1;
    return lh_stage_down(a, f, 2, lh_render_ao_tile(a, cam, x0, y0, w, h, ps, gather_nsamples, seed, f[0].dev, f[1].dev, stats, a->stream));
}

/* ------------------------------------------------------------------------ */
/* a caller's batch of hit records: its own compaction, then ao_stage         */
/* ------------------------------------------------------------------------ */

/* what the three entry points refuse before they look at the accelerator's scene; 1: go on, 0: nothing to do (n_rays == 0) */
static int ao_batch_args(const char *what, const lh_accel_t *a, size_t n_rays, bool have_arrays, int gather_nsamples,
                         const void *key, const void *uniforms, const void *index, size_t n_index, const void *count,
                         const void *out32_a, const void *out32_b)
{
    if (gather_nsamples < 1) return fail("%s: gather_nsamples must be at least 1 (%d given)", what, gather_nsamples);
    if (n_rays >= ((size_t)1 << 31)) return fail("%s: 2^31 - 1 rays at most in one batch (%zu given)", what, n_rays);
    if (n_index > ((size_t)1 << 30)) return fail("%s: a list holds 2^30 entries at most (%zu given)", what, n_index);
    if ((((uintptr_t)index | (uintptr_t)count) & 3u) != 0) return fail("%s: the list and its count are 32-bit words: a pointer is not 4-byte aligned", what);
    if ((((uintptr_t)key | (uintptr_t)uniforms) & 7u) != 0) return fail("%s: keys and uniforms are 64-bit words: a pointer is not 8-byte aligned", what);
    if ((((uintptr_t)out32_a | (uintptr_t)out32_b) & 3u) != 0) return fail("%s: the outputs are 32-bit words: a pointer is not 4-byte aligned", what);
    if (!a || !a->committed) return fail("%s: accel not committed", what);
    if (n_rays == 0) return 0;
    if (!have_arrays) return fail("%s: NULL ray or record array", what);
    return 1;
}

/* lh_accel_ao_device / _dirt_device / _env_device behind their refusals: the same list, compaction and stage; the kind (p) has its origin, scratch of
 * its own and its resolve (d_occluded_count / d_radiance are near_hits / value for DIRT, the count and float[3 n_rays] for ENV) */
static int ao_batch_device(const char *what, lh_accel_t *a, const gather_params &p, size_t n_rays, const void *d_org, const void *d_dir, const void *d_prim,
                           const void *d_t, const void *d_u, const void *d_v, int gather_nsamples, uint64_t seed, const void *d_key,
                           const void *d_uniforms, const void *d_index, size_t n_index, const void *d_count,
                           void *d_occluded_count, void *d_radiance, void *stream)
{
    const int go = ao_batch_args(what, a, n_rays, d_org && d_dir && d_prim && d_t && d_u && d_v, gather_nsamples, d_key, d_uniforms,
                                 d_index, n_index, d_count, d_occluded_count, d_radiance);
    if (go <= 0) return go;
    if (!d_occluded_count && !d_radiance) return fail("%s: both outputs are NULL", what);
    const size_t L = (d_index || d_count || n_index) ? n_index : n_rays;          /* list entries; all NULL / 0: every ray */
    if (L == 0) return 0;
    HIPCHK(hipSetDevice(a->device));
    hipStream_t s = (hipStream_t)stream;
    const ao_grid g = gather_grid(p, gather_nsamples);
    gather_desc d;
    gather_describe(a, p, LH_GATHER_BATCH, &d);
    if (p.kind == LH_GATHER_AREA) d.p.area.uniforms = (const double *)d_uniforms;          /* the ray kernel and the resolve read them: 3 per item */
    lh_gather_scratch *b = d.b;
    if (ensure_buf(&b->totals, sizeof(unsigned long long) * 65)) return -1;
    unsigned long long *d_nhit = (unsigned long long *)b->totals.p, *d_nocc = d_nhit + 1;      /* the hits; the resolve's 64 counters */
    /* 6. per-ray count and value, scattered to the rays' own slots; slot_of_entry NULL: an empty scene */
    lh_resolve_list_t to = {L, n_rays, (const uint32_t *)d_index, (const uint32_t *)d_count, NULL, (uint32_t *)d_occluded_count, (float *)d_radiance};
    if (a->hs->bvh.ntris == 0) {          /* an empty scene: every traced ray is a miss, no record array is read */
        HIPCHK(hipMemsetAsync(d_nocc, 0, sizeof(unsigned long long) * 64, s));
        const lh_gather_left_t left = gather_left(d, g, seed, false, NULL, d_nocc);
        if (lh_render_launch_list_resolve(&to, &left, s) != 0)
            return fail("%s: resolve kernel launch failed: %s", what, hipGetErrorString(hipGetLastError()));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    }
    const unsigned nb = (unsigned)((L + 255) / 256);
    if (ensure_buf(&b->blocks, (size_t)nb * 4) || ensure_buf(&b->slot, L * 4) || ensure_buf(&b->hitrec, L * 96) ||
        ensure_buf(&b->key, L * 8)) return -1;                     /* worst case: every entry hits */
    to.slot_of_entry = (const uint32_t *)b->slot.p;
    unsigned long long *cnt = a->stat_on ? a->d_counters : NULL;          /* lh_accel_trace_statistics: as the tile pipelines' stage */
    if (cnt) HIPCHK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * LH_CNT_DEV, s));
    /* 3. compaction: hits in list order, the count stays on the device */
    if (lh_render_launch_batch_compact(&a->dev, (const double *)a->d_nrm9, L, n_rays, to.index, to.count, (const double *)d_org, (const double *)d_dir,
                                       (const uint32_t *)d_prim, (const double *)d_t, (const double *)d_u, (const double *)d_v,
                                       (const unsigned long long *)d_key, (uint32_t *)b->blocks.p, (uint32_t *)b->slot.p,
                                       (double *)b->hitrec.p, (unsigned long long *)b->key.p, d_nhit, NULL, p.eps, s) != 0)
        return fail("%s: compaction kernels failed: %s", what, hipGetErrorString(hipGetLastError()));
    /* 4-6.  Fused and late or not: lh_gather.h (a batch is not asked to read the count first) */
    const lh_gather_plan_t plan = lh_gather_plan(p.kind, LH_GATHER_BATCH, L, (size_t)g.N, a->ao_fused, d_uniforms != NULL, (int)a->dev.ao_group,
                                                 d.sun_dir != NULL, 0);
    auto resolve = [&](const lh_gather_left_t &left) -> int {
        if (lh_render_launch_list_resolve(&to, &left, s) != 0) return fail("%s: resolve kernel launch failed", what);
        return 0;
    };
    ao_totals tot;
    if (ao_stage(a, d, L, g, seed, d_uniforms, d_nhit, d_nocc, cnt, lh_launch_opt(), NULL, plan, resolve, s, &tot) != 0) return -1;
    if (cnt) lh_stat_add(a, tot.cnt, gather_kinds[p.kind].item ? tot.nhit * (unsigned long long)g.N : tot.cnt[LH_CNT_RAYS], tot.nocc, true);      /* (an item kind counts its work items, traced or not) */
    if (cnt && p.kind != LH_GATHER_AO) a->last_retraced = tot.cnt[LH_CNT_RETRACED];          /* the gather rays that went through the fix-up queue (lh_accel_last_retraced) */
    return 0;
}

/* the three device entry points: the parameters' refusal first, as ever */
static int gather_batch_device(const char *what, int kind, const void *params, lh_accel_t *a, size_t n_rays, const void *d_org, const void *d_dir,
                               const void *d_prim, const void *d_t, const void *d_u, const void *d_v, int gather_nsamples, uint64_t seed, const void *d_key,
                               const void *d_uniforms, const void *d_index, size_t n_index, const void *d_count, void *d_count_out, void *d_value_out,
                               void *stream)
{
    lh_guard guard(a);
    gather_params p;
    if (gather_check(what, kind, params, &p) != 0) return -1;
    return ao_batch_device(what, a, p, n_rays, d_org, d_dir, d_prim, d_t, d_u, d_v, gather_nsamples, seed, d_key, d_uniforms, d_index, n_index,
                           d_count, d_count_out, d_value_out, stream);
}

extern "C" int lh_accel_ao_device(lh_accel_t *a, size_t n_rays, const void *d_org, const void *d_dir, const void *d_prim, const void *d_t,
                                  const void *d_u, const void *d_v, int gather_nsamples, uint64_t seed, const void *d_key,
                                  const void *d_uniforms, const void *d_index, size_t n_index, const void *d_count,
                                  void *d_occluded_count, void *d_radiance, void *stream)
{
    return gather_batch_device("lh_accel_ao_device", LH_GATHER_AO, NULL, a, n_rays, d_org, d_dir, d_prim, d_t, d_u, d_v, gather_nsamples, seed, d_key,
                               d_uniforms, d_index, n_index, d_count, d_occluded_count, d_radiance, stream);
}

extern "C" int lh_accel_dirt_device(lh_accel_t *a, size_t n_rays, const void *d_org, const void *d_dir, const void *d_prim, const void *d_t,
                                    const void *d_u, const void *d_v, int gather_nsamples, const lh_dirt_params_t *params, uint64_t seed,
                                    const void *d_key, const void *d_uniforms, const void *d_index, size_t n_index, const void *d_count,
                                    void *d_near_hits, void *d_value, void *stream)
{
    return gather_batch_device("lh_accel_dirt_device", LH_GATHER_DIRT, params, a, n_rays, d_org, d_dir, d_prim, d_t, d_u, d_v, gather_nsamples, seed, d_key,
                               d_uniforms, d_index, n_index, d_count, d_near_hits, d_value, stream);
}

extern "C" int lh_accel_env_device(lh_accel_t *a, size_t n_rays, const void *d_org, const void *d_dir, const void *d_prim, const void *d_t,
                                   const void *d_u, const void *d_v, int gather_nsamples, const lh_env_params_t *params, uint64_t seed,
                                   const void *d_key, const void *d_uniforms, const void *d_index, size_t n_index, const void *d_count,
                                   void *d_occluded_count, void *d_rgb, void *stream)
{
    return gather_batch_device("lh_accel_env_device", LH_GATHER_ENV, params, a, n_rays, d_org, d_dir, d_prim, d_t, d_u, d_v, gather_nsamples, seed, d_key,
                               d_uniforms, d_index, n_index, d_count, d_occluded_count, d_rgb, stream);
}

/* lh_accel_ao_rays_device / _light_rays_device / _area_light_rays_device behind the refusal of their parameters (p: from gather_check; AO has none): only
 * the gather rays of the batch's hits, for a caller who traces them itself -- the compaction's slots and count, then the kind's ray kernel with the count
 * read on the device.  doubles: how the alignment refusal names the double outputs; d_tmax_out: an item kind's bounds, d_weight_out (or NULL): the area
 * kind's weights.  Asynchronous: a table of lights travels in the ray kernel's arguments, nothing is read back */
static int gather_rays_device(const char *what, lh_accel_t *a, gather_params p, size_t n_rays, const void *d_org, const void *d_dir, const void *d_prim,
                              const void *d_t, const void *d_u, const void *d_v, int gather_nsamples, uint64_t seed, const void *d_key, const void *d_uniforms,
                              void *d_slot_of_ray, void *d_nslots, void *d_org_out, void *d_dir_out, void *d_tmax_out, void *d_weight_out, const char *doubles,
                              size_t capacity_rays, void *stream)
{
    const bool item = gather_kinds[p.kind].item;
    if ((((uintptr_t)d_org_out | (uintptr_t)d_dir_out | (uintptr_t)d_tmax_out | (uintptr_t)d_weight_out) & 7u) != 0)
        return fail("%s: the %s arrays are doubles: a pointer is not 8-byte aligned", what, doubles);
    const int go = ao_batch_args(what, a, n_rays, d_org && d_dir && d_prim && d_t && d_u && d_v, gather_nsamples, d_key, d_uniforms,
                                 NULL, 0, NULL, d_slot_of_ray, d_nslots);
    if (go < 0) return go;
    hipStream_t s = (hipStream_t)stream;
    if (go == 0) {
        if (d_nslots) { HIPCHK(hipSetDevice(a->device)); HIPCHK(hipMemsetAsync(d_nslots, 0, sizeof(uint32_t), s)); }
        return 0;
    }
    if (!d_slot_of_ray || !d_nslots || !d_org_out || !d_dir_out || (item && !d_tmax_out)) return fail("%s: NULL output array", what);
    const ao_grid g = gather_grid(p, gather_nsamples);
    const size_t N = (size_t)g.N;
    if (capacity_rays / N < n_rays || (!item && capacity_rays < n_rays * N))
        return fail("%s: capacity_rays %zu does not cover the worst case n_rays * %s = %zu x %zu", what, capacity_rays,
                    p.kind == LH_GATHER_AO ? "N" : p.kind == LH_GATHER_LIGHT ? "nlights" : "nlights * nsamples", n_rays, N);
    if (!item && (n_rays * N + 255) / 256 > 0x7fffffffu) return fail("%s: more than 2^39 AO rays in one call", what);
    HIPCHK(hipSetDevice(a->device));
    if (a->hs->bvh.ntris == 0) {
        HIPCHK(hipMemsetAsync(d_slot_of_ray, 0xFF, n_rays * 4, s));
        HIPCHK(hipMemsetAsync(d_nslots, 0, sizeof(uint32_t), s));
        return 0;
    }
    const unsigned nb = (unsigned)((n_rays + 255) / 256);
    lh_gather_scratch *b = &a->gather[p.kind][LH_GATHER_BATCH];
    if (ensure_buf(&b->totals, sizeof(unsigned long long) * 65) || ensure_buf(&b->blocks, (size_t)nb * 4) ||
        ensure_buf(&b->hitrec, n_rays * 96) || ensure_buf(&b->key, n_rays * 8)) return -1;
    unsigned long long *d_nhit = (unsigned long long *)b->totals.p;
    if (lh_render_launch_batch_compact(&a->dev, (const double *)a->d_nrm9, n_rays, n_rays, NULL, NULL, (const double *)d_org, (const double *)d_dir,
                                       (const uint32_t *)d_prim, (const double *)d_t, (const double *)d_u, (const double *)d_v,
                                       (const unsigned long long *)d_key, (uint32_t *)b->blocks.p, (uint32_t *)d_slot_of_ray,
                                       (double *)b->hitrec.p, (unsigned long long *)b->key.p, d_nhit, (uint32_t *)d_nslots, p.eps, s) != 0)
        return fail("%s: compaction kernels failed: %s", what, hipGetErrorString(hipGetLastError()));
    switch (p.kind) {
    case LH_GATHER_LIGHT:
        if (lh_render_launch_light_rays(n_rays, d_nhit, p.lights, p.nlights, (const double *)b->hitrec.p, (double *)d_org_out, (double *)d_dir_out,
                                        (double *)d_tmax_out, s) != 0)
            return fail("%s: light ray kernel launch failed: %s", what, hipGetErrorString(hipGetLastError()));
        return 0;
    case LH_GATHER_AREA:
        p.area.uniforms = (const double *)d_uniforms;
        if (lh_render_launch_area_rays(n_rays, d_nhit, &p.area, seed, (const double *)b->hitrec.p, (const unsigned long long *)b->key.p, (double *)d_org_out,
                                       (double *)d_dir_out, (double *)d_tmax_out, (double *)d_weight_out, s) != 0)
            return fail("%s: area-light ray kernel launch failed: %s", what, hipGetErrorString(hipGetLastError()));
        return 0;
    default:
        if (lh_render_launch_ao_rays_counted(n_rays, d_nhit, g.ntheta, g.nphi, seed, (const double *)b->hitrec.p, (const double *)d_uniforms,
                                             (const unsigned long long *)b->key.p, (double *)d_org_out, (double *)d_dir_out, s) != 0)
            return fail("%s: AO ray kernel launch failed: %s", what, hipGetErrorString(hipGetLastError()));
        return 0;
    }
}

extern "C" int lh_accel_ao_rays_device(lh_accel_t *a, size_t n_rays, const void *d_org, const void *d_dir, const void *d_prim, const void *d_t,
                                       const void *d_u, const void *d_v, int gather_nsamples, uint64_t seed, const void *d_key,
                                       const void *d_uniforms, void *d_slot_of_ray, void *d_nslots, void *d_ao_org, void *d_ao_dir,
                                       size_t capacity_rays, void *stream)
{
    lh_guard guard(a);
    const char *what = "lh_accel_ao_rays_device";
    gather_params p;
    if (gather_check(what, LH_GATHER_AO, NULL, &p) != 0) return -1;          /* (no parameters: the double outputs' alignment is its first refusal) */
    return gather_rays_device(what, a, p, n_rays, d_org, d_dir, d_prim, d_t, d_u, d_v, gather_nsamples, seed, d_key, d_uniforms, d_slot_of_ray, d_nslots,
                              d_ao_org, d_ao_dir, NULL, NULL, "ray", capacity_rays, stream);
}

/* lh_accel_ao_host / _dirt_host / _env_host (radiance: 3 floats per ray for ENV): the parameters' refusal first, then host arrays up, the device call
 * on the accelerator's stream, the outputs down */
static int gather_batch_host(const char *what, int kind, const void *params, lh_accel_t *a, size_t n_rays, const double *org, const double *dir,
                             const uint32_t *prim, const double *t, const double *u, const double *v, int gather_nsamples, uint64_t seed, const uint64_t *key,
                             const double *uniforms, size_t nuniforms, uint32_t *occluded_count, float *radiance)
{
    lh_guard guard(a);
    gather_params p;
    if (gather_check(what, kind, params, &p) != 0) return -1;
    const int go = ao_batch_args(what, a, n_rays, org && dir && prim && t && u && v, gather_nsamples, NULL, NULL, NULL, 0, NULL, NULL, NULL);
    if (go <= 0) return go;
    if (!occluded_count && !radiance) return fail("%s: both outputs are NULL", what);
    const size_t n = n_rays;
    const gather_kind &K = gather_kinds[kind];
    const size_t need = uniforms ? (size_t)K.uniforms_per_item * gather_grid(p, gather_nsamples).N * n : 0;          /* worst case: every ray hits */
    if (nuniforms < need) return fail("%s: %zu uniforms given, the batch may consume %zu", what, nuniforms, need);
    HIPCHK(hipSetDevice(a->device));
    const size_t b_ray = sizeof(double) * 3 * n, b_d = sizeof(double) * n, b_u32 = sizeof(uint32_t) * n;
    enum { ORG, DIR, T, U, V, PRIM, KEY, UNI, CNT, RAD, NF };
    lh_field_t f[NF] = {lh_field_up(org, b_ray), lh_field_up(dir, b_ray), lh_field_up(t, b_d), lh_field_up(u, b_d), lh_field_up(v, b_d), lh_field_up(prim, b_u32),
                        lh_field_up(key, sizeof(uint64_t) * n), lh_field_up(uniforms, need * sizeof(double)),
                        lh_field_down(occluded_count, b_u32), lh_field_down(radiance, sizeof(float) * K.radiance_floats * n)};
    if (lh_stage_up(a, f, NF) != 0) return -1;
    return lh_stage_down(a, f, NF, ao_batch_device(K.device_name, a, p, n, f[ORG].dev, f[DIR].dev, f[PRIM].dev, f[T].dev, f[U].dev, f[V].dev, gather_nsamples, seed,
                                                   f[KEY].dev, f[UNI].dev, NULL, 0, NULL, f[CNT].dev, f[RAD].dev, a->stream));
}

extern "C" int lh_accel_ao_host(lh_accel_t *a, size_t n_rays, const double *org, const double *dir, const uint32_t *prim, const double *t,
                                const double *u, const double *v, int gather_nsamples, uint64_t seed, const uint64_t *key,
                                const double *uniforms, size_t nuniforms, uint32_t *occluded_count, float *radiance)
{
    return gather_batch_host("lh_accel_ao_host", LH_GATHER_AO, NULL, a, n_rays, org, dir, prim, t, u, v, gather_nsamples, seed, key, uniforms, nuniforms,
                             occluded_count, radiance);
}

extern "C" int lh_accel_dirt_host(lh_accel_t *a, size_t n_rays, const double *org, const double *dir, const uint32_t *prim, const double *t,
                                  const double *u, const double *v, int gather_nsamples, const lh_dirt_params_t *params, uint64_t seed,
                                  const uint64_t *key, const double *uniforms, size_t nuniforms, uint32_t *near_hits, float *value)
{
    return gather_batch_host("lh_accel_dirt_host", LH_GATHER_DIRT, params, a, n_rays, org, dir, prim, t, u, v, gather_nsamples, seed, key, uniforms, nuniforms,
                             near_hits, value);
}

extern "C" int lh_accel_env_host(lh_accel_t *a, size_t n_rays, const double *org, const double *dir, const uint32_t *prim, const double *t,
                                 const double *u, const double *v, int gather_nsamples, const lh_env_params_t *params, uint64_t seed,
                                 const uint64_t *key, const double *uniforms, size_t nuniforms, uint32_t *occluded_count, float *rgb)
{
    return gather_batch_host("lh_accel_env_host", LH_GATHER_ENV, params, a, n_rays, org, dir, prim, t, u, v, gather_nsamples, seed, key, uniforms, nuniforms,
                             occluded_count, rgb);
}

/* ---- direct light (lh_lights.h): the same list, compaction, stage and resolves with a light per "sample"; no keys, seed or uniforms ---- */
extern "C" int lh_accel_lights_device(lh_accel_t *a, size_t n_rays, const void *d_org, const void *d_dir, const void *d_prim, const void *d_t,
                                      const void *d_u, const void *d_v, const lh_light_t *lights, int nlights, const lh_lights_params_t *params,
                                      const void *d_index, size_t n_index, const void *d_count, void *d_visible, void *d_rgb, void *stream)
{
    const lights_in in = {lights, nlights, params};
    return gather_batch_device("lh_accel_lights_device", LH_GATHER_LIGHT, &in, a, n_rays, d_org, d_dir, d_prim, d_t, d_u, d_v, 1, 0, NULL, NULL,
                               d_index, n_index, d_count, d_visible, d_rgb, stream);
}

extern "C" int lh_accel_lights_host(lh_accel_t *a, size_t n_rays, const double *org, const double *dir, const uint32_t *prim, const double *t,
                                    const double *u, const double *v, const lh_light_t *lights, int nlights, const lh_lights_params_t *params,
                                    uint32_t *visible, float *rgb)
{
    const lights_in in = {lights, nlights, params};
    return gather_batch_host("lh_accel_lights_host", LH_GATHER_LIGHT, &in, a, n_rays, org, dir, prim, t, u, v, 1, 0, NULL, NULL, 0, visible, rgb);
}

extern "C" int lh_render_lights_tile(lh_accel_t *a, const lh_camera_t *cam, int x0, int y0, int w, int h, int ps, const lh_light_t *lights, int nlights,
                                     const lh_lights_params_t *params, void *d_rgb, lh_tile_stats_t *stats, void *stream)
{
    const lights_in in = {lights, nlights, params};
    return gather_tile("lh_render_lights_tile", LH_GATHER_LIGHT, &in, a, cam, x0, y0, w, h, ps, 1, 0, NULL, d_rgb, stats, stream);
}

/* the shadow rays alone (gather_rays_device): ray (slot, l) and its bound at element slot * L + l */
extern "C" int lh_accel_light_rays_device(lh_accel_t *a, size_t n_rays, const void *d_org, const void *d_dir, const void *d_prim, const void *d_t,
                                          const void *d_u, const void *d_v, const lh_light_t *lights, int nlights, const lh_lights_params_t *params,
                                          void *d_slot_of_ray, void *d_nslots, void *d_org_out, void *d_dir_out, void *d_tmax_out,
                                          size_t capacity_rays, void *stream)
{
    lh_guard guard(a);
    const char *what = "lh_accel_light_rays_device";
    const lights_in in = {lights, nlights, params};
    gather_params p;
    if (gather_check(what, LH_GATHER_LIGHT, &in, &p) != 0) return -1;
    return gather_rays_device(what, a, p, n_rays, d_org, d_dir, d_prim, d_t, d_u, d_v, 1, 0, NULL, NULL, d_slot_of_ray, d_nslots, d_org_out, d_dir_out,
                              d_tmax_out, NULL, "ray and bound", capacity_rays, stream);
}

/* ---- area lights (lh_area.h): the light stage's pipeline with S samples per light, the AO stage's seed, keys and replayed uniforms ---- */

/* the emitter table: records made on the host (lh_area_emitter), one block on the device that the accelerator owns.  A block that is replaced or removed
 * is released behind a device-wide synchronise, as a texture's (lh_tex.hip): every launch enqueued earlier that may read it has finished.  Nothing of a
 * commit or re-commit touches it */
extern "C" int lh_accel_set_emitters(lh_accel_t *a, const double *tri_xyz, size_t ntris)
{
    lh_guard guard(a);
    const char *what = "lh_accel_set_emitters";
    const bool remove = !tri_xyz && ntris == 0;
    if (!remove) {          /* the array first: refused whatever the accelerator is, before anything touches a device */
        if (!tri_xyz || ntris == 0) return fail("%s: bad emitters (a NULL array with a count, or an array of no triangles)", what);
        if ((uint64_t)ntris >= LH_AREA_EMITTERS_MAX) return fail("%s: bad emitters (%zu triangles: fewer than 2^31)", what, ntris);
        if (((uintptr_t)tri_xyz & 7u) != 0) return fail("%s: bad emitters (vertices are doubles: the pointer is not 8-byte aligned)", what);
        for (size_t k = 0; k < 9 * ntris; k++)
            if (!lh_area_fin(tri_xyz[k])) return fail("%s: bad emitters (triangle %zu has a vertex that is not finite)", what, k / 9);
    }
    if (!a || !a->committed) return fail("%s: accel not committed", what);
    HIPCHK(hipSetDevice(a->device));
    void *d_new = NULL;
    if (!remove) {
        lh_emitter_t *rec = (lh_emitter_t *)malloc(sizeof(lh_emitter_t) * ntris);
        if (!rec) return fail("%s: out of memory", what);
        for (size_t k = 0; k < ntris; k++) lh_area_emitter(tri_xyz + 9 * k, rec + k);
        hipError_t e = hipMalloc(&d_new, sizeof(lh_emitter_t) * ntris);          /* (256-byte aligned: every record is one line) */
        if (e == hipSuccess) e = hipMemcpy(d_new, rec, sizeof(lh_emitter_t) * ntris, hipMemcpyHostToDevice);
        free(rec);
        if (e != hipSuccess) { (void)hipGetLastError(); if (d_new) (void)hipFree(d_new); return fail("%s: uploading the table failed: %s", what, hipGetErrorString(e)); }
    }
    if (a->d_emitters) { HIPCHK(hipDeviceSynchronize()); (void)hipFree(a->d_emitters); }
    a->d_emitters = d_new; a->nemit = remove ? 0 : (uint64_t)ntris;
    return 0;
}

extern "C" int lh_accel_area_lights_device(lh_accel_t *a, size_t n_rays, const void *d_org, const void *d_dir, const void *d_prim, const void *d_t,
                                           const void *d_u, const void *d_v, const lh_area_light_t *lights, int nlights, const lh_area_params_t *params,
                                           uint64_t seed, const void *d_key, const void *d_uniforms, const void *d_index, size_t n_index, const void *d_count,
                                           void *d_visible, void *d_rgb, void *stream)
{
    lh_guard guard(a);          /* (recursive: the table's count is read under the lock the stage then holds) */
    const area_in in = {lights, nlights, params, a};
    return gather_batch_device("lh_accel_area_lights_device", LH_GATHER_AREA, &in, a, n_rays, d_org, d_dir, d_prim, d_t, d_u, d_v, 1, seed, d_key, d_uniforms,
                               d_index, n_index, d_count, d_visible, d_rgb, stream);
}

extern "C" int lh_accel_area_lights_host(lh_accel_t *a, size_t n_rays, const double *org, const double *dir, const uint32_t *prim, const double *t,
                                         const double *u, const double *v, const lh_area_light_t *lights, int nlights, const lh_area_params_t *params,
                                         uint64_t seed, const uint64_t *key, const double *uniforms, size_t nuniforms, uint32_t *visible, float *rgb)
{
    lh_guard guard(a);
    const area_in in = {lights, nlights, params, a};
    return gather_batch_host("lh_accel_area_lights_host", LH_GATHER_AREA, &in, a, n_rays, org, dir, prim, t, u, v, 1, seed, key, uniforms, nuniforms, visible, rgb);
}

extern "C" int lh_render_area_lights_tile(lh_accel_t *a, const lh_camera_t *cam, int x0, int y0, int w, int h, int ps, const lh_area_light_t *lights, int nlights,
                                          const lh_area_params_t *params, uint64_t seed, void *d_rgb, lh_tile_stats_t *stats, void *stream)
{
    lh_guard guard(a);
    const area_in in = {lights, nlights, params, a};
    return gather_tile("lh_render_area_lights_tile", LH_GATHER_AREA, &in, a, cam, x0, y0, w, h, ps, 1, seed, NULL, d_rgb, stats, stream);
}

/* the rays alone (gather_rays_device): item (slot, l, s) with its bound and weight (d_weight_out may be NULL) at element (slot * L + l) * S + s */
extern "C" int lh_accel_area_light_rays_device(lh_accel_t *a, size_t n_rays, const void *d_org, const void *d_dir, const void *d_prim, const void *d_t,
                                               const void *d_u, const void *d_v, const lh_area_light_t *lights, int nlights, const lh_area_params_t *params,
                                               uint64_t seed, const void *d_key, const void *d_uniforms, void *d_slot_of_ray, void *d_nslots,
                                               void *d_org_out, void *d_dir_out, void *d_tmax_out, void *d_weight_out, size_t capacity_rays, void *stream)
{
    lh_guard guard(a);
    const char *what = "lh_accel_area_light_rays_device";
    const area_in in = {lights, nlights, params, a};
    gather_params p;
    if (gather_check(what, LH_GATHER_AREA, &in, &p) != 0) return -1;
    return gather_rays_device(what, a, p, n_rays, d_org, d_dir, d_prim, d_t, d_u, d_v, 1, seed, d_key, d_uniforms, d_slot_of_ray, d_nslots, d_org_out, d_dir_out,
                              d_tmax_out, d_weight_out, "ray, bound and weight", capacity_rays, stream);
}

/* the fetch alone: ri_texture_ibl_fetch (env_fetch, lh_pt.h) of the accelerator's environment for n directions.  Asynchronous, nothing read back */
extern "C" int lh_accel_environment_device(lh_accel_t *a, size_t n, const void *d_dir, void *d_rgb, void *stream)
{
    lh_guard guard(a);
    const char *what = "lh_accel_environment_device";
    if (!a || !a->committed) return fail("%s: accel not committed", what);
    if (n == 0) return 0;
    if (!d_dir || !d_rgb) return fail("%s: NULL array", what);
    if (((uintptr_t)d_dir & 7u) != 0) return fail("%s: directions are doubles: the pointer is not 8-byte aligned", what);
    if (((uintptr_t)d_rgb & 3u) != 0) return fail("%s: the output holds floats: the pointer is not 4-byte aligned", what);
    if (n >= ((size_t)1 << 39)) return fail("%s: more than 2^39 directions in one call", what);
    HIPCHK(hipSetDevice(a->device));
    const lh_env_src_t esrc = lh_env_source(a);
    if (lh_render_launch_env_fetch(n, &esrc, (const double *)d_dir, (float *)d_rgb, stream) != 0)
        return fail("%s: kernel launch failed: %s", what, hipGetErrorString(hipGetLastError()));
    return 0;
}

/* the same for HOST arrays: copies up, the device call on the accelerator's stream, copies down */
extern "C" int lh_accel_environment_host(lh_accel_t *a, size_t n, const double *dir, float *rgb)
{
    lh_guard guard(a);
    const char *what = "lh_accel_environment_host";
    if (!a || !a->committed) return fail("%s: accel not committed", what);
    if (n == 0) return 0;
    if (!dir || !rgb) return fail("%s: NULL array", what);
    if (n >= ((size_t)1 << 39)) return fail("%s: more than 2^39 directions in one call", what);
    HIPCHK(hipSetDevice(a->device));
    lh_field_t f[] = {lh_field_up(dir, sizeof(double) * 3 * n), lh_field_down(rgb, sizeof(float) * 3 * n)};
    if (lh_stage_up(a, f, 2) != 0) return -1;
    return lh_stage_down(a, f, 2, lh_accel_environment_device(a, n, f[0].dev, f[1].dev, a->stream));
}

/* the sun-and-sky light (lh_sky.h): set after commit, as the environment; the struct is copied, its Perez denominators are made here; NULL removes it */
extern "C" int lh_accel_set_sky(lh_accel_t *a, const lh_sky_t *sky)
{
    lh_guard guard(a);
    if (sky && !lh_sky_ok(sky)) return fail("lh_accel_set_sky: bad sky parameters (every field finite, flags within LH_SKY_SUN)");
    if (!a || !a->committed) return fail("lh_accel_set_sky: accel not committed");
    if (!sky) { memset(&a->sky, 0, sizeof(a->sky)); a->sky_set = 0; return 0; }
    a->sky.sky = *sky;
    lh_sky_den(sky, a->sky.den);
    a->sky_set = 1;
    return 0;
}

/* the fetch alone: lh_sky_rgb of the accelerator's sky for n directions.  Asynchronous, nothing read back */
extern "C" int lh_accel_sky_device(lh_accel_t *a, size_t n, const void *d_dir, void *d_rgb, void *stream)
{
    lh_guard guard(a);
    const char *what = "lh_accel_sky_device";
    if (!a || !a->committed) return fail("%s: accel not committed", what);
    if (!a->sky_set) return fail("%s: no sky is set (lh_accel_set_sky)", what);
    if (n == 0) return 0;
    if (!d_dir || !d_rgb) return fail("%s: NULL array", what);
    if (((uintptr_t)d_dir & 7u) != 0) return fail("%s: directions are doubles: the pointer is not 8-byte aligned", what);
    if (((uintptr_t)d_rgb & 3u) != 0) return fail("%s: the output holds floats: the pointer is not 4-byte aligned", what);
    if (n >= ((size_t)1 << 39)) return fail("%s: more than 2^39 directions in one call", what);
    HIPCHK(hipSetDevice(a->device));
    if (lh_render_launch_sky_fetch(n, &a->sky, (const double *)d_dir, (float *)d_rgb, stream) != 0)
        return fail("%s: kernel launch failed: %s", what, hipGetErrorString(hipGetLastError()));
    return 0;
}

/* the same for HOST arrays: copies up, the device call on the accelerator's stream, copies down */
extern "C" int lh_accel_sky_host(lh_accel_t *a, size_t n, const double *dir, float *rgb)
{
    lh_guard guard(a);
    const char *what = "lh_accel_sky_host";
    if (!a || !a->committed) return fail("%s: accel not committed", what);
    if (!a->sky_set) return fail("%s: no sky is set (lh_accel_set_sky)", what);
    if (n == 0) return 0;
    if (!dir || !rgb) return fail("%s: NULL array", what);
    if (n >= ((size_t)1 << 39)) return fail("%s: more than 2^39 directions in one call", what);
    HIPCHK(hipSetDevice(a->device));
    lh_field_t f[] = {lh_field_up(dir, sizeof(double) * 3 * n), lh_field_down(rgb, sizeof(float) * 3 * n)};
    if (lh_stage_up(a, f, 2) != 0) return -1;
    return lh_stage_down(a, f, 2, lh_accel_sky_device(a, n, f[0].dev, f[1].dev, a->stream));
}

extern "C" int lh_render_scratch(lh_accel_t *a, int which, void **d_ptr, size_t *count)
{
    lh_guard guard(a);
    if (!a || !a->committed || !d_ptr || !count) return fail("lh_render_scratch: bad argument");
    lh_gather_scratch *t = &a->gather[LH_GATHER_AO][LH_GATHER_TILE];          /* the last AO tile's */
    lh_buf *b[] = {&a->r_org, &a->r_dir, &a->r_prim, &a->r_t, &a->r_u, &a->r_v, &t->slot, &t->hitrec, &t->aorg, &t->adir, &t->occ};
    if (which < 0 || which > 10) return fail("lh_render_scratch: unknown buffer %d", which);
    *d_ptr = b[which]->p;
    *count = which <= 6 ? a->r_nsamples : (which == 7 ? a->r_nslots : a->r_nao);
    return 0;
}

/* ------------------------------------------------------------------------ */
/* hit epilogue for a batch (ri_intersection_state_build)                   */
/* ------------------------------------------------------------------------ */

extern "C" int lh_accel_state_build_device(lh_accel_t *a, size_t n, const void *d_org, const void *d_dir, const void *d_prim,
                                           const void *d_t, const void *d_u, const void *d_v, void *d_state, void *stream)
{
    lh_guard guard(a);
    if (!a || !a->committed) return fail("lh_accel_state_build_device: accel not committed");
    if (n == 0 || a->hs->bvh.ntris == 0) return 0;
    if (!d_org || !d_dir || !d_prim || !d_t || !d_u || !d_v || !d_state) return fail("lh_accel_state_build_device: NULL argument");
    HIPCHK(hipSetDevice(a->device));
    if (lh_render_launch_state_build(n, &a->dev, (const double *)a->d_nrm9, (const double *)a->d_attr9[0], (const double *)a->d_attr9[1],
                                     (const double *)a->d_attr9[2], (const double *)a->d_st6, (const uint8_t *)a->d_inside,
                                     (const double *)d_org, (const double *)d_dir, (const uint32_t *)d_prim, (const double *)d_t,
                                     (const double *)d_u, (const double *)d_v, (double *)d_state, stream) != 0)
        return fail("state-build kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

extern "C" int lh_accel_state_build_host(lh_accel_t *a, size_t n, const double *org, const double *dir, const uint32_t *prim,
                                         const double *t, const double *u, const double *v, double *state)
{
    lh_guard guard(a);
    if (!a || !a->committed) return fail("lh_accel_state_build_host: accel not committed");
    if (n == 0) return 0;
    if (!org || !dir || !prim || !t || !u || !v || !state) return fail("lh_accel_state_build_host: NULL argument");
    HIPCHK(hipSetDevice(a->device));
    const size_t b_ray = sizeof(double) * 3 * n, b_d = sizeof(double) * n, b_state = sizeof(double) * LH_STATE_DOUBLES * n;
    enum { STATE, ORG, DIR, T, U, V, PRIM, NF };
    lh_field_t f[NF] = {lh_field_down(state, b_state), lh_field_up(org, b_ray), lh_field_up(dir, b_ray), lh_field_up(t, b_d), lh_field_up(u, b_d), lh_field_up(v, b_d),
                        lh_field_up(prim, sizeof(uint32_t) * n)};
    if (lh_stage_up(a, f, NF) != 0) return -1;
    const hipError_t e = hipMemsetAsync(f[STATE].dev, 0, b_state, a->stream);          /* a miss's state, and every state of an empty scene, is zeros */
    return lh_stage_down(a, f, NF, e != hipSuccess ? fail("hipMemsetAsync of the states failed: %s", hipGetErrorString(e))
                                                   : lh_accel_state_build_device(a, n, f[ORG].dev, f[DIR].dev, f[PRIM].dev, f[T].dev, f[U].dev, f[V].dev, f[STATE].dev, a->stream));
}

/* ------------------------------------------------------------------------ */
/* materials / environment of the path tracer                               */
/* ------------------------------------------------------------------------ */
extern "C" int lh_accel_set_material(lh_accel_t *a, uint32_t mesh, const lh_material_t *mat)
{
    lh_guard guard(a);
    if (!a || !mat) return fail("lh_accel_set_material: NULL argument");
    const uint32_t nm = a->committed ? a->hs->nmeshes : a->nmeshes + a->ndmeshes;          /* host or device meshes, never both */
    if (mesh != LH_ALL_MESHES && mesh >= nm) return fail("lh_accel_set_material: mesh %u out of range", mesh);
    for (int k = 0; k < 3; k++) {
        if (!(mat->kd[k] >= 0.0f && mat->ks[k] >= 0.0f && mat->kt[k] >= 0.0f)) return fail("lh_accel_set_material: negative or NaN reflectance");
    }
    const double sum = (mat->kd[0] + mat->kd[1] + mat->kd[2] + mat->ks[0] + mat->ks[1] + mat->ks[2] + mat->kt[0] + mat->kt[1] + mat->kt[2]) / 3.0;
    if (sum > 1.0 + 1e-6) return fail("lh_accel_set_material: kd + ks + kt averages exceed 1 (pathtrace.c:419 asserts d + s + t <= 1)");
    if (!(mat->ior > 0.0f)) return fail("lh_accel_set_material: ior must be positive");
    if (a->nmaterials < nm) {
        lh_material_t *nmats = (lh_material_t *)realloc(a->materials, sizeof(lh_material_t) * (nm ? nm : 1));
        if (!nmats) return fail("out of memory");
        for (uint32_t k = a->nmaterials; k < nm; k++) {        /* ri_material_new (material.c:20-40): kd 1, ks 0, kt 0, ior 1 */
            memset(&nmats[k], 0, sizeof(lh_material_t));
            nmats[k].kd[0] = nmats[k].kd[1] = nmats[k].kd[2] = 1.0f; nmats[k].ior = 1.0f;
        }
        a->materials = nmats; a->nmaterials = nm;
    }
    for (uint32_t k = 0; k < a->nmaterials; k++) if (mesh == LH_ALL_MESHES || mesh == k) a->materials[k] = *mat;
    a->materials_dirty = 1;
    return 0;
}

extern "C" int lh_accel_set_environment(lh_accel_t *a, const lh_environment_t *env)
{
    lh_guard guard(a);
    if (!a) return fail("lh_accel_set_environment: NULL argument");
    if (!a->committed) return fail("lh_accel_set_environment: accel not committed");
    if (!env) {                  /* back to the default: constant white, no map */
        if (a->d_env_map) { (void)hipFree(a->d_env_map); a->d_env_map = NULL; }
        memset(&a->env, 0, sizeof(a->env)); a->env_set = 0;
        return 0;
    }
    if (env->map_rgba && (env->width < 1 || env->height < 1)) return fail("lh_accel_set_environment: bad map size");
    HIPCHK(hipSetDevice(a->device));
    if (a->d_env_map) { (void)hipFree(a->d_env_map); a->d_env_map = NULL; }
    a->env = *env; a->env.map_rgba = NULL; a->env_set = 1;
    if (env->map_rgba) {
        const size_t b = sizeof(float) * 4 * (size_t)env->width * env->height;
        HIPCHK(hipMalloc(&a->d_env_map, b));
        HIPCHK(hipMemcpy(a->d_env_map, env->map_rgba, b, hipMemcpyHostToDevice));
    }
    return 0;
}

static int sync_materials(lh_accel_t *a)
{
    const uint32_t nm = a->hs->nmeshes ? a->hs->nmeshes : 1;
    if (a->nmaterials < nm) {
        lh_material_t def; memset(&def, 0, sizeof(def)); def.kd[0] = def.kd[1] = def.kd[2] = 1.0f; def.ior = 1.0f;
        lh_material_t *nmats = (lh_material_t *)realloc(a->materials, sizeof(lh_material_t) * nm);
        if (!nmats) return fail("out of memory");
        for (uint32_t k = a->nmaterials; k < nm; k++) nmats[k] = def;
        a->materials = nmats; a->nmaterials = nm; a->materials_dirty = 1;
    }
    if (a->materials_dirty || !a->d_materials) {
        if (a->d_materials) { (void)hipFree(a->d_materials); a->d_materials = NULL; }
        const size_t mb = lh_pt_material_bytes();
        std::vector<char> packed(mb * a->nmaterials);
        for (uint32_t k = 0; k < a->nmaterials; k++) lh_pt_material_pack(&a->materials[k], packed.data() + mb * k);
        HIPCHK(hipMalloc(&a->d_materials, packed.size()));
        HIPCHK(hipMemcpy(a->d_materials, packed.data(), packed.size(), hipMemcpyHostToDevice));
        a->materials_dirty = 0;
    }
    return lh_ensure_prim_mesh(a);
}

int lh_ensure_prim_mesh(lh_accel_t *a)
{
    if (!a->d_prim_mesh && a->hs->bvh.ntris) {
        HIPCHK(hipMalloc(&a->d_prim_mesh, sizeof(uint32_t) * (size_t)a->hs->bvh.ntris));
        HIPCHK(hipMemcpy(a->d_prim_mesh, a->hs->bvh.prim_geom, sizeof(uint32_t) * (size_t)a->hs->bvh.ntris, hipMemcpyHostToDevice));
    }
    return 0;
}

/* ------------------------------------------------------------------------ */
/* wavefront path tracer (kernels: lh_render.hip, arithmetic: lh_pt.h)       */
/* ------------------------------------------------------------------------ */

/* what the _lit and _lights entry points add to a pass (lh_ptl.h; all NULL: the pass as it ever was): the checked light list as the light stage
 * takes it, the checked area list as the area stage takes it, and the caller's path-vertex sink */
struct pt_lit { const char *what; const gather_params *lights; const lh_pt_sink_t *sink; const gather_params *area; };
static const pt_lit pt_unlit = {NULL, NULL, NULL, NULL};

/* the sink's refusals: its double arrays 8-byte aligned, the others 4-byte */
static int pt_sink_ok(const char *what, const lh_pt_sink_t *k)
{
    if ((((uintptr_t)k->d_org | (uintptr_t)k->d_dir | (uintptr_t)k->d_t | (uintptr_t)k->d_u | (uintptr_t)k->d_v) & 7u) != 0)
        return fail("%s: the sink's org, dir, t, u and v arrays are doubles: a pointer is not 8-byte aligned", what);
    if ((((uintptr_t)k->d_path | (uintptr_t)k->d_depth | (uintptr_t)k->d_prim | (uintptr_t)k->d_thr | (uintptr_t)k->d_direct | (uintptr_t)k->d_counts) & 3u) != 0)
        return fail("%s: the sink's path, depth, prim, thr, direct and counts arrays are 32-bit words: a pointer is not 4-byte aligned", what);
    return 0;
}

/* the statistics words of the launches so far, off the device before a stage of a lit bounce resets and counts them for itself */
static int pt_take_counters(const unsigned long long *cnt, unsigned long long *closest_cnt, hipStream_t s)
{
    unsigned long long hc[LH_CNT_N];
    HIPCHK(hipMemcpyAsync(hc, cnt, sizeof(hc), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int k = 0; k < LH_CNT_N; k++) closest_cnt[k] += hc[k];
    return 0;
}

/* what a lit pass does between the closest-hit launch of bounce `depth` and its shading pass: the light stages over the bounce's entries and their
 * direct light into the pixels (with lights), the entries into the sink (with one).  org / dir / path / thr: the bounce's own sets (NULL at bounce 0);
 * value: where the hits' one value and then r stand (p_value; p_value2 with area lights alone) or NULL; spp_total, seed: the pass's, for the area
 * stage's keys and seed; cnt: the statistics words or NULL, closest_cnt: where the closest-hit launches' words are kept while a stage counts */
static int pt_lit_bounce(lh_accel_t *a, const pt_lit &lit, size_t S, int depth, int spp, int spp_total, uint64_t seed, const lh_material_t *override_mat,
                         const void *d_cam, const uint32_t *counts, const double *org, const double *dir, const uint32_t *path, const float *thr,
                         float *value, unsigned long long *cnt, unsigned long long *closest_cnt, hipStream_t s)
{
    /* bounce 0 has no ray in memory: the light stage and the sink read the camera rays from the second ray set, free until the swap after bounce 0 */
    if (depth == 0) {
        if (lh_pt_launch_camera_rays(S, d_cam, (double *)a->p_org2.p, (double *)a->p_dir2.p, a->ncus, s) != 0) return fail("pt camera ray launch failed");
        org = (const double *)a->p_org2.p; dir = (const double *)a->p_dir2.p;
    }
    if (lit.lights) {
        /* the light stage of a caller's batch over the bounce's entries, behind the guard this call holds: the identity list with its count on
         * the device.  It resets and counts the statistics words for itself */
        if (cnt && pt_take_counters(cnt, closest_cnt, s) != 0) return -1;
        if (ao_batch_device(lit.what, a, *lit.lights, S, org, dir, a->r_prim.p, a->r_t.p, a->r_u.p, a->r_v.p, 1, 0, NULL, NULL, NULL, S, counts + depth,
                            NULL, value, s) != 0) return -1;
        if (cnt) HIPCHK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * LH_CNT_DEV, s));
    }
    if (lit.area) {
        /* the area stage likewise, keyed per entry by (frame pixel, sample) and seeded per bounce (lh_ptl.h), no uniforms replayed; with delta lights
         * too its answer goes beside theirs and the two are folded into the hits' one value */
        float *area_value = lit.lights ? (float *)a->p_value2.p : value;
        if (lh_pt_launch_area_keys(S, depth, spp_total, d_cam, counts, path, (unsigned long long *)a->p_key.p, a->ncus, s) != 0)
            return fail("pt area key launch failed: %s", hipGetErrorString(hipGetLastError()));
        if (cnt && pt_take_counters(cnt, closest_cnt, s) != 0) return -1;
        if (ao_batch_device(lit.what, a, *lit.area, S, org, dir, a->r_prim.p, a->r_t.p, a->r_u.p, a->r_v.p, 1, lh_ptl_area_seed(seed, depth), a->p_key.p, NULL,
                            NULL, S, counts + depth, NULL, area_value, s) != 0) return -1;
        if (cnt) HIPCHK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * LH_CNT_DEV, s));
        if (lit.lights && lh_pt_launch_value_add(S, depth, counts, value, area_value, a->ncus, s) != 0)
            return fail("pt value fold launch failed: %s", hipGetErrorString(hipGetLastError()));
    }
    if (lit.lights || lit.area) {
        if (lh_pt_launch_direct(S, (const double *)a->d_attr9[0], (const uint32_t *)a->d_prim_mesh, a->d_materials, override_mat, depth, spp, counts,
                                (const uint32_t *)a->r_prim.p, (const double *)a->r_u.p, (const double *)a->r_v.p, path, thr, value,
                                lit.sink && lit.sink->d_direct, (unsigned long long *)a->p_rad.p, a->ncus, s) != 0)
            return fail("pt direct light launch failed: %s", hipGetErrorString(hipGetLastError()));
    }
    if (lit.sink && lh_pt_launch_sink(S, depth, counts, org, dir, (const uint32_t *)a->r_prim.p, (const double *)a->r_t.p, (const double *)a->r_u.p,
                                      (const double *)a->r_v.p, path, thr, value, lit.sink, a->ncus, s) != 0)
        return fail("pt sink launch failed: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

/* the pass over a w-wide region of h lines = full bands of band_rows lines, band k starting at frame line y0 + k * band_stride
 * (an ordinary tile: band_rows = h) */
static int pt_tile(lh_accel_t *a, const lh_camera_t *cam, int x0, int y0, int w, int h, int band_rows, int band_stride, int s0, int spp, int spp_total, int max_vertices,
                   const lh_material_t *override_mat, const float env_rgb[3], const void *d_env_map, int env_w, int env_h, int flags,
                   uint64_t seed, void *d_rgb, lh_pt_stats_t *stats, void *stream, const pt_lit &lit)
{
    if (w <= 0 || h <= 0 || spp < 1 || spp_total < spp || max_vertices < 2 || max_vertices > 65536 || band_rows < 1 || h % band_rows != 0)
        return fail("lh_render_pt_tile: bad arguments");
    /* with area lights an entry's key is (frame pixel, sample) and the stage's generator reads 34 bits of it (lh_ptl.h) */
    if (lit.area && !lh_ptl_area_keys_ok(cam->width, cam->height, spp_total))
        return fail("%s: with area lights width x height x spp_total = %d x %d x %d exceeds the 2^34 keys of the area stage's generator", lit.what,
                    cam->width, cam->height, spp_total);
    HIPCHK(hipSetDevice(a->device));
    if (sync_materials(a) != 0) return -1;
    hipStream_t s = (hipStream_t)stream;
    const size_t S = (size_t)w * h * spp;
    if (S > ((size_t)1 << 30)) return fail("lh_render_pt_tile: more than 2^30 paths in one pass; lower spp_count or the tile size");
    if (spp > 4096) return fail("lh_render_pt_tile: more than 4096 samples of a pixel in one pass (the pixels' fixed-point sums); lower spp_count");
    /* with lights every entry of every bounce may add a term to its pixel (a hit its direct light, a miss the environment): a path up to max_vertices - 1 */
    if ((lit.lights || lit.area) && (size_t)spp * (size_t)(max_vertices - 1) > 4096)
        return fail("%s: with lights spp_count x (max_path_vertices - 1) = %d x %d exceeds 4096 terms of a pixel in one pass (the pixels' fixed-point sums); "
                    "lower spp_count", lit.what, spp, max_vertices - 1);
    unsigned long long *cnt = (a->stat_on && a->hs->bvh.ntris) ? a->d_counters : NULL;      /* lh_accel_trace_statistics */
    if (cnt) HIPCHK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * LH_CNT_DEV, s));
    const int nbounce = max_vertices - 1;                  /* bounce d traces the ray to path vertex d + 2; the last vertex scatters nothing */
    if (ensure_buf(&a->r_org, S * 24) || ensure_buf(&a->r_dir, S * 24) || ensure_buf(&a->p_org2, S * 24) ||
        ensure_buf(&a->p_dir2, S * 24) || ensure_buf(&a->r_prim, S * 4) || ensure_buf(&a->r_t, S * 8) ||
        ensure_buf(&a->r_u, S * 8) || ensure_buf(&a->r_v, S * 8) || ensure_buf(&a->p_path, S * 4) ||
        ensure_buf(&a->p_path2, S * 4) || ensure_buf(&a->p_thr, S * 12) || ensure_buf(&a->p_thr2, S * 12) ||
        ensure_buf(&a->p_rad, (size_t)w * h * 24) || ensure_buf(&a->p_counts, ((size_t)nbounce + 2) * 4 + 64 + lh_pt_cam_bytes())) return -1;
    const bool lit_pass = lit.lights || lit.area || lit.sink;          /* lh_ptl.h; none: not one launch or buffer more than before */
    if (lit.lights && ensure_buf(&a->p_value, S * 12)) return -1;
    if (lit.area && (ensure_buf(&a->p_value2, S * 12) || ensure_buf(&a->p_key, S * 8))) return -1;
    float *value = lit.lights ? (float *)a->p_value.p : (lit.area ? (float *)a->p_value2.p : NULL);
    unsigned long long closest_cnt[LH_CNT_N] = {0};       /* with lights: the closest-hit launches' words, taken before the light stage resets them */
    /* the chain's ray / path-word / throughput records alternate between two sets; bounce 0 reads none (its rays are the camera
     * rays, generated inside the closest-hit kernel and again by the shading pass for the paths that go on) */
    double *org = NULL, *dir = NULL, *org2 = (double *)a->r_org.p, *dir2 = (double *)a->r_dir.p;
    uint32_t *path = NULL, *path2 = (uint32_t *)a->p_path.p, *counts = (uint32_t *)a->p_counts.p;
    float *thr = NULL, *thr2 = (float *)a->p_thr.p;
    void *d_cam = (char *)a->p_counts.p + (((size_t)nbounce + 2) * 4 + 63) / 64 * 64;
    /* counts[d] = rays of bounce d: [0] = S here, [d + 1] accumulated by bounce d's shading pass.  The host never reads a count
     * inside the chain (every launch gets S as its upper bound and the count's address) -- except every 8th bounce of a long
     * chain (a furnace test's 400 vertices), to stop once every path has ended */
    /* the pixels' radiance sums (three 64-bit fixed-point words each, lh_render.hip pt_accumulate): the resolve leaves them zero, but
     * the buffer may be new, grown, or left by a pass that failed */
    HIPCHK(hipMemsetAsync(a->p_rad.p, 0, (size_t)w * h * 24, s));
    if (lh_pt_launch_begin(cam, x0, y0, w, h, band_rows, band_stride, spp, s0, seed, d_cam, counts, nbounce + 2, s) != 0) return fail("pt begin launch failed");
    int rc = 0;
    for (int depth = 0; depth < nbounce && rc == 0; depth++) {
        lh_launch_opt opt; opt.n_dev = counts + depth; opt.cam_src = depth == 0 ? d_cam : NULL;
        rc = lh_launch(a, lh_batch_t{S, LH_MODE_CLOSEST, org, dir, a->r_prim.p, a->r_t.p, a->r_u.p, a->r_v.p, NULL, cnt}, LH_VARIANT_SPEC, s, false, opt);
        if (rc != 0) break;
        if (lit_pass) {
            rc = pt_lit_bounce(a, lit, S, depth, spp, spp_total, seed, override_mat, d_cam, counts, org, dir, path, thr, value, cnt, closest_cnt, s);
            if (rc != 0) break;
        }
        if (lh_pt_launch_shade(S, &a->dev, (const double *)a->d_nrm9, (const double *)a->d_attr9[0], (const uint32_t *)a->d_prim_mesh,
                               a->d_materials, override_mat, env_rgb, d_env_map, env_w, env_h, (flags & LH_PT_REFERENCE_WEIGHTS) != 0,
                               depth, max_vertices, seed, s0, spp, x0, y0, w, band_rows, band_stride, cam->width, d_cam, counts, org, dir, (const uint32_t *)a->r_prim.p,
                               (const double *)a->r_t.p, (const double *)a->r_u.p, (const double *)a->r_v.p, path, thr, (unsigned long long *)a->p_rad.p,
                               org2, dir2, path2, thr2, a->ncus, s) != 0)
            return fail("pt shade launch failed: %s", hipGetErrorString(hipGetLastError()));
        if (depth == 0) {
            org = org2; dir = dir2; path = path2; thr = thr2;
            org2 = (double *)a->p_org2.p; dir2 = (double *)a->p_dir2.p; path2 = (uint32_t *)a->p_path2.p; thr2 = (float *)a->p_thr2.p;
        } else {
            { double *t1 = org; org = org2; org2 = t1; t1 = dir; dir = dir2; dir2 = t1; }
            { uint32_t *t2 = path; path = path2; path2 = t2; float *t3 = thr; thr = thr2; thr2 = t3; }
        }
        if ((depth & 7) == 7 && depth + 1 < nbounce) {
            uint32_t left = 0;
            HIPCHK(hipMemcpyAsync(&left, counts + depth + 1, sizeof(left), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            if (left == 0) break;
        }
    }
    if (rc != 0) return -1;
    if (lh_pt_launch_resolve(w, h, band_rows, 1.0f / (float)spp_total, (unsigned long long *)a->p_rad.p, (float *)d_rgb, s) != 0)
        return fail("pt resolve launch failed");
    /* the sink's counts: the entries of every bounce, then zeros (a chain that ended early; the last vertex scatters nothing) */
    if (lit.sink && lit.sink->d_counts)
        HIPCHK(hipMemcpyAsync(lit.sink->d_counts, counts, sizeof(uint32_t) * (size_t)max_vertices, hipMemcpyDeviceToDevice, s));
    std::vector<uint32_t> hcounts((size_t)nbounce + 1);
    HIPCHK(hipMemcpyAsync(hcounts.data(), counts, hcounts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (cnt) {
        unsigned long long hc[LH_CNT_N];
        HIPCHK(hipMemcpy(hc, cnt, sizeof(hc), hipMemcpyDeviceToHost));
        for (int k = 0; k < LH_CNT_N; k++) hc[k] += closest_cnt[k];
        lh_stat_add(a, hc, hc[LH_CNT_RAYS], 0);
    }
    if (stats) {
        uint64_t rays = 0, depth = 0;
        for (int d = 0; d < nbounce; d++) { rays += hcounts[d]; if (hcounts[d]) depth = (uint64_t)d + 1; }
        stats->paths = S; stats->rays = rays; stats->max_depth_reached = depth;
    }
    return 0;
}

/* round-1 entry point: one diffuse reflectance for every mesh, constant environment */
extern "C" int lh_render_pt_tile(lh_accel_t *a, const lh_camera_t *cam, int x0, int y0, int w, int h, int s0, int spp,
                                 int spp_total, int max_vertices, float kd, const float env[3], uint64_t seed,
                                 void *d_rgb, lh_pt_stats_t *stats, void *stream)
{
    lh_guard guard(a);
    if (!a || !a->committed) return fail("lh_render_pt_tile: accel not committed");
    if (!cam || !d_rgb || !env) return fail("lh_render_pt_tile: NULL argument");
    if (!(kd > 0.0f) || kd > 1.0f) return fail("lh_render_pt_tile: bad arguments");
    lh_material_t m; memset(&m, 0, sizeof(m)); m.kd[0] = m.kd[1] = m.kd[2] = kd; m.ior = 1.0f;
    return pt_tile(a, cam, x0, y0, w, h, h, 0, s0, spp, spp_total, max_vertices, &m, env, NULL, 0, 0, 0, seed, d_rgb, stats, stream, pt_unlit);
}

/* per-mesh materials (lh_accel_set_material) and the accelerator's environment (lh_accel_set_environment) */
extern "C" int lh_render_pt_tile2(lh_accel_t *a, const lh_camera_t *cam, int x0, int y0, int w, int h, int s0, int spp,
                                  int spp_total, int max_vertices, int flags, uint64_t seed, void *d_rgb, lh_pt_stats_t *stats, void *stream)
{
    lh_guard guard(a);
    if (!a || !a->committed) return fail("lh_render_pt_tile2: accel not committed");
    if (!cam || !d_rgb) return fail("lh_render_pt_tile2: NULL argument");
    float one[3] = {1.0f, 1.0f, 1.0f};
    const float *rgb = a->env_set ? a->env.rgb : one;          /* never set: constant white; an explicit black environment stays black */
    return pt_tile(a, cam, x0, y0, w, h, h, 0, s0, spp, spp_total, max_vertices, NULL, rgb, a->d_env_map, a->env.width, a->env.height, flags,
                   seed, d_rgb, stats, stream, pt_unlit);
}

/* the _lit forms' own refusals, before anything is enqueued: the list as the light stage refuses it (nlights == 0: none), the sink's pointers.
 * The _lights forms' area list likewise, as the area stage refuses it (area NULL or nlights == 0: none).  p, pa: the checked lists; out: what pt_tile
 * takes */
static int pt_lit_check(const char *what, const lh_light_t *lights, int nlights, const lh_lights_params_t *params, const area_in *area,
                        const lh_pt_sink_t *sink, gather_params *p, gather_params *pa, pt_lit *out)
{
    *out = pt_lit{what, NULL, sink, NULL};
    if (nlights != 0) {
        const lights_in in = {lights, nlights, params};
        if (gather_check(what, LH_GATHER_LIGHT, &in, p) != 0) return -1;
        out->lights = p;
    }
    if (area && area->nlights != 0) {
        if (gather_check(what, LH_GATHER_AREA, area, pa) != 0) return -1;
        out->area = pa;
    }
    return sink ? pt_sink_ok(what, sink) : 0;
}

/* the _lights forms' lh_pt_lights_t (NULL: no lights at all): its reserved words, then both lists through pt_lit_check; the area list's runs must lie
 * in a's emitter table (none, or no accelerator: "bad area lights") */
static int pt_lights_check(const char *what, const lh_accel_t *a, const lh_pt_lights_t *l, const lh_pt_sink_t *sink, gather_params *p, gather_params *pa,
                           pt_lit *out)
{
    static const lh_pt_lights_t none = {NULL, 0, 0, NULL, NULL, 0, 0, NULL};
    if (!l) l = &none;
    if (l->reserved0 != 0 || l->reserved1 != 0) return fail("%s: the reserved words of lh_pt_lights_t must be 0", what);
    const area_in area = {l->area, l->narea, l->area_params, a};
    return pt_lit_check(what, l->lights, l->nlights, l->params, &area, sink, p, pa, out);
}

/* the lit forms behind their lists' and sink's refusals: lh_render_pt_tile2 / lh_render_pt_bands with what `lit` adds */
static int pt_lit_tile(lh_accel_t *a, const lh_camera_t *cam, int x0, int y0, int w, int h, int s0, int spp, int spp_total, int max_vertices, int flags,
                       uint64_t seed, void *d_rgb, lh_pt_stats_t *stats, void *stream, const pt_lit &lit)
{
    if (!a || !a->committed) return fail("%s: accel not committed", lit.what);
    if (!cam || !d_rgb) return fail("%s: NULL argument", lit.what);
    float one[3] = {1.0f, 1.0f, 1.0f};
    const float *rgb = a->env_set ? a->env.rgb : one;
    return pt_tile(a, cam, x0, y0, w, h, h, 0, s0, spp, spp_total, max_vertices, NULL, rgb, a->d_env_map, a->env.width, a->env.height, flags,
                   seed, d_rgb, stats, stream, lit);
}

static int pt_lit_bands(lh_accel_t *a, const lh_camera_t *cam, int y0_first, int band_rows, int band_stride, int nbands, int s0, int spp, int spp_total,
                        int max_vertices, int flags, const lh_material_t *override_mat, uint64_t seed, void *d_rgb, lh_pt_stats_t *stats, void *stream,
                        const pt_lit &lit)
{
    const char *what = lit.what;
    if (!a || !a->committed) return fail("%s: accel not committed", what);
    if (!cam || !d_rgb) return fail("%s: NULL argument", what);
    if (nbands < 1 || band_rows < 1 || y0_first < 0 || (nbands > 1 && band_stride < band_rows) ||
        (long long)y0_first + (long long)(nbands - 1) * band_stride + band_rows > cam->height)
        return fail("%s: bands must be disjoint and inside the frame", what);
    float one[3] = {1.0f, 1.0f, 1.0f};
    const float *rgb = a->env_set ? a->env.rgb : one;
    return pt_tile(a, cam, 0, y0_first, cam->width, nbands * band_rows, band_rows, band_stride, s0, spp, spp_total, max_vertices, override_mat, rgb,
                   a->d_env_map, a->env.width, a->env.height, flags, seed, d_rgb, stats, stream, lit);
}

/* lh_render_pt_tile2 with direct light from a light list at every path vertex and a path-vertex sink (lh_ptl.h) */
extern "C" int lh_render_pt_tile_lit(lh_accel_t *a, const lh_camera_t *cam, int x0, int y0, int w, int h, int s0, int spp, int spp_total,
                                     int max_vertices, int flags, const lh_light_t *lights, int nlights, const lh_lights_params_t *params,
                                     const lh_pt_sink_t *sink, uint64_t seed, void *d_rgb, lh_pt_stats_t *stats, void *stream)
{
    lh_guard guard(a);
    const char *what = "lh_render_pt_tile_lit";
    gather_params p; pt_lit lit;
    if (pt_lit_check(what, lights, nlights, params, NULL, sink, &p, NULL, &lit) != 0) return -1;
    return pt_lit_tile(a, cam, x0, y0, w, h, s0, spp, spp_total, max_vertices, flags, seed, d_rgb, stats, stream, lit);
}

/* lh_render_pt_tile_lit with area lights beside, or instead of, the delta lights (lh_ptl.h) */
extern "C" int lh_render_pt_tile_lights(lh_accel_t *a, const lh_camera_t *cam, int x0, int y0, int w, int h, int s0, int spp, int spp_total,
                                        int max_vertices, int flags, const lh_pt_lights_t *lights, const lh_pt_sink_t *sink, uint64_t seed,
                                        void *d_rgb, lh_pt_stats_t *stats, void *stream)
{
    lh_guard guard(a);          /* (held from here on: the emitter table's count is read under the lock the stages then hold) */
    gather_params p, pa; pt_lit lit;
    if (pt_lights_check("lh_render_pt_tile_lights", a, lights, sink, &p, &pa, &lit) != 0) return -1;
    return pt_lit_tile(a, cam, x0, y0, w, h, s0, spp, spp_total, max_vertices, flags, seed, d_rgb, stats, stream, lit);
}

/* a rank's interleaved full-width bands of a sharded frame as ONE pass: nbands bands of band_rows lines, band k starting at
 * frame line y0_first + k * band_stride (all inside the frame).  d_rgb: [nbands][band_rows][width][3], every band in image
 * orientation (lh_render_ao_bands' layout).  override_mat NULL: the accelerator's per-mesh materials. */
extern "C" int lh_render_pt_bands(lh_accel_t *a, const lh_camera_t *cam, int y0_first, int band_rows, int band_stride, int nbands,
                                  int s0, int spp, int spp_total, int max_vertices, int flags, const lh_material_t *override_mat,
                                  uint64_t seed, void *d_rgb, lh_pt_stats_t *stats, void *stream)
{
    lh_guard guard(a);
    if (!a || !a->committed) return fail("lh_render_pt_bands: accel not committed");
    if (!cam || !d_rgb) return fail("lh_render_pt_bands: NULL argument");
    if (nbands < 1 || band_rows < 1 || y0_first < 0 || (nbands > 1 && band_stride < band_rows) ||
        (long long)y0_first + (long long)(nbands - 1) * band_stride + band_rows > cam->height)
        return fail("lh_render_pt_bands: bands must be disjoint and inside the frame");
    float one[3] = {1.0f, 1.0f, 1.0f};
    const float *rgb = a->env_set ? a->env.rgb : one;          /* never set: constant white; an explicit black environment stays black */
    return pt_tile(a, cam, 0, y0_first, cam->width, nbands * band_rows, band_rows, band_stride, s0, spp, spp_total, max_vertices, override_mat, rgb,
                   a->d_env_map, a->env.width, a->env.height, flags, seed, d_rgb, stats, stream, pt_unlit);
}

/* lh_render_pt_bands with the light list and the sink of lh_render_pt_tile_lit */
extern "C" int lh_render_pt_bands_lit(lh_accel_t *a, const lh_camera_t *cam, int y0_first, int band_rows, int band_stride, int nbands,
                                      int s0, int spp, int spp_total, int max_vertices, int flags, const lh_material_t *override_mat,
                                      const lh_light_t *lights, int nlights, const lh_lights_params_t *params, const lh_pt_sink_t *sink,
                                      uint64_t seed, void *d_rgb, lh_pt_stats_t *stats, void *stream)
{
    lh_guard guard(a);
    const char *what = "lh_render_pt_bands_lit";
    gather_params p; pt_lit lit;
    if (pt_lit_check(what, lights, nlights, params, NULL, sink, &p, NULL, &lit) != 0) return -1;
    return pt_lit_bands(a, cam, y0_first, band_rows, band_stride, nbands, s0, spp, spp_total, max_vertices, flags, override_mat, seed, d_rgb, stats, stream, lit);
}

/* lh_render_pt_bands_lit with the lights of lh_render_pt_tile_lights */
extern "C" int lh_render_pt_bands_lights(lh_accel_t *a, const lh_camera_t *cam, int y0_first, int band_rows, int band_stride, int nbands,
                                         int s0, int spp, int spp_total, int max_vertices, int flags, const lh_material_t *override_mat,
                                         const lh_pt_lights_t *lights, const lh_pt_sink_t *sink, uint64_t seed, void *d_rgb, lh_pt_stats_t *stats,
                                         void *stream)
{
    lh_guard guard(a);
    gather_params p, pa; pt_lit lit;
    if (pt_lights_check("lh_render_pt_bands_lights", a, lights, sink, &p, &pa, &lit) != 0) return -1;
    return pt_lit_bands(a, cam, y0_first, band_rows, band_stride, nbands, s0, spp, spp_total, max_vertices, flags, override_mat, seed, d_rgb, stats, stream, lit);
}

/* ------------------------------------------------------------------------ */
/* whole frame into host memory (render_frame_controller + bucket_write)     */
/* ------------------------------------------------------------------------ */

extern "C" int lh_render_ao_frame_host(lh_accel_t *a, const lh_camera_t *cam, int ps, int gather_nsamples,
                                       uint64_t seed, int tile, float *rgb, lh_tile_stats_t *stats)
{
    lh_guard guard(a);
    if (!a || !a->committed) return fail("lh_render_ao_frame_host: accel not committed");
    if (!cam || !rgb) return fail("lh_render_ao_frame_host: NULL argument");
    if (cam->width <= 0 || cam->height <= 0) return fail("lh_render_ao_frame_host: bad resolution");
    if (tile <= 0) {
        /* default tile: the largest power of two (<= 4096) whose scratch stays under ~6 GB.  Per sub-sample: ~200 B of ray /
         * hit / epilogue records, plus 49 B per AO ray when the AO stage has to materialise its rays (LH_AO_FUSED=0):
         * ambient_occlusion.rib's own 3 x 3 pixel samples x 64 AO rays would otherwise ask for 30 GB per 1024^2 tile */
        const int N = gather_nsamples > 0 ? gather_nsamples : 1;
        const double per_pixel = (double)(ps > 0 ? ps : 1) * (ps > 0 ? ps : 1) * (200.0 + (a->ao_fused ? 0.0 : 49.0 * N));
        tile = 4096;
        while (tile > 64 && (double)tile * tile * per_pixel > 6.0e9) tile /= 2;
    }
    HIPCHK(hipSetDevice(a->device));
    const int W = cam->width, H = cam->height;
    std::vector<float> host((size_t)tile * tile * 3);
    lh_tile_stats_t tot = {0, 0, 0, 0};
    for (int y0 = 0; y0 < H; y0 += tile)
        for (int x0 = 0; x0 < W; x0 += tile) {
            const int w = (x0 + tile <= W) ? tile : W - x0, h = (y0 + tile <= H) ? tile : H - y0;
            lh_tile_stats_t st;
            lh_field_t f[] = {lh_field_down(host.data(), (size_t)w * h * 3 * sizeof(float))};          /* the device tile is the staging block: the first tile is the largest */
            if (lh_stage_up(a, f, 1) != 0) return -1;
            if (lh_stage_down(a, f, 1, lh_render_ao_tile(a, cam, x0, y0, w, h, ps, gather_nsamples, seed, NULL, f[0].dev, &st, a->stream)) != 0) return -1;
            /* the tile comes back with its rows already flipped (row 0 = pixel row y0+h-1) */
            for (int r = 0; r < h; r++)
                memcpy(rgb + ((size_t)(H - (y0 + h) + r) * W + x0) * 3, host.data() + (size_t)r * w * 3, (size_t)w * 3 * sizeof(float));
            tot.primary_rays += st.primary_rays; tot.primary_hits += st.primary_hits;
            tot.ao_rays += st.ao_rays; tot.ao_occluded += st.ao_occluded;
        }
    if (stats) *stats = tot;
    return 0;
}

/*
 * lh_query.hip -- the ray queries of the C ABI: accel_intersect_func (src/render/accel.h:30-34) as device-resident, host
 * and pipelined host batches, one synchronous ray, traversal statistics (src/render/bvh.c:669-706) and beam visibility
 * (ri_bvh_intersect_beam_visibility, bvh.c:612-667).  The kernels are in lh_kernels.hip / lh_beam.hip.
 *
 * Large plain device dumps are traced from a copy in bin order (lh_launch; the passes are in lh_order.hip, the order in lh_order.h): fp64 rays with
 * fp64 records or any-hit bytes, the default walk, "dump_order_min" rays or more.  Every other call -- fp32 rays, 16-byte records, indexed and bounded
 * dumps, per-ray diagnostics, the tile pipelines' batches, smaller dumps -- takes the path it always took, unchanged.
 */
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

#include "lh_internal.h"

/* fill record slots without touching the scene: entry k < min(*count, n) -> slot index[k] (or k), ids beyond nrays skipped -- the listed slots of
 * an indexed launch (lh_accel_intersect_device_indexed), or all n of a dense one (index, count NULL, nrays = n).  miss: the records of an empty
 * scene's rays; else: LH_POISON_OUTPUTS' 0x77 bytes -- in the LISTED slots alone, the others are not ours.  rec16 (or NULL): 16-byte records
 * instead of prim / t / u / v */
__global__ void k_fill_listed(size_t n, const uint32_t *index, const uint32_t *count, uint32_t nrays, int miss,
                              uint32_t *prim, double *t, double *u, double *v, uint8_t *occ, uint4 *rec16, unsigned long long *counters)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (count && *count < n) n = *count;
    if (k >= n) return;
    const uint32_t i = index ? index[k] : (uint32_t)k;
    if (i >= nrays) return;
    const uint32_t w = miss ? LH_MISS_PRIM : 0x77777777u;
    const unsigned long long d = 0x7777777777777777ull;
    if (rec16) { uint4 r; r.x = w; r.y = miss ? __float_as_uint((float)LH_T_INF) : w; r.z = r.w = miss ? __float_as_uint(0.0f) : w; rec16[i] = r; }
    if (prim) prim[i] = w;
    if (t) t[i] = miss ? LH_T_INF : __longlong_as_double((long long)d);
    if (u) u[i] = miss ? 0.0 : __longlong_as_double((long long)d);
    if (v) v[i] = miss ? 0.0 : __longlong_as_double((long long)d);
    if (occ) occ[i] = miss ? 0 : 0x77;
    if (counters) atomicAdd(&counters[LH_CNT_RAYS], 1ull);
}

/* the fix-up queue for launches on `s`: launches on one stream are ordered, so they share a slot (queue, second stream,
 * events); different streams (replicas' tile loops, the pipelined host path) get their own */
int lh_aoq_slot(lh_accel_t *a, hipStream_t s)
{
    int k, free_k = -1;
    for (k = 0; k < LH_AOQ_SLOTS; k++) {
        if (a->aoq[k].used && a->aoq[k].stream == s) return k;
        if (!a->aoq[k].used && free_k < 0) free_k = k;
    }
    if (free_k < 0) {
        /* more concurrent streams than slots: wait for the device, then recycle slot 0 */
        HIPCHK(hipDeviceSynchronize());
        free_k = 0;
    }
    k = free_k;
    lh_fixq_t *q = &a->aoq[k].q;
    if (!q->ev_done) {              /* ev_done is set last: a slot whose set-up failed half-way is not "ready" */
        void *queue = NULL; uint32_t *qcount = NULL; hipStream_t aux = NULL; hipEvent_t e0 = NULL, e1 = NULL;
        bool ok = hipMalloc(&queue, (size_t)LH_AO_QCAP * sizeof(unsigned long long)) == hipSuccess &&
                  hipMalloc((void **)&qcount, (4 + 4096) * sizeof(uint32_t)) == hipSuccess &&       /* counters + the consumer groups' heads (LH_Q_GROUPS) */
                  hipMemset(queue, 0, (size_t)LH_AO_QCAP * sizeof(unsigned long long)) == hipSuccess &&
                  hipMemset(qcount, 0, (4 + 4096) * sizeof(uint32_t)) == hipSuccess;
        /* the consumer's stream gets the highest priority: streams of one priority share a handful of hardware queues round
         * robin (four by default), and a consumer that lands on its producer's queue runs BEHIND it instead of next to it
         * (bench.py's second accelerator: config-5 frame 89 -> 122 ms); priority streams have queues of their own */
        if (ok) {
            int prio_lo = 0, prio_hi = 0;
            if (hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess || prio_hi == prio_lo ||
                hipStreamCreateWithPriority(&aux, hipStreamNonBlocking, prio_hi) != hipSuccess)
                ok = hipStreamCreateWithFlags(&aux, hipStreamNonBlocking) == hipSuccess;
        }
        ok = ok && hipEventCreateWithFlags(&e0, hipEventDisableTiming) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&e1, hipEventDisableTiming) == hipSuccess;
        if (!ok) {                  /* nothing half-built stays behind */
            const hipError_t e = hipGetLastError();
            if (e1) (void)hipEventDestroy(e1);
            if (e0) (void)hipEventDestroy(e0);
            if (aux) (void)hipStreamDestroy(aux);
            if (qcount) (void)hipFree(qcount);
            if (queue) (void)hipFree(queue);
            return fail("the fix-up queue of a launch stream could not be set up: %s", hipGetErrorString(e));
        }
        q->queue = queue; q->qcount = qcount; q->qcap = LH_AO_QCAP;
        q->aux_stream = (void *)aux; q->ev_ready = (void *)e0; q->ev_done = (void *)e1;
    }
    a->aoq[k].stream = s; a->aoq[k].used = 1;
    return k;
}

/* hot set of a ray dump (4-wide nodes + 48-byte triangle records) against the Infinity Cache */
static bool wide8_pays(const lh_accel_t *a)
{
    const lh_bvh_t *b = &a->hs->bvh;
    return sizeof(lh_q4node_t) * (size_t)b->nq4nodes + sizeof(lh_tri32_t) * (size_t)b->ntris > ((size_t)256 << 20);
}

/* the 8-wide nodes exist or can be made: always for a host-built tree (lh_bvh_ensure_q8), by a second run of the build for a
 * tree built on this device (lh_ensure_formats), never for a scene received from another rank without them */
static bool q8_available(const lh_accel_t *a)
{
    if (a->d_q8nodes || !a->hs->device_built) return true;
    return !a->hs->received && a->hs->bvh.nq4nodes > 1;
}

/* ray dumps of this variant walk the 8-wide nodes on this scene: "wide8" forced, or left to the size of the hot set */
static bool dump_walks_q8(const lh_accel_t *a, int variant)
{
    return variant == LH_VARIANT_SPEC && q8_available(a) && (a->wide8 == 1 || (a->wide8 == -1 && wide8_pays(a)));
}

/* what the batch entry points check first, the same check winning whichever of them is asked: 1 = go on, 0 = no rays (nothing to do),
 * -1 = refused (lh_last_error: "<what>: ...") */
static int batch_args(const lh_accel_t *a, const char *what, size_t n, bool have_arrays, const char *arrays, int mode)
{
    if (!a || !a->committed) return fail("%s: accel not committed", what);
    if (n == 0) return 0;
    if (!have_arrays) return fail("%s: NULL %s", what, arrays);
    if (mode != LH_MODE_CLOSEST && mode != LH_MODE_ANY) return fail("%s: unknown mode %d", what, mode);
    return 1;
}

/* the workspace of the stream of slot qk for a dump in bin order (lh_order.h), grown on demand and kept; NULL: the dump is traced as given -- its
 * workspace would exceed "dump_order_max_mb", or the memory is not to be had */
static void *order_workspace(lh_accel_t *a, int qk, const lh_order_plan_t &p)
{
    lh_buf *w = &a->aoq[qk].order_ws;
    if (a->dump_order_max_mb && p.bytes > (a->dump_order_max_mb << 20)) return NULL;
    if (w->p && w->cap >= p.bytes) return w->p;
    lh_free_buf(w);          /* hipFree waits for the launches that still read it */
    if (hipMalloc(&w->p, p.bytes) != hipSuccess) { (void)hipGetLastError(); w->p = NULL; return NULL; }
    w->cap = p.bytes;
    return w->p;
}

int lh_launch(lh_accel_t *a, const lh_batch_t &b, int variant, hipStream_t s, bool dump, const lh_launch_opt &opt)
{
    const int go = batch_args(a, "intersect", b.n, (b.org && b.dir) || opt.cam_src, "ray arrays", b.mode);
    if (go <= 0) return go;
    const size_t n = b.n;
    const bool closest = b.mode == LH_MODE_CLOSEST, rec16 = closest && (opt.io_fmt & LH_IO_REC16);
    if (rec16 && (!b.prim || b.t || b.u || b.v)) return fail("intersect: 16-byte records go to one array (t, u, v must be NULL)");
    if (closest && !rec16 && (!b.prim || !b.t || !b.u || !b.v)) return fail("intersect: closest mode needs prim,t,u,v outputs");
    if (!closest && !b.occ) return fail("intersect: any mode needs the occluded output");
    HIPCHK(hipSetDevice(a->device));
    /* an empty scene: every ray misses -- all of a dense batch, the listed ones of an indexed batch (which are counted: how many there are is
     * known on the device alone).  LH_POISON_OUTPUTS: the listed slots alone are the launch's to spoil; a dense batch's arrays take a memset */
    const bool miss = a->hs->bvh.ntris == 0;
    if (miss || (opt.indexed && dump && a->poison_outputs)) {
        const size_t step = (size_t)1 << 30;          /* the fill kernel's slot ids are 32 bits wide (a list holds 2^30 entries at most) */
        for (size_t off = 0; off < n; off += step) {
            const lh_batch_t f = lh_batch_sub(b, opt.io_fmt, off, n - off < step ? n - off : step);
            hipLaunchKernelGGL(k_fill_listed, dim3((unsigned)((f.n + 255) / 256)), dim3(256), 0, s, f.n, opt.indexed ? opt.index : NULL,
                               opt.indexed ? opt.n_dev : NULL, opt.indexed ? opt.idx_nrays : (uint32_t)f.n, miss ? 1 : 0,
                               closest && !rec16 ? (uint32_t *)f.prim : NULL, (double *)(closest ? f.t : NULL), (double *)(closest ? f.u : NULL),
                               (double *)(closest ? f.v : NULL), closest ? NULL : (uint8_t *)f.occ, rec16 ? (uint4 *)f.prim : NULL,
                               miss && opt.indexed ? f.counters : NULL);
            HIPCHK(hipGetLastError());
        }
        if (miss) return 0;
    }
    if (dump && a->poison_outputs && !opt.indexed) {          /* LH_POISON_OUTPUTS: every answer slot must be written by the launch */
        if (rec16) HIPCHK(hipMemsetAsync(b.prim, 0x77, n * 16, s));
        else if (closest) {
            HIPCHK(hipMemsetAsync(b.prim, 0x77, n * sizeof(uint32_t), s)); HIPCHK(hipMemsetAsync(b.t, 0x77, n * sizeof(double), s));
            HIPCHK(hipMemsetAsync(b.u, 0x77, n * sizeof(double), s)); HIPCHK(hipMemsetAsync(b.v, 0x77, n * sizeof(double), s));
        } else HIPCHK(hipMemsetAsync(b.occ, 0x77, n, s));
    }
    /* a device-built scene: lucille's own tree (exact-t tie winners, fragile hits) is built by a background host thread.
     * Queries are exact by default -- the first launch waits for it; set_param("fast_start", 1) / LH_FAST_START=1 launches
     * at once and attaches the tree when it is ready (until then ties resolve to the larger primitive id) */
    if (a->hs->device_built && !a->d_ref_nodes && lh_sync_ref(a, !a->fast_start) != 0) return -1;
    if (variant == LH_VARIANT_DEFAULT) variant = a->default_variant;
    if (opt.indexed) variant = LH_VARIANT_SPEC;          /* the list is read by the default walk's kernels */
    if (variant != LH_VARIANT_DIRECT && variant != LH_VARIANT_SPEC)
        return fail("intersect: unknown variant %d (%d: the textbook reference walk, %d: the default)", variant, LH_VARIANT_DIRECT, LH_VARIANT_SPEC);
    /* a tree built on the device exists only as 4-wide nodes: the textbook walk runs as the default walk there */
    if (a->hs->device_built) variant = LH_VARIANT_SPEC;
    if (lh_ensure_formats(a, lh_trace_formats_needed(variant)) != 0) return -1;     /* the textbook walk's nodes: uploaded on first use */
    /* ray dumps (incoherent by assumption) over a scene whose hot set does not fit the 256 MiB Infinity Cache walk the 8-wide
     * nodes: each record then costs a 128-byte line of HBM traffic whatever its size, and an 8-wide record uses all of it
     * (S-soup-10M: 57 -> 40 records per ray).  The tile pipelines' coherent rays stay on the 4-wide nodes. */
    const bool q8 = dump && dump_walks_q8(a, variant);
    if (q8 && lh_ensure_formats(a, LH_FMT_Q8) != 0) return -1;
    const int qk = lh_aoq_slot(a, s);             /* the stream's fix-up queue (rays out of visit budget -> the cooperative walk) */
    if (qk < 0) return -1;
    /* the launch's own scene: the resident one and what this launch alone is run with */
    lh_dev_scene_t sc = a->dev;
    sc.prefer_q8 = q8;
    /* ray dumps are incoherent by assumption: a wave's iterations serve 64 unrelated rays, a ray's age in iterations runs to
     * several times its own steps -- the tile pipelines' budget (128) would send half the batch to the cooperative walk */
    if (dump) sc.ray_budget = a->dump_budget;
    else if (sc.ray_chunk < LH_TILE_CHUNK) sc.ray_chunk = LH_TILE_CHUNK;       /* the tile pipelines' batches are coherent in batch order */
    sc.io_fmt = opt.io_fmt & (closest ? (LH_IO_RAYS_F32 | LH_IO_REC16) : LH_IO_RAYS_F32);
    sc.diag_out = opt.diag_out; sc.n_dev = opt.n_dev; sc.cam_src = opt.cam_src; sc.diag_clock = opt.diag_clock;
    sc.index = opt.indexed ? opt.index : NULL; sc.idx_nrays = opt.indexed ? opt.idx_nrays : 0u;          /* idx_nrays > 0 (the entry points return before a launch without rays): what makes the launch an indexed one */
    if (opt.tmax && (!opt.indexed || !dump || variant != LH_VARIANT_SPEC)) return fail("intersect: per-ray bounds are read by the default walk's indexed ray dumps only");
    sc.tmax = opt.tmax;
    /* a ray dump over the 4-wide nodes regroups a little later and passes over parked leaves a little sooner than the tile
     * pipelines' coherent batches want (tools/experiments/knob_sweep3.py / knob_sweep4.py, r05: S-soup-1M 2 233 -> 2 266 Mrays/s
     * closest hit, 2 735 -> 2 772 any hit; the 8-wide walk and the AO stage are best where they are) */
    const bool dump4 = dump && !q8 && !a->knobs_user;
    const bool dump8 = dump && q8 && !a->knobs_user;
    const int min_active = dump4 ? LH_DUMP_MIN_ACTIVE : dump8 ? LH_DUMP8_MIN_ACTIVE : a->min_active, tri_batch = dump4 ? LH_DUMP_TRI_BATCH : dump8 ? LH_DUMP8_TRI_BATCH : a->tri_batch;
    lh_launch_ctx_t ctx = {NULL, a->grid_blocks, min_active, tri_batch, &a->aoq[qk].q, a->ncus, (void *)s};          /* d_cursor: a block of its own per launch */
    /* a large plain dump is traced from a copy in bin order (lh_order.h): each XCD's L2 then sees one region of the scene at a time.  Plain: fp64 rays
     * (on 16-byte boundaries: the count's loads; a dump that starts on an odd multiple of 8 bytes is traced as given) with fp64 records or any-hit bytes, the default walk, every ray of the arrays, no bound, no count on the device, no
     * diagnostics.  Everything else -- fp32 rays, 16-byte records, indexed and bounded dumps, the tile pipelines -- is traced as given, and so is a dump
     * whose workspace cannot be had.  On the caller's stream, without a host synchronisation once the workspace is large enough (growing it frees the old
     * one, and hipFree waits for the device): count, scan, copy; the walk, with its fix-up queue, its
     * cooperative walk and k_fixups, on a batch that names the workspace's arrays; the records back.  More than 2^30 rays: part by part, each ordered by itself */
    const bool ordered = dump && a->dump_order && n >= a->dump_order_min && variant == LH_VARIANT_SPEC && sc.io_fmt == 0u && !opt.indexed && !opt.tmax &&
                         !opt.cam_src && !opt.n_dev && !opt.diag_out && !opt.diag_clock && !(((uintptr_t)b.org | (uintptr_t)b.dir) & 15u);
    if (ordered) {
        const size_t step = (size_t)1 << 30;
        const uint32_t octant = a->dump_order_bits == 1u;          /* the two 6-bit keys: one bit per axis under the octant, two bits per axis alone */
        char *ws = (char *)order_workspace(a, qk, lh_order_plan(n < step ? n : step, a->dump_order_bits, octant, closest));
        const lh_order_grid_t g = lh_order_grid(sc.grid_lo, sc.grid_step, a->dump_order_bits, octant);
        /* the ordered copy over the 4-wide nodes has thresholds of its own (lh_device.h); a caller's knobs hold here as everywhere */
        lh_launch_ctx_t octx = ctx;
        if (dump4) { octx.min_active = LH_ORDERED_MIN_ACTIVE; octx.tri_batch = LH_ORDERED_TRI_BATCH; }
        for (size_t off = 0; ws && off < n; off += step) {
            const lh_batch_t part = lh_batch_sub(b, 0u, off, n - off < step ? n - off : step);
            const lh_order_plan_t p = lh_order_plan(part.n, a->dump_order_bits, octant, closest);
            if (a->poison_outputs) HIPCHK(hipMemsetAsync(ws + (closest ? p.t : p.occ), 0x77, p.dest - (closest ? p.t : p.occ), s));          /* the ordered records too: the walk writes every one */
            if (lh_order_run(&p, &g, part.org, part.dir, ws, s) != 0) return fail("ordering a ray dump failed: %s", hipGetErrorString(hipGetLastError()));
            const lh_batch_t o = {part.n, b.mode, ws + p.org, ws + p.dir, closest ? ws + p.prim : NULL, closest ? ws + p.t : NULL, closest ? ws + p.u : NULL,
                                  closest ? ws + p.v : NULL, closest ? NULL : ws + p.occ, b.counters};
            octx.d_cursor = lh_next_cursor(a);
            if (lh_launch_trace(&sc, &o, variant, &octx) != 0 ||
                lh_order_back(&p, closest ? 1 : 0, ws, part.prim, part.t, part.u, part.v, part.occ, s) != 0)
                return fail("kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
            a->order_stat[0]++; a->order_stat[1] += part.n;
        }
        if (ws) return 0;
    }
    ctx.d_cursor = lh_next_cursor(a);
    if (lh_launch_trace(&sc, &b, variant, &ctx) != 0) return fail("kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

extern "C" int lh_accel_intersect_device(lh_accel_t *a, size_t n, const void *d_org, const void *d_dir,
                                         void *d_prim, void *d_t, void *d_u, void *d_v, void *d_occ,
                                         int mode, int variant, void *stream)
{
    lh_guard guard(a);
    return lh_launch(a, lh_batch_t{n, mode, d_org, d_dir, d_prim, d_t, d_u, d_v, d_occ, NULL}, variant, (hipStream_t)stream, true);
}

/* a counted launch: a->d_counters zeroed on the launch's stream before it, read back on that stream behind it (waits for the stream).  A caller
 * that keeps statistics adds what is its own to say: how many rays, how many hits */
static int counted_begin(lh_accel_t *a, hipStream_t s) { HIPCHK(hipMemsetAsync(a->d_counters, 0, sizeof(unsigned long long) * LH_CNT_DEV, s)); return 0; }
static int counted_collect(lh_accel_t *a, hipStream_t s, unsigned long long h[LH_CNT_DEV])
{
    HIPCHK(hipMemcpyAsync(h, a->d_counters, sizeof(unsigned long long) * LH_CNT_DEV, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    a->last_retraced = h[LH_CNT_RETRACED];
    return 0;
}

extern "C" int lh_accel_intersect_device_counted(lh_accel_t *a, size_t n, const void *d_org, const void *d_dir,
                                                 void *d_prim, void *d_t, void *d_u, void *d_v, void *d_occ,
                                                 int mode, int variant, uint64_t counters[4])
{
    lh_guard guard(a);
    if (!a || !a->committed) return fail("intersect: accel not committed");
    if (!counters) return fail("intersect_counted: counters is NULL");
    HIPCHK(hipSetDevice(a->device));
    if (counted_begin(a, a->stream) != 0) return -1;
    HIPCHK(hipDeviceSynchronize());
    const bool empty = a->hs->bvh.ntris == 0;          /* answered without a walk: nothing is counted on the device */
    if (empty) { counters[0] = counters[1] = counters[2] = 0; counters[3] = n; }
    int rc = lh_launch(a, lh_batch_t{n, mode, d_org, d_dir, d_prim, d_t, d_u, d_v, d_occ, a->d_counters}, variant, a->stream, true);
    if (rc != 0) return rc;
    if (empty) { HIPCHK(hipStreamSynchronize(a->stream)); return 0; }
    unsigned long long h[LH_CNT_DEV];
    if (counted_collect(a, a->stream, h) != 0) return -1;
    for (int k = 0; k < LH_CNT_N; k++) counters[k] = h[k];
    if (getenv("LH_DEBUG_COUNTERS"))
        fprintf(stderr, "[lucille_hip] lane slots: node steps %llu of %llu, triangle steps %llu of %llu, regroup iterations %llu; "
                        "rays through the reference walk %llu\n",
                h[LH_CNT_NODES], h[LH_CNT_NODE_SLOTS], h[LH_CNT_TRIS], h[LH_CNT_TRI_SLOTS], h[LH_CNT_REGROUP_SLOTS], h[LH_CNT_RETRACED]);
    return 0;
}

/* bytes of the node record a ray dump walks on this scene: 128 when the 8-wide nodes are in use (hot set beyond the
 * Infinity Cache, or "wide8" forced), else the default format's */
extern "C" int lh_accel_dump_node_bytes(const lh_accel_t *a)
{
    if (!a || !a->committed || a->hs->bvh.ntris == 0) return 0;
    return dump_walks_q8(a, a->default_variant) ? (int)sizeof(lh_q8node_t) : 64;
}

extern "C" uint64_t lh_accel_last_retraced(const lh_accel_t *a) { return a ? a->last_retraced : 0; }

extern "C" int lh_accel_order_statistics(lh_accel_t *a, uint64_t out[2], int clear)
{
    lh_guard guard(a);
    if (!a || !out) return fail("lh_accel_order_statistics: NULL argument");
    out[0] = a->order_stat[0]; out[1] = a->order_stat[1];
    if (clear) a->order_stat[0] = a->order_stat[1] = 0;
    return 0;
}

/* ---- large host batches: chunks pipelined through pinned staging -----------------------------------
 * A pageable hipMemcpy moves ~12 GB/s; the link does ~50.  Rays are cut into chunks of `cap` rays; chunk k is copied into pinned
 * block k % depth by a pool of host threads, sent, traced and brought back on stream k & 1 while the host stages the next chunks
 * and un-stages the finished ones.
 *
 * Rounds 2-5: two blocks of 2 M rays, whole chunks on two alternating streams, eight threads spawned per copy: 520 Mrays/s closest hit,
 * 640 any hit (S-soup-1M, 20 M rays) where the link alone does 57 GB/s each way = 1 190 Mrays/s of 48-byte rays.  Round 6 looked at the
 * timeline (profiles/r06_hostpath.txt): the host's copies were NOT the bound (3 .. 12 threads, memcpy or streaming stores: the same) --
 * the two streams ran in step, and streams that share one of the runtime's four hardware queues run one after the other.  Now: a stream
 * per direction of the link, a ring of `depth` blocks, the pipeline's streams on hardware queues of their own (the low-priority pool),
 * a pool of copy threads that lives with the process (stage + un-stage of an iteration as one set of slices): 845 / 1 030 Mrays/s.
 * LH_PIPE_CHUNK (rays), LH_PIPE_DEPTH (2 .. 8), LH_COPY_THREADS, LH_PIPE_PRIORITY, LH_PIPE_DIAG=1 (the calling thread's time). */
#define LH_PIPE_CHUNK_DEFAULT ((size_t)1 << 21)
#define LH_PIPE_DEPTH_DEFAULT 3
#define LH_PIPE_MIN   ((size_t)1 << 21)   /* below it the plain path (pageable copies, one launch) is as fast or faster: profiles/r06_hostpath.txt 7 */
#define LH_COPY_SLICE ((size_t)1 << 20)

namespace {
struct CopyJob { char *dst; const char *src; size_t bytes; std::atomic<size_t> *left; };
struct CopyPool {
    std::mutex mu; std::condition_variable cv;
    std::deque<CopyJob> q;
    int nthreads;
};
CopyPool *g_pool;
std::once_flag g_pool_once;

bool pool_take(CopyPool *P, CopyJob &j, bool wait)
{
    std::unique_lock<std::mutex> lk(P->mu);
    if (wait) P->cv.wait(lk, [&] { return !P->q.empty(); });
    if (P->q.empty()) return false;
    j = P->q.front(); P->q.pop_front();
    return true;
}

void pool_worker(CopyPool *P)
{
    for (;;) {
        CopyJob j;
        pool_take(P, j, true);
        memcpy(j.dst, j.src, j.bytes);
        j.left->fetch_sub(1, std::memory_order_release);
    }
}

/* the pool lives as long as the process: its threads sleep on the queue and are never joined (a library that may be dlclose()d
 * at exit must not run thread joins from a static destructor) */
CopyPool *copy_pool()
{
    std::call_once(g_pool_once, [] {
        CopyPool *P = new CopyPool();
        const unsigned hw = std::thread::hardware_concurrency();
        int nt = hw >= 16 ? 8 : (hw >= 4 ? 3 : 0);             /* + the calling thread */
        const char *e = getenv("LH_COPY_THREADS");
        if (e && atoi(e) >= 0 && atoi(e) <= 64) nt = atoi(e);
        P->nthreads = nt;
        for (int k = 0; k < nt; k++) std::thread(pool_worker, P).detach();
        g_pool = P;
    });
    return g_pool;
}

struct CopySet {                      /* copies submitted together; run() returns when all of them are done */
    std::vector<CopyJob> jobs;
    std::atomic<size_t> left{0};
    void add(void *dst, const void *src, size_t bytes)
    {
        for (size_t b = 0; b < bytes; b += LH_COPY_SLICE)
            jobs.push_back({(char *)dst + b, (const char *)src + b, bytes - b < LH_COPY_SLICE ? bytes - b : LH_COPY_SLICE, &left});
    }
    void run()
    {
        if (jobs.empty()) return;
        CopyPool *P = copy_pool();
        left.store(jobs.size(), std::memory_order_relaxed);
        if (P->nthreads == 0) { for (auto &j : jobs) memcpy(j.dst, j.src, j.bytes); jobs.clear(); return; }
        { std::lock_guard<std::mutex> lk(P->mu); for (auto &j : jobs) P->q.push_back(j); }
        P->cv.notify_all();
        CopyJob j;                    /* the caller copies too (any set's slices), then waits for its own set's stragglers */
        while (left.load(std::memory_order_acquire) != 0 && pool_take(P, j, false)) { memcpy(j.dst, j.src, j.bytes); j.left->fetch_sub(1, std::memory_order_release); }
        while (left.load(std::memory_order_acquire) != 0) LH_CPU_RELAX();
        jobs.clear();
    }
};
}  // namespace

static int pipe_init(lh_accel_t *a)
{
    if (a->pipe.ready) return 0;
    size_t C = LH_PIPE_CHUNK_DEFAULT; int depth = LH_PIPE_DEPTH_DEFAULT;
    const char *e = getenv("LH_PIPE_CHUNK");
    if (e && atoll(e) >= (1 << 16) && atoll(e) <= (1 << 24)) C = (size_t)atoll(e);
    e = getenv("LH_PIPE_DEPTH");
    if (e && atoi(e) >= 2 && atoi(e) <= LH_PIPE_DEPTH_MAX) depth = atoi(e);
    const size_t in_b = sizeof(double) * 6 * C, out_b = (sizeof(double) * 3 + sizeof(uint32_t)) * C;
    for (int b = 0; b < depth; b++) {
        HIPCHK(hipHostMalloc(&a->pipe.h_in[b], in_b, hipHostMallocDefault));
        HIPCHK(hipHostMalloc(&a->pipe.h_out[b], out_b, hipHostMallocDefault));
        HIPCHK(hipMalloc(&a->pipe.d_in[b], in_b));
        HIPCHK(hipMalloc(&a->pipe.d_out[b], out_b));
        HIPCHK(hipEventCreateWithFlags(&a->pipe.in_done[b], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&a->pipe.done[b], hipEventDisableTiming));
    }
    /* the three streams come from the LOW-priority pool of hardware queues: the runtime maps the streams of one priority onto four
     * hardware queues (GPU_MAX_HW_QUEUES), this process has more than four at normal priority by now (the caller's, the accelerator's,
     * other accelerators') and the fix-up queues' consumer streams fill the high-priority pool (lh_aoq_slot) -- two of the pipeline's
     * stages on ONE in-order hardware queue run one after the other whatever the streams say (closest hit 660 Mrays/s; with the stages
     * on queues of their own 850: profiles/r06_hostpath.txt).  LH_PIPE_PRIORITY = -1 / 0 / 1: high / normal / low */
    int prio_least = 0, prio_greatest = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    int prio = prio_least;
    e = getenv("LH_PIPE_PRIORITY");
    if (e) prio = atoi(e) < 0 ? prio_greatest : (atoi(e) > 0 ? prio_least : 0);
    for (int b = 0; b < 3; b++) HIPCHK(hipStreamCreateWithPriority(&a->pipe.s[b], hipStreamNonBlocking, prio));
    a->pipe.cap = C; a->pipe.depth = depth; a->pipe.ready = 1;
    return 0;
}

/* io_fmt (LH_IO_*): every stage moves the format's own bytes -- RB bytes per ray and array up (24 fp64, 12 fp32), 16 per record
 * down for LH_IO_REC16 (the walk writes them into the block's device buffer), 28 for SoA fp64 records, 1 per any-hit ray.  The
 * blocks are allocated for the largest format (fp64 rays and records) and laid out by the batch's own */
static int intersect_host_pipelined(lh_accel_t *a, size_t n, const void *org, const void *dir,
                                    uint32_t *prim, double *t, double *u, double *v, uint8_t *occ, int mode, uint32_t io_fmt)
{
    if (pipe_init(a) != 0) return -1;
    const size_t RB = (io_fmt & LH_IO_RAYS_F32) ? 3 * sizeof(float) : 3 * sizeof(double);
    const bool rec16 = mode == LH_MODE_CLOSEST && (io_fmt & LH_IO_REC16);
    /* CAP: rays a staging block holds (the arrays inside it are CAP apart); C: rays per chunk of THIS batch -- a batch of less than four
     * blocks is cut in four, so that its upload, launch and download overlap too (2 / 3 / 6 pieces: no better, tools/hostpath_sizes.py) */
    const size_t CAP = a->pipe.cap, D = (size_t)a->pipe.depth;
    size_t C = CAP;
    if (n < 4 * CAP) { C = ((n + 3) / 4 + 4095) & ~(size_t)4095; if (C < ((size_t)1 << 16)) C = (size_t)1 << 16; if (C > CAP) C = CAP; }
    const size_t nchunks = (n + C - 1) / C;
    /* where a block's arrays start (bytes): in: org | dir, out: t | u | v | prim -- CAP rays apart whatever a chunk holds; the 16-byte records
     * and the occluded bytes start their block.  back: the arrays the caller wants, in the order they come back */
    const struct { size_t dir, t, u, v, prim; } at = {RB * CAP, 0, sizeof(double) * CAP, 2 * sizeof(double) * CAP, 3 * sizeof(double) * CAP};
    struct { void *user; size_t at, bytes; } back[4]; int nback = 0;
    if (rec16) back[nback++] = {prim, 0, 16};
    else if (mode == LH_MODE_CLOSEST) {
        if (t) back[nback++] = {t, at.t, sizeof(double)};
        if (u) back[nback++] = {u, at.u, sizeof(double)};
        if (v) back[nback++] = {v, at.v, sizeof(double)};
        if (prim) back[nback++] = {prim, at.prim, sizeof(uint32_t)};
    } else if (occ) back[nback++] = {occ, 0, 1};
    CopySet cs;
    auto unstage = [&](size_t k) {
        const size_t b = k % D, first = k * C, m = (first + C <= n) ? C : n - first;
        for (int o = 0; o < nback; o++) cs.add((char *)back[o].user + back[o].bytes * first, (const char *)a->pipe.h_out[b] + back[o].at, back[o].bytes * m);
    };
    size_t unstaged = 0;              /* chunks [0, unstaged) are back in the caller's arrays */
    static const bool diag = getenv("LH_PIPE_DIAG") != NULL;          /* where the calling thread's time goes: waits / copies / enqueues, ms */
    double t_wait = 0, t_copy = 0, t_enq = 0;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    for (size_t k = 0; k < nchunks; k++) {
        const size_t b = k % D, first = k * C, m = (first + C <= n) ? C : n - first;
        /* block b is free once chunk k - depth has been un-staged: wait for that one; take along every later chunk that has come back */
        double c0 = diag ? now() : 0;
        if (k >= D) { HIPCHK(hipEventSynchronize(a->pipe.done[b])); }
        double c1 = diag ? now() : 0; t_wait += c1 - c0;
        while (unstaged < k && (unstaged + D <= k || hipEventQuery(a->pipe.done[unstaged % D]) == hipSuccess)) unstage(unstaged++);
        (void)hipGetLastError();          /* a query that says "not ready" must not be the next launch check's last error */
        char *hi = (char *)a->pipe.h_in[b], *di = (char *)a->pipe.d_in[b], *dout = (char *)a->pipe.d_out[b];
        cs.add(hi, (const char *)org + RB * first, RB * m);
        cs.add(hi + at.dir, (const char *)dir + RB * first, RB * m);
        cs.run();
        double c2 = diag ? now() : 0; t_copy += c2 - c1;
        /* the rays go up on a stream of their own; trace + records down alternate between two more: chunk k + 1's rays cross the link while
         * chunk k is traced, and its launch may start while chunk k's records go back (the runtime moves those with a copy KERNEL, which
         * shares the chip with the launch).  Rounds 2-5 ran whole chunks -- up, trace, down -- on two alternating streams: both fell into
         * step (two uploads sharing the link, then two launches sharing the chip, then two downloads) and nothing overlapped:
         * profiles/r06_hostpath.txt */
        hipStream_t s_in = a->pipe.s[0], s_tr = a->pipe.s[1 + (k & 1)];
        if (m == CAP) HIPCHK(hipMemcpyAsync(di, hi, 2 * RB * CAP, hipMemcpyHostToDevice, s_in));
        else {
            HIPCHK(hipMemcpyAsync(di, hi, RB * m, hipMemcpyHostToDevice, s_in));
            HIPCHK(hipMemcpyAsync(di + at.dir, hi + at.dir, RB * m, hipMemcpyHostToDevice, s_in));
        }
        HIPCHK(hipEventRecord(a->pipe.in_done[b], s_in));
        HIPCHK(hipStreamWaitEvent(s_tr, a->pipe.in_done[b], 0));
        const lh_batch_t chunk = rec16 ? lh_batch_t{m, mode, di, di + at.dir, dout, NULL, NULL, NULL, NULL, NULL}
                                       : lh_batch_t{m, mode, di, di + at.dir, dout + at.prim, dout + at.t, dout + at.u, dout + at.v, dout, NULL};
        const int rc = lh_launch(a, chunk, LH_VARIANT_DEFAULT, s_tr, true, lh_launch_opt{io_fmt});
        if (rc != 0) return rc;
        char *ho = (char *)a->pipe.h_out[b];
        for (int o = 0; o < nback; o++) HIPCHK(hipMemcpyAsync(ho + back[o].at, dout + back[o].at, back[o].bytes * m, hipMemcpyDeviceToHost, s_tr));
        HIPCHK(hipEventRecord(a->pipe.done[b], s_tr));
        if (diag) t_enq += now() - c2;
    }
    const double c3 = diag ? now() : 0;
    for (; unstaged < nchunks; unstaged++) {
        HIPCHK(hipEventSynchronize(a->pipe.done[unstaged % D])); unstage(unstaged); cs.run();
    }
    if (diag) fprintf(stderr, "[lucille_hip] pipelined host batch: %zu chunks of %zu rays, ring of %zu: waits %.2f ms, copies %.2f, enqueues %.2f, tail %.2f\n", nchunks, C, D, t_wait, t_copy, t_enq, now() - c3);
    return 0;
}

/* the staging block of a host batch of m rays, as device pointers: org | dir | [tmax] | (16-byte aligned) t | u | v | prim | [diag] | occ.  16-byte
 * records (rec16) start where t does -- fp64 rays without bounds: exactly behind the rays -- and t, u, v are NULL then */
struct lh_staged { char *org, *dir, *tmax; double *t, *u, *v; uint32_t *prim, *diag; uint8_t *occ; };
static int staged_block(lh_accel_t *a, size_t m, size_t el, bool rec16, bool bounded, bool diag, lh_staged *d)
{
    const size_t b_ray = el * 3 * m, b_out = (2 * b_ray + (bounded ? el * m : 0) + 15) & ~(size_t)15, b_diag = diag ? sizeof(uint32_t) * 4 * m : 0;
    if (lh_ensure_buf(&a->stage, b_out + 3 * sizeof(double) * m + sizeof(uint32_t) * m + b_diag + m + 64) != 0) return -1;
    char *base = (char *)a->stage.p;
    d->org = base; d->dir = base + b_ray; d->tmax = bounded ? base + 2 * b_ray : NULL;
    d->t = (double *)(base + b_out); d->u = d->t + m; d->v = d->u + m;
    d->prim = (uint32_t *)(d->v + m); d->diag = diag ? d->prim + m : NULL;
    d->occ = (uint8_t *)(d->prim + m) + b_diag;
    if (rec16) { d->prim = (uint32_t *)d->t; d->t = d->u = d->v = NULL; }
    return 0;
}

/* rays [off, off + m) of a host batch's arrays in the formats io_fmt (LH_IO_*): pageable copies through the staging block, one launch on the accelerator's
 * stream, the records into those of the caller's arrays that are not NULL; returns when they are there.  tmax (or NULL): the batch's bounds -- the launch is
 * then the identity list over the chunk's rays (per-ray bounds are read by indexed ray dumps), else a dense one.  diag (or NULL): four counts per ray from the
 * sequential walk (lh_accel_intersect_diag_host).  The caller holds the accelerator's lock, has checked the arguments and set the device */
static int host_chunk(lh_accel_t *a, size_t off, size_t m, const void *org, const void *dir, const void *tmax, uint32_t io_fmt,
                      void *prim, double *t, double *u, double *v, uint8_t *occ, int mode, uint32_t *diag = NULL)
{
    const bool closest = mode == LH_MODE_CLOSEST, rec16 = closest && (io_fmt & LH_IO_REC16);
    const size_t el = (io_fmt & LH_IO_RAYS_F32) ? sizeof(float) : sizeof(double), w = rec16 ? 4 : 1;          /* w: words per record's prim */
    hipStream_t s = a->stream;
    lh_staged d;
    if (staged_block(a, m, el, rec16, tmax != NULL, diag != NULL, &d) != 0) return -1;
    HIPCHK(hipMemcpyAsync(d.org, (const char *)org + el * 3 * off, el * 3 * m, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d.dir, (const char *)dir + el * 3 * off, el * 3 * m, hipMemcpyHostToDevice, s));
    if (tmax) HIPCHK(hipMemcpyAsync(d.tmax, (const char *)tmax + el * off, el * m, hipMemcpyHostToDevice, s));
    if (a->stat_on && counted_begin(a, s) != 0) return -1;
    lh_launch_opt opt{io_fmt};
    opt.diag_out = d.diag;
    if (tmax) { opt.indexed = true; opt.idx_nrays = (uint32_t)m; opt.tmax = d.tmax; }
    const int rc = lh_launch(a, lh_batch_t{m, mode, d.org, d.dir, d.prim, d.t, d.u, d.v, d.occ, a->stat_on ? a->d_counters : NULL},
                             diag ? LH_VARIANT_SPEC : LH_VARIANT_DEFAULT, s, true, opt);
    if (rc != 0) return rc;
    if (a->stat_on) {
        /* hits are counted from the device outputs whatever the caller asked to copy back */
        std::vector<uint32_t> hp; std::vector<uint8_t> ho; unsigned long long h[LH_CNT_DEV] = {0}, nh = 0;
        if (closest) { hp.resize(w * m); HIPCHK(hipMemcpyAsync(hp.data(), d.prim, sizeof(uint32_t) * w * m, hipMemcpyDeviceToHost, s)); }
        else { ho.resize(m); HIPCHK(hipMemcpyAsync(ho.data(), d.occ, m, hipMemcpyDeviceToHost, s)); }
        if (diag) {          /* the totals alone: a diagnostic batch does not report retraced rays (counted_collect) */
            HIPCHK(hipMemcpyAsync(h, a->d_counters, sizeof(unsigned long long) * LH_CNT_N, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        } else if (counted_collect(a, s, h) != 0) return -1;          /* an empty scene's batch leaves them zero */
        for (size_t i = 0; i < m; i++) nh += closest ? (hp[w * i] != LH_MISS_PRIM) : (ho[i] != 0);
        lh_stat_add(a, h, m, nh);
    }
    if (diag) HIPCHK(hipMemcpyAsync(diag + 4 * off, d.diag, sizeof(uint32_t) * 4 * m, hipMemcpyDeviceToHost, s));
    if (rec16) HIPCHK(hipMemcpyAsync((char *)prim + 16 * off, d.prim, 16 * m, hipMemcpyDeviceToHost, s));
    else if (closest) {
        if (prim) HIPCHK(hipMemcpyAsync((uint32_t *)prim + off, d.prim, sizeof(uint32_t) * m, hipMemcpyDeviceToHost, s));
        if (t) HIPCHK(hipMemcpyAsync(t + off, d.t, sizeof(double) * m, hipMemcpyDeviceToHost, s));
        if (u) HIPCHK(hipMemcpyAsync(u + off, d.u, sizeof(double) * m, hipMemcpyDeviceToHost, s));
        if (v) HIPCHK(hipMemcpyAsync(v + off, d.v, sizeof(double) * m, hipMemcpyDeviceToHost, s));
    } else if (occ) HIPCHK(hipMemcpyAsync(occ + off, d.occ, m, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));          /* a next chunk reuses the staging block */
    return 0;
}

/* the host batch in the formats io_fmt (LH_IO_*): pipelined from LH_PIPE_MIN rays on, else the plain path -- one chunk, one dense launch.  The caller holds
 * the accelerator's lock and has checked the arguments */
static int intersect_host_fmt(lh_accel_t *a, size_t n, const void *org, const void *dir,
                              uint32_t *prim, double *t, double *u, double *v, uint8_t *occ, int mode, uint32_t io_fmt)
{
    HIPCHK(hipSetDevice(a->device));
    static const size_t pipe_min = getenv("LH_PIPE_MIN") && atoll(getenv("LH_PIPE_MIN")) > 0 ? (size_t)atoll(getenv("LH_PIPE_MIN")) : LH_PIPE_MIN;
    if (n >= pipe_min && !a->stat_on && !getenv("LH_HOST_SIMPLE"))
        return intersect_host_pipelined(a, n, org, dir, prim, t, u, v, occ, mode, io_fmt);
    return host_chunk(a, 0, n, org, dir, NULL, io_fmt, prim, t, u, v, occ, mode);
}

extern "C" int lh_accel_intersect_host(lh_accel_t *a, size_t n, const double *org, const double *dir,
                                       uint32_t *prim, double *t, double *u, double *v, uint8_t *occ, int mode)
{
    lh_guard guard(a);
    const int go = batch_args(a, "intersect", n, org && dir, "ray arrays", mode);
    if (go <= 0) return go;
    return intersect_host_fmt(a, n, org, dir, prim, t, u, v, occ, mode, 0u);
}

/* the formats of an _ex call -> LH_IO_* bits, or -1 (lh_last_error) for a combination the contract refuses (lucille_hip.h).  n == 0
 * writes nothing: the record array is not looked at then (it may be NULL, as an empty tensor's pointer is) */
static int ex_formats(const char *what, size_t n, int ray_format, int record_format, int mode, const void *rec, const void *t, const void *u, const void *v)
{
    if (ray_format != LH_RAYS_F64 && ray_format != LH_RAYS_F32) return fail("%s: unknown ray format %d", what, ray_format);
    if (record_format != LH_REC_F64 && record_format != LH_REC16) return fail("%s: unknown record format %d", what, record_format);
    if (mode != LH_MODE_CLOSEST && mode != LH_MODE_ANY) return fail("%s: unknown mode %d", what, mode);
    if (record_format == LH_REC16) {
        if (mode == LH_MODE_ANY) return fail("%s: LH_REC16 is a closest-hit record format (any-hit writes occluded bytes)", what);
        if (t || u || v) return fail("%s: LH_REC16 writes whole records to prim_or_rec16: t, u, v must be NULL", what);
        if (n == 0) return 0;
        if (!rec) return fail("%s: LH_REC16 needs the record array", what);
        if (((uintptr_t)rec & 15u) != 0) return fail("%s: the LH_REC16 record array is not 16-byte aligned", what);
    }
    return (int)((ray_format == LH_RAYS_F32 ? LH_IO_RAYS_F32 : 0u) | (record_format == LH_REC16 ? LH_IO_REC16 : 0u));
}

/* per-ray maximum distance (lucille_hip.h; the rule: lh_tmax.h): the checks of a bounded call that need no device, after ex_formats':
 * -1 (lh_last_error) or 0 */
static int tmax_args(const char *what, size_t n_rays, const void *tmax, int ray_format, bool device)
{
    if (device && n_rays > ((size_t)1 << 30)) return fail("%s: a bounded call holds 2^30 rays at most (%zu given)", what, n_rays);
    const uintptr_t el = ray_format == LH_RAYS_F32 ? sizeof(float) : sizeof(double);
    if (((uintptr_t)tmax & (el - 1u)) != 0) return fail("%s: tmax not aligned to its %zu-byte elements", what, (size_t)el);
    return 0;
}

/* lh_accel_intersect_host_ex (tmax NULL) and the bounded lh_accel_intersect_host_tmax.  The bounded form is the plain path (host_chunk) in chunks of
 * LH_TMAX_HOST_CHUNK rays, whatever n is -- the bounds do not travel through the pinned ring of the pipelined host path */
#define LH_TMAX_HOST_CHUNK ((size_t)1 << 21)
static int host_batch(lh_accel_t *a, const char *what, size_t n, const void *org, const void *dir, const void *tmax, int ray_format, int record_format,
                      void *prim_or_rec16, double *t, double *u, double *v, uint8_t *occ, int mode)
{
    lh_guard guard(a);
    const int io = ex_formats(what, n, ray_format, record_format, mode, prim_or_rec16, t, u, v);
    if (io < 0) return -1;
    if (tmax && tmax_args(what, n, tmax, ray_format, false) != 0) return -1;
    const int go = batch_args(a, "intersect", n, org && dir, "ray arrays", mode);
    if (go <= 0) return go;
    if (!tmax) return intersect_host_fmt(a, n, org, dir, (uint32_t *)prim_or_rec16, t, u, v, occ, mode, (uint32_t)io);
    HIPCHK(hipSetDevice(a->device));
    for (size_t off = 0; off < n; off += LH_TMAX_HOST_CHUNK) {
        const int rc = host_chunk(a, off, n - off < LH_TMAX_HOST_CHUNK ? n - off : LH_TMAX_HOST_CHUNK, org, dir, tmax, (uint32_t)io, prim_or_rec16, t, u, v, occ, mode);
        if (rc != 0) return rc;
    }
    return 0;
}

extern "C" int lh_accel_intersect_host_ex(lh_accel_t *a, size_t n, const void *org, const void *dir, int ray_format, int record_format,
                                          void *prim_or_rec16, double *t, double *u, double *v, uint8_t *occ, int mode)
{
    return host_batch(a, "lh_accel_intersect_host_ex", n, org, dir, NULL, ray_format, record_format, prim_or_rec16, t, u, v, occ, mode);
}

extern "C" int lh_accel_intersect_host_tmax(lh_accel_t *a, size_t n, const void *org, const void *dir, const void *tmax, int ray_format, int record_format,
                                            void *prim_or_rec16, double *t, double *u, double *v, uint8_t *occ, int mode)
{
    if (!tmax) return lh_accel_intersect_host_ex(a, n, org, dir, ray_format, record_format, prim_or_rec16, t, u, v, occ, mode);          /* no bounds: the unbounded entry point itself */
    return host_batch(a, "lh_accel_intersect_host_tmax", n, org, dir, tmax, ray_format, record_format, prim_or_rec16, t, u, v, occ, mode);
}

extern "C" int lh_accel_intersect_device_ex(lh_accel_t *a, size_t n, const void *d_org, const void *d_dir, int ray_format, int record_format,
                                            void *d_prim_or_rec16, void *d_t, void *d_u, void *d_v, void *d_occ, int mode, void *stream)
{
    lh_guard guard(a);
    const int io = ex_formats("lh_accel_intersect_device_ex", n, ray_format, record_format, mode, d_prim_or_rec16, d_t, d_u, d_v);
    if (io < 0) return -1;
    return lh_launch(a, lh_batch_t{n, mode, d_org, d_dir, d_prim_or_rec16, d_t, d_u, d_v, d_occ, NULL}, LH_VARIANT_DEFAULT, (hipStream_t)stream, true, lh_launch_opt{(uint32_t)io});
}

/* hits among the listed records of a bounded launch, for the statistics: entry k < min(*count, n) -> slot index[k] (or k), ids beyond nrays skipped,
 * as the launch enumerated them (an id listed twice counts twice, as its ray does).  prim: the records' first words, `stride` words apart */
__global__ void k_count_listed_hits(size_t n, const uint32_t *index, const uint32_t *count, uint32_t nrays, const uint32_t *prim, uint32_t stride,
                                    const uint8_t *occ, unsigned long long *out)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (count && *count < n) n = *count;
    bool hit = false;
    if (k < n) {
        const uint32_t i = index ? index[k] : (uint32_t)k;
        if (i < nrays) hit = prim ? prim[(size_t)stride * i] != LH_MISS_PRIM : occ[i] != 0;
    }
    const unsigned long long m = __ballot(hit);
    if (m != 0ull && (threadIdx.x & 63) == 0) atomicAdd(out, (unsigned long long)__popcll(m));
}

/* rays listed by ids: the records of the listed rays go to THEIR slots, every other slot stays as it is (lucille_hip.h) -- lh_accel_intersect_device_indexed
 * (d_tmax NULL) and the bounded lh_accel_intersect_device_tmax, whose dense call (no list, no count) is the identity list over its rays */
static int listed_launch(lh_accel_t *a, const char *what, size_t n_rays, const void *d_org, const void *d_dir, const void *d_tmax, int ray_format, int record_format,
                         void *d_prim_or_rec16, void *d_t, void *d_u, void *d_v, void *d_occ, int mode, const void *d_index, size_t n_index, const void *d_count, void *stream)
{
    lh_guard guard(a);
    const size_t n_list = (d_tmax && d_index == NULL && n_index == 0 && d_count == NULL) ? n_rays : n_index;
    const int io = ex_formats(what, (n_rays && n_list) ? n_rays : 0, ray_format, record_format, mode, d_prim_or_rec16, d_t, d_u, d_v);
    if (io < 0) return -1;
    if (n_index > ((size_t)1 << 30)) return fail("%s: a list holds 2^30 entries at most (%zu given)", what, n_index);
    if (d_tmax) { if (tmax_args(what, n_rays, d_tmax, ray_format, true) != 0) return -1; }
    else if (n_rays > 0xFFFFFFFFull) return fail("%s: ray ids are 32 bits wide: 2^32 - 1 rays at most (%zu given)", what, n_rays);
    if ((((uintptr_t)d_index | (uintptr_t)d_count) & 3u) != 0) return fail("%s: the list and its count are 32-bit words: a pointer is not 4-byte aligned", what);
    const int go = batch_args(a, "intersect", (n_list && n_rays) ? n_list : 0, d_org && d_dir, "ray arrays", mode);
    if (go <= 0) return go;
    lh_launch_opt opt;
    opt.io_fmt = (uint32_t)io; opt.indexed = true; opt.index = (const uint32_t *)d_index; opt.idx_nrays = (uint32_t)n_rays;
    opt.n_dev = (const uint32_t *)d_count; opt.tmax = d_tmax;
    hipStream_t s = (hipStream_t)stream;
    const lh_batch_t b = {n_list, mode, d_org, d_dir, d_prim_or_rec16, d_t, d_u, d_v, d_occ, a->stat_on ? a->d_counters : NULL};
    /* statistics: the counting kernels, and one read-back -- how many rays the launch traced is known on the device alone */
    if (a->stat_on) { HIPCHK(hipSetDevice(a->device)); if (counted_begin(a, s) != 0) return -1; }
    if (lh_launch(a, b, LH_VARIANT_DEFAULT, s, true, opt) != 0) return -1;
    if (!a->stat_on) return 0;
    unsigned long long h[LH_CNT_DEV], nh = 0;
    if (counted_collect(a, s, h) != 0) return -1;
    /* hits: an unbounded call's are not counted (the records stay on the device); a bounded call's are those that are left after the bound, counted from
     * the records on the device */
    if (d_tmax) {
        const bool closest = mode == LH_MODE_CLOSEST;
        HIPCHK(hipMemsetAsync(a->d_counters, 0, sizeof(unsigned long long), s));
        hipLaunchKernelGGL(k_count_listed_hits, dim3((unsigned)((n_list + 255) / 256)), dim3(256), 0, s, n_list, opt.index, opt.n_dev, opt.idx_nrays,
                           closest ? (const uint32_t *)d_prim_or_rec16 : NULL, (io & LH_IO_REC16) ? 4u : 1u, closest ? NULL : (const uint8_t *)d_occ, a->d_counters);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&nh, a->d_counters, sizeof(nh), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    lh_stat_add(a, h, h[LH_CNT_RAYS], nh);
    return 0;
}

extern "C" int lh_accel_intersect_device_indexed(lh_accel_t *a, size_t n_rays, const void *d_org, const void *d_dir, int ray_format, int record_format,
                                                 void *d_prim_or_rec16, void *d_t, void *d_u, void *d_v, void *d_occ, int mode,
                                                 const void *d_index, size_t n_index, const void *d_count, void *stream)
{
    return listed_launch(a, "lh_accel_intersect_device_indexed", n_rays, d_org, d_dir, NULL, ray_format, record_format, d_prim_or_rec16, d_t, d_u, d_v, d_occ, mode,
                         d_index, n_index, d_count, stream);
}

extern "C" int lh_accel_intersect_device_tmax(lh_accel_t *a, size_t n_rays, const void *d_org, const void *d_dir, const void *d_tmax,
                                              int ray_format, int record_format, void *d_prim_or_rec16, void *d_t, void *d_u, void *d_v,
                                              void *d_occ, int mode, const void *d_index, size_t n_index, const void *d_count, void *stream)
{
    /* no bounds: the unbounded entry point itself */
    if (!d_tmax)
        return d_index == NULL && n_index == 0 && d_count == NULL
                   ? lh_accel_intersect_device_ex(a, n_rays, d_org, d_dir, ray_format, record_format, d_prim_or_rec16, d_t, d_u, d_v, d_occ, mode, stream)
                   : lh_accel_intersect_device_indexed(a, n_rays, d_org, d_dir, ray_format, record_format, d_prim_or_rec16, d_t, d_u, d_v, d_occ, mode,
                                                       d_index, n_index, d_count, stream);
    return listed_launch(a, "lh_accel_intersect_device_tmax", n_rays, d_org, d_dir, d_tmax, ray_format, record_format, d_prim_or_rec16, d_t, d_u, d_v, d_occ, mode,
                         d_index, n_index, d_count, stream);
}

extern "C" int lh_accel_trace_statistics(lh_accel_t *a, int enable)
{
    lh_guard guard(a);
    if (!a) return fail("lh_accel_trace_statistics: NULL accel");
    a->stat_on = enable != 0;
    return 0;
}

extern "C" int lh_accel_statistics(lh_accel_t *a, uint64_t counters[5], int clear)
{
    lh_guard guard(a);
    if (!a) return fail("lh_accel_statistics: NULL accel");
    if (counters) for (int k = 0; k < 5; k++) counters[k] = a->stat[k];
    if (clear) for (int k = 0; k < 5; k++) a->stat[k] = 0;
    return 0;
}

extern "C" int lh_accel_slot_statistics(lh_accel_t *a, uint64_t slots[3], int clear)
{
    lh_guard guard(a);
    if (!a) return fail("lh_accel_slot_statistics: NULL accel");
    if (slots) for (int k = 0; k < 3; k++) slots[k] = a->stat_slots[k];
    if (clear) for (int k = 0; k < 3; k++) a->stat_slots[k] = 0;
    return 0;
}

/* ------------------------------------------------------------------------ */
/* one synchronous ray: accel_intersect_func as lucille calls it              */
/* ------------------------------------------------------------------------ */
/* lucille calls accel->intersect(accel, ray, state, user) for ONE ray from up to 16 render threads at once (raytrace.c:31-69,
 * render.c:1043-1105; 18 call sites in whitted.c, shader.c, ibl.c).  A launch per call is ~100 us of copies, launch and
 * synchronisation for ~1 us of work, and the calls serialise on the accelerator's lock: ~10 000 rays/s whatever the thread
 * count (rounds 1-3).  Here concurrent callers are COALESCED (flat combining): a caller writes its ray into the open batch --
 * a slot of a pinned, device-visible block -- and either finds a batch in flight (it sleeps until its own batch is done) or
 * becomes the leader: it waits a few microseconds for the other render threads (which come back from their previous ray
 * at about the same time), closes the batch, launches it straight out of the pinned block (no copies: the kernel reads the
 * rays and writes the records over the link), and wakes the batch's owners.  While a batch runs the next one fills (two
 * blocks).  Records are the batch path's, bit for bit.  set_param("combine", 0) restores one launch per call. */
#define LH_COMB_CAP 64
struct lh_combiner {
    pthread_mutex_t mu; pthread_cond_t cv;
    unsigned long long open_gen, done_gen;      /* the batch that accepts rays; batches finished (done_gen > g: batch g is done) */
    int leader_active;
    volatile int n_pending;                     /* rays in the open batch */
    int readers_left[2], rc[2], expect;
    char err[2][256];
    void *block; double *org[2], *dir[2], *t[2], *u[2], *v[2]; uint32_t *prim[2];       /* pinned host memory the device reads / writes */
    void *d_block; double *d_org[2], *d_dir[2], *d_t[2], *d_u[2], *d_v[2]; uint32_t *d_prim[2];
    hipStream_t stream;
    unsigned long long batches, rays;
};

static int comb_create(lh_accel_t *a)
{
    lh_combiner *c = (lh_combiner *)calloc(1, sizeof(*c));
    if (!c) return fail("out of memory");
    const size_t per = sizeof(double) * (3 + 3 + 1 + 1 + 1) * LH_COMB_CAP + sizeof(uint32_t) * LH_COMB_CAP;
    if (hipHostMalloc(&c->block, 2 * per, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer(&c->d_block, c->block, 0) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        const hipError_t e = hipGetLastError();
        if (c->block) (void)hipHostFree(c->block);
        free(c);
        return fail("lh_accel_intersect1: the pinned block of the combiner could not be set up: %s", hipGetErrorString(e));
    }
    for (int b = 0; b < 2; b++) {
        char *h = (char *)c->block + (size_t)b * per, *d = (char *)c->d_block + (size_t)b * per;
        c->org[b] = (double *)h; c->dir[b] = c->org[b] + 3 * LH_COMB_CAP; c->t[b] = c->dir[b] + 3 * LH_COMB_CAP; c->u[b] = c->t[b] + LH_COMB_CAP;
        c->v[b] = c->u[b] + LH_COMB_CAP; c->prim[b] = (uint32_t *)(c->v[b] + LH_COMB_CAP);
        c->d_org[b] = (double *)d; c->d_dir[b] = c->d_org[b] + 3 * LH_COMB_CAP; c->d_t[b] = c->d_dir[b] + 3 * LH_COMB_CAP; c->d_u[b] = c->d_t[b] + LH_COMB_CAP;
        c->d_v[b] = c->d_u[b] + LH_COMB_CAP; c->d_prim[b] = (uint32_t *)(c->d_v[b] + LH_COMB_CAP);
    }
    pthread_mutex_init(&c->mu, NULL); pthread_cond_init(&c->cv, NULL);
    c->expect = 1;
    __atomic_store_n(&a->comb, c, __ATOMIC_RELEASE);          /* published last: a caller that sees the pointer (acquire) sees the mutex and the block pointers */
    return 0;
}

void lh_comb_destroy(lh_accel_t *a)
{
    lh_combiner *c = a->comb;
    if (!c) return;
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->block) (void)hipHostFree(c->block);
    pthread_mutex_destroy(&c->mu); pthread_cond_destroy(&c->cv);
    free(c); a->comb = NULL;
}

static int comb_run(lh_accel_t *a, lh_combiner *c, int b, int n)
{
    lh_guard guard(a);                       /* the accelerator's device state: one launch at a time */
    HIPCHK(hipSetDevice(a->device));
    if (lh_launch(a, lh_batch_t{(size_t)n, LH_MODE_CLOSEST, c->d_org[b], c->d_dir[b], c->d_prim[b], c->d_t[b], c->d_u[b], c->d_v[b], NULL, NULL},
                  LH_VARIANT_DEFAULT, c->stream, true) != 0) return -1;
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int lh_accel_combine_statistics(lh_accel_t *a, uint64_t out[2], int clear)
{
    if (!a || !out) return fail("lh_accel_combine_statistics: NULL argument");
    out[0] = out[1] = 0;
    lh_combiner *c = a->comb;
    if (!c) return 0;
    pthread_mutex_lock(&c->mu);
    out[0] = c->batches; out[1] = c->rays;
    if (clear) c->batches = c->rays = 0;
    pthread_mutex_unlock(&c->mu);
    return 0;
}

extern "C" int lh_accel_intersect1(lh_accel_t *a, const double org[3], const double dir[3],
                                   uint32_t *prim, double *t, double *u, double *v)
{
    uint32_t p = LH_MISS_PRIM; double tt = LH_T_INF, uu = 0.0, vv = 0.0;
    if (!a || !a->committed) return fail("lh_accel_intersect1: accel not committed");
    if (!org || !dir) return fail("lh_accel_intersect1: NULL ray");
    /* One ray, on the calling thread, over the host copy of the trees (lh_hostwalk.c): a device answers a
     * single ray in ~20 us whatever its kernel does, the host walks lucille's example scenes in 0.2-0.3 us -- and sixteen render
     * threads walk side by side instead of queueing for one launch.  Same filter, same fp64 test, same tie and fragile-hit rules:
     * the same record.  For scenes whose trees live on the host (host-built commits; a device-built or received scene has none),
     * while a walk stays cheaper than the device's amortised answer (LH_HOST_WALK_MAX_NS, 8 us: the incoherent rays of a
     * million-triangle soup cost the host 5-10 us of cache misses each); statistics and per-ray diagnostics stay on the device. */
    if (__atomic_load_n(&a->host_walk, __ATOMIC_RELAXED) && !__atomic_load_n(&a->stat_on, __ATOMIC_RELAXED)) {
        const lh_host_scene *hs = a->hs;
        const bool trees_here = !hs->device_built && !hs->received && hs->bvh.q4nodes && hs->bvh.tri32 && hs->bvh.tri64 &&
                                (!hs->have_ref || (!hs->ref_on_device && __atomic_load_n(&hs->ref_state, __ATOMIC_ACQUIRE) == 2 && hs->ref.nodes));
        static const bool cpu_fma = __builtin_cpu_supports("fma");          /* lh_hostwalk.o is compiled with -mfma */
        if (trees_here && cpu_fma && (hs->bvh.ntris == 0 || __atomic_load_n(&a->hw_gpu_left, __ATOMIC_RELAXED) <= 0)) {
            static const double max_ns = getenv("LH_HOST_WALK_MAX_NS") ? atof(getenv("LH_HOST_WALK_MAX_NS")) : 8000.0;
            static thread_local unsigned long long tl_calls = 0;          /* per thread: sixteen render threads must not share a counter's cache line */
            const unsigned long long k = tl_calls++;
            const bool timed = (k & 63ull) == 63ull;         /* one call in 64 is timed (never the first: cold caches, page faults) */
            if (timed) __atomic_fetch_add(&a->hw_calls, 64ull, __ATOMIC_RELAXED);
            const double t0 = timed ? lh_now_s() : 0.0;
            const int hit = lh_host_walk_closest(&hs->bvh, hs->have_ref ? &hs->ref : NULL, org, dir, &p, &tt, &uu, &vv);
            if (timed) {
                const double ns = (lh_now_s() - t0) * 1e9, old = a->hw_ns;
                const double mean = old > 0.0 ? 0.75 * old + 0.25 * ns : ns;
                a->hw_ns = mean;                              /* racy by design: a statistic */
                if (mean > max_ns && k >= 255ull) __atomic_store_n(&a->hw_gpu_left, 65536, __ATOMIC_RELAXED);       /* long walks (four samples or more agree): the device for a while, then another look */
            }
            if (hit != -2) {
                if (prim) *prim = p;
                if (t) *t = tt;
                if (u) *u = uu;
                if (v) *v = vv;
                return hit;
            }
            p = LH_MISS_PRIM; tt = LH_T_INF; uu = vv = 0.0;          /* the host walk ran out of stack rows: this ray through the device */
        }
        if (trees_here) __atomic_fetch_sub(&a->hw_gpu_left, 1, __ATOMIC_RELAXED);
    }
    if (!__atomic_load_n(&a->combine, __ATOMIC_RELAXED) || __atomic_load_n(&a->stat_on, __ATOMIC_RELAXED)) {         /* statistics are per launch: counted launches stay one ray each */
        if (lh_accel_intersect_host(a, 1, org, dir, &p, &tt, &uu, &vv, NULL, LH_MODE_CLOSEST) != 0) return -1;
    } else {
        lh_combiner *c = __atomic_load_n(&a->comb, __ATOMIC_ACQUIRE);
        if (!c) {
            lh_guard guard(a);
            if (!a->comb) { HIPCHK(hipSetDevice(a->device)); if (comb_create(a) != 0) return -1; }
            c = a->comb;
        }
        int rc = 0;
        pthread_mutex_lock(&c->mu);
        while (c->n_pending >= LH_COMB_CAP) pthread_cond_wait(&c->cv, &c->mu);
        const unsigned long long g = c->open_gen;
        const int b = (int)(g & 1ull), slot = c->n_pending;
        for (int k = 0; k < 3; k++) { c->org[b][3 * slot + k] = org[k]; c->dir[b][3 * slot + k] = dir[k]; }
        __atomic_store_n(&c->n_pending, slot + 1, __ATOMIC_RELEASE);
        for (;;) {
            if (__atomic_load_n(&c->done_gen, __ATOMIC_ACQUIRE) > g) break;      /* somebody ran my batch */
            if (!c->leader_active && c->open_gen == g) {
                if (c->readers_left[b] != 0) { pthread_cond_wait(&c->cv, &c->mu); continue; }     /* owners of batch g - 2 still copy their records out of this block */
                c->leader_active = 1;
                /* the other render threads come back from their previous ray about now: wait for as many as the last batches
                 * held, a few microseconds at most */
                static const double gather_us = getenv("LH_COMB_GATHER_US") ? atof(getenv("LH_COMB_GATHER_US")) : 50.0;
                if (gather_us > 0.0 && c->expect > 1 && c->n_pending < c->expect) {
                    pthread_mutex_unlock(&c->mu);
                    const double t0 = lh_now_s();
                    while (__atomic_load_n(&c->n_pending, __ATOMIC_ACQUIRE) < c->expect && lh_now_s() - t0 < gather_us * 1e-6) { }
                    pthread_mutex_lock(&c->mu);
                }
                const int n = c->n_pending;
                c->n_pending = 0; c->open_gen = g + 1;                   /* closed: arrivals fill the other block */
                pthread_cond_broadcast(&c->cv);                           /* callers waiting for room */
                pthread_mutex_unlock(&c->mu);
                const int r = comb_run(a, c, b, n);
                pthread_mutex_lock(&c->mu);
                c->rc[b] = r;
                if (r != 0) { snprintf(c->err[b], sizeof(c->err[b]), "%s", lh_last_error()); }
                c->readers_left[b] = n; c->leader_active = 0;
                __atomic_store_n(&c->done_gen, g + 1, __ATOMIC_RELEASE);
                c->batches++; c->rays += (unsigned long long)n;
                c->expect = n > c->expect ? n : (n + 3 * c->expect) / 4;     /* follows the callers' concurrency, decays slowly */
                if (c->expect < 1) c->expect = 1;
                pthread_cond_broadcast(&c->cv);
                break;
            }
            /* a batch is ~100 us away at most: watch for it without the mutex for a while (a condition variable's wake-up costs
             * tens of microseconds and sixteen owners take the mutex one after the other), then sleep */
            pthread_mutex_unlock(&c->mu);
            {
                static const double spin_us = getenv("LH_COMB_SPIN_US") ? atof(getenv("LH_COMB_SPIN_US")) : 300.0;
                const double t0 = lh_now_s(); int spins = 0;
                if (spin_us > 0.0) while (__atomic_load_n(&c->done_gen, __ATOMIC_ACQUIRE) <= g && !(__atomic_load_n(&c->leader_active, __ATOMIC_RELAXED) == 0 && __atomic_load_n(&c->open_gen, __ATOMIC_RELAXED) == g)) {
                    LH_CPU_RELAX();
                    if ((++spins & 255) == 0 && lh_now_s() - t0 > spin_us * 1e-6) break;
                }
            }
            pthread_mutex_lock(&c->mu);
            if (__atomic_load_n(&c->done_gen, __ATOMIC_ACQUIRE) > g) break;
            if (!c->leader_active && c->open_gen == g) continue;          /* the leader's seat is free: take it */
            pthread_cond_wait(&c->cv, &c->mu);
        }
        rc = c->rc[b];
        if (rc == 0) { p = c->prim[b][slot]; tt = c->t[b][slot]; uu = c->u[b][slot]; vv = c->v[b][slot]; }
        else lh_fail("%s", c->err[b]);
        if (--c->readers_left[b] == 0) pthread_cond_broadcast(&c->cv);
        pthread_mutex_unlock(&c->mu);
        if (rc != 0) return -1;
    }
    if (prim) *prim = p;
    if (t) *t = tt;
    if (u) *u = uu;
    if (v) *v = vv;
    return p != LH_MISS_PRIM;
}


/* ------------------------------------------------------------------------ */
/* per-ray traversal diagnostics (ri_bvh_diag_t, bvh.h:103-110)               */
/* ------------------------------------------------------------------------ */
/* ri_bvh_intersect zeroes and (built with RI_BVH_ENABLE_DIAGNOSTICS) fills a caller-supplied ri_bvh_diag_t through `user`
 * (bvh.c:451-456,1127,1146,827): inner-node visits, leaf visits, leaf tests of THAT ray -- the testbed's heat maps
 * (simplerender.cpp:202-218).  Here: the same three numbers for THIS build's tree, per ray, from the sequential walk
 * (k_trace_small; the numbers of a speculative walk would depend on its wave-mates): diag = n x 4 u32 -- 4-wide node visits,
 * leaf visits, triangle records through the fp32 filter, fp64 tests.  Records are the batch path's.  A diagnostic path: a
 * lane per ray, no regrouping. */
extern "C" int lh_accel_intersect_diag_host(lh_accel_t *a, size_t n, const double *org, const double *dir, uint32_t *prim,
                                            double *t, double *u, double *v, uint32_t *diag)
{
    lh_guard guard(a);
    const int go = batch_args(a, "intersect_diag", n, org && dir && diag, "argument", LH_MODE_CLOSEST);
    if (go <= 0) return go;
    if (n > 0x7fffffffull) return fail("intersect_diag: more than 2^31 rays");
    HIPCHK(hipSetDevice(a->device));
    if (a->hs->bvh.ntris == 0) {
        memset(diag, 0, sizeof(uint32_t) * 4 * n);
        for (size_t i = 0; i < n; i++) { if (prim) prim[i] = LH_MISS_PRIM; if (t) t[i] = LH_T_INF; if (u) u[i] = 0.0; if (v) v[i] = 0.0; }
        return 0;
    }
    return host_chunk(a, 0, n, org, dir, NULL, 0u, prim, t, u, v, NULL, LH_MODE_CLOSEST, diag);
}

/* the same for rays resident on the device, closest- or any-hit: d_diag n x 4 u32 (see lh_accel_intersect_diag_host); the hit
 * records go to a block of their own (diag_drop: this call writes it on the CALLER's stream and does not wait) and are dropped.  What a cost map of a frame is made of (tools/ao_cost_map.py). */
extern "C" int lh_accel_intersect_diag_device(lh_accel_t *a, size_t n, const void *d_org, const void *d_dir, int mode, void *d_diag, void *stream)
{
    lh_guard guard(a);
    const int go = batch_args(a, "intersect_diag_device", n, d_org && d_dir && d_diag, "argument", mode);
    if (go <= 0) return go;
    if (n > 0x7fffffffull) return fail("intersect_diag_device: more than 2^31 rays");
    HIPCHK(hipSetDevice(a->device));
    hipStream_t s = (hipStream_t)stream;
    if (a->hs->bvh.ntris == 0) { HIPCHK(hipMemsetAsync(d_diag, 0, sizeof(uint32_t) * 4 * n, s)); return 0; }
    const size_t b_d = sizeof(double) * n;
    lh_field_t f[] = {lh_field_scratch(b_d), lh_field_scratch(b_d), lh_field_scratch(b_d), lh_field_scratch(sizeof(uint32_t) * n), lh_field_scratch(n)};      /* t | u | v | prim | occ */
    if (lh_stage_carve(&a->diag_drop, f, 5) != 0) return -1;
    lh_launch_opt opt; opt.diag_out = (uint32_t *)d_diag;
    return lh_launch(a, lh_batch_t{n, mode, d_org, d_dir, f[3].dev, f[0].dev, f[1].dev, f[2].dev, f[4].dev, NULL}, LH_VARIANT_SPEC, s, true, opt);
}

/* ------------------------------------------------------------------------ */
/* beam visibility                                                          */
/* ------------------------------------------------------------------------ */
extern "C" int lh_launch_beam_visibility(const lh_dev_scene_t *sc, size_t n, const double *d_org, const double *d_dirs,
                                         int32_t *d_result, void *stream, const lh_beam_set_t *d_preset);

__global__ void k_fill_i32(size_t n, int32_t *p, int32_t v)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

static int beam_visibility_launch(lh_accel_t *a, size_t n, const void *d_org, const void *d_dirs, void *d_result, void *stream, const lh_beam_set_t *d_preset);

extern "C" int lh_accel_beam_visibility_device(lh_accel_t *a, size_t n, const void *d_org, const void *d_dirs,
                                               void *d_result, void *stream)
{
    return beam_visibility_launch(a, n, d_org, d_dirs, d_result, stream, NULL);
}

static int beam_visibility_launch(lh_accel_t *a, size_t n, const void *d_org, const void *d_dirs, void *d_result, void *stream, const lh_beam_set_t *d_preset)
{
    lh_guard guard(a);
    if (!a || !a->committed) return fail("beam_visibility: accel not committed");
    if (n == 0) return 0;
    if ((!d_preset && (!d_org || !d_dirs)) || !d_result) return fail("beam_visibility: NULL argument");
    if (!a->hs->have_ref) return fail("beam_visibility: the reference-order tree was disabled (LH_REFTREE=0)");
    if (lh_sync_ref(a, true) != 0) return -1;
    HIPCHK(hipSetDevice(a->device));
    lh_dev_scene_t sc = a->dev;
    if (a->hs->bvh.ntris == 0) { sc.ref_empty = 1; }
    if (lh_launch_beam_visibility(&sc, n, (const double *)d_org, (const double *)d_dirs, (int32_t *)d_result, stream, d_preset) != 0)
        return fail("beam kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

/* both host forms: the beams' own arrays (org | dirs) or the caller's preset beams, whichever the entry point has; the absent ones are absent fields */
static int beam_visibility_host(lh_accel_t *a, size_t n, bool have_beams, const double *org, const double *dirs, const lh_beam_set_t *beams, int32_t *result)
{
    lh_guard guard(a);
    if (!a || !a->committed) return fail("beam_visibility: accel not committed");
    if (n == 0) return 0;
    if (!have_beams || !result) return fail("beam_visibility: NULL argument");
    HIPCHK(hipSetDevice(a->device));
    lh_field_t f[] = {lh_field_up(org, sizeof(double) * 3 * n), lh_field_up(dirs, sizeof(double) * 12 * n), lh_field_up(beams, sizeof(lh_beam_set_t) * n),
                      lh_field_down(result, sizeof(int32_t) * n)};
    if (lh_stage_up(a, f, 4) != 0) return -1;
    return lh_stage_down(a, f, 4, beam_visibility_launch(a, n, f[0].dev, f[1].dev, f[3].dev, a->stream, (const lh_beam_set_t *)f[2].dev));
}

extern "C" int lh_accel_beam_visibility_host(lh_accel_t *a, size_t n, const double *org, const double *dirs, int32_t *result)
{
    return beam_visibility_host(a, n, org && dirs, org, dirs, NULL, result);
}

/* beams the caller's own ri_beam_set has set up (lh_beam_set_t: ri_bvh_intersect_beam_visibility's argument, bvh.h:208-221) */
extern "C" int lh_accel_beam_visibility_set_host(lh_accel_t *a, size_t n, const lh_beam_set_t *beams, int32_t *result)
{
    return beam_visibility_host(a, n, beams != NULL, NULL, NULL, beams, result);
}

/* ------------------------------------------------------------------------ */
/* the beam-raster path (ri_bvh_intersect_beam, bvh.c:544-609)               */
/* ------------------------------------------------------------------------ */
extern "C" int lh_launch_beam_raster(const lh_dev_scene_t *sc, size_t n, const double *d_org, const double *d_dirs, const double *d_corner,
                                     const lh_raster_plane_t *plane, double ktan, double *d_t, int32_t *d_status, unsigned long long *d_flags,
                                     void *stream, const lh_beam_set_t *d_preset);

static int beam_raster_launch(lh_accel_t *a, size_t n, const void *d_org, const void *d_dirs, const void *d_corner, const lh_raster_plane_t *plane,
                              void *d_t, void *d_status, void *d_flags, void *stream, const lh_beam_set_t *d_preset);

extern "C" int lh_accel_beam_raster_device(lh_accel_t *a, size_t n, const void *d_org, const void *d_dirs, const void *d_corner,
                                           const lh_raster_plane_t *plane, void *d_t, void *d_status, void *d_flags, void *stream)
{
    return beam_raster_launch(a, n, d_org, d_dirs, d_corner, plane, d_t, d_status, d_flags, stream, NULL);
}

static int beam_raster_launch(lh_accel_t *a, size_t n, const void *d_org, const void *d_dirs, const void *d_corner, const lh_raster_plane_t *plane,
                              void *d_t, void *d_status, void *d_flags, void *stream, const lh_beam_set_t *d_preset)
{
    lh_guard guard(a);
    if (!a || !a->committed) return fail("beam_raster: accel not committed");
    if (n == 0) return 0;
    if ((!d_preset && (!d_org || !d_dirs)) || !d_corner || !plane || !d_t || !d_status) return fail("beam_raster: NULL argument");
    if (plane->width <= 0 || plane->height <= 0) return fail("beam_raster: the raster window is %d x %d", plane->width, plane->height);
    if (!a->hs->have_ref) return fail("beam_raster: the reference-order tree was disabled (LH_REFTREE=0)");
    if (lh_sync_ref(a, true) != 0) return -1;
    HIPCHK(hipSetDevice(a->device));
    lh_dev_scene_t sc = a->dev;
    if (a->hs->bvh.ntris == 0) { sc.ref_empty = 1; }
    /* (1.0 / tan(0.5 * fov_rad)) exactly as raster.c:120,135-136 evaluates it, on the host */
    const double fov_rad = plane->fov * M_PI / 180.0;
    const double ktan = 1.0 / tan(0.5 * fov_rad);
    if (lh_launch_beam_raster(&sc, n, (const double *)d_org, (const double *)d_dirs, (const double *)d_corner, plane, ktan, (double *)d_t,
                              (int32_t *)d_status, (unsigned long long *)d_flags, stream, d_preset) != 0)
        return fail("beam raster kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

/* both host forms, as beam_visibility_host.  t_out goes up AND down: planes that are not traced keep the caller's contents */
static int beam_raster_host(lh_accel_t *a, size_t n, bool have_beams, const double *org, const double *dirs, const lh_beam_set_t *beams, const double *corner,
                            const lh_raster_plane_t *plane, double *t_out, int32_t *status, uint64_t *flags)
{
    lh_guard guard(a);
    if (!a || !a->committed) return fail("beam_raster: accel not committed");
    if (n == 0) return 0;
    if (!have_beams || !corner || !plane || !t_out || !status) return fail("beam_raster: NULL argument");
    if (plane->width <= 0 || plane->height <= 0) return fail("beam_raster: the raster window is %d x %d", plane->width, plane->height);
    HIPCHK(hipSetDevice(a->device));
    const size_t px = (size_t)plane->width * (size_t)plane->height;
    lh_field_t f[] = {lh_field_up(org, sizeof(double) * 3 * n), lh_field_up(dirs, sizeof(double) * 12 * n), lh_field_up(beams, sizeof(lh_beam_set_t) * n),
                      lh_field_up(corner, sizeof(double) * 3 * n), lh_field_both(t_out, sizeof(double) * px * n), lh_field_down(status, sizeof(int32_t) * n),
                      lh_field_down(flags, sizeof(uint64_t) * 4 * n)};
    if (lh_stage_up(a, f, 7) != 0) return -1;
    return lh_stage_down(a, f, 7, beam_raster_launch(a, n, f[0].dev, f[1].dev, f[3].dev, plane, f[4].dev, f[5].dev, f[6].dev, a->stream, (const lh_beam_set_t *)f[2].dev));
}

extern "C" int lh_accel_beam_raster_host(lh_accel_t *a, size_t n, const double *org, const double *dirs, const double *corner,
                                         const lh_raster_plane_t *plane, double *t_out, int32_t *status, uint64_t *flags)
{
    return beam_raster_host(a, n, org && dirs, org, dirs, NULL, corner, plane, t_out, status, flags);
}

extern "C" int lh_accel_beam_raster_set_host(lh_accel_t *a, size_t n, const lh_beam_set_t *beams, const double *corner,
                                             const lh_raster_plane_t *plane, double *t_out, int32_t *status, uint64_t *flags)
{
    return beam_raster_host(a, n, beams != NULL, NULL, NULL, beams, corner, plane, t_out, status, flags);
}

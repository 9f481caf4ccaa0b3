/*
 * lh_internal.h -- what the translation units of liblucille_hip.so share: the accelerator object, the refcounted host
 * scene, error reporting and the launch helpers.  Internal (the public C ABI is include/lucille_hip.h).
 *
 *   lh_commit.hip   lifetime: create / add meshes / commit (host or device build) / replicas / destroy / parameters
 *   lh_query.hip    ray queries: device, host and pipelined host batches, statistics, beam visibility; lh_launch(accel, batch, ...), the
 *                   one way a batch of rays (lh_batch_t) reaches the kernels' launcher (lh_kernels.hip lh_launch_trace)
 *   lh_plan.h       the geometry of a persistent launch (rows, checked pushes, the top of the tree in LDS, workgroups per CU, the cooperative
 *                   walk beside it, the cursor chunk): plain C, read by the launchers, by size_grid and by tests/cpu_model/lh_plan_check.c
 *   lh_stage.h      the layout of a host form's staging block (fields in order, each on a 16-byte boundary): plain C, read by lh_stage_carve below and by
 *                   tests/cpu_model/lh_stage_check.c
 *   lh_gather.h     the kinds of gather stage (AO, dirt, environment, direct light, area lights) and its plan -- fused, late -- for a tile or a batch: plain C, read by
 *                   lh_tile.hip and by tests/cpu_model/lh_gather_check.c
 *   lh_tile.hip     the callers on either side: AO tiles / bands / frames, hit epilogue, path-traced tiles
 *   lh_whitted.hip  the refraction chain (the reference's Whitted transport): its bounce kernel, its wavefront loop, its entry points
 */
#ifndef LH_INTERNAL_H
#define LH_INTERNAL_H

#include <hip/hip_runtime.h>

#include <math.h>
#include <pthread.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "../../include/lucille_hip.h"
#include "lh_bvh.h"
#include "lh_refbvh.h"
#include "lh_device.h"
#include "lh_order.h"
#include "lh_tex.h"
#include "lh_stage.h"

/* lh_last_error() of the calling thread; lh_fail formats it and returns -1 */
int lh_fail(const char *fmt, ...);
#define fail lh_fail
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) \
    return lh_fail("%s failed: %s", #x, hipGetErrorString(e_)); } while (0)

/* attribute kinds of lh_accel_set_attribute: per-vertex xyz (colour, tangent, binormal), per-vertex st,
 * per-index st (texcoords_unshared) -- the optional members of ri_geom_t that ri_intersection_state_build reads */
struct lh_mesh_copy { uint32_t npos, nidx; double *pos; uint32_t *idx; double *nrm; int two_side;
                      double *attr[5]; };

/* a mesh handed over as device arrays (lh_accel_add_mesh_device): the library's own device copy of what the flatten kernel reads --
 * one block, the vertices in the caller's format and stride, then the indices -- and, for the kernel, its descriptor (lh_flatten.hip) */
struct lh_dmesh_attr { void *block; size_t stride; int fmt, has; };          /* has: the mesh carries the attribute (block stays NULL for a mesh without triangles) */
#define LH_DATTR_NORMAL 5         /* slot of the normals behind the five LH_ATTR_* kinds */
#define LH_DATTR_SLOTS 6
struct lh_dmesh { void *block; const void *pos; const uint32_t *idx; size_t stride; uint32_t npos, ntris; int fmt;
                  uint32_t nidx; int two_side;
                  lh_dmesh_attr attr[LH_DATTR_SLOTS];      /* lh_accel_set_normals_device / _set_attribute_device: own copies, caller's format and stride */
                  void *pos_own; };      /* the vertices an update handed over in another format or stride than block's (lh_accel_update_mesh_device); pos points into it then */
typedef struct lh_dmesh_desc { const void *pos; const uint32_t *idx; unsigned long long stride; uint32_t npos, fmt; } lh_dmesh_desc_t;
/* what k_gather_attributes reads of a mesh beside its lh_dmesh_desc_t: data[k] NULL = the mesh lacks slot k */
typedef struct lh_dmesh_attr_desc { const void *data[LH_DATTR_SLOTS]; unsigned long long stride[LH_DATTR_SLOTS]; uint32_t f32_mask, two_side, nidx, pad; } lh_dmesh_attr_desc_t;
/* the per-primitive arrays the gather fills; NULL = no mesh of the scene has it */
typedef struct lh_gather_out { double *nrm9, *attr9[3], *st6; uint8_t *inside; } lh_gather_out_t;
struct lh_dmesh_event { hipStream_t stream; hipEvent_t ev; };          /* the last copy enqueued on a caller's stream: the commit waits for it */

struct lh_buf { void *p; size_t cap; };
/* the accelerator's sun-and-sky light as the launchers take it (lh_accel_set_sky; lh_sky.h): the caller's struct and the three Perez denominators,
 * which depend on the sky alone and are made once, on the host, when it is set */
typedef struct lh_sky_src { lh_sky_t sky; float den[3]; } lh_sky_src_t;
/* material textures (lh_tex.h, lh_tex.hip).  A block of texels, shared by the meshes one setter call gave it to: a host copy until the first call
 * that needs it on the device (lh_accel_set_texture works without a device, before commit), or the device copy lh_accel_set_texture_device
 * enqueued on the caller's stream (ev: recorded behind that copy, waited for once) */
struct lh_tex_block { int refs, width, height; float *host; void *dev; hipEvent_t ev; int ev_live; };
/* what a textured resolve and k_tex_batch read beside the per-sample slots: the closest-hit records by sample / ray id, the texture coordinates
 * per primitive (NULL: no mesh has any), the mesh ordinal per primitive, the per-mesh descriptor table */
typedef struct lh_tex_args { const uint32_t *prim; const double *u, *v, *st6; const uint32_t *prim_mesh; const lh_tex_desc_t *table; } lh_tex_args_t;
/* what the gather stage (lh_tile.hip ao_stage) owns for one transport (LH_GATHER_*, lh_gather.h) and one caller (the tile pipeline, a caller's batch):
 * one entry of lh_accel::gather.  lh_buf members only (LH_GATHER_BUFS of them: the release is a loop).  Slot of every sample / list entry, hit
 * records, slot keys, per-slot occlusion counts (fused AO), the materialised rays and the any-hit bytes (of a fused environment gather too), the
 * compaction's block counts; */
struct lh_gather_scratch {
    lh_buf slot, hitrec, key, occcount, aorg, adir, occ, blocks;
    lh_buf t, bound, prim, uv;          /* the dirt stage (lh_dirt.h): the t of its bounded closest-hit records; materialised, the bounds and the rest of the records */
    lh_buf totals;                      /* a batch: the hits, then the resolve's 64 counters (a tile's are d_total) */
    lh_buf rays;                        /* a dirt or environment tile: its camera rays and their records (org | dir | t | u | v | prim); the AO tile's are r_org ... r_v */
    lh_buf sun;                         /* the sun's shadow rays and their any-hit bytes, per hit slot: org | dir | occ */
};
#define LH_GATHER_BUFS 15
#define LH_AOQ_SLOTS 4
#define LH_PIPE_DEPTH_MAX 8   /* staging blocks of a pipelined host batch (lh_query.hip) */

/* the host side of a committed scene: ONE build, any number of device replicas (lh_multi.hip
 * uploads it to every GPU of the node; SURVEY.md 8e "replicated BVH") */
struct lh_host_scene {
    int refs;                 /* guarded by g_scene_mu */
    lh_bvh_t bvh;
    lh_refbvh_t ref;          /* reference-order tree (ties, beams, the reference walk) */
    int have_ref;
    double ref_build_seconds;
    double *nrm9;             /* per-primitive vertex normals (9 doubles, NaN = none) or NULL */
    double *attr9[3];         /* colour / tangent / binormal per primitive (9 doubles, NaN = none) or NULL */
    double *st6;              /* texture coordinates per primitive (6 doubles, NaN = none) or NULL */
    uint8_t *inside;          /* per primitive: the back half of a two-sided mesh (intersection_state.c:233-241) or NULL */
    uint32_t nmeshes;         /* meshes the scene was committed with */
    /* device build (lh_build.hip): the host holds the flattened primitives only; the reference-order tree is built by a
     * background thread and attached to the replicas when it is ready (ref_state: 0 none, 1 building, 2 ready, -1 failed) */
    int device_built;
    int received;             /* the scene arrived as an image from another rank (lh_dist.hip): device arrays only */
    int ref_on_device;        /* lucille's own tree of a device-built scene was built on the device too (lh_refbuild.hip): no host copy */
    int device_meshes;        /* the scene came from device arrays (lh_accel_add_mesh_device): no host copy of its triangles, one device, no export */
    int ref_state; pthread_t ref_thread; int ref_thread_live; int ref_threads;
    void **trash; uint32_t ntrash;   /* host blocks the device-side commit no longer needs: freed by the background thread (unmapping 0.5 GB takes 0.1 s) */
};
extern pthread_mutex_t g_scene_mu;

struct lh_accel {
    int device;
    int committed;
    int commit_failed;        /* a commit that failed half-way: device memory is released by destroy, a retry is refused */
    /* staged meshes (host copies, packed xyz) */
    lh_mesh_copy *meshes; uint32_t nmeshes;
    /* ... or staged device meshes (never both): device copies until the commit has flattened them */
    lh_dmesh *dmeshes; uint32_t ndmeshes; unsigned long long dmesh_tris;
    lh_dmesh_event *dmesh_events; uint32_t ndmesh_events;
    /* "updatable" = 1: the commit keeps dmeshes and dmesh_events (ndmeshes stays non-zero on a committed accelerator: the only one), updates stage
     * into them and lh_accel_recommit rebuilds from them.  update_fellback: the commit took dmesh_host_fallback, which needs the blocks gone */
    int updatable, update_fellback, staged_pos, staged_attr;
    int build_depth_cap;               /* 4-wide levels a device-built tree may have (beyond: the outcome LH_SIDE_TOO_DEEP of lh_route.h -- the host builders; a replica and a re-commit fail) */
    lh_host_scene *hs;        /* never NULL after create */
    void *d_ref_lca, *d_prim_leafpos, *d_ref_nodes, *d_ref_leaf_prims;   /* lucille's own tree: owned here, published in dev (lh_commit.hip publish_scene) */
    void *d_danger;                    /* 8 + LH_DANGER_MAX x 6 doubles: the count, then the boxes of lh_dev_scene_t.danger (lh_commit.hip lh_danger_scan) */
    /* device */
    lh_dev_scene_t dev;                /* what the kernels get: the resident scene (written by lh_commit.hip publish_scene only) and the knobs of
                                          create / set_param; its per-launch fields stay zero here -- a launch sets them in a copy (lh_launch) */
    void *d_nodes, *d_tri32, *d_tri64, *d_q4nodes, *d_q8nodes;   /* the owners of the scene's arrays (lh_commit.hip scene_rows) */
    int ncus;                          /* compute units of the device */
    int wide8;                         /* ray dumps walk the 8-wide nodes: -1 when the hot set exceeds the Infinity Cache (default), 0 never, 1 always */
    unsigned long long *d_cursor, *d_counters;   /* d_cursor: LH_NCURSOR blocks of LH_CURSOR_WORDS words (a line per cursor + the drained mask), one block per launch in flight */
    unsigned cursor_next;
    pthread_mutex_t mu;                /* serialises the entry points of ONE accelerator (recursive) */
    int stat_on;                       /* lh_accel_trace_statistics */
    unsigned long long stat[5];        /* nodes, filter tests, fp64 tests, rays, hits */
    unsigned long long stat_slots[3];  /* lane slots (64 per wave iteration) of node steps, triangle passes, regroups (tile pipelines, lh_accel_slot_statistics) */
    hipStream_t stream;
    uint64_t device_bytes;
    double upload_seconds;
    int grid_blocks;
    int grid_user;                     /* the persistent grid was set by the caller (set_param "grid", LH_GRID_BLOCKS): launches do not resize it */
    int min_active;
    uint32_t ray_chunk;                /* rays reserved per cursor atomic (LH_RAY_CHUNK) */
    int tri_batch;
    int knobs_user;                    /* min_active / tri_batch were set by the caller (set_param, LH_MIN_ACTIVE, LH_TRI_BATCH): ray dumps do not pick their own */
    int default_variant;
    /* per-stream fix-up queues of the persistent launches (rays out of visit budget / stack rows, fragile AO hits) */
    struct { hipStream_t stream; int used; lh_fixq_t q; lh_buf order_ws; } aoq[LH_AOQ_SLOTS];      /* order_ws: the stream's workspace for dumps traced in bin order (lh_order.h) */
    /* THE staging block of every entry point that takes host arrays (lh_stage_up / lh_stage_down below; the ray batches' host_chunk carves it itself):
     * such a call holds the lock, runs on `stream` and synchronises before it returns, so one block serves them all, at the largest size any asked for */
    lh_buf stage;
    lh_buf diag_drop;                  /* lh_accel_intersect_diag_device: the hit records it throws away.  Its own block: it alone writes scratch on a CALLER's stream and returns unsynchronised */
    /* pipelined host batches: a ring of pinned in/out staging blocks and their device twins; rays up on s[0]; trace + records down alternate between s[1] and s[2] */
    struct { void *h_in[LH_PIPE_DEPTH_MAX], *h_out[LH_PIPE_DEPTH_MAX], *d_in[LH_PIPE_DEPTH_MAX], *d_out[LH_PIPE_DEPTH_MAX]; hipStream_t s[3];
             hipEvent_t in_done[LH_PIPE_DEPTH_MAX], done[LH_PIPE_DEPTH_MAX]; size_t cap; int depth, ready; } pipe;
    void *d_nrm9;                      /* hs->nrm9 on the device */
    void *d_attr9[3], *d_st6, *d_inside;            /* colour / tangent / binormal, st, inside flags (uploaded at commit if present) */
    void *d_prim_mesh;                 /* mesh ordinal per primitive (materials; uploaded on first use) */
    lh_material_t *materials; uint32_t nmaterials; void *d_materials; int materials_dirty;
    lh_tex_block **tex; uint32_t ntex_slots, ntex;      /* per mesh (NULL: none), and how many meshes have one: > 0 makes the AO and dirt tiles multiply */
    void *d_tex_table; uint32_t tex_table_n; int tex_dirty;     /* lh_tex_desc_t per mesh on the device, rebuilt by lh_tex_sync after a setter */
    lh_environment_t env; void *d_env_map; int env_set;      /* env_set: lh_accel_set_environment was called (else the path tracer's environment is constant white) */
    lh_buf r_diag;                     /* LH_STAGE_TIMING: wave start / exit clocks */
    lh_buf r_bands;                    /* lh_render_ao_bands: first line of every band */
    void *h_read;                      /* 1 KiB of pinned host memory: the read-backs at the end of an AO batch (occlusion totals, hit count, queue flags) */
    /* tile-render scratch (lh_render_ao_tile): camera rays and closest-hit records */
    lh_buf r_org, r_dir, r_prim, r_t, r_u, r_v;
    /* the gather stage's scratch, [LH_GATHER_*][LH_GATHER_TILE | LH_GATHER_BATCH]: every transport and either caller has a set of its own, so that
     * lh_render_scratch keeps showing the last AO tile whatever ran since */
    lh_gather_scratch gather[LH_GATHER_KINDS][2];
    /* the sun-and-sky light (lh_accel_set_sky; lh_sky.h): sky_set 0 = none, the gather reads the environment */
    lh_sky_src_t sky; int sky_set;
    /* the emitter table of the area lights (lh_accel_set_emitters; lh_area.h): nemit records of 128 bytes on the device, NULL / 0 = none */
    void *d_emitters; uint64_t nemit;
    /* the refraction chain (lh_whitted.hip; lh_whitted.h): the chain's compacted rays, ids and records, sized by list entries; its counts (one per depth);
     * the tile's camera rays, their records and the samples' colours */
    lh_buf w_chain, w_counts, w_tile;
    uint64_t last_retraced;            /* rays the last counted launch finished outside the main kernel */
    int ao_fused;                      /* AO rays generated inside the any-hit kernel (default); 0: materialised in HBM */
    uint32_t ao_budget;                /* visit budget of the fused AO stage (0: dev.ray_budget) */
    int ao_budget_user;                /* set by the caller (set_param / LH_AO_BUDGET / "ray_budget"): taken as it is, whatever the launch's size */
    uint32_t dump_budget;              /* visit budget of ray-dump launches (the tile pipelines': dev.ray_budget) */
    /* ray dumps traced from a copy in bin order (lh_order.h, lh_query.hip lh_launch): "dump_order" 1 / 0; "dump_order_min": the smallest dump that is ordered;
     * "dump_order_bits": cell bits per axis of the key (2: the cell alone, 1: under the direction octant); "dump_order_max_mb": 0, or the largest workspace a stream may hold -- a dump that needs more is traced as given */
    int dump_order; size_t dump_order_min; uint32_t dump_order_bits; size_t dump_order_max_mb;
    unsigned long long order_stat[2];  /* dumps (parts of 2^30 rays at most) traced in bin order, and their rays (lh_accel_order_statistics) */
    int build_auto;                    /* the commit chose the builders by the size of the scene: a failing device build falls back to the host */
    int poison_outputs;                /* LH_POISON_OUTPUTS=1 (tests, tools/fuzz_*): a ray dump's output arrays are filled with 0x77 before the launch -- an answer slot that nobody
                                          writes shows up as a wrong record instead of as whatever the buffer held (the lost any-hit rays of r05 hid behind recycled buffers) */
    int fast_start;                    /* device-built scenes: launch before lucille's own tree is attached (ties by primitive id until then) */
    lh_buf p_org2, p_dir2, p_path, p_path2, p_thr, p_thr2, p_rad, p_counts;   /* path tracer */
    lh_buf p_value;                    /* ... with lights (lh_ptl.h): 12 bytes per entry of a bounce, the light stage's value, then the hit's direct light */
    lh_buf p_value2, p_key;            /* ... with area lights: 12 bytes per entry, the area stage's value, and the entry's 8-byte key for its generator */
    unsigned long long *d_total;
    size_t r_nsamples, r_nslots, r_nao;
    struct lh_combiner *comb;          /* lh_accel_intersect1: concurrent single-ray callers coalesced into one launch (lh_query.hip) */
    int combine;                       /* 1 (default): coalesce; 0: one launch per call, as in rounds 1-3 */
    /* lh_accel_intersect1 on the calling thread, over the host copy of the trees (lh_hostwalk.c): host_walk 1 (default) / 0;
     * hw_ns: what a host walk costs on this scene (ns, running mean of timed samples); hw_calls: calls answered there; hw_gpu_left:
     * calls still to send to the device before the host is probed again (a scene whose walks are long: S-soup-1M's incoherent rays
     * cost 5-10 us of cache misses each on the host, the coalesced device path amortises to about that) */
    int host_walk; unsigned long long hw_calls; double hw_ns; int hw_gpu_left;
};

#define LH_NCURSOR 64
#define LH_BUILD_DEPTH_MAX 86     /* 3 d + 5 <= 264: the rows of k_overflow_fix's private stack */

/* lucille calls accel->intersect from up to 16 render threads at once (render.c:1043-1105): every
 * entry point that touches the accelerator's buffers holds its lock */
struct lh_guard {
    pthread_mutex_t *m;
    explicit lh_guard(const lh_accel_t *a) : m(a ? (pthread_mutex_t *)&a->mu : NULL) { if (m) pthread_mutex_lock(m); }
    ~lh_guard() { if (m) pthread_mutex_unlock(m); }
};


/* a spin-wait hint that is not x86-only */
#if defined(__x86_64__) || defined(__i386__)
#define LH_CPU_RELAX() __builtin_ia32_pause()
#elif defined(__aarch64__)
#define LH_CPU_RELAX() __asm__ __volatile__("yield")
#else
#define LH_CPU_RELAX() ((void)0)
#endif

static inline double lh_now_s(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }
#define now_s lh_now_s

/* node formats a walk can read; only the one the default kernel uses is uploaded at commit, the
 * others (the textbook variant's 2-wide fp32 nodes, the 8-wide nodes of large ray dumps) on first use */
enum { LH_FMT_F32 = 1, LH_FMT_Q16X4 = 4, LH_FMT_Q8 = 32 };

/* lh_commit.hip */
int  lh_ensure_formats(lh_accel_t *a, int mask);
int  lh_sync_ref(lh_accel_t *a, bool wait);          /* attach the background-built reference-order tree (wait: block for it) */
int  lh_ensure_buf(lh_buf *b, size_t bytes);
/* A host form is: fields, up, device form, down.
 *     lh_field_t f[] = {lh_field_up(dir, 24 * n), lh_field_down(rgb, 12 * n)};          -- the block's layout, in order (lh_stage.h)
 *     if (lh_stage_up(a, f, 2) != 0) return -1;
 *     return lh_stage_down(a, f, 2, lh_accel_environment_device(a, n, f[0].dev, f[1].dev, a->stream));
 * lh_stage_carve: lays the fields out (lh_stage.h), grows `block` to hold them and sets every f[k].dev (NULL for an absent field).
 * lh_stage_up: carves a->stage, then enqueues a copy up on a->stream for every field that has one.
 * lh_stage_down: rc is the device form's answer; if it is 0, enqueues a copy down for every field that has one; synchronises a->stream and returns rc,
 * or -1 for a copy that failed.  Both synchronise before they return a failure, so that no copy from the caller's arrays is still in flight then, and
 * leave lh_last_error at what failed FIRST.  The caller holds the accelerator's lock and has set the device */
int  lh_stage_carve(lh_buf *block, lh_field_t *f, int nf);
int  lh_stage_up(lh_accel_t *a, lh_field_t *f, int nf);
int  lh_stage_down(lh_accel_t *a, const lh_field_t *f, int nf, int rc);
int  lh_device_array_ok(const lh_accel_t *a, const void *p, size_t bytes, const char *who, const char *what);      /* `bytes` at p are memory of the accelerator's device: asked of the runtime */
/* lh_tex.hip */
void lh_tex_release(lh_accel_t *a);                  /* every texture block and the table (lh_accel_destroy) */
int  lh_tex_sync(lh_accel_t *a);                     /* pending textures onto the device, the descriptor table, d_prim_mesh; a committed accelerator, its device current */
int  lh_ensure_prim_mesh(lh_accel_t *a);             /* d_prim_mesh, uploaded on first use (materials, textures) */
/* the arguments of a textured resolve over records prim / u / v, or NULL when no mesh has a texture (after lh_tex_sync) */
static inline const lh_tex_args_t *lh_tex_args(const lh_accel_t *a, const void *prim, const void *u, const void *v, lh_tex_args_t *out)
{
    if (!a->ntex) return NULL;
    *out = lh_tex_args_t{(const uint32_t *)prim, (const double *)u, (const double *)v, (const double *)a->d_st6, (const uint32_t *)a->d_prim_mesh,
                         (const lh_tex_desc_t *)a->d_tex_table};
    return out;
}
void lh_free_buf(lh_buf *b);
/* the scene image (lh_commit.hip): one rank's committed scene handed to the others (lh_dist.hip) */
typedef struct lh_scene_image {
    uint32_t magic, ntris, nnodes, max_depth, nleaves, nq4, q4_depth, q4_stack, nq8, q8_depth, ref_nnodes, nmeshes;
    int      have_ref, ref_empty, has_nrm, has_attr[3], has_st, has_inside;
    float    bmin[3], bmax[3], grid_lo[3], grid_step[3];
    double   ref_bmin[3], ref_bmax[3], build_seconds, ref_build_seconds;
    double   deg_dcap; uint32_t nlive, pad_;        /* lh_bvh_t: the triangles outside the traversal tree and the rays that need the reference walk for them */
} lh_scene_image_t;
int  lh_scene_image_header(lh_accel_t *a, lh_scene_image_t *h);
int  lh_scene_image_arrays(lh_accel_t *a, const lh_scene_image_t *h, void **ptr, size_t *bytes, int cap);
uint32_t *lh_scene_image_prim_geom(lh_accel_t *a);
uint32_t *lh_scene_image_prim_index(lh_accel_t *a);
int  lh_scene_image_alloc(lh_accel_t *a, const lh_scene_image_t *h);
int  lh_scene_image_finish(lh_accel_t *a);
/* lh_flatten.hip: the staged device meshes -> lh_tri64_t[ntris] in primitive-id order, one launch */
int  lh_flatten_launch(uint32_t ntris, uint32_t nmeshes, const lh_dmesh_desc_t *d_desc, const uint32_t *d_first, void *d_tri64,
                       uint32_t *d_status, hipStream_t stream);
/* ... and their per-vertex normals and attributes -> the per-primitive arrays of `out`, one launch, after a clean flatten */
int  lh_gather_launch(uint32_t ntris, uint32_t nmeshes, const lh_dmesh_desc_t *d_desc, const lh_dmesh_attr_desc_t *d_attr, const uint32_t *d_first,
                      lh_gather_out_t out, hipStream_t stream);
/* lh_hostwalk.c */
extern "C" int lh_host_walk_closest(const lh_bvh_t *b, const lh_refbvh_t *ref, const double o[3], const double d[3], uint32_t *prim, double *t, double *u, double *v);
/* ... and its bounded variant (lh_tmax.h), closest or any hit: the record of lh_host_walk_closest if it is a hit with t < tmax, else the miss record --
 * by a walk the bound prunes.  How the rule of the bounded launches is checked without a device (tests/cpu_model/lh_tmax_model.c) */
extern "C" int lh_host_walk_tmax(const lh_bvh_t *b, const lh_refbvh_t *ref, const double o[3], const double d[3], double tmax, int anyhit,
                                 uint32_t *prim, double *t, double *u, double *v);
/* lh_query.hip */
void lh_comb_destroy(lh_accel_t *a);                 /* the single-ray combiner's pinned block and stream (lh_accel_destroy) */
/* one batch of rays (lh_batch_t, lh_device.h: rays, records, the LH_CNT_DEV statistics counters or NULL) through the hot path, from a
 * copy of a->dev that carries the launch's own inputs: dump (a ray dump: incoherent rays, dump_budget, the 8-wide nodes where they
 * pay; else a tile pipeline's batch: ray_budget, LH_TILE_CHUNK) and, in lh_launch_opt, what only some callers have */
struct lh_launch_opt {
    uint32_t io_fmt = 0u;                      /* LH_IO_* (lh_device.h): ray dumps in fp32 rays / 16-byte records */
    uint32_t *diag_out = NULL;                 /* four counts per ray (lh_accel_intersect_diag_*) */
    const uint32_t *n_dev = NULL;              /* the ray count lives on the device, n is its upper bound (the path tracer's bounce chain) */
    const void *cam_src = NULL;                /* the rays are the camera rays of a path-traced pass: d_org / d_dir may be NULL */
    unsigned long long *diag_clock = NULL;     /* LH_STAGE_TIMING: start / exit clocks of the launch's waves */
    /* an indexed ray dump (lh_accel_intersect_device_indexed): n is the number of list entries, the arrays hold idx_nrays rays; index NULL: the
     * identity list; n_dev (above): the number of entries to trace, clamped to n */
    bool indexed = false; const uint32_t *index = NULL; uint32_t idx_nrays = 0u;
    /* a bounded ray dump (lh_accel_intersect_device_tmax; with indexed): idx_nrays bounds by ray id, in the rays' type (lh_tmax.h) */
    const void *tmax = NULL;
};
int  lh_launch(lh_accel_t *a, const lh_batch_t &batch, int variant, hipStream_t s, bool dump, const lh_launch_opt &opt = lh_launch_opt());
/* the cursor block of the next persistent launch: LH_NCURSOR of them, taken in turn (one per launch in flight) */
static inline unsigned long long *lh_next_cursor(lh_accel_t *a)
{
    return (unsigned long long *)((uint32_t *)a->d_cursor + (size_t)LH_CURSOR_WORDS * (a->cursor_next++ % LH_NCURSOR));
}
int  lh_aoq_slot(lh_accel_t *a, hipStream_t s);
/* lh_order.hip: a dump's rays into bin order (passes 1 and 2), its records back into the caller's order (pass 3); the walk between them is the caller's */
int  lh_order_run(const lh_order_plan_t *p, const lh_order_grid_t *g, const void *d_org, const void *d_dir, void *d_ws, hipStream_t stream);
int  lh_order_back(const lh_order_plan_t *p, int closest, const void *d_ws, void *d_prim, void *d_t, void *d_u, void *d_v, void *d_occ, hipStream_t stream);
/* a counted launch's words h (LH_CNT_*) into the accelerator's statistics; the caller says what is its own to say: how many rays, how many
 * hits.  slots: the lane-slot words too (the tile pipelines' batches; h holds LH_CNT_DEV words then) */
static inline void lh_stat_add(lh_accel_t *a, const unsigned long long *h, unsigned long long rays, unsigned long long hits, bool slots = false)
{
    a->stat[0] += h[LH_CNT_NODES]; a->stat[1] += h[LH_CNT_TRIS]; a->stat[2] += h[LH_CNT_EXACT];
    a->stat[3] += rays; a->stat[4] += hits;
    if (slots) { a->stat_slots[0] += h[LH_CNT_NODE_SLOTS]; a->stat_slots[1] += h[LH_CNT_TRI_SLOTS]; a->stat_slots[2] += h[LH_CNT_REGROUP_SLOTS]; }
}

/* lh_render.hip: the launchers lh_tile.hip calls (stream is a hipStream_t).  lh_render.hip includes this file too, so a prototype that drifts
 * from its definition does not compile -- under extern "C" it would still link */
extern "C" int lh_render_launch_primary(const lh_camera_t *cam, int x0, int y0, int w, int h, int xs, int ys,
                                        double *d_org, double *d_dir, void *stream);
extern "C" int lh_render_launch_compact(const lh_dev_scene_t *sc, const double *d_nrm9, size_t n, const double *d_org,
                                        const double *d_dir, const uint32_t *d_prim, const double *d_t,
                                        const double *d_u, const double *d_v, uint32_t *d_block_counts,
                                        uint32_t *d_slot_of_sample, double *d_hitrec,
                                        unsigned long long *d_slot_key, int x0, int w, int nbands, int band_rows,
                                        const int *d_band_y0, int y0, int spp, int full_width,
                                        unsigned long long *d_total, double eps, void *stream);
extern "C" int lh_render_launch_primary_region(const lh_camera_t *cam, int x0, int w, int nbands, int band_rows, const int *d_band_y0,
                                               int y0, int height_limit, int xs, int ys, double *d_org, double *d_dir, void *stream);
extern "C" int lh_render_launch_ao_rays(size_t nslots, int ntheta, int nphi, unsigned long long seed,
                                        const double *d_hitrec, const double *d_rnd,
                                        const unsigned long long *d_slot_key, double *d_org, double *d_dir, void *stream);
extern "C" int lh_render_launch_tex_batch(size_t n_list, size_t n_rays, const uint32_t *d_index, const uint32_t *d_count,
                                          const lh_tex_args_t *tex, uint32_t ntris, double *d_rgba, void *stream);
extern "C" int lh_render_launch_batch_compact(const lh_dev_scene_t *sc, const double *d_nrm9, size_t n_list, size_t n_rays,
                                              const uint32_t *d_index, const uint32_t *d_count, const double *d_org, const double *d_dir,
                                              const uint32_t *d_prim, const double *d_t, const double *d_u, const double *d_v,
                                              const unsigned long long *d_key, uint32_t *d_block_counts, uint32_t *d_slot_of_entry,
                                              double *d_hitrec, unsigned long long *d_slot_key, unsigned long long *d_total,
                                              uint32_t *d_nslots32, double eps, void *stream);
extern "C" int lh_render_launch_ao_rays_counted(size_t nslots_max, const unsigned long long *d_nslots, int ntheta, int nphi,
                                                unsigned long long seed, const double *d_hitrec, const double *d_rnd,
                                                const unsigned long long *d_slot_key, double *d_org, double *d_dir, void *stream);
extern "C" int lh_render_launch_dirt_bounds(size_t n, double far_clip, double *d_bound, void *stream);
/* the accelerator's environment as the launchers take it (lh_accel_set_environment; never set: constant white) */
typedef struct lh_env_src { float rgb[3]; const void *map; int w, h; } lh_env_src_t;
/* ... as it stands now (never set: constant white; an explicit black environment stays black) */
static inline lh_env_src_t lh_env_source(const lh_accel_t *a)
{
    lh_env_src_t e;
    for (int k = 0; k < 3; k++) e.rgb[k] = a->env_set ? a->env.rgb[k] : 1.0f;
    e.map = a->d_env_map; e.w = a->env.width; e.h = a->env.height;
    return e;
}
/* the gather stage's resolves: what the stage left, and where its result goes -- a tile's pixels or a batch's per-ray outputs.
 * lh_gather_left_t: the kind (LH_GATHER_*), the hemisphere's grid and the generator's seed; the per-slot counts of a fused AO stage (occ_count, or NULL:
 * N any-hit bytes per slot at occ), the any-hit byte of every gather ray (occ: AO materialised, ENV either way), the dirt stage's t of every gather ray and
 * its clips; for ENV the hit records and keys, the materialised directions (adir, or NULL: a fused stage, the resolve makes them again), the scale and the
 * light -- the environment, or (sky != NULL) the sun-and-sky light with the sun's any-hit byte per slot (sun_occ, or NULL: no sun); total: 64 counters */
typedef struct lh_gather_left {
    int kind, ntheta, nphi; unsigned long long seed;
    const unsigned int *occ_count; const uint8_t *occ; const double *t;
    const double *hitrec; const unsigned long long *key; const double *adir;
    double near_clip, far_clip, scale;
    const lh_env_src_t *env; const lh_sky_src_t *sky; const uint8_t *sun_occ;
    const lh_light_t *lights;          /* LH_GATHER_LIGHT: the HOST table of ntheta lights (nphi is 1); occ holds the byte of every item, hitrec the records */
    const struct lh_area_tab *area;    /* LH_GATHER_AREA: the call's lights, emitter table, bound and replayed uniforms (lh_area.h; HOST memory; ntheta = its S, nphi = its L); occ, hitrec and key as above */
    unsigned long long *total;
} lh_gather_left_t;
/* a region of w x h pixels (h = nbands * band_rows lines), xs * ys samples each, with the hit slot of every sample; tex or NULL: no mesh has a texture */
typedef struct lh_resolve_tile { int w, h, band_rows, xs, ys; const uint32_t *slot_of_sample; float *rgb; const lh_tex_args_t *tex; } lh_resolve_tile_t;
/* a list over n_rays rays (index, count: as lh_accel_intersect_device_indexed) with the hit slot of every entry (NULL: an empty scene, every traced ray
 * is a miss); count_out[id] / value_out[id] (3 floats for ENV): either may be NULL */
typedef struct lh_resolve_list { size_t n_list, n_rays; const uint32_t *index, *count, *slot_of_entry; uint32_t *count_out; float *value_out; } lh_resolve_list_t;
extern "C" int lh_render_launch_tile_resolve(const lh_resolve_tile_t *to, const lh_gather_left_t *g, void *stream);
extern "C" int lh_render_launch_list_resolve(const lh_resolve_list_t *to, const lh_gather_left_t *g, void *stream);
extern "C" int lh_render_launch_env_fetch(size_t n, const lh_env_src_t *env, const double *d_dir, float *d_rgb, void *stream);
extern "C" int lh_render_launch_sky_fetch(size_t n, const lh_sky_src_t *sky, const double *d_dir, float *d_rgb, void *stream);
/* one ray per hit slot from the slot's hit record along sun_dir (d_nslots or NULL: the slot count on the device, nslots its upper bound) */
extern "C" int lh_render_launch_sun_rays(size_t nslots, const unsigned long long *d_nslots, const double *d_hitrec, const double sun_dir[3],
                                         double *d_org, double *d_dir, void *stream);
extern "C" int lh_render_launch_light_rays(size_t nslots, const unsigned long long *d_nslots, const lh_light_t *lights, int n, const double *d_hitrec,
                                           double *d_org, double *d_dir, double *d_tmax, void *stream);
/* the rays, bounds and (d_weight or NULL) weights of nslots hit records' area-light items (lh_area.h), item (slot, l, s) at element (slot * L + l) * S + s */
extern "C" int lh_render_launch_area_rays(size_t nslots, const unsigned long long *d_nslots, const struct lh_area_tab *area, unsigned long long seed,
                                          const double *d_hitrec, const unsigned long long *d_slot_key, double *d_org, double *d_dir, double *d_tmax,
                                          double *d_weight, void *stream);
extern "C" int lh_render_launch_state_build(size_t n, const lh_dev_scene_t *sc, const double *d_nrm9, const double *d_col9,
                                            const double *d_tan9, const double *d_bin9, const double *d_st6, const uint8_t *d_inside,
                                            const double *d_org, const double *d_dir, const uint32_t *d_prim, const double *d_t,
                                            const double *d_u, const double *d_v, double *d_state, void *stream);
extern "C" size_t lh_pt_material_bytes(void);
extern "C" void lh_pt_material_pack(const lh_material_t *m, void *out);
extern "C" int lh_pt_launch_begin(const lh_camera_t *cam, int x0, int y0, int w, int h, int band_rows, int band_stride, int spp, int s0,
                                  unsigned long long seed, void *d_cam, uint32_t *d_counts, int ncounts, void *stream);
extern "C" size_t lh_pt_cam_bytes(void);
extern "C" int lh_pt_launch_shade(size_t n_max, const lh_dev_scene_t *sc, const double *d_nrm9, const double *d_col9,
                                  const uint32_t *d_prim_mesh, const void *d_materials, const lh_material_t *override_mat,
                                  const float env_rgb[3], const void *d_env_map, int env_w, int env_h, int ref_weights,
                                  int depth, int max_depth, unsigned long long seed, int s0, int spp, int x0, int y0, int w,
                                  int band_rows, int band_stride, int full_width, const void *d_cam, uint32_t *d_counts, const double *d_org, const double *d_dir, const uint32_t *d_prim,
                                  const double *d_t, const double *d_u, const double *d_v, const uint32_t *d_path_of,
                                  const float *d_thr, unsigned long long *d_accum, double *d_org2, double *d_dir2, uint32_t *d_path_of2,
                                  float *d_thr2, int ncus, void *stream);
extern "C" int lh_pt_launch_resolve(int w, int h, int band_rows, float inv_total_spp, unsigned long long *d_accum, float *d_rgb, void *stream);
/* the lit pass (lh_ptl.h): the camera rays into memory, a bounce's direct light from the light stage's values, a bounce's entries into the caller's sink */
extern "C" int lh_pt_launch_camera_rays(size_t n, const void *d_cam, double *d_org, double *d_dir, int ncus, void *stream);
extern "C" int lh_pt_launch_direct(size_t n_max, const double *d_col9, const uint32_t *d_prim_mesh, const void *d_materials,
                                   const lh_material_t *override_mat, int depth, int spp, const uint32_t *d_counts, const uint32_t *d_prim,
                                   const double *d_u, const double *d_v, const uint32_t *d_path_of, const float *d_thr, float *d_value, int keep,
                                   unsigned long long *d_accum, int ncus, void *stream);
/* ... with area lights: a bounce's keys for the area stage's generator, and the two stages' values folded into one */
extern "C" int lh_pt_launch_area_keys(size_t n_max, int depth, int spp_total, const void *d_cam, const uint32_t *d_counts, const uint32_t *d_path_of,
                                      unsigned long long *d_key, int ncus, void *stream);
extern "C" int lh_pt_launch_value_add(size_t n_max, int depth, const uint32_t *d_counts, float *d_value, const float *d_area, int ncus, void *stream);
extern "C" int lh_pt_launch_sink(size_t n_max, int depth, const uint32_t *d_counts, const double *d_org, const double *d_dir, const uint32_t *d_prim,
                                 const double *d_t, const double *d_u, const double *d_v, const uint32_t *d_path_of, const float *d_thr,
                                 const float *d_direct, const lh_pt_sink_t *sink, int ncus, void *stream);

#endif

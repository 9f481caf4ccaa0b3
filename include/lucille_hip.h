/*
 * lucille_hip.h -- C ABI of liblucille_hip.so: the MI355X (gfx950) accelerator
 * for lucille's ray-query hot path.  Plain C, plain pointers and sizes; no
 * C++/torch types cross this boundary.  Every function returns 0 on success
 * and -1 on failure (lh_last_error() holds a message); nothing throws.
 *
 * Each entry point names the reference interface it stands in for (paths are
 * relative to the lucille source tree).  The reference-side glue a lucille
 * maintainer adds (a new RI_ACCEL_HIP case in ri_accel_bind that forwards to
 * these functions) is shown in INTEGRATION.md and lives, compilable against
 * the reference's own headers, in integration/ri_accel_hip.c.
 */
#ifndef LUCILLE_HIP_H
#define LUCILLE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LH_MISS      0xFFFFFFFFu     /* prim id of a miss                     */
#define LH_INFINITY  1.0e38          /* t of a miss == RI_INFINITY (include/ri.h:47) */

/* query modes */
#define LH_MODE_CLOSEST 0            /* ri_bvh_intersect semantics            */
#define LH_MODE_ANY     1            /* boolean occlusion: the value calculate_occlusion
                                        actually consumes (ambientocclusion.c:123-129) */

/* kernel variants: LH_VARIANT_DEFAULT picks the tuned walk (= 4); 0 is the textbook walk kept as in-process reference */
#define LH_VARIANT_DEFAULT (-1)

typedef struct lh_accel lh_accel_t;  /* opaque: host BVH + device SoA copies  */
typedef struct lh_rib_scene lh_rib_scene_t;   /* a parsed RIB (below)         */

typedef struct lh_accel_info {
    uint32_t ntriangles;
    uint32_t nnodes;
    uint32_t nleaves;
    uint32_t max_depth;
    uint64_t device_bytes;           /* HBM footprint of the scene: the node format the default
                                        kernel walks + triangles + the reference-order tree;
                                        other node formats are uploaded when a variant first asks */
    double   build_seconds;          /* host build of the traversal tree      */
    double   upload_seconds;
    int      device;
    double   ref_build_seconds;      /* host build of the reference-order tree (lucille's own tree,
                                        kept for ties / fragile hits / beams): part of every commit */
    uint32_t nnodes_traversal;       /* 4-wide nodes the default kernel walks  */
    uint32_t ntriangles_in_tree;     /* ntriangles minus the zero-area triangles the reference can never report (two equal
                                        vertices: its determinant test, bvh.c:754, rejects them for every ray): those keep their
                                        primitive ids and stay in lucille's own tree, but no leaf of the traversal tree holds them */
} lh_accel_info_t;

/* ---- runtime ----------------------------------------------------------- */
int         lh_device_count(void);
const char *lh_last_error(void);

/* ---- accelerator lifetime: accel_build_func / accel_free_func ----------
 * reference: src/render/accel.h:24-28; ri_bvh_build src/render/bvh.c:276-379;
 * ri_bvh_free bvh.c:381-387.  The reference's build() walks scene->geom_list;
 * across the C ABI the same walk is three calls: create, add_mesh per
 * ri_geom_t in list order (this fixes primitive ids exactly as
 * create_triangle_list does, bvh.c:1736-1826), commit. */
int  lh_accel_create(lh_accel_t **out, int device);
/* positions: first double of vertex 0; stride_bytes between vertices
 * (32 for lucille's ri_vector_t = double[4], 24 for packed xyz).  The data is
 * copied (the reference copies too, bvh.c:320-321). */
int  lh_accel_add_mesh(lh_accel_t *accel, uint32_t npositions, const double *positions,
                       size_t stride_bytes, uint32_t nindices, const uint32_t *indices);
/* builds the BVH on the host (build_threads <= 0: all cores) and uploads the
 * SoA scene to the device.  An empty scene commits to an always-miss accel
 * (bvh.c:311-315,446-449).  Fails (-1, lh_last_error) on an out-of-range vertex index, on a NaN /
 * infinite / > 1e30 vertex coordinate (the fp32 filter cannot bound it) and on >= 2^29 triangles.
 * Every entry point taking an accelerator holds its lock: calls from several threads are safe and
 * serialised (lucille's render threads call accel->intersect concurrently, render.c:1043-1105). */
int  lh_accel_commit(lh_accel_t *accel, int build_threads);
/* build_threads == LH_BUILD_ON_DEVICE (or LH_BUILD=device in the environment): both trees are built on the GPU -- the
 * traversal tree (LBVH + SAH -> the same 4-wide nodes) and lucille's own tree (ri_bvh_build, bvh.c:276-379, restated level by
 * level, bit for bit: exact-t tie winners, fragile hits and beams depend on it): a fraction of a second instead of seconds;
 * lucille re-builds its accelerator in every ri_scene_setup (scene.c:84-98).  LH_REF_BUILD=host leaves lucille's own tree to
 * a background host thread as in round 2: queries are exact by default (the first one waits for it, lh_accel_wait_exact does so
 * explicitly); lh_accel_set_param(accel, "fast_start", 1) (or LH_FAST_START=1) lets them run before it is attached, exact-t
 * ties resolving to the larger primitive id until then.  Hit records are otherwise independent of the trees. */
#define LH_BUILD_ON_DEVICE (-2)
/* build_threads == LH_BUILD_ON_HOST (or LH_BUILD=host), or a thread count > 0: the host builders (binned SAH for traversal,
 * lucille's own tree beside it on the same thread pool): the better traversal tree (frames ~2 % faster), seconds for tens of
 * millions of triangles.  build_threads == 0 lets the library choose: the device builders from LH_AUTO_DEVICE_TRIANGLES
 * triangles on (what `lsh_hip --build auto` always did: lucille sets its scene up in front of every frame), the host builders
 * below; an automatic device build that cannot be done (memory, a degenerate tree) is redone on the host. */
#define LH_BUILD_ON_HOST (-3)
#define LH_AUTO_DEVICE_TRIANGLES 1000000ull
/* ---- meshes that live on the device: lh_accel_add_mesh for vertices a kernel produced (a deformation, a simulation step, a
 * tessellation, any torch tensor), with no copy to the host, no host flatten and no upload in front of the build.
 * d_positions / d_indices are device memory of the accelerator's device (hipMalloc; a CUDA torch tensor): npositions vertices of
 * 3 doubles (LH_POS_F64; stride_bytes >= 24 and a multiple of 8: 32 for ri_vector_t) or 3 floats (LH_POS_F32; stride_bytes >= 12
 * and a multiple of 4), and nindices uint32_t triangle corners.  An fp32 vertex IS the fp64 vertex (double)x, (double)y, (double)z:
 * trees, hit records and frames are bit-equal to those of a host mesh holding the widened values.
 *   - Primitive ids as for lh_accel_add_mesh: meshes in add order, mesh g's triangle i = first_prim[g] + i; the trailing nindices % 3
 *     indices are ignored; a zero-area triangle keeps its id.  lh_accel_prim_lookup answers from the triangle counts alone.
 *   - The arrays are read by copies enqueued on `stream` (hipStream_t as void*; NULL = the default stream) before the call returns:
 *     the library keeps its own device copy, so the caller may overwrite or free them in stream order afterwards.  lh_accel_commit
 *     waits for those copies through an event per caller stream (no device-wide synchronise).
 *   - lh_accel_commit accepts build_threads == 0 or LH_BUILD_ON_DEVICE and always takes the device path: ONE kernel flattens every
 *     mesh straight into the fp64 triangle records, then both device builders run as for LH_BUILD_ON_DEVICE.  No host copy of the
 *     triangles is made and there is no background host thread; LH_BUILD=host and LH_REF_BUILD=host in the environment do not apply
 *     to these accelerators.  The one exception: a scene whose trees the device builders cannot make (an LBVH deeper than the walks'
 *     stacks: exponentially spaced geometry) has its flattened triangles copied to the host once and both trees built there -- what
 *     commits from host arrays commits from device arrays.
 *   - Found on the device, reported by lh_accel_commit (-1; the accelerator is then in the failed-commit state, create a new one):
 *     an index >= npositions ("index I out of range (npositions N)": detected before it addresses anything) and a NaN / infinite /
 *     > 1e30 coordinate of a REFERENCED vertex (lh_accel_commit's message; an unreferenced vertex may hold anything).
 *   - An empty scene (no meshes, or only empty ones) commits to the always-miss accelerator.
 *   - Per-vertex normals, colours, tangents, binormals and texture coordinates come from device arrays too:
 *     lh_accel_set_normals_device and lh_accel_set_attribute_device (below, beside lh_accel_set_attribute).  The commit gathers them
 *     into the per-primitive arrays of a host scene with ONE more kernel behind the flatten; a scene that falls back to the host
 *     builders keeps them (the gathered arrays are copied out with the triangles).
 * Refused, -1 with lh_last_error holding the quoted words, nothing enqueued, nothing changed: "unknown position format"; "bad
 * stride"; "positions not aligned" (to 8 / 4 bytes); "indices not 4-byte aligned"; "NULL array" (with a non-zero count); "not a
 * device pointer" (what hipPointerGetAttributes does not report as device memory of the accelerator's device -- host memory, another
 * device's: asked, never dereferenced; "extends past its allocation" where the runtime knows the range); "2^29 triangles" (the
 * scene's total); "already committed"; "cannot be mixed" (lh_accel_add_mesh and lh_accel_add_mesh_device on one accelerator, in
 * either order).  On an accelerator with "device meshes" -- each message says so -- also: lh_accel_set_normals and
 * lh_accel_set_attribute (the host-pointer setters: device meshes take lh_accel_set_normals_device and
 * lh_accel_set_attribute_device), lh_accel_commit with LH_BUILD_ON_HOST or a thread count,
 * lh_accel_export, lh_accel_commit_replica / lh_multi_commit from it, lh_dist_broadcast_scene from it. */
#define LH_POS_F64 0      /* 3 doubles per vertex at stride_bytes (>= 24, multiple of 8; 32 for ri_vector_t)   */
#define LH_POS_F32 1      /* 3 floats per vertex at stride_bytes (>= 12, multiple of 4); vertex = (double)float */
int  lh_accel_add_mesh_device(lh_accel_t *accel, uint32_t npositions, const void *d_positions, int position_format,
                              size_t stride_bytes, uint32_t nindices, const void *d_indices /* uint32_t */, void *stream);
/* ---- updatable device meshes: new vertices, then a re-commit in place.  For a caller whose vertices move every step and who
 * would otherwise destroy the accelerator and set every mesh, normal, attribute, material, texture, environment, sky and knob
 * again -- and lose the streams, the fix-up queues, the pinned ring and every scratch buffer the old one had grown.
 *   lh_accel_set_param(accel, "updatable", 1), before the commit, on an accelerator of device meshes.  The commit then KEEPS the
 *     library's device copies of the positions, the index lists, the normals and the attributes -- the blocks lh_accel_add_mesh_device
 *     and the set_*_device calls made, in the caller's format and stride -- and the per-stream events.  Memory: an updatable
 *     accelerator holds the bytes the caller handed over for as long as it lives, beside the scene built from them.  Refused after
 *     the commit ("before the commit") and on an accelerator that holds host meshes; lh_accel_add_mesh on an updatable accelerator
 *     is refused the same way ("cannot be mixed").  An accelerator that never sets it behaves as it always did, in every call.
 *   lh_accel_update_mesh_device, after the commit: new positions for mesh `mesh` (add order).  npositions must equal the mesh's;
 *     the format and the stride may differ from those of the add.  The array is read by a copy enqueued on `stream` into the
 *     library's block before the call returns, the stream's event recorded behind it: the caller may overwrite or free the array in
 *     stream order afterwards.  An update only STAGES: no scene array and no tree is touched, and until lh_accel_recommit returns
 *     every query answers from the old geometry.  A second update of a mesh replaces the first -- in stream order: two updates
 *     of one mesh on different streams are not ordered by the library, the caller orders the streams; a mesh without triangles
 *     accepts the call and does nothing.  Refused, -1 with lh_last_error, nothing enqueued, nothing changed: "accel is NULL"; "not
 *     committed"; "not updatable" (the parameter was not set, or the commit fell back to the host builders -- the message says
 *     which); "mesh M out of range"; "N positions given, the mesh has M"; and lh_accel_add_mesh_device's "unknown position format",
 *     "bad stride", "positions not aligned", "NULL array", "not a device pointer", "extends past its allocation".
 *   lh_accel_set_normals_device / lh_accel_set_attribute_device are accepted after the commit on such an accelerator, with the same
 *     arguments and refusals, replacing and removing as before it; what they set is staged like a position update.
 *   lh_accel_recommit: synchronous, like the commit.  Nothing staged: returns 0, no launch, no allocation.  Positions staged: waits
 *     for the staged copies through their events, flattens every mesh into a NEW array of records and compares it with the resident
 *     one; equal word for word, the trees stand; otherwise the traversal tree, lucille's own tree and the danger list are built
 *     from the new records BESIDE the resident scene (the 8-wide nodes too when the scene had them or "wide8" is 1).  Positions or
 *     attributes staged: the per-primitive normals and attributes are gathered again, into new arrays.  Then, and only when all of
 *     that has succeeded, the call WAITS FOR THE DEVICE (hipDeviceSynchronize: a launch the caller enqueued earlier, on any stream,
 *     may still read the old arrays), swaps the new arrays in, frees the old ones and sizes the grid again unless the caller set
 *     it.  Memory: during a re-commit the scene's arrays exist twice.  After a successful return the accelerator is, for every entry
 *     point, the one a caller would get from lh_accel_create, the same index lists with the new positions, the same settings and
 *     lh_accel_commit; everything set on it survives.  *info (may be NULL) says what was redone.
 *     Failure, -1 with lh_last_error: a NaN / infinite / > 1e30 coordinate of a referenced vertex (the commit's message), or a scene
 *     whose trees the device builders cannot make ("the device builders cannot build the updated scene (...): it needs a new
 *     accelerator" -- there is no host fallback here: it would release arrays an accelerator in use still holds).  Everything built
 *     aside is freed, the accelerator stays committed and answers from the old geometry bit for bit, what was staged stays staged:
 *     the caller may stage a repaired mesh and call again.
 *   lh_accel_set_param(accel, "build_depth_cap", d) is for TESTS of the two paths above that no ordinary scene reaches any more: the levels
 *     of a device-built traversal tree beyond which the device builders are given up (a commit falls back to the host builders, a
 *     re-commit fails with "needs a new accelerator").  Default 86, what the walks' stacks take (3 d + 5 <= 264 rows); 1 .. 86; it
 *     applies to every later commit AND re-commit of the accelerator.  A renderer has no reason to set it. */
typedef struct lh_recommit_info {
    int    flattened;        /* the meshes were flattened into new records (positions were staged) */
    int    rebuilt_trees;    /* the records differed from the resident ones: both trees and the danger list were rebuilt */
    int    regathered;       /* the per-primitive normals and attributes were gathered again */
    double seconds;          /* the whole call */
} lh_recommit_info_t;
int  lh_accel_update_mesh_device(lh_accel_t *accel, uint32_t mesh, uint32_t npositions, const void *d_positions, int position_format,
                                 size_t stride_bytes, void *stream);
int  lh_accel_recommit(lh_accel_t *accel, lh_recommit_info_t *info /* may be NULL */);
int  lh_accel_wait_exact(lh_accel_t *accel);
/* lucille's own tree as the kernels read it, for inspection (tests compare the device-built tree with the host-built one):
 * *nnodes nodes of 128 bytes (lh_refbvh.h: two child boxes of 6 doubles, child[2], axis, is_leaf, first, count, parent, depth;
 * root = 0) and the ntriangles primitive ids in leaf order.  Either pointer may be NULL.  Fails if the tree is not attached. */
int  lh_accel_ref_tree(lh_accel_t *accel, uint32_t *nnodes, void *nodes_out, uint32_t *leaf_prims_out);
/* The traversal trees as the walks read them, for inspection too (tests check every node, box and stack figure of a tree the device built: hit
 * records show a box one grid code too tight, or a stack count one row short, on next to no ray).  A read-only image: the DEVICE arrays, copied back,
 * never a host copy; nothing is built and no kernel runs.  info: the figures the launches use -- ntris records of 48 bytes (leaf order; the first
 * nlive are in the leaves) and of 72 bytes (primitive-id order), nq4 4-wide nodes of 64 bytes (12 words lo | hi << 16 on the 16-bit grid, 4 child
 * references), their levels and the stack rows the builder counted (0: 3 x q4_depth + 5 rows), nq8 8-wide nodes of 128 bytes and their levels
 * (both 0 while the 8-wide nodes are not resident), whether the device built the trees, the scene box, the grid and the radius the rays' set-up is
 * given.  Every pointer may be NULL; an array is written only up to the counts info reports (call once for the counts, once for the arrays). */
typedef struct lh_tree_image {
    uint32_t ntris, nlive, nq4, q4_depth, q4_stack, nq8, q8_depth, device_built;
    float    bmin[3], bmax[3], grid_lo[3], grid_step[3], scene_r;
} lh_tree_image_t;
int  lh_accel_tree_image(lh_accel_t *accel, lh_tree_image_t *info, void *q4nodes, void *q8nodes, void *tri32, void *tri64);
/* The danger list as the walks read it, for inspection too (tests compare a re-committed accelerator's with a fresh one's: the hit records
 * cannot show a stale list, it only routes other rays to the reference's own walk).  *ndevice: 0 = every ray beyond the cap is routed, else
 * the number of listed leaves behind the ONE box device_box[3] (lo | hi << 16 per axis on the scene's 16-bit grid; zeros with 0);
 * *nhost / host_boxes (room for 16 x 6 doubles: bmin xyz, bmax xyz): the list the one-ray host walk reads.  Any pointer may be NULL. */
int  lh_accel_danger_list(const lh_accel_t *accel, uint32_t *ndevice, uint32_t device_box[3], uint32_t *nhost, double *host_boxes);
void lh_accel_destroy(lh_accel_t *accel);
int  lh_accel_info(const lh_accel_t *accel, lh_accel_info_t *out);

/* primitive id -> (mesh ordinal in add order, index = 3*i into that mesh's
 * index list): what state->geom / state->index carry in the reference
 * (bvh.c:855-860), so the host can run ri_intersection_state_build. */
int  lh_accel_prim_lookup(const lh_accel_t *accel, uint32_t prim, uint32_t *mesh,
                          uint32_t *index);

/* ---- queries: accel_intersect_func (src/render/accel.h:30-34) ----------
 * Rays are fp64 xyz triples exactly as ri_ray_t.org/.dir (src/render/ray.h:
 * 24-25); dir need not be normalised, t is in units of |dir|.
 * Closest mode writes prim (LH_MISS on miss), t (1e38 on miss), u, v as the
 * reference does (bvh.c:850-861,1187).  Any mode writes occluded[i] in {0,1}.
 * Unused outputs may be NULL. */

/* one synchronous ray: the reference's calling convention, kept correct (a
 * batch of one through the same kernel). Returns 1 hit / 0 miss / -1 error. */
int  lh_accel_intersect1(lh_accel_t *accel, const double org[3], const double dir[3],
                         uint32_t *prim, double *t, double *u, double *v);
/* Per-ray traversal diagnostics: what ri_bvh_intersect reports through its `user` argument (a ri_bvh_diag_t, bvh.h:103-110,
 * bvh.c:451-456) for THIS build's tree.  diag: n x 4 u32 -- 4-wide node visits, leaf visits, triangle records through the fp32
 * filter, fp64 tests -- of the sequential walk (nearest child first, as tests/cpu_model walks); records as every other path's.
 * With lh_accel_trace_statistics on, the launch's totals are the sums of these rows. */
int  lh_accel_intersect_diag_host(lh_accel_t *accel, size_t n, const double *org_xyz, const double *dir_xyz,
                                  uint32_t *prim_id, double *t, double *u, double *v, uint32_t *diag);
/* ... for rays resident on the device, closest- or any-hit (mode: LH_MODE_*); d_diag: n x 4 u32 on the device, hit records dropped */
int  lh_accel_intersect_diag_device(lh_accel_t *accel, size_t n, const void *d_org_xyz, const void *d_dir_xyz, int mode,
                                    void *d_diag, void *stream);
/* Concurrent lh_accel_intersect1 callers (lucille's render threads) are coalesced into one launch per batch of callers
 * (lh_query.hip "flat combining"); set_param("combine", 0) / LH_COMBINE=0 restores one launch per call.
 * out[0] = launches, out[1] = rays they carried since the last clear. */
int  lh_accel_combine_statistics(lh_accel_t *accel, uint64_t out[2], int clear);

/* host-resident batch (the batch form of accel_intersect_func, accel.h:30-34: rays and records in the caller's arrays).  Below 2 M rays:
 * copy up, one launch, copy down on the accel's own stream.  From 2 M rays: chunks through a ring of pinned staging blocks -- the rays of
 * chunk k + 1 cross the link while chunk k is traced and chunk k - 1's records go back (lh_query.hip; 860 Mrays/s closest hit over PCIe,
 * profiles/r06_hostpath.txt).  Outputs the caller does not need may be NULL.  Synchronous: the arrays are complete on return */
int  lh_accel_intersect_host(lh_accel_t *accel, size_t n, const double *org_xyz,
                             const double *dir_xyz, uint32_t *prim, double *t, double *u,
                             double *v, uint8_t *occluded, int mode);

/* device-resident batch on a caller stream (hipStream_t as void*; NULL =
 * default stream).  Asynchronous: returns after enqueue. */
int  lh_accel_intersect_device(lh_accel_t *accel, size_t n, const void *d_org_xyz,
                               const void *d_dir_xyz, void *d_prim, void *d_t, void *d_u,
                               void *d_v, void *d_occluded, int mode, int variant,
                               void *stream);

/* ---- ray and record formats of the batch entry points (lh_accel_intersect_host_ex / _device_ex) ----
 * LH_RAYS_F64: org_xyz / dir_xyz hold 3 doubles per ray (the format of lh_accel_intersect_host / _device).
 * LH_RAYS_F32: the same layout with 3 floats per ray.  A float ray is traced as the fp64 ray ((double)org[k], (double)dir[k]):
 *   its records are bit-equal to what the fp64 entry points return for those widened rays, and the fp64 path's rules (the
 *   reference's |dir.y| <= 1e-14 exclusions among them) apply to the widened ray.
 * LH_REC_F64: closest-hit records as SoA arrays prim (u32), t, u, v (f64) -- the format of the fp64 entry points.
 * LH_REC16: closest-hit records as an array of lh_rec16_t (16-byte aligned): prim unchanged, t, u, v each (float) of the fp64
 *   record -- exactly the rounding lh_dist_pack_records16 applies to the wire.  A miss is prim = LH_MISS, t = (float)1e38, and
 *   u, v whatever the fp64 miss record rounds to.
 * Any-hit mode writes the occluded byte per ray with either ray format; LH_REC16 does not apply to it. */
#define LH_RAYS_F64 0
#define LH_RAYS_F32 1
#define LH_REC_F64  0
#define LH_REC16    1
typedef struct lh_rec16 { uint32_t prim; float t, u, v; } lh_rec16_t;
#ifdef __cplusplus
static_assert(sizeof(lh_rec16_t) == 16, "lh_rec16_t is 16 bytes");
#else
_Static_assert(sizeof(lh_rec16_t) == 16, "lh_rec16_t is 16 bytes");
#endif
/* lh_accel_intersect_host / _device with a ray format (LH_RAYS_*) and a record format (LH_REC_*).  prim_or_rec16: the prim
 * array (LH_REC_F64) or the lh_rec16_t array (LH_REC16); t, u, v: the f64 arrays of LH_REC_F64, NULL with LH_REC16.
 * The host form is synchronous and moves each format's own bytes over the link (24 bytes per fp32 ray up, 16 per LH_REC16
 * record down, 1 per any-hit ray; pipelined like lh_accel_intersect_host from 2 M rays on); the device form enqueues the
 * default variant on `stream` and returns.  -1 (lh_last_error), nothing written: an unknown format or mode, a misaligned
 * LH_REC16 pointer, LH_REC16 in any-hit mode, non-NULL t / u / v with LH_REC16.  n == 0 returns 0 (the record array is not
 * looked at, it may be NULL; an unknown format or mode is still refused).  With
 * lh_accel_trace_statistics on, they count as lh_accel_intersect_host / _device do. */
int  lh_accel_intersect_host_ex(lh_accel_t *accel, size_t n, const void *org_xyz, const void *dir_xyz, int ray_format,
                                int record_format, void *prim_or_rec16, double *t, double *u, double *v,
                                uint8_t *occluded, int mode);
int  lh_accel_intersect_device_ex(lh_accel_t *accel, size_t n, const void *d_org_xyz, const void *d_dir_xyz, int ray_format,
                                  int record_format, void *d_prim_or_rec16, void *d_t, void *d_u, void *d_v,
                                  void *d_occluded, int mode, void *stream);

/* ---- indexed ray batches: trace SOME of the rays of a device-resident batch, chosen on the device ----
 * What a wavefront transport needs between two waves of rays (a shadow pass for the rays that hit, the next bounce for the paths
 * that survived, a re-trace of a changed subset) without reading records back, gathering rays and scattering records:
 * d_org_xyz / d_dir_xyz and the record arrays describe n_rays rays exactly as for lh_accel_intersect_device_ex (formats, alignment,
 * the any-hit byte); d_index holds n_index uint32_t ray ids (device; NULL: the identity list 0 .. n_index-1); d_count (device; NULL: all
 * n_index entries) is ONE uint32_t, the number of list entries to trace -- min(*d_count, n_index) are traced, and *d_count is read by
 * the launch on `stream`, not by the host: it may be written by work enqueued on `stream` before this call (lh_accel_compact_device).
 *   - For every traced entry k the ray id = index[k] is traced and its record written to slot id of the record arrays (not slot k):
 *     bit-equal to what lh_accel_intersect_device_ex writes for that ray.
 *   - The records of rays that are not listed are not touched, byte for byte -- whatever they hold.
 *   - An id >= n_rays is skipped: nothing is read or written for it.  An id may be listed more than once: its record is the ray's answer.
 *   - Asynchronous on `stream`; the default variant (the tuned walk), whatever "variant" was set to.
 *   - Every refusal of lh_accel_intersect_device_ex applies and leaves nothing written; so do n_index > 2^30, n_rays >= 2^32 and a list or
 *     count pointer that is not 4-byte aligned.  n_index == 0 or n_rays == 0 returns 0 and looks at no array.
 *   - With lh_accel_trace_statistics on, the call counts (node visits, tests, and `rays` advances by the number of rays traced: listed
 *     entries within the count whose id is < n_rays) and is then synchronous: the count is known on the device alone. */
int  lh_accel_intersect_device_indexed(lh_accel_t *accel, size_t n_rays, const void *d_org_xyz, const void *d_dir_xyz, int ray_format,
                                       int record_format, void *d_prim_or_rec16, void *d_t, void *d_u, void *d_v, void *d_occluded,
                                       int mode, const void *d_index, size_t n_index, const void *d_count, void *stream);

/* the records of a batch -> a list for lh_accel_intersect_device_indexed, on the device.  n records: closest-hit records in
 * d_prim_or_rec16 (record_format LH_REC_F64: the prim array; LH_REC16: the lh_rec16_t array) for LH_SELECT_HIT (prim != LH_MISS) /
 * LH_SELECT_MISS, or any-hit bytes in d_occluded for LH_SELECT_OCCLUDED (byte != 0) / LH_SELECT_UNOCCLUDED; the array the selection
 * does not read may be NULL (record_format is then ignored).  The candidates are the entries of the input list, given as above
 * (d_index_in / n_index_in / d_count_in; ids >= n are skipped); all three NULL / 0: all n records.  d_index_out (room for as many
 * entries as there are candidates: n_index_in, or n) receives the selected ids in the order they have in the input list --
 * ascending for the identity list: the same list for the same records, run after run; d_count_out receives their number (one
 * uint32_t).  Asynchronous on `stream`, no host synchronisation, no accelerator: it runs on the calling thread's current device.
 * The output list and count must not alias or overlap the input list and count (the input is read while the output is written): to
 * compact a list again, alternate between two buffers.
 * -1 (lh_last_error), nothing written: an unknown select or record format, a missing or misaligned array, more than 2^30 candidates,
 * an output that aliases an input. */
#define LH_SELECT_HIT        0
#define LH_SELECT_MISS       1
#define LH_SELECT_OCCLUDED   2
#define LH_SELECT_UNOCCLUDED 3
int  lh_accel_compact_device(size_t n, int record_format, const void *d_prim_or_rec16, const void *d_occluded, int select,
                             const void *d_index_in, size_t n_index_in, const void *d_count_in,
                             void *d_index_out, void *d_count_out, void *stream);

/* ---- per-ray maximum distance (tmax): "only up to here", for closest- and any-hit batches ----
 * Shadow rays toward a point on a light, distance-limited occlusion, visibility between two path vertices, proximity queries.  The
 * bound prunes the walk; it is not a filter behind an unbounded launch.
 * The contract is a filter on what the library already guarantees.  For a ray and a bound tmax (the unit of t: multiples of |dir|) let
 * R = (prim, t, u, v) be the record the unbounded entry points (lh_accel_intersect_device_ex / _indexed / _host_ex) return -- the
 * reference's, bit for bit.
 *   - Closest hit: the answer is R if R.prim != LH_MISS and R.t < tmax, the comparison made in fp64; otherwise the miss record of the
 *     unbounded call (LH_MISS, 1e38, 0.0, 0.0).  LH_REC16: the same record through the same rounding.
 *   - Any hit: occluded = (R.prim != LH_MISS && R.t < tmax) ? 1 : 0.
 *   - The comparison is strict, and IEEE's: a NaN, zero or negative tmax gives a miss; +inf, and any value above every t, gives
 *     exactly the unbounded answer.
 *   - LH_RAYS_F32: the bounds are floats and a bound IS (double)tmax; LH_RAYS_F64: they are doubles.
 *   (It is NOT "the reference's walk started with t_best = tmax": the reference has no such parameter -- ri_ray_t.max_t is ignored --
 *   and that walk culls boxes against t_best.)
 * The device form.  Rays, records, formats and alignment as for lh_accel_intersect_device_ex.  d_tmax holds n_rays bounds of the ray
 * format's type, one per ray id (an indexed call addresses it by id, not by list position).  d_index == NULL && n_index == 0 &&
 * d_count == NULL: every ray is traced and every record slot written.  Otherwise the list has exactly the semantics of
 * lh_accel_intersect_device_indexed (NULL d_index with n_index > 0: the identity list; min(*d_count, n_index) read on the stream; ids >=
 * n_rays skipped; duplicates allowed; unlisted slots untouched, byte for byte).  d_tmax == NULL forwards to lh_accel_intersect_device_ex
 * (no list) or lh_accel_intersect_device_indexed: the unbounded call by construction.  Asynchronous on `stream`; the default variant; over
 * the 4-wide or the 8-wide nodes as ray dumps are.
 *   - -1 (lh_last_error), nothing written or enqueued: everything those two refuse, with their message under this entry point's name; a
 *     d_tmax that is not aligned to its element size ("tmax not aligned"); n_rays > 2^30 ("2^30 rays").  n_rays == 0 returns 0.  On the
 *     empty scene every traced ray gets the miss record / 0.
 *   - With lh_accel_trace_statistics on, the call counts as lh_accel_intersect_device_indexed does (and is then synchronous), and
 *     counters[4] (hits) advances by the traced rays whose answer is a hit after the bound.
 * The host form is synchronous and correct for every n.  It takes the plain path -- pageable copies through the staging block, one
 * bounded launch -- in chunks of 2^21 rays, whatever n is: the bounds do not travel through the pinned ring lh_accel_intersect_host_ex
 * uses from 2 M rays on.  tmax == NULL forwards to lh_accel_intersect_host_ex.  The same refusals (no 2^30 limit). */
int  lh_accel_intersect_device_tmax(lh_accel_t *accel, size_t n_rays, const void *d_org_xyz, const void *d_dir_xyz,
                                    const void *d_tmax, int ray_format, int record_format,
                                    void *d_prim_or_rec16, void *d_t, void *d_u, void *d_v, void *d_occluded, int mode,
                                    const void *d_index, size_t n_index, const void *d_count, void *stream);
int  lh_accel_intersect_host_tmax(lh_accel_t *accel, size_t n, const void *org_xyz, const void *dir_xyz, const void *tmax,
                                  int ray_format, int record_format, void *prim_or_rec16, double *t, double *u, double *v,
                                  uint8_t *occluded, int mode);

/* same launch with traversal statistics: counters[4] (host) receives
 * {inner-node visits, triangle tests, fp64 resolves, rays}; synchronous. */
int  lh_accel_intersect_device_counted(lh_accel_t *accel, size_t n, const void *d_org_xyz,
                                       const void *d_dir_xyz, void *d_prim, void *d_t,
                                       void *d_u, void *d_v, void *d_occluded, int mode,
                                       int variant, uint64_t counters[4]);
/* rays of the last counted launch (lh_accel_intersect_device_counted, or a host batch -- lh_accel_intersect_host / _host_ex --
 * with lh_accel_trace_statistics on) that were finished outside the main kernel: the reference-order walk (exact-t ties,
 * fragile hits), the cooperative walk, and the private-stack walk for rays whose LDS stack column would have overflowed */
uint64_t lh_accel_last_retraced(const lh_accel_t *accel);
/* bytes of the node record the ray-dump entry points (lh_accel_intersect_host / _device) walk on this scene: 64 (4-wide
 * 16-bit-grid node), or 128 (8-wide, one cache line) when the scene's hot set does not fit the 256 MiB Infinity Cache --
 * there every record fetched costs a 128-byte line of HBM traffic.  lh_accel_set_param("wide8", -1 auto / 0 / 1). */
int lh_accel_dump_node_bytes(const lh_accel_t *accel);
/* Large plain ray dumps (lh_accel_intersect_device / _device_counted: fp64 rays on 16-byte boundaries, fp64 records or any-hit bytes, the default
 * walk) are traced from a copy in bin order -- the Morton code of the origin's cell on the scene's bounds -- and their
 * records copied back to the caller's slots: incoherent rays then meet each XCD's L2 one region of the scene at a time.  Records do not change.
 * The copy lives in a workspace per stream (82 bytes a ray: 8.2 GB for 100 M rays; sized by the largest dump the stream has seen, never shrunk, freed with
 * the accelerator; up to four streams keep one each; growing it waits for the device; "dump_order_max_mb" caps it); a dump whose workspace cannot be had
 * is traced as given.  lh_accel_set_param: "dump_order" 1 (default) / 0 -- a caller whose dumps are coherent already (camera rays in pixel order, rays
 * sorted upstream) switches it off: the passes cost what an incoherent dump wins; "dump_order_min": rays of the smallest dump that is ordered;
 * "dump_order_bits": the key, 64 bins either way -- 2 (default): the cell at two bits per axis, 1: one bit per axis under the direction octant; "dump_order_max_mb": 0 (no cap) or the largest workspace in MiB.  LH_DUMP_ORDER=0: off.
 * fp32 rays, 16-byte records, indexed and bounded dumps, host batches' chunks below "dump_order_min" and the tile pipelines are traced as given.
 * out[0]: dumps traced in bin order so far (a dump of more than 2^30 rays counts once per part), out[1]: their rays */
int lh_accel_order_statistics(lh_accel_t *accel, uint64_t out[2], int clear);

/* ---- traversal statistics: ri_bvh_clear_stat_traversal / ri_bvh_report_stat_traversal ----
 * reference: src/render/bvh.c:669-706 (globals filled under -DRI_BVH_TRACE_STATISTICS,
 * :681-706, 829-831, 1149-1151).  While enabled, every lh_accel_intersect1/_host call and every
 * batch of the tile pipelines (lh_render_ao_tile / _bands / _frame_host, lh_render_pt_tile*) runs
 * the counting kernel variant and accumulates: counters[0] node visits (one per 4-wide node
 * record fetched), [1] triangles put through the fp32 filter, [2] triangles re-tested in
 * fp64, [3] rays, [4] rays that hit (AO pipeline: camera-ray hits + occluded AO rays; not counted by
 * the path tracer).  Counts describe THIS build's tree, not lucille's. */
int  lh_accel_trace_statistics(lh_accel_t *accel, int enable);
int  lh_accel_statistics(lh_accel_t *accel, uint64_t counters[5], int clear);
/* lane slots of the tile pipelines' counted launches: 64 per wave iteration that made a node step / ran a triangle pass / regrouped.
 * counters[0] / slots[0] = lane use of the node steps, counters[1] / slots[1] = of the triangle passes */
int  lh_accel_slot_statistics(lh_accel_t *accel, uint64_t slots[3], int clear);

/* number of persistent workgroups the persistent variants launch */
int  lh_accel_set_grid(lh_accel_t *accel, int blocks);
/* knobs by name: "grid", "min_active", "tri_batch", "ray_chunk" (sweeps), "variant" (0: the textbook reference walk, 4: the
 * default), "ao_fused", "wide8" (-1 auto / 0 / 1), "fast_start", "combine", "top_nodes", "ao_group";
 * "stack_cap": LDS stack rows of the default walk -- 0 (default): a launch of 65 536 rays or more walks at most 34 CHECKED rows
 * (four workgroups per CU; a ray that would overrun them is finished by the cooperative walk), smaller launches up to 64
 * unchecked; 8 .. 64: that many at most (64 = rounds 1-3's unchecked rows; small values: tests of the overflow path);
 * "min_active" / "tri_batch": working lanes below which a wave regroups / lanes holding a parked leaf from which it runs a triangle
 * pass -- 24 / 12 for the tile pipelines; left alone, ray dumps use 24 / 8 over the 4-wide nodes and 40 / 20 over the 8-wide ones,
 * once either is set here (or by LH_MIN_ACTIVE / LH_TRI_BATCH) every launch uses the caller's pair;
 * "ray_budget" (wave iterations after which a ray leaves the persistent walk for the cooperative one; sets "dump_budget" and
 * "ao_budget" with it), "dump_budget" (ray dumps: 2048), "ao_budget" (the fused AO stage: 384; 0: "ray_budget") */
int  lh_accel_set_param(lh_accel_t *accel, const char *name, int value);

/* ---- tile rendering: the callers on either side of the query, on the device ----
 * reference: subsample / render_bucket / bucket_write (src/render/render.c:715-823,
 * 1107-1166, 919-983), ri_camera_get_pos_and_dir (src/ri/camera.c:248-318),
 * ri_intersection_state_build (src/render/intersection_state.c:99-248),
 * ri_transport_ambientocclusion + calculate_occlusion
 * (src/transport/ambientocclusion.c:42-151,332-415). */

typedef struct lh_camera {
    int    width, height;       /* camera->horizontal/vertical_resolution             */
    int    rh;                  /* Orientation "rh" (camera->is_rh)                   */
    int    ortho;               /* 1: Projection "orthographic" (the reference's default when no
                                 * "fov" is given, camera.c:100,428); 0: perspective        */
    double flength;             /* 1/tan(fov/2) (camera.c:219)                         */
    double cam2world[16];       /* camera->camera_to_world, row-major, row vectors     */
} lh_camera_t;

typedef struct lh_tile_stats {
    uint64_t primary_rays;      /* w*h*pixel_samples^2                                 */
    uint64_t primary_hits;
    uint64_t ao_rays;           /* primary_hits * floor(sqrt(gather_nsamples))^2       */
    uint64_t ao_occluded;
} lh_tile_stats_t;

/* optional per-vertex normals of mesh `mesh` (add order), before commit:
 * geom->normals / geom->two_side as ri_intersection_state_build reads them */
int  lh_accel_set_normals(lh_accel_t *accel, uint32_t mesh, const double *normals,
                          size_t stride_bytes, int two_side);

/* camera rays of the tile [x0,x0+w) x [y0,y0+h), pixel_samples^2 per pixel, written to
 * device arrays of w*h*pixel_samples^2 xyz triples (sample id = ((ly*w+lx)*ps+sy)*ps+sx) */
int  lh_render_primary_rays(lh_accel_t *accel, const lh_camera_t *cam, int x0, int y0, int w, int h,
                            int pixel_samples, void *d_org_xyz, void *d_dir_xyz, void *stream);

/* one AO tile entirely on the device: camera rays -> closest hit -> hit epilogue ->
 * gather_nsamples AO rays per hit -> any-hit -> radiance, times the texture of the hit's mesh
 * where it has one (lh_accel_set_texture; else the three channels are equal).  d_rgb: float[h][w][3] in image
 * orientation (row 0 = the tile's TOP row of the output image, as bucket_write flips y).
 * d_uniforms: NULL for the built-in counter-based RNG (seed), or 2 doubles per AO ray in
 * (hit slot, j, i) order -- how a caller replays the reference's MT19937 stream.
 * Synchronous on `stream` (one 8-byte read-back of the hit count). */
int  lh_render_ao_tile(lh_accel_t *accel, const lh_camera_t *cam, int x0, int y0, int w, int h,
                       int pixel_samples, int gather_nsamples, uint64_t seed,
                       const void *d_uniforms, void *d_rgb, lh_tile_stats_t *stats, void *stream);

/* nbands full-width bands of band_rows lines each (band b = frame lines band_y0[b] .. + band_rows, clipped at the frame)
 * as ONE device batch -- how a rank renders ALL of its interleaved shards of a frame (image space sharded
 * over the GPUs) with one set of kernel launches: every launch of the persistent traversal kernel ends with a drain
 * as long as its slowest ray (~1.7 ms on BASELINE config 5), paid once per batch instead of once per shard.
 * band_y0: nbands ints (HOST).  d_rgb: float[nbands][band_rows][width][3], every band in image orientation. */
int  lh_render_ao_bands(lh_accel_t *accel, const lh_camera_t *cam, int nbands, const int *band_y0, int band_rows,
                        int pixel_samples, int gather_nsamples, uint64_t seed, void *d_rgb, lh_tile_stats_t *stats,
                        void *stream);

/* the same tile for a plain-C host (the batched frame loop inside lucille, integration/ri_render_hip.c): rgb is
 * HOST memory (h rows of w RGB floats, image orientation); uniforms (HOST, may be NULL) as d_uniforms above --
 * nuniforms must cover the worst case 2 * floor(sqrt(gather_nsamples))^2 * w * h * pixel_samples^2; the tile
 * consumes the first 2 * N * stats->primary_hits of them. */
int  lh_render_ao_tile_host(lh_accel_t *accel, const lh_camera_t *cam, int x0, int y0, int w, int h,
                            int pixel_samples, int gather_nsamples, uint64_t seed, const double *uniforms,
                            size_t nuniforms, float *rgb, lh_tile_stats_t *stats);

/* ---- the AO stage for a caller's batch of hit records: ri_transport_ambientocclusion's occlusion term per hit ----
 * What lh_render_ao_tile does after its closest-hit launch, for rays that are not camera samples (the second vertex of a path,
 * texel or vertex positions of a bake, a transport's own rays): d_org_xyz / d_dir_xyz are n_rays fp64 rays as for
 * lh_accel_intersect_device, d_prim / d_t / d_u / d_v their LH_REC_F64 closest-hit records -- same generator, slot keys, replay
 * path and fused any-hit kernel as the tile pipeline.
 *   - N = floor(sqrt(gather_nsamples))^2 AO rays per hit, ntheta = nphi = floor(sqrt(gather_nsamples)) (ambientocclusion.c:378-380).
 *   - d_index / n_index / d_count: a list as for lh_accel_intersect_device_indexed (ids, the identity list when d_index is NULL, the
 *     count read on `stream`); all NULL / 0: every ray.  A traced ray is a listed entry within the count whose id is < n_rays; a traced
 *     ray with prim != LH_MISS is a hit.  Hit slots number the hits in list order (ray order for the identity list): the tile
 *     pipeline's deterministic compaction.
 *   - For a hit: P, Ng, Ns (the accelerator's per-vertex normals where the mesh has them -- lh_accel_set_normals, or
 *     lh_accel_set_normals_device for device meshes -- else the geometric normal), the ortho basis and the 1e-6 offset as the tile pipeline computes them, the self-primitive skip of a
 *     flat-shaded non-degenerate hit included.  d_key (n_rays uint64, or NULL: the key of ray i is i): its low 34 bits key the built-in
 *     generator, as the absolute sample position does in a frame.  d_uniforms (or NULL: the built-in generator): 2 doubles per AO ray
 *     in (hit slot, j, i) order, the replay path of lh_render_ao_tile; 2 * N * hits of them are consumed.
 *   - d_occluded_count[id] (uint32, may be NULL) = the occluded rays among the hit's N, under the any-hit semantics of the pipeline;
 *     d_radiance[id] (float, may be NULL) = (float)(1.0 * (N - count) / N) in double arithmetic.  A traced miss gets LH_AO_NO_HIT and
 *     0.0f.  The slots of rays that are not traced are not touched, byte for byte.  An id listed twice gets two slots (with uniforms
 *     it consumes two sets); its output is that ray's answer.
 *   - Synchronous on `stream` (the outputs are complete on return; one host read-back, for the fix-up queue's overflow flag).  Fused
 *     (no AO ray in memory) when "ao_fused" is on, no uniforms are given, the scene is not empty and list entries x N < 2^31; else the
 *     rays are materialised in HBM and traced in any-hit mode -- also the second try of a fused launch whose queue overflowed.  Both
 *     give the same bytes.
 *   - An empty scene: every traced ray is a miss, no record array is read.
 *   - -1 (lh_last_error), nothing enqueued or written: an uncommitted accelerator, a NULL ray or record array with n_rays > 0,
 *     gather_nsamples < 1, n_rays >= 2^31, n_index > 2^30, a list / count / output pointer that is not 4-byte aligned or a key /
 *     uniform pointer that is not 8-byte aligned, both outputs NULL.  n_rays == 0 returns 0 and looks at no array.
 *   - With lh_accel_trace_statistics on it counts as the tile pipelines' AO stage does: `rays` advances by the AO rays traced (hits x N),
 *     counters[4] by the occluded rays.
 *   - Its scratch is its own: lh_render_scratch keeps showing the last tile call. */
#define LH_AO_NO_HIT 0xFFFFFFFFu
int  lh_accel_ao_device(lh_accel_t *accel, size_t n_rays, const void *d_org_xyz, const void *d_dir_xyz,
                        const void *d_prim, const void *d_t, const void *d_u, const void *d_v,
                        int gather_nsamples, uint64_t seed, const void *d_key, const void *d_uniforms,
                        const void *d_index, size_t n_index, const void *d_count,
                        void *d_occluded_count, void *d_radiance, void *stream);
/* the same for HOST arrays: copies up, runs lh_accel_ao_device on the accelerator's stream, copies down (every ray is traced).
 * uniforms (may be NULL): nuniforms must cover the worst case 2 * N * n_rays.  occluded_count or radiance may be NULL, not both. */
int  lh_accel_ao_host(lh_accel_t *accel, size_t n_rays, const double *org_xyz, const double *dir_xyz, const uint32_t *prim,
                      const double *t, const double *u, const double *v, int gather_nsamples, uint64_t seed, const uint64_t *key,
                      const double *uniforms, size_t nuniforms, uint32_t *occluded_count, float *radiance);
/* only the AO rays -- what stage 4 of the tile pipeline writes -- of every ray of the batch, for a caller who traces them itself:
 * d_slot_of_ray[i] (n_rays uint32) = the hit slot of ray i, LH_AO_NO_HIT for a miss; *d_nslots (one uint32) = the number of hits;
 * ray (slot, r) at element slot * N + r of d_ao_org_xyz / d_ao_dir_xyz (fp64 xyz), the first *d_nslots * N elements written.
 * Asynchronous on `stream`, nothing is read back: capacity_rays (elements of the two ray arrays) must cover the worst case
 * n_rays * N, else the call is refused and nothing is enqueued.  Refusals as above, and a NULL or misaligned output.  n_rays == 0
 * writes *d_nslots = 0 and nothing else. */
int  lh_accel_ao_rays_device(lh_accel_t *accel, size_t n_rays, const void *d_org_xyz, const void *d_dir_xyz,
                             const void *d_prim, const void *d_t, const void *d_u, const void *d_v, int gather_nsamples, uint64_t seed,
                             const void *d_key, const void *d_uniforms, void *d_slot_of_ray, void *d_nslots,
                             void *d_ao_org_xyz, void *d_ao_dir_xyz, size_t capacity_rays, void *stream);

/* ---- the dirtmap transport: range-limited, distance-weighted occlusion (ri_transport_dirtmap, src/transport/dirtmap.c:84-292) ----
 * "AO with a range": the same stratified cosine hemisphere about Ns and the same ortho basis as the AO stage, the origin P + eps Ns,
 * and for every gather ray its CLOSEST hit, weighted by where that hit lies between a near and a far clip; beyond the far clip a hit
 * counts as no hit.  R is the record the bounded closest-hit contract of lh_accel_intersect_device_tmax gives the gather ray with
 * tmax = far_clip: a hit only if the unbounded record is a hit with t < far_clip (fp64, strict).
 *   weight c of one gather ray:  R is a miss -> 1;  R.t <= near_clip -> 0;  else a = R.t - near_clip, b = far_clip - near_clip,
 *     q = a / b, x = 1 - q, p = x clamped to [0, 1], c = 1 - p -- fp64, in this order (the reference's base colour 1, dirt colour 0 and
 *     gain 1 are not parameters: its pow(x, 1 / gain) is x).
 *   value of one hit: with N = floor(sqrt(gather_nsamples))^2 rays, sum = 0; for r = 0 .. N - 1 (r = j * ntheta + i): sum = sum + c_r;
 *     value = sum / N, in fp64.  The order is part of the contract.
 *   parameters: all finite, 0 <= near_clip < far_clip <= 1e38, eps >= 0; NULL: LH_DIRT_DEFAULTS.  Anything else, NaN included, is
 *     refused ("bad dirt parameters").  The self-primitive skip of a flat-shaded hit is applied only when eps >= 1e-6.
 * lh_accel_dirt_device: as lh_accel_ao_device, word for word -- list, count and key semantics, hit slots in list order, the uniforms
 *   replay (2 doubles per gather ray in (slot, j, i) order), untouched slots of rays that are not traced, synchronous on `stream`, the
 *   empty scene, scratch of its own (lh_render_scratch keeps showing the last AO tile), its refusals.  d_near_hits[id] (uint32, may
 *   be NULL) = the hit's gather rays whose bounded record is a hit; d_value[id] (float, may be NULL) = (float)value.  A traced miss
 *   gets LH_AO_NO_HIT and 0.0f.  Fused when "ao_fused" is on, no uniforms are given, the scene is not empty and list entries x N
 *   < 2^31: a closest-hit kernel makes the gather rays itself, walks them under the one bound far_clip and keeps one double per ray
 *   (the bounded record's t); else, and as the second try of a fused launch whose queue overflowed, the rays are materialised in HBM
 *   and traced by one bounded closest-hit launch whose bounds are all far_clip.  Both give the same bytes.  With
 *   lh_accel_trace_statistics on, `rays` advances by hits x N and counters[4] by the bounded hits.
 * lh_render_dirt_tile: ri_transport_dirtmap per camera sample -- a miss gives 0, a hit its value, times the texture of its mesh where it
 *   has one (lh_accel_set_texture below; lh_accel_dirt_device / _host return the value alone); sub-samples accumulated and written as lh_render_ao_tile does, keys are the absolute sample position (a frame does not depend on
 *   its tiling); stats->ao_rays = hits x N, stats->ao_occluded = the sum of the hits' near_hits. */
typedef struct lh_dirt_params { double near_clip, far_clip, eps; } lh_dirt_params_t;
#define LH_DIRT_DEFAULTS { 0.1, 0.5, 1.0e-5 }          /* dirtmap.c:98,110-111 */
int  lh_accel_dirt_device(lh_accel_t *accel, size_t n_rays, const void *d_org_xyz, const void *d_dir_xyz,
                          const void *d_prim, const void *d_t, const void *d_u, const void *d_v,
                          int gather_nsamples, const lh_dirt_params_t *params, uint64_t seed, const void *d_key, const void *d_uniforms,
                          const void *d_index, size_t n_index, const void *d_count,
                          void *d_near_hits, void *d_value, void *stream);
int  lh_accel_dirt_host(lh_accel_t *accel, size_t n_rays, const double *org_xyz, const double *dir_xyz, const uint32_t *prim,
                        const double *t, const double *u, const double *v, int gather_nsamples, const lh_dirt_params_t *params,
                        uint64_t seed, const uint64_t *key, const double *uniforms, size_t nuniforms, uint32_t *near_hits, float *value);
int  lh_render_dirt_tile(lh_accel_t *accel, const lh_camera_t *cam, int x0, int y0, int w, int h, int pixel_samples,
                         int gather_nsamples, const lh_dirt_params_t *params, uint64_t seed,
                         const void *d_uniforms, void *d_rgb, lh_tile_stats_t *stats, void *stream);

/* ---- the environment-lit gather: sky light through the AO stage (gather_sunsky's loop, src/transport/ambientocclusion.c:206-324, and
 *      ri_ibl_sample_cosweight, src/render/ibl.c:52-227, with ri_texture_ibl_fetch as the radiance of a miss) ----
 * AO with a colour: the same stratified cosine hemisphere about Ns and the same ortho basis as the AO stage, the origin P + eps Ns, an
 * any-hit answer per gather ray; a ray that is not occluded sees the accelerator's environment (lh_accel_set_environment below: the
 * angular map scaled by rgb, or the constant rgb; constant white if none was set) in its direction, an occluded ray sees nothing.
 *   input of gather ray r:  occ_r, its any-hit answer under the pipeline's semantics (the reference's);  rad_r[k] (k = 0, 1, 2), three
 *     floats: ri_texture_ibl_fetch of the ray's unnormalised fp64 direction, with the environment as it stands when the call is made.
 *   value of one hit: with N = floor(sqrt(gather_nsamples))^2 rays, per channel sum_k = 0; for r = 0 .. N - 1 (r = j * ntheta + i):
 *     if (!occ_r) sum_k = sum_k + (double)rad_r[k]; value_k = (float)((scale * sum_k) / N), in fp64.  count = the occluded rays.  The
 *     order is part of the contract.
 *   parameters: eps, the origin's offset along Ns (gather_sunsky: 1e-5, ibl.c: 1e-4); scale, the reference's m (0.3183098861837907 is
 *     gather_sunsky's 1 / M_PI, 1.0 is ri_ibl_sample_cosweight's pi * (1 / pi)).  Both finite, eps >= 0, scale >= 0; NULL:
 *     LH_ENV_DEFAULTS.  Anything else, NaN included, is refused ("bad environment-gather parameters").  The self-primitive skip of a
 *     flat-shaded hit is applied only when eps >= 1e-6.
 * lh_accel_env_device: as lh_accel_dirt_device, word for word -- list, count and key semantics, hit slots in list order, the uniforms
 *   replay (2 doubles per gather ray in (slot, j, i) order), untouched slots of rays that are not traced (12 bytes per ray of d_rgb),
 *   an id listed twice, synchronous on `stream`, the empty scene, scratch of its own, its refusals.  d_occluded_count[id] (uint32, may
 *   be NULL) = count; d_rgb[3 id ..] (3 floats, may be NULL) = value.  A traced miss gets LH_AO_NO_HIT and three 0.0f.  The value
 *   alone: no texture multiply.  Fused when "ao_fused" is on, no uniforms are given, the scene is not empty and list entries x N < 2^31:
 *   the AO stage's any-hit kernel makes the gather rays itself and whoever finishes a ray stores its answer as one byte; else, and as
 *   the second try of a fused launch whose queue overflowed, the rays are materialised in HBM and traced by one any-hit launch.  A
 *   resolve with a group of lanes per hit then fetches the colours of the rays that are not occluded and adds them in r order.  Both
 *   give the same bytes.  With lh_accel_trace_statistics on, `rays` advances by hits x N and counters[4] by the occluded rays.
 * lh_render_env_tile: per camera sample -- a miss gives 0 (ambientocclusion.c:407-411), a hit its value_k (the float), times the texture
 *   of its mesh where it has one, per channel as the AO and dirt tiles multiply; sub-samples accumulated and written as
 *   lh_render_ao_tile does, keys are the absolute sample position (a frame does not depend on its tiling); stats->ao_rays = hits x N,
 *   stats->ao_occluded = the sum of the hits' counts.  lh_render_scratch keeps showing the last AO tile.
 * lh_accel_environment_device: the fetch alone for n fp64 directions (3 doubles each, need not be unit vectors), 3 floats each to
 *   d_rgb_out: what a caller needs to light a camera miss.  Asynchronous on `stream`, nothing is read back.  A zero or non-finite
 *   direction gives an unspecified colour; the texel index stays inside the map.  -1: an uncommitted accelerator, a NULL or misaligned
 *   array with n > 0.  lh_accel_environment_host: the same for HOST arrays (copies up, the device call, copies down).
 * The Preetham sky of sunsky.c and the sun's shadow ray (contribution_from_sunlight) are another radiance source for the same stage:
 *   the sun-and-sky light below (lh_accel_set_sky).  Not built: the qmc branch of ibl.c. */
typedef struct lh_env_params { double eps, scale; } lh_env_params_t;
#define LH_ENV_DEFAULTS { 1.0e-5, 1.0 }
int  lh_accel_env_device(lh_accel_t *accel, size_t n_rays, const void *d_org_xyz, const void *d_dir_xyz,
                         const void *d_prim, const void *d_t, const void *d_u, const void *d_v,
                         int gather_nsamples, const lh_env_params_t *params, uint64_t seed, const void *d_key, const void *d_uniforms,
                         const void *d_index, size_t n_index, const void *d_count,
                         void *d_occluded_count, void *d_rgb, void *stream);
int  lh_accel_env_host(lh_accel_t *accel, size_t n_rays, const double *org_xyz, const double *dir_xyz, const uint32_t *prim,
                       const double *t, const double *u, const double *v, int gather_nsamples, const lh_env_params_t *params,
                       uint64_t seed, const uint64_t *key, const double *uniforms, size_t nuniforms, uint32_t *occluded_count, float *rgb);
int  lh_render_env_tile(lh_accel_t *accel, const lh_camera_t *cam, int x0, int y0, int w, int h, int pixel_samples,
                        int gather_nsamples, const lh_env_params_t *params, uint64_t seed,
                        const void *d_uniforms, void *d_rgb, lh_tile_stats_t *stats, void *stream);
int  lh_accel_environment_device(lh_accel_t *accel, size_t n, const void *d_dir_xyz, void *d_rgb_out, void *stream);
int  lh_accel_environment_host(lh_accel_t *accel, size_t n, const double *dir_xyz, float *rgb_out);

/* ---- the sun-and-sky light of the gather above (gather_sunsky with a sunsky light: ri_sunsky_get_sky_rgb, src/render/sunsky.c:329-415,
 *      and contribution_from_sunlight, src/transport/ambientocclusion.c:153-199,312-321; the rule: lucille_amd/csrc/lh_sky.h) ----
 * While a sky is set (lh_accel_set_sky), lh_accel_env_device, lh_accel_env_host and lh_render_env_tile read it in place of the
 * environment:
 *   rad_r = the analytic Preetham sky in the direction of gather ray r, rounded to float first: y and z swapped, zero below the horizon,
 *     a direction within 0.001 of it pulled up and normalised, theta / phi / gamma and the three Perez functions in the reference's float
 *     order, M1 and M2 from the chromaticity; from there rgb_k = Y (C0_k + M1 C1_k + M2 C2_k) / (L0 + M1 L1 + M2 L2) with C_j =
 *     basis_rgb[j], L_j = basis_y[j]: the caller's colour pipeline's rgb and CIE y of the daylight basis spectra S0, S1, S2 (the
 *     reference's 41-sample sum is linear in them).  The collapsed sum rounds differently from the reference's: the sky stays within
 *     a measured bound of ri_sunsky_get_sky_rgb (|got - ref| <= 7.12e-6 max_k |ref_k|: four times the largest seen, tests/test_sky_rule.py), everything built on
 *     its colours is bit for bit.  A direction that is not of unit length gives an unspecified colour (NaN possibly), never a fault.
 *   with LH_SKY_SUN in flags, every hit traces one more any-hit ray from the gather's origin P + eps Ns along sun_dir, answered by a
 *     plain any-hit launch (the semantics of lh_accel_intersect_device: no self-primitive skip -- a sun behind the surface is
 *     shadowed by the hit's own triangle, as in the reference); where it is not occluded, sum_k = sum_k + (double)sun_rgb[k] after
 *     the N gather rays, before value_k = (float)((scale * sum_k) / N).  The sun's ray draws nothing (the uniforms replay is
 *     unchanged) and is not counted: count, stats->ao_rays, stats->ao_occluded and the trace statistics stay those of the N rays.
 *   the tile does not multiply by the material texture (the reference's sunsky branch fetches none, ambientocclusion.c:369-375).
 *   the reference's own call: gather_nsamples 64, eps 1e-5, scale 1 / pi.
 * The path tracer and the refraction chain keep reading the environment.  With no sky set the three calls launch what they always did.
 * Layout (168 bytes, 8-byte aligned; fixed): sun_theta 0, sun_phi 4, perez_x 8, perez_y 28, perez_Y 48, zenith_x 68, zenith_y 72,
 *   zenith_Y 76, basis_rgb 80 ([j][k]: channel k of S_j), basis_y 116, sun_rgb 128, flags 140, sun_dir 144.
 * lh_sky_from_site: the parts of ri_sunsky_init / init_sun_theta_phi that need no table, for a site (degrees; standard_meridian in hours,
 *   as the reference multiplies it by 15), a day of the year, a time of day (hours) and a turbidity: the angles, the fifteen Perez
 *   coefficients, the three zenith values and sun_dir in the reference's light convention (y and z swapped, lightsource.c:156-158).
 *   basis_rgb, basis_y, sun_rgb and flags are left alone.  Host only, no accelerator.  -1: NULL or a non-finite argument.
 * lh_accel_set_sky: after commit, as lh_accel_set_environment; the struct is copied; NULL removes the sky.  A struct with a non-finite
 *   field or an undefined flag is refused ("bad sky parameters").
 * lh_accel_sky_device / _host: the fetch alone, shaped like lh_accel_environment_device / _host; -1 with a message when no sky is set.
 * Not built: the sky as a source of the path tracer and the refraction chain, create_sunsky_image, the RIB reader's
 *   AreaLightSource "sunsky", and the glue's frame controller, which still declines a sunsky light. */
#define LH_SKY_SUN   1u          /* trace the sun's shadow ray */
#define LH_SKY_FLAGS 1u          /* the defined bits */
typedef struct lh_sky {
    float sun_theta, sun_phi;
    float perez_x[5], perez_y[5], perez_Y[5];
    float zenith_x, zenith_y, zenith_Y;
    float basis_rgb[3][3];   /* the caller's colour pipeline's rgb of S0, S1, S2 */
    float basis_y[3];        /* its CIE y of the same */
    float sun_rgb[3];
    uint32_t flags;          /* LH_SKY_SUN: trace the sun's shadow ray */
    double sun_dir[3];       /* world space, as the reference's light->direction */
} lh_sky_t;
int  lh_sky_from_site(lh_sky_t *sky, float latitude, float longitude, float standard_meridian, int julian_day, float time_of_day,
                      float turbidity);
int  lh_accel_set_sky(lh_accel_t *accel, const lh_sky_t *sky);
int  lh_accel_sky_device(lh_accel_t *accel, size_t n, const void *d_dir_xyz, void *d_rgb_out, void *stream);
int  lh_accel_sky_host(lh_accel_t *accel, size_t n, const double *dir_xyz, float *rgb_out);

/* ---- direct light: shadow rays from a batch of hits to a short list of lights (contribution_from_sunlight,
 *      src/transport/ambientocclusion.c:153-199, for the directional and point lights of ri_light_t, src/render/light.h:26-32; the rule:
 *      lucille_amd/csrc/lh_lights.h) ----
 * For every hit and every light of the list one plain any-hit ray from the gather stages' origin O = P + eps Ns (P and Ns as
 * lh_accel_state_build_device gives them, Ns taken as it is): which lights the hit sees, and what they add.  Everything in fp64 in the
 * order written, nothing contracted:
 *   ray of light l:  directional (no LH_LIGHT_POINT): dir = v, the direction TOWARDS the light, unbounded.  Point: dir[k] = v[k] - O[k],
 *     not normalised, bound tmax = 1.0: the ray is open iff the bounded any-hit contract of lh_accel_intersect_device_tmax answers 0
 *     for (O, dir, 1.0) -- strict: an occluder exactly at the light does not shadow it.  No self-primitive skip (the semantics of
 *     lh_accel_intersect_device): a light behind the surface is shadowed by the hit's own triangle, as the sky's sun.
 *   weight:  w = 1; with LH_LIGHT_COSINE, nn = (Ns0 Ns0 + Ns1 Ns1) + Ns2 Ns2, dd the same sum of dir, nd = (Ns0 d0 + Ns1 d1) + Ns2 d2,
 *     c = nd / sqrt(nn * dd), w = c > 0 ? c : 0 (a NaN gives 0); with LH_LIGHT_INVSQ, w = w / dd afterwards.
 *   a ray whose direction is the zero vector or has a non-finite component is dark and is never traced; nor is a ray with !(w > 0).
 *   bit l = (the ray is not dark && w > 0 && it is open);  value: sum_k = 0, for l = 0 .. L - 1 in list order: if (bit l)
 *     sum_k = sum_k + w * rgb_l[k]; value_k = (float)sum_k.  The order is part of the contract.  With no flags this is the reference's
 *     Lo[k] += light->col[k] per light.
 *   parameters: eps finite and >= 0 (NULL: LH_LIGHTS_DEFAULTS); 1 <= nlights <= LH_LIGHTS_MAX; every v and rgb finite; a directional v
 *     not the zero vector; flags within the three bits, reserved 0; LH_LIGHT_INVSQ only with LH_LIGHT_POINT.  Anything else is refused
 *     ("bad lights") and nothing is enqueued.  A shadow ray with |dir.y| <= 1e-14 is outside the contract (reference UB, bvh.c:483-487).
 *   LH_LIGHTS_MAX is 31, not 32: a traced miss is marked LH_AO_NO_HIT in d_visible, and a hit that saw 32 lights would carry the same
 *     word.  `lights` is HOST memory and is copied: the table travels by value in the arguments of every kernel that reads it (1 736
 *     bytes), so there is no device block whose release would have to wait for a launch.
 * lh_accel_lights_device: as lh_accel_env_device, word for word -- list, count and id semantics, hit slots in list order, untouched
 *   slots of rays that are not traced (4 bytes of d_visible, 12 of d_rgb), an id listed twice, synchronous on `stream`, the empty scene,
 *   scratch of its own, its refusals; no keys, seed or uniforms: the stage draws nothing.  d_visible[id] (uint32, may be NULL) = the bit
 *   mask, LH_AO_NO_HIT for a traced miss; d_rgb[3 id ..] (3 floats, may be NULL) = value, three 0.0f for a miss; not both NULL.  Fused
 *   when "ao_fused" is on, the scene is not empty and list entries x nlights < 2^31: the persistent any-hit walk makes ray (slot, l) in
 *   its refill from the hit record and the light table, walks it under its bound and stores its answer as one byte; else, and as the
 *   second try of a fused launch whose queue overflowed, one kernel writes rays and bounds and one bounded any-hit launch answers
 *   them.  Both give the same bytes.  With lh_accel_trace_statistics on, `rays` advances by hits x nlights (work items, traced or not)
 *   and counters[4] by the items whose bit is clear.
 * lh_accel_lights_host: the same for HOST arrays (copies up, the device call on the accelerator's stream, copies down).
 * lh_accel_light_rays_device: the shadow rays alone, shaped like lh_accel_ao_rays_device: d_slot_of_ray, d_nslots, and ray (slot, l) at
 *   element slot * nlights + l of d_org_out / d_dir_out (3 doubles each) and of d_tmax_out (doubles): +inf for a directional light, 1.0
 *   for a point light, 0.0 for a ray that is not traced (dark, or !(w > 0)) -- its bit is clear whatever a launch answers for it.
 *   lh_accel_intersect_device_tmax in any-hit mode on these arrays gives exactly the stage's bytes.  Asynchronous, nothing read back;
 *   capacity_rays >= n_rays * nlights or it is refused.
 * lh_render_lights_tile: per camera sample -- a miss gives 0, a hit its value_k (the float); sub-samples are widened, added per channel
 *   in sample order, scaled, converted, clamped and written as lh_render_env_tile does; a frame does not depend on its tiling.
 *   stats->ao_rays = hits x nlights, stats->ao_occluded = the items whose bit is clear.
 * Not built: the texture multiply (the reference's sun branch fetches none, ambientocclusion.c:369-375), the sky's own sun
 *   ray through this stage (lh_accel_set_sky keeps its launch), bands and the multi-device forms. */
#define LH_LIGHT_POINT  1u   /* v is a position; without it v is the direction TOWARDS the light, as the reference's light->direction */
#define LH_LIGHT_COSINE 2u   /* weight by the cosine between Ns and the ray */
#define LH_LIGHT_INVSQ  4u   /* point lights only: divide by the squared distance */
#define LH_LIGHTS_MAX  31
typedef struct lh_light { double v[3]; double rgb[3]; uint32_t flags, reserved; } lh_light_t;   /* 56 bytes */
typedef struct lh_lights_params { double eps; } lh_lights_params_t;
#define LH_LIGHTS_DEFAULTS { 1.0e-5 }                                /* ambientocclusion.c:166 */
int  lh_accel_lights_device(lh_accel_t *accel, size_t n_rays, const void *d_org_xyz, const void *d_dir_xyz,
                            const void *d_prim, const void *d_t, const void *d_u, const void *d_v,
                            const lh_light_t *lights, int nlights, const lh_lights_params_t *params,
                            const void *d_index, size_t n_index, const void *d_count,
                            void *d_visible, void *d_rgb, void *stream);
int  lh_accel_lights_host(lh_accel_t *accel, size_t n_rays, const double *org_xyz, const double *dir_xyz, const uint32_t *prim,
                          const double *t, const double *u, const double *v, const lh_light_t *lights, int nlights,
                          const lh_lights_params_t *params, uint32_t *visible, float *rgb);
int  lh_accel_light_rays_device(lh_accel_t *accel, size_t n_rays, const void *d_org_xyz, const void *d_dir_xyz,
                                const void *d_prim, const void *d_t, const void *d_u, const void *d_v,
                                const lh_light_t *lights, int nlights, const lh_lights_params_t *params,
                                void *d_slot_of_ray, void *d_nslots, void *d_org_out, void *d_dir_out, void *d_tmax_out,
                                size_t capacity_rays, void *stream);
int  lh_render_lights_tile(lh_accel_t *accel, const lh_camera_t *cam, int x0, int y0, int w, int h, int pixel_samples,
                           const lh_light_t *lights, int nlights, const lh_lights_params_t *params,
                           void *d_rgb, lh_tile_stats_t *stats, void *stream);

/* ---- area lights: soft shadows from triangle emitters (the mesh an ri_light_t carries: light->geom, ri_light_attach_geom, src/render/light.c:107-111;
 *      the point and normal drawn on it: ri_light_sample_pos_and_normal, light.c:113-147; the rule: lucille_amd/csrc/lh_area.h) ----
 * For every hit, every light of the list and every sample s < S one any-hit ray from the gather stages' origin O = P + eps Ns to a point drawn on the
 * light's emitter triangles: which lights the hit sees, and the mean of what their samples add.  Everything in fp64 in the order written:
 *   emitters: lh_accel_set_emitters gives the accelerator a table of triangles (HOST memory, 9 doubles each: v0 v1 v2), after commit, at any time;
 *     NULL / 0 removes it.  The library keeps one 128-byte record per triangle on the device (v0 v1 v2 n area: e1 = v1 - v0, e2 = v2 - v0, c = e1 x e2,
 *     norm2 = (c0 c0 + c1 c1) + c2 c2, len = sqrt(norm2), n = c * (1.0 / len) where norm2 > (double)1.0e-17f, else n = c; area = 0.5 * len).  A
 *     replaced or removed block is released behind a device-wide synchronise, as a texture's; the table is kept across lh_accel_recommit (emitters are
 *     no scene geometry: a caller who wants them to occlude adds them as a mesh too).  Refused before anything touches a device: a non-finite vertex,
 *     ntris >= 2^31 ("bad emitters").
 *   light l is the run [first_tri, first_tri + ntris) of the table.  Sample (l, s) with uniforms (x0, x1, x2): j = (int)(x0 * (double)ntris) clamped to
 *     [0, ntris - 1]; a NaN x0 makes the item dark; sq = sqrt(x1), t = x2, pos[k] = (double)(float)((v0[k] * (1.0 - sq) + v1[k] * (sq - t * sq)) +
 *     (v2[k] * sq) * t) on triangle first_tri + j -- the reference's expression and its rounding to float -- and n that triangle's.
 *   ray: dir = pos - O, not normalised, under the bound params.bound (0 < bound <= 1): open iff the bounded any-hit contract of
 *     lh_accel_intersect_device_tmax answers 0 for (O, dir, bound).  No self-primitive skip.  The float-rounded pos lies off its triangle's plane: where
 *     the emitter triangles are scene geometry too, at bound 1 an emitter may or may not shadow itself; pass a little less (1 - 1e-4).  A zero or
 *     non-finite dir is dark.
 *   weight: w = 1, dd = (d0 d0 + d1 d1) + d2 d2, then in this order: LH_AREA_COSINE, the surface cosine, LH_LIGHT_COSINE's expression;
 *     LH_AREA_FACING, cl = -((n0 d0 + n1 d1) + n2 d2) / sqrt(dd), w = w * (cl > 0 ? cl : 0) (a one-sided emitter); LH_AREA_INVSQ, w = w / dd;
 *     LH_AREA_PDF, w = w * ((double)ntris * area_j) (the pick is uniform by index: 1 / pdf).  A dark item and one with !(w > 0) is never traced.
 *   value: sum_k = 0; for l in list order, for s = 0 .. S - 1: if item (l, s) is traced and open, sum_k = sum_k + w * rgb_l[k];
 *     value_k = (float)(sum_k / (double)S); bit l of the mask: any sample of light l is open.  The order is part of the contract.
 *   uniforms: d_uniforms (or NULL) replays 3 doubles per item in (hit slot, l, s) order, 3 * nlights * S * hits are consumed.  Built in (NULL):
 *     c = ((key & (2^34 - 1)) * (uint64)(L S) + (uint64)(l S + s)) * 4, k = (seed * 0x9E3779B97F4A7C15) ^ c, x_j = (double)mix32(k + j) * 2^-32,
 *     mix32 the AO stage's; the key of a hit is its entry of d_key, as lh_accel_ao_device takes it.  The built-in path is the replay rule fed by this
 *     generator.
 *   parameters: NULL is LH_AREA_DEFAULTS; eps finite and >= 0, bound finite with 0 < bound <= 1, 1 <= nsamples <= LH_AREA_SAMPLES_MAX, reserved 0;
 *     1 <= nlights <= LH_AREA_LIGHTS_MAX (31, for LH_LIGHTS_MAX's reason); every rgb finite, flags within the four bits, reserved 0, ntris >= 1 and
 *     first_tri + ntris <= the table's count.  Anything else is refused ("bad area lights") and nothing is enqueued.  `lights` is HOST memory and
 *     travels by value in the kernels' arguments.  A ray with |dir.y| <= 1e-14 is outside the contract, as every shadow ray's.
 * lh_accel_area_lights_device: as lh_accel_lights_device, word for word -- list, count and id semantics, hit slots in list order, untouched slots of
 *   rays that are not traced, an id listed twice, synchronous on `stream`, the empty scene, scratch of its own, its refusals -- with seed, d_key and
 *   d_uniforms as lh_accel_ao_device takes them.  Fused when "ao_fused" is on, no uniforms are replayed and list entries x nlights x S < 2^31: ray
 *   source 4 of the persistent any-hit walk makes item (slot, l, s) in its refill -- the hit record, three uniforms, ONE gathered emitter record --
 *   walks it under the bound and stores its answer as a byte.  Else, and as the second try after a queue overflow, one kernel writes rays, bounds and
 *   weights and one bounded any-hit launch per 2^30 items answers them.  Both give the same bytes.  With lh_accel_trace_statistics on, `rays` advances
 *   by hits x nlights x S and counters[4] by the items that are not open.
 * lh_accel_area_lights_host: the same for HOST arrays; nuniforms >= 3 * nlights * S * n_rays where uniforms are given.
 * lh_accel_area_light_rays_device: the rays alone, shaped like lh_accel_light_rays_device: item (slot, l, s) at element (slot * nlights + l) * S + s of
 *   d_org_out / d_dir_out (3 doubles), d_tmax_out (the bound, 0.0 for an item that is not traced) and d_weight_out (doubles, may be NULL).
 *   lh_accel_intersect_device_tmax in any-hit mode on these arrays gives exactly the stage's bytes.  Asynchronous, nothing read back;
 *   capacity_rays >= n_rays * nlights * S or it is refused.
 * lh_render_area_lights_tile: per camera sample, as lh_render_lights_tile; the built-in generator only, keyed by the absolute sample position: a frame
 *   does not depend on its tiling.  stats->ao_rays = hits x nlights x S, stats->ao_occluded = the items that are not open.
 * Not built: the device-pointer emitter table, the qmc sampler (ri_light_sample_pos_and_normal_qmc, light.c:149-194), a texture multiply, bands and
 *   the multi-device forms, AreaLightSource in the RIB reader. */
#define LH_AREA_COSINE 1u   /* weight by the cosine between Ns and the ray */
#define LH_AREA_FACING 2u   /* weight by the cosine at the emitter, clamped at 0: one-sided */
#define LH_AREA_INVSQ  4u   /* divide by the squared distance */
#define LH_AREA_PDF    8u   /* multiply by ntris x the sampled triangle's area */
#define LH_AREA_LIGHTS_MAX  31
#define LH_AREA_SAMPLES_MAX 1024
typedef struct lh_area_light { uint32_t first_tri, ntris; double rgb[3]; uint32_t flags, reserved; } lh_area_light_t;   /* 40 bytes */
typedef struct lh_area_params { double eps, bound; int32_t nsamples; uint32_t reserved; } lh_area_params_t;              /* 24 bytes */
#define LH_AREA_DEFAULTS { 1.0e-5, 1.0, 16, 0 }
int  lh_accel_set_emitters(lh_accel_t *accel, const double *tri_xyz, size_t ntris);
int  lh_accel_area_lights_device(lh_accel_t *accel, size_t n_rays, const void *d_org_xyz, const void *d_dir_xyz,
                                 const void *d_prim, const void *d_t, const void *d_u, const void *d_v,
                                 const lh_area_light_t *lights, int nlights, const lh_area_params_t *params,
                                 uint64_t seed, const void *d_key, const void *d_uniforms,
                                 const void *d_index, size_t n_index, const void *d_count,
                                 void *d_visible, void *d_rgb, void *stream);
int  lh_accel_area_lights_host(lh_accel_t *accel, size_t n_rays, const double *org_xyz, const double *dir_xyz, const uint32_t *prim,
                               const double *t, const double *u, const double *v, const lh_area_light_t *lights, int nlights,
                               const lh_area_params_t *params, uint64_t seed, const uint64_t *key, const double *uniforms, size_t nuniforms,
                               uint32_t *visible, float *rgb);
int  lh_accel_area_light_rays_device(lh_accel_t *accel, size_t n_rays, const void *d_org_xyz, const void *d_dir_xyz,
                                     const void *d_prim, const void *d_t, const void *d_u, const void *d_v,
                                     const lh_area_light_t *lights, int nlights, const lh_area_params_t *params,
                                     uint64_t seed, const void *d_key, const void *d_uniforms,
                                     void *d_slot_of_ray, void *d_nslots, void *d_org_out, void *d_dir_out, void *d_tmax_out, void *d_weight_out,
                                     size_t capacity_rays, void *stream);
int  lh_render_area_lights_tile(lh_accel_t *accel, const lh_camera_t *cam, int x0, int y0, int w, int h, int pixel_samples,
                                const lh_area_light_t *lights, int nlights, const lh_area_params_t *params, uint64_t seed,
                                void *d_rgb, lh_tile_stats_t *stats, void *stream);

/* ---- the refraction chain: the reference's Whitted transport (trace_whitted, src/transport/whitted.c:32-151; ri_refract and
 *      ri_reflect, src/render/reflection.c:26-128) ----
 * No random number anywhere: a hit sends ONE ray on -- the refraction of the incoming direction at the interpolated normal, or its
 * mirror image where the refraction does not exist -- and what that ray hits sends the next, max_depth rays at most; the chain's
 * value is the accelerator's environment (lh_accel_set_environment: the angular map scaled by rgb, or the constant rgb; constant
 * white if none was set -- the reference's "no environment map: black" is a constant black environment) seen by the ray that leaves
 * the scene.
 *   one bounce, from the hit's state as lh_accel_state_build_device gives it (P: doubles 0-2; n = Ns: doubles 6-8, not normalised
 *     when it is interpolated; I: doubles 20-22), fp64 in this order, nothing contracted:
 *       cos1 = (I0 n0 + I1 n1) + I2 n2;  cos1 < 0: c = -cos1, e = 1 / eta, N = n;  else: c = cos1, e = eta, N = -n
 *       coeff = 1 - (e e) (1 - c c)
 *       coeff <= 0 (total internal reflection): s = (double)(2.0f * (float)cos1), R = I - n s;  else q = e c - sqrt(coeff), R = q N + e I
 *       n2 = (R0 R0 + R1 R1) + R2 R2;  n2 > (double)1.0e-17f: R = R * (1 / sqrt(n2))
 *       next ray: org = P + eps R, dir = R
 *   the chain of one hit record (state 0), d = 1 .. max_depth: ray d is the bounce of state d - 1, a closest-hit ray under the
 *     pipeline's semantics (no self-primitive skip).  A miss: the chain escapes -- bounces = d, value = the three floats
 *     lh_accel_environment_device gives for the direction of ray d.  A hit with d == max_depth: the chain is cut -- bounces =
 *     d | LH_WHITTED_CUT, value = 0, 0, 0.  Any other hit: state d, from ray d and its record.  max_depth 0: bounces = LH_WHITTED_CUT.
 *   parameters: eps finite and >= 0, eta finite and > 0, 0 <= max_depth <= 64, reserved == 0; NULL: LH_WHITTED_DEFAULTS.  Anything
 *     else, NaN included, is refused ("bad refraction parameters").
 * lh_accel_whitted_rays_device: the bounce alone for a caller's closest-hit records (LH_REC_F64) -- the next ray of every traced hit,
 *   three doubles each into d_org_out / d_dir_out by ray id; the slots of misses and of rays that are not traced stay as they are.
 *   Asynchronous on `stream`, nothing is read back.  List and count as for lh_accel_ao_device.
 * lh_accel_whitted_device: the whole chain, list and count as for lh_accel_ao_device (an id listed twice gets that ray's answer
 *   twice).  d_bounces[id] (uint32) = LH_AO_NO_HIT for a traced record that is a miss, else as above; d_end_org / d_end_dir[3 id ..]
 *   (doubles) = the last ray traced for the id -- a miss record, and a hit with max_depth == 0, leave them as they are; d_rgb[3 id ..]
 *   (floats) = value, three 0.0f for a miss record.  Any of the four may be NULL.  A record whose primitive id is not one of the
 *   scene's counts as a miss: in an empty scene every record does, no chain starts.  Synchronous on `stream`: one launch pair per
 *   depth over lists that stay on the device, one read-back at the end.  With lh_accel_trace_statistics on, `rays` advances by the
 *   chain rays traced.  Scratch of its own, sized by list entries.
 *   -1 (lh_last_error), nothing enqueued or written: bad parameters, n_rays >= 2^31, n_index > 2^30, a list / count / bounces / rgb
 *   pointer that is not 4-byte aligned, a ray / record / end-ray pointer that is not 8-byte aligned (prim: 4), an uncommitted
 *   accelerator, a NULL ray or record array with n_rays > 0.  n_rays == 0 returns 0 and looks at no array.
 * lh_accel_whitted_host: the same for HOST arrays (copies up, the device call on the accelerator's stream, copies down; every ray
 *   is traced).
 * lh_render_whitted_tile: ri_transport_whitted per camera sample (the samples of lh_render_primary_rays) -- a camera miss gives the
 *   environment in the camera ray's direction (whitted.c:135-139), a hit its chain's value; no texture multiply (whitted.c has
 *   none); sub-samples are widened to double, added per channel in sample order, scaled, converted, clamped and written in image
 *   orientation as lh_render_env_tile does.  stats->paths = camera samples, stats->rays = camera rays + chain rays,
 *   stats->max_depth_reached = the largest d traced.  A frame does not depend on its tiling. */
typedef struct lh_whitted_params { double eps, eta; int max_depth, reserved; } lh_whitted_params_t;
#define LH_WHITTED_DEFAULTS { 1.0e-7, 1.33, 8, 0 }   /* whitted.c:38,46,24 */
#define LH_WHITTED_CUT 0x80000000u
int  lh_accel_whitted_rays_device(lh_accel_t *accel, size_t n_rays, const void *d_org_xyz, const void *d_dir_xyz,
                                  const void *d_prim, const void *d_t, const void *d_u, const void *d_v,
                                  const lh_whitted_params_t *params, const void *d_index, size_t n_index, const void *d_count,
                                  void *d_org_out, void *d_dir_out, void *stream);
int  lh_accel_whitted_device(lh_accel_t *accel, size_t n_rays, const void *d_org_xyz, const void *d_dir_xyz,
                             const void *d_prim, const void *d_t, const void *d_u, const void *d_v,
                             const lh_whitted_params_t *params, const void *d_index, size_t n_index, const void *d_count,
                             void *d_bounces, void *d_end_org, void *d_end_dir, void *d_rgb, void *stream);
int  lh_accel_whitted_host(lh_accel_t *accel, size_t n_rays, const double *org_xyz, const double *dir_xyz, const uint32_t *prim,
                           const double *t, const double *u, const double *v, const lh_whitted_params_t *params,
                           uint32_t *bounces, double *end_org, double *end_dir, float *rgb);

/* ---- material textures: the multiply both occlusion transports end with (src/transport/ambientocclusion.c:393-401, dirtmap.c:273-281) ----
 * Where the hit's mesh has a texture: ri_texture_fetch(texcol, texture, s, t); radiance[k] *= texcol[k].
 *   texture: height rows of width texels, 4 floats (RGBA) each, row 0 first (ri_texture_t.data, src/render/texture.h:21-29), no flip.
 *   fetch(s, t) = ri_texture_fetch (src/render/texture.c:86-235, the scanline branch), fp64 in this order, no contraction:
 *     u = s - floor(s), v = t - floor(t); each clamped: < 0 -> 0, >= 1 -> 1; px = u * (width - 1), py = v * (height - 1);
 *     x = (int)px, y = (int)py; dx = px - x, dy = py - y; w0 = (1-dx)(1-dy), w1 = (1-dx)dy, w2 = dx(1-dy), w3 = dx dy over the texels
 *     (x,y), (x,y+1), (x+1,y), (x+1,y+1) widened to double, a neighbour outside the image counting as 0.0 (the reference's edge rule);
 *     out[i] = ((w0 e0[i] + w1 e1[i]) + w2 e2[i]) + w3 e3[i] for the four channels.
 *   s, t: doubles 18 and 19 of lh_accel_state_build_* for the hit (lerp_uv; 0, 0 for a mesh without texture coordinates).  A non-finite
 *     s or t (undefined in the reference) gives an unspecified colour; the texel index stays inside the image.
 *   per camera sample: rad_k = rad * texcol[k] (k = 0, 1, 2) where the hit's mesh has a texture, else rad_k = rad, with rad the double the
 *     tile computes without textures; sub-samples accumulate per channel in the same order, then the same scale, (float) conversion and
 *     clamp of negatives to 0, per channel.  A miss contributes 0.
 * lh_render_ao_tile / _bands / _tile_host, lh_render_ao_frame_host, lh_render_dirt_tile, lh_render_env_tile, lh_multi_render_ao_frame_host and
 *   lh_dist_render_ao_frame_host multiply as soon as the accelerator holds at least one texture; with none they launch the kernels
 *   they always launched, with the same arguments.  Tile statistics, the replay uniforms and the fused / materialised stages do not
 *   depend on textures.  The sun-and-sky branch is built and, as in the reference, fetches no texture: lh_render_env_tile does not
 *   multiply while a sky is set (lh_accel_set_sky).  Not covered: mip-maps, textures in the path tracer (lh_render_pt_*), and
 *   `Surface "texture"` in the RIB reader (it needs the reference's image loaders).
 * lh_accel_set_texture: rgba is HOST memory (width x height x 4 floats) and is copied.  Allowed for any mesh already added, before or
 *   after commit (trees do not depend on it; no device is touched before the first call that needs the texture there).  rgba == NULL
 *   with width == height == 0 removes the texture; a second call replaces the first and takes effect for calls made after it returns.
 *   A block that is replaced or removed is released only after every launch enqueued earlier that may read it has finished.  Texel
 *   values are not validated.  With LH_ALL_MESHES the meshes share one block.
 * lh_accel_set_texture_device: the same for an array in the memory of the accelerator's device; it is read by a copy enqueued on
 *   `stream` before the call returns, into a block the library owns: the caller may overwrite or free it in stream order afterwards.
 * Both refuse, -1 with lh_last_error, nothing changed: "accel is NULL"; "mesh M out of range"; "bad texture size" (width or height
 *   outside [1, 65536]); "NULL array" (with a non-zero size); "not 4-byte aligned"; the device form: "not a device pointer" /
 *   "extends past its allocation" (asked of the runtime, never dereferenced), as lh_accel_add_mesh_device. */
int  lh_accel_set_texture(lh_accel_t *accel, uint32_t mesh /* or LH_ALL_MESHES */, const float *rgba, int width, int height);
int  lh_accel_set_texture_device(lh_accel_t *accel, uint32_t mesh /* or LH_ALL_MESHES */, const void *d_rgba, int width, int height,
                                 void *stream);
/* the fetch alone for a caller's batch of hit records (a bake, a transport of the caller's own): d_prim / d_u / d_v are the LH_REC_F64
 * closest-hit records of n_rays rays; d_index / n_index / d_count: a list as for lh_accel_ao_device (ids, the identity list when
 * d_index is NULL, the count read on `stream`; all NULL / 0: every ray; a traced ray is a listed entry within the count whose id is
 * < n_rays).  d_rgba_out[4 * id ..] (doubles) = fetch(s, t) of the hit, or 1, 1, 1, 1 where its mesh has no texture; a traced miss
 * (LH_MISS, or an id beyond the scene's primitives) gets four zeros.  The slots of rays that are not traced are not touched, byte for
 * byte; an id listed twice is written twice with the same values.  Asynchronous on `stream`, nothing is read back.  An empty scene:
 * every traced ray is a miss, no record array is read.  -1 (lh_last_error), nothing enqueued or written: an uncommitted accelerator,
 * a NULL record or output array with n_rays > 0, n_rays >= 2^31, n_index > 2^30, a list / count / id pointer that is not 4-byte
 * aligned or a u / v / output pointer that is not 8-byte aligned.  n_rays == 0 returns 0 and looks at no array. */
int  lh_accel_texture_device(lh_accel_t *accel, size_t n_rays, const void *d_prim, const void *d_u, const void *d_v,
                             const void *d_index, size_t n_index, const void *d_count, void *d_rgba_out, void *stream);
/* the same for HOST arrays: copies up, runs lh_accel_texture_device on the accelerator's stream, copies down (every ray is traced) */
int  lh_accel_texture_host(lh_accel_t *accel, size_t n_rays, const uint32_t *prim, const double *u, const double *v, double *rgba_out);

/* one path-traced tile on the device (BASELINE config 4: the reference's pathtrace.c is dead
 * code; its documented structure -- camera sample, Russian roulette on the reflectance,
 * cosine-sampled diffuse bounces to a vertex limit, environment radiance on escape -- re-expressed
 * as closest-hit batches, every bounce through the same kernel as ri_raytrace).  Adds
 * spp_count samples (numbered spp_begin...) of spp_total to d_rgb (float[h][w][3], image
 * orientation; the caller zeroes it before the first pass).  kd: diffuse reflectance in (0,1];
 * env_rgb: constant environment radiance.  stats: rays traced / paths.
 * One pass holds at most 2^30 paths (w x h x spp_count) and at most 4096 samples of a pixel: a path's radiance goes into
 * its pixel's 64-bit fixed-point sums (32 fraction bits, a sample clamped to +-2^18, a NaN channel dropped), so a pixel
 * does not depend on the order its paths end in -- tiling, sharding and slot order leave the image bit for bit the same. */
typedef struct lh_pt_stats { uint64_t paths, rays, max_depth_reached; } lh_pt_stats_t;

int  lh_render_pt_tile(lh_accel_t *accel, const lh_camera_t *cam, int x0, int y0, int w, int h,
                       int spp_begin, int spp_count, int spp_total, int max_path_vertices,
                       float kd, const float env_rgb[3], uint64_t seed, void *d_rgb,
                       lh_pt_stats_t *stats, void *stream);
/* the refraction chain's tile (described with lh_accel_whitted_device above; its statistics are this struct's) */
int  lh_render_whitted_tile(lh_accel_t *accel, const lh_camera_t *cam, int x0, int y0, int w, int h, int pixel_samples,
                            const lh_whitted_params_t *params, void *d_rgb, lh_pt_stats_t *stats, void *stream);

/* ---- path tracer with the reference's three reflection types (src/transport/pathtrace.c:189-314,407-537) ----
 * Per-mesh material = ri_material_t (src/render/material.h:21-30; defaults of ri_material_new: kd 1, ks 0, kt 0,
 * ior 1): diffuse / specular / transmission reflectances (their averages d, s, t drive the Russian roulette and the
 * choice of reflection type: d + s + t <= 1) and the index of refraction.  Environment = the light source of
 * light_sample / ri_texture_ibl_fetch (src/render/texture.c:238-276): an angular-map light probe (RGBA float rows,
 * bilinear), scaled by rgb; map NULL: the constant radiance rgb. */
typedef struct lh_material { float kd[3], ks[3], kt[3]; float ior; } lh_material_t;
typedef struct lh_environment { float rgb[3]; const float *map_rgba; int width, height; } lh_environment_t;
#define LH_ALL_MESHES 0xFFFFFFFFu
#define LH_PT_REFERENCE_WEIGHTS 1     /* throughput *= the reference's brdf() value (kd / pi, ks, kt) instead of the
                                         unbiased weight of the same sampling scheme */
int  lh_accel_set_material(lh_accel_t *accel, uint32_t mesh /* or LH_ALL_MESHES */, const lh_material_t *material);
int  lh_accel_set_environment(lh_accel_t *accel, const lh_environment_t *environment);   /* after commit; the map is copied; NULL: back to the default (constant white) */
/* as lh_render_pt_tile, with the accelerator's materials and environment */
int  lh_render_pt_tile2(lh_accel_t *accel, const lh_camera_t *cam, int x0, int y0, int w, int h,
                        int spp_begin, int spp_count, int spp_total, int max_path_vertices, int flags,
                        uint64_t seed, void *d_rgb, lh_pt_stats_t *stats, void *stream);

/* a rank's interleaved full-width bands of an image-space sharded frame (BASELINE config 4 on N GPUs) as ONE pass: nbands bands
 * of band_rows lines, band k starting at frame line y0_first + k * band_stride, all inside the frame.  d_rgb:
 * [nbands][band_rows][width][3] float32, every band in image orientation (lh_render_ao_bands' layout).  Uses the accelerator's
 * environment; override NULL: its per-mesh materials, else that material for every mesh.  Paths are keyed by (frame pixel,
 * sample, bounce): the bands of all ranks together are the frame lh_render_pt_tile2 renders, bit for bit. */
int  lh_render_pt_bands(lh_accel_t *accel, const lh_camera_t *cam, int y0_first, int band_rows, int band_stride, int nbands,
                        int spp_begin, int spp_count, int spp_total, int max_path_vertices, int flags,
                        const lh_material_t *override_material, uint64_t seed, void *d_rgb, lh_pt_stats_t *stats, void *stream);

/* ---- the path tracer with direct light from a light list, and a path-vertex sink (the rule: lucille_amd/csrc/lh_ptl.h) ----
 * lh_render_pt_tile_lit / lh_render_pt_bands_lit: lh_render_pt_tile2 / lh_render_pt_bands, word for word, plus
 *   lights   `lights` / nlights / params as lh_accel_lights_device takes them (HOST memory, copied; nlights == 0: none, `lights` may be NULL
 *     then; else refused as that call refuses them -- "bad lights" -- with nothing enqueued).  Bounce d (0-based) of a pass traces the ray that
 *     arrives at path vertex d + 2.  Every hit of a bounce -- its path may go on, be ended by the roulette or end at the vertex limit -- adds
 *       r_k = ((G_k * kd_k) * col_k) * value_k          float32, three IEEE multiplies in this order
 *     to its path's pixel: G the throughput the arriving ray carries (1, 1, 1 for camera rays), kd the diffuse reflectance of the hit's
 *     material, col the interpolated vertex colour (1 where the mesh has none), value the three floats lh_accel_lights_device gives for this
 *     hit record, list and eps (origin P + eps Ns, one bounded any-hit shadow ray per light, no self-primitive skip).  r goes into the
 *     pixel's fixed-point sums as a path's radiance does: a channel that is NaN or 0 adds nothing, a term is clamped to +-2^18, and the frame
 *     stays the same bit for bit under tiling, banding and slot order.  No 1 / pi is applied (fold it into the lights' colours); no specular
 *     or transmissive lobe is lit.  The environment is collected as before: the list's lights are delta lights no sampled direction finds.
 *     The stage runs once per bounce over the bounce's entries, fused or materialised as for any caller (entries x nlights >= 2^31:
 *     materialised), synchronous; with lh_accel_trace_statistics on, its items are counted as lh_accel_lights_device counts them, on top of
 *     the closest-hit rays.  lh_pt_stats_t is unchanged.
 *     Limits and cost of a pass with lights: every entry of every bounce may add a term to its pixel's sums, so spp_count x
 *     (max_path_vertices - 1) <= 4096 or the call is refused (without lights: spp_count <= 4096, as before).  The stage compacts a
 *     bounce into the scratch of lh_accel_lights_device, sized for the worst case of every path hitting: about 120 + nlights bytes per
 *     path of the pass (a 96-byte hit record, key, slot, 12 bytes of value, a byte per shadow ray; 56 more per shadow ray when the stage
 *     runs materialised) on top of the pass's own ~164, allocated at the first lit call and kept by the accelerator until it is destroyed
 *     -- 2 GB at 2^24 paths and one light.
 *   sink     NULL, or device arrays that receive every entry of every bounce, misses included: bounce d's block starts at record
 *     counts[0] + .. + counts[d - 1] and holds the bounce's entries in its slot order (from bounce 1 on that order depends on scheduling;
 *     the set of records does not).  Each array may be NULL (skipped).  A record at a position >= capacity is not written and nothing
 *     beyond capacity is touched; d_counts always holds the true counts (max_path_vertices words: the entries of every bounce, then
 *     zeros); the call returns 0 and the caller compares their sum with its capacity.  Refused (-1, nothing enqueued): a d_org / d_dir /
 *     d_t / d_u / d_v pointer that is not 8-byte aligned, any other pointer that is not 4-byte aligned.
 *   With nlights == 0 and no sink the calls enqueue exactly what lh_render_pt_tile2 / lh_render_pt_bands enqueue.
 * Area lights at the path vertices are the _lights forms below; the sky's sun is a directional light: a caller puts it into the list.
 * Not built: the texture multiply, the multi-device and distributed frames, LightSource in the RIB reader, lsh_hip options. */
typedef struct lh_pt_sink {            /* device arrays, each may be NULL (skipped); capacity in records */
    void *d_path;    /* uint32: pixel_of_pass * spp + sample, interior bit cleared */
    void *d_depth;   /* uint32: bounce d */
    void *d_org, *d_dir;               /* 3 doubles each */
    void *d_prim, *d_t, *d_u, *d_v;    /* the bounce's hit record, LH_MISS_PRIM for a miss */
    void *d_thr;     /* 3 floats: G of the arriving ray */
    void *d_direct;  /* 3 floats: r of the rule; 0 for a miss or without lights */
    void *d_counts;  /* uint32 [max_vertices]: entries per bounce, then zeros */
    size_t capacity;
} lh_pt_sink_t;
int  lh_render_pt_tile_lit(lh_accel_t *accel, const lh_camera_t *cam, int x0, int y0, int w, int h,
                           int spp_begin, int spp_count, int spp_total, int max_path_vertices, int flags,
                           const lh_light_t *lights, int nlights, const lh_lights_params_t *params, const lh_pt_sink_t *sink,
                           uint64_t seed, void *d_rgb, lh_pt_stats_t *stats, void *stream);
int  lh_render_pt_bands_lit(lh_accel_t *accel, const lh_camera_t *cam, int y0_first, int band_rows, int band_stride, int nbands,
                            int spp_begin, int spp_count, int spp_total, int max_path_vertices, int flags,
                            const lh_material_t *override_material, const lh_light_t *lights, int nlights,
                            const lh_lights_params_t *params, const lh_pt_sink_t *sink, uint64_t seed, void *d_rgb,
                            lh_pt_stats_t *stats, void *stream);

/* ---- the path tracer with soft shadows: area lights at every path vertex (the rule: lucille_amd/csrc/lh_ptl.h) ----
 * lh_render_pt_tile_lights / lh_render_pt_bands_lights: the _lit forms, word for word, with the two lists in one lh_pt_lights_t:
 *   lights / nlights / params          the delta lights, as the _lit forms take them (nlights == 0: none);
 *   area / narea / area_params         area lights over the accelerator's emitter table (lh_accel_set_emitters), as lh_accel_area_lights_device
 *     takes them (HOST memory, copied; narea == 0: none, `area` may be NULL then; else refused as that call refuses them -- "bad area lights",
 *     which includes no emitter table -- with nothing enqueued).  `lights` NULL is no lights at all; with narea == 0 the call is the _lit call:
 *     the same launches, buffers and bytes.
 *   The area value of a hit of bounce d is exactly what lh_accel_area_lights_device answers for that hit record, `area`, area_params, the seed
 *     seed + (uint64)(d + 1) * 0xD1B54A32D192ED03 (modulo 2^64), the entry's key and no replayed uniforms: origin P + eps Ns, area_params.nsamples
 *     samples per light, the bound, no self-primitive skip, lights and samples in order.  The key of an entry is that of its path, sample s of the
 *     pass at frame pixel (px, py): ((uint64)py * cam->width + px) * spp_total + (spp_begin + s) -- frame coordinates, so a frame does not
 *     depend on its tiling, banding or passes over the samples.  The bounce is in the seed because the generator reads 34 bits of a key; the
 *     path's own draws use `seed` itself.
 *   A hit still adds ONE term r_k = ((G_k * kd_k) * col_k) * value_k: with one kind of light value is that stage's three floats, with both
 *     value_k = delta_k + area_k, one float32 add.  The sink's d_direct receives r; lh_pt_sink_t is unchanged.  No 1 / pi is applied, no specular
 *     or transmissive lobe is lit, and an emitter is seen by no sampled direction: emitters are no scene geometry (a caller who wants them to
 *     occlude adds them as a mesh and passes a bound a little below 1), so nothing is counted twice.
 *   Refused (-1, nothing enqueued or written): everything the _lit forms refuse; the area list and parameters; a non-zero reserved word;
 *     cam->width x cam->height x spp_total > 2^34 with area lights (the keys' 34 bits); spp_count x (max_path_vertices - 1) > 4096 with
 *     either kind of light (one term per entry of every bounce).
 *   Per bounce: the delta stage (if any), a kernel that writes the keys, the area stage over the bounce's entries -- fused or materialised as
 *     for any caller (entries x narea x S >= 2^31: materialised), synchronous -- a kernel that folds the two values where there are both, the
 *     direct-light kernel, the sink.  With lh_accel_trace_statistics on `rays` advances by the closest-hit rays + hits x nlights + hits x
 *     narea x S.
 *   Memory a pass with area lights costs on top of the _lit forms', allocated at the first such call and kept by the accelerator: 8 bytes a
 *     path of keys, 12 of value, and the scratch of lh_accel_area_lights_device sized for every path hitting -- about 108 bytes a path (a
 *     96-byte hit record, key, slot) plus one byte per path, light and sample (56 more per shadow ray when the stage runs materialised):
 *     2.4 GB at 2^24 paths, one light and 16 samples.  The two stages compact a bounce each for itself; sharing that is a later change.
 * Not built: a texture multiply, the sky as the path tracer's environment, the multi-device and distributed frames, AreaLightSource /
 *   LightSource in the RIB reader, lsh_hip options, the qmc sampler. */
typedef struct lh_pt_lights {          /* 48 bytes */
    const lh_light_t *lights;   int32_t nlights; uint32_t reserved0; const lh_lights_params_t *params;       /* as the _lit forms take them */
    const lh_area_light_t *area; int32_t narea;  uint32_t reserved1; const lh_area_params_t *area_params;    /* as lh_accel_area_lights_device takes them */
} lh_pt_lights_t;
int  lh_render_pt_tile_lights(lh_accel_t *accel, const lh_camera_t *cam, int x0, int y0, int w, int h,
                              int spp_begin, int spp_count, int spp_total, int max_path_vertices, int flags,
                              const lh_pt_lights_t *lights, const lh_pt_sink_t *sink, uint64_t seed, void *d_rgb,
                              lh_pt_stats_t *stats, void *stream);
int  lh_render_pt_bands_lights(lh_accel_t *accel, const lh_camera_t *cam, int y0_first, int band_rows, int band_stride, int nbands,
                               int spp_begin, int spp_count, int spp_total, int max_path_vertices, int flags,
                               const lh_material_t *override_material, const lh_pt_lights_t *lights, const lh_pt_sink_t *sink,
                               uint64_t seed, void *d_rgb, lh_pt_stats_t *stats, void *stream);

/* ---- the whole hit epilogue: ri_intersection_state_build (src/render/intersection_state.c:99-248) ----
 * Optional per-vertex attributes of mesh `mesh`, before commit (geom.h:34-48): colours, tangents, binormals
 * (xyz, `count` = vertices), texture coordinates (s, t per vertex) or texcoords_unshared (s, t per INDEX: `count` =
 * indices).  lh_accel_state_build_*: for n rays and their hit records, LH_STATE_DOUBLES per ray --
 * P[3] Ng[3] Ns[3] tangent[3] binormal[3] color[3] st[2] I[3] inside -- in the reference's operation order (fp64,
 * no contraction); records of misses are left as they are (device) / zero (host). */
#define LH_ATTR_COLOR 0
#define LH_ATTR_TANGENT 1
#define LH_ATTR_BINORMAL 2
#define LH_ATTR_TEXCOORD 3
#define LH_ATTR_TEXCOORD_UNSHARED 4
#define LH_STATE_DOUBLES 24
int  lh_accel_set_attribute(lh_accel_t *accel, uint32_t mesh, int kind, const double *data, size_t stride_bytes, uint32_t count);
/* The same for meshes added with lh_accel_add_mesh_device, before commit (on an "updatable" accelerator after it as well: staged for
 * lh_accel_recommit, above); mesh = ordinal in add order.  d_normals / d_data are
 * device memory of the accelerator's device: 3 components per vertex (normals, colours, tangents, binormals), 2 per vertex
 * (LH_ATTR_TEXCOORD) or 2 per index (LH_ATTR_TEXCOORD_UNSHARED), as doubles (LH_POS_F64: stride_bytes >= 8 x components and a
 * multiple of 8, pointer 8-byte aligned) or floats (LH_POS_F32: >= 4 x components, a multiple of 4, 4-byte aligned; a value IS
 * (double)value).  nnormals / count must equal the mesh's npositions (the unshared kind: the nindices given at the add).
 *   - d_normals == NULL with nnormals == 0 sets two_side alone; a second call for a mesh and kind replaces the first; d_data ==
 *     NULL with count == 0 removes it.  Shared texture coordinates win over unshared ones, as on the host.
 *   - The array is read by a copy enqueued on `stream` before the call returns, into a block the library owns (the caller's format
 *     and stride): the caller may overwrite or free it in stream order afterwards.  lh_accel_commit waits through the per-stream
 *     events of the mesh copies (no device-wide synchronise) and gathers every mesh and kind with one kernel into the
 *     per-primitive arrays the hit epilogue, the AO stage and the path tracer read; a mesh lacking a kind another mesh has is
 *     "absent" there exactly as on the host path.  Values are not validated (a NaN normal means "no normal").  The blocks are freed
 *     when the commit returns, however it ends, and by lh_accel_destroy (an "updatable" accelerator keeps them until then).
 *   - Refused, -1 with lh_last_error, nothing enqueued, nothing changed: "accel is NULL"; "already committed"; an accelerator that
 *     holds host meshes or none ("for device meshes": the message names the host form); "mesh M out of range"; "unknown attribute
 *     kind"; "unknown format"; "bad stride"; "not aligned"; "NULL array" (with a non-zero count); "not a device pointer" /
 *     "extends past its allocation" (asked of the runtime, never dereferenced); "N values given, the mesh needs M". */
int  lh_accel_set_normals_device(lh_accel_t *accel, uint32_t mesh, uint32_t nnormals, const void *d_normals,
                                 int format /* LH_POS_F64 | LH_POS_F32 */, size_t stride_bytes, int two_side, void *stream);
int  lh_accel_set_attribute_device(lh_accel_t *accel, uint32_t mesh, int kind /* LH_ATTR_* */, uint32_t count,
                                   const void *d_data, int format, size_t stride_bytes, void *stream);
int  lh_accel_state_build_device(lh_accel_t *accel, size_t n, const void *d_org_xyz, const void *d_dir_xyz, const void *d_prim,
                                 const void *d_t, const void *d_u, const void *d_v, void *d_state, void *stream);
int  lh_accel_state_build_host(lh_accel_t *accel, size_t n, const double *org_xyz, const double *dir_xyz, const uint32_t *prim,
                               const double *t, const double *u, const double *v, double *state);

/* ---- the G GPUs of one node from ONE process ----
 * reference role: the bucket queue drained by render threads (src/render/render.c:1043-1207) and the compiled-out MPI
 * design "every rank renders, rank 0 owns the display" (render.c:468-514, src/base/parallel.c:62-232).  One host build,
 * replicated to every device; frames: a dynamic queue of tiles, one host thread per device, finished tile slabs copied
 * device-to-device (hipMemcpyPeerAsync, one xGMI link per peer) to device 0 = the display owner, which places them
 * (bucket_write's row order) and delivers the frame; ray dumps: contiguous slices.  `devices` may list a device more
 * than once (replicas on one GPU: how the sharded path is tested on a one-GPU box); NULL: devices 0 .. n-1
 * (ndevices <= 0: all).  device_seconds (ndevices doubles, may be NULL): busy time of each replica's tile loop. */
typedef struct lh_multi lh_multi_t;
int  lh_multi_create(lh_multi_t **out, int ndevices, const int *devices);
void lh_multi_destroy(lh_multi_t *multi);
int  lh_multi_ndevices(const lh_multi_t *multi);
lh_accel_t *lh_multi_accel(lh_multi_t *multi, int replica);          /* borrowed: queries on one replica */
int  lh_multi_add_mesh(lh_multi_t *multi, uint32_t npositions, const double *positions, size_t stride_bytes,
                       uint32_t nindices, const uint32_t *indices);
int  lh_multi_set_normals(lh_multi_t *multi, uint32_t mesh, const double *normals, size_t stride_bytes, int two_side);
int  lh_multi_add_rib_scene(lh_multi_t *multi, const lh_rib_scene_t *scene);
int  lh_multi_commit(lh_multi_t *multi, int build_threads);
int  lh_multi_set_material(lh_multi_t *multi, uint32_t mesh, const lh_material_t *material);
int  lh_multi_set_environment(lh_multi_t *multi, const lh_environment_t *environment);
/* lh_accel_set_texture on every replica (after lh_multi_commit, as the materials): lh_multi_render_ao_frame_host then renders textured frames */
int  lh_multi_set_texture(lh_multi_t *multi, uint32_t mesh /* or LH_ALL_MESHES */, const float *rgba, int width, int height);
int  lh_multi_intersect_host(lh_multi_t *multi, size_t n, const double *org_xyz, const double *dir_xyz, uint32_t *prim,
                             double *t, double *u, double *v, uint8_t *occluded, int mode);
int  lh_multi_render_ao_frame_host(lh_multi_t *multi, const lh_camera_t *cam, int pixel_samples, int gather_nsamples,
                                   uint64_t seed, int tile, float *rgb, lh_tile_stats_t *stats, double *device_seconds);
int  lh_multi_render_pt_frame_host(lh_multi_t *multi, const lh_camera_t *cam, int spp, int spp_chunk, int max_path_vertices,
                                   int flags, uint64_t seed, int tile, float *rgb, lh_pt_stats_t *stats, double *device_seconds);

/* ---- one process per GPU: lucille's compiled-out MPI layer over RCCL ----
 * reference: ri_parallel_init / _barrier / _bcast / _gather / _send / _recv (src/base/parallel.c:62-232) and the frame
 * protocol on top of it, "every rank renders, rank 0 owns the display" (src/render/render.c:468-514).  One lh_dist_t per
 * process = one rank = one GPU.  Scene load: ONE host build on rank 0, then ncclBroadcast of the flattened arrays into
 * every rank's HBM (lh_dist_broadcast_scene).  Frames: image space in interleaved bands, a rank's bands one device batch,
 * ONE exchange step -- ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd of the ranks' slabs to rank 0.  RCCL is loaded at
 * run time (librccl.so.1).  LH_DIST_SHM: the same interface over a POSIX shared-memory segment, for ranks that share a
 * device (RCCL refuses those): how the N > 1 path is tested on a one-GPU box.
 * Rendezvous: the caller distributes the 128-byte id of rank 0 (lh_dist_unique_id) by its own means (torch.distributed, MPI),
 * or names a file on a shared file system (lh_dist_init_file: a fresh path per job). */
typedef struct lh_dist lh_dist_t;
#define LH_DIST_ID_BYTES 128
#define LH_DIST_RCCL 0
#define LH_DIST_SHM  1
int  lh_dist_unique_id(void *id128);                                        /* rank 0: ncclGetUniqueId */
int  lh_dist_init(lh_dist_t **out, const void *id128, int rank, int world, int device, int transport);   /* ncclCommInitRank */
int  lh_dist_init_file(lh_dist_t **out, const char *rendezvous_path, int rank, int world, int device);
void lh_dist_destroy(lh_dist_t *dist);
int  lh_dist_rank(const lh_dist_t *dist);
int  lh_dist_world(const lh_dist_t *dist);
int  lh_dist_transport(const lh_dist_t *dist);
int  lh_dist_barrier(lh_dist_t *dist);
/* the ranks of ONE node meet in shared memory (microseconds; host only -- synchronise the device first): what brackets a timed
 * frame.  lh_dist_barrier goes through the transport (RCCL: a one-byte gather and broadcast) and works across nodes. */
int  lh_dist_host_barrier(lh_dist_t *dist);
/* device buffers; stream NULL: the communicator's own.  gather: d_recv (rank 0 only) holds world * bytes */
int  lh_dist_broadcast(lh_dist_t *dist, void *d_buf, size_t bytes, void *stream);
int  lh_dist_gather(lh_dist_t *dist, const void *d_send, size_t bytes, void *d_recv, void *stream);
/* hit records for the wire: n records (prim u32 | t | u | v f64, the arrays lh_accel_intersect_device wrote) -> n 16-byte records
 * {prim u32, t, u, v f32 rounded to nearest from the fp64 bits} in d_rec16 (device, 16-byte aligned).  A dump service that returns
 * every record to ONE host is bound by the xGMI links at 28 bytes a ray (8 ranks: 350 MB per peer against 5.4 ms of tracing);
 * 16 bytes keep the exchange behind the tracing.  The fp64 records stay with the rank that traced them; fp32 t / u / v are within
 * 6e-8 relative of them (north_star: 1e-5); a miss keeps prim 0xFFFFFFFF and t = 1e38.  No communicator needed. */
int  lh_dist_pack_records16(size_t n, const void *d_prim, const void *d_t, const void *d_u, const void *d_v, void *d_rec16, void *stream);
/* rank 0: a committed accelerator; the others: a fresh one (lh_accel_create), committed on return -- no build, no host
 * copy of the tree on those ranks (lh_accel_export and replicas of it are refused).  The image does not carry material textures:
 * every rank calls lh_accel_set_texture on its own accelerator after the broadcast (the setter is allowed after commit) */
int  lh_dist_broadcast_scene(lh_dist_t *dist, lh_accel_t *accel);
/* the AO frame sharded over the ranks: bands of band_rows lines (<= 0: 16), dealt out in serpentine order (groups of `world`
 * bands, even groups in rank order, odd groups reversed: a steady change of cost down the image cancels); rgb (rank 0 only): height
 * rows of width RGB floats, top row first; stats: the frame's totals on rank 0, the rank's own elsewhere */
int  lh_dist_render_ao_frame_host(lh_dist_t *dist, lh_accel_t *accel, const lh_camera_t *cam, int pixel_samples,
                                  int gather_nsamples, uint64_t seed, int band_rows, float *rgb, lh_tile_stats_t *stats);

/* device scratch of the last lh_render_ao_tile call (for tests / pipelines):
 * which: 0 primary org, 1 primary dir, 2 prim, 3 t, 4 u, 5 v, 6 slot_of_sample,
 *        7 hit records (12 doubles: AO origin, tangent, binormal, Ns), 8 AO org, 9 AO dir,
 *        10 AO occluded */
int  lh_render_scratch(lh_accel_t *accel, int which, void **d_ptr, size_t *count);

/* ---- beam (frustum) visibility: ri_beam_set + ri_bvh_intersect_beam_visibility ----
 * reference: src/render/beam.c:331-465, src/render/bvh.c:612-667 (+ :1997-2281, :2435-2542,
 * :2648-2746), constants src/render/beam.h:27-29.  A beam is a common origin and 4 corner
 * directions (n x 4 x 3 doubles).  result[i]: LH_BEAM_MISS_COMPLETELY / _HIT_COMPLETELY /
 * _HIT_PARTIALLY exactly as the reference returns them (the answer depends on ITS tree, so the
 * query runs on the reference-order tree kept beside the traversal tree), or LH_BEAM_INVALID
 * where ri_beam_set returns -1 (corner directions straddle an octant, beam.c:352-376). */
#define LH_BEAM_MISS_COMPLETELY 0
#define LH_BEAM_HIT_COMPLETELY  1
#define LH_BEAM_HIT_PARTIALLY   2
#define LH_BEAM_INVALID        (-1)

int  lh_accel_beam_visibility_host(lh_accel_t *accel, size_t n, const double *org_xyz,
                                   const double *corner_dirs_xyz, int32_t *result);
int  lh_accel_beam_visibility_device(lh_accel_t *accel, size_t n, const void *d_org_xyz,
                                     const void *d_corner_dirs_xyz, void *d_result, void *stream);

/* The same queries for beams the CALLER has already set up with lucille's own ri_beam_set: what
 * ri_bvh_intersect_beam_visibility(accel, ri_beam_t *, user) / ri_bvh_intersect_beam(accel, ri_beam_t *, plane, user) are
 * handed (src/render/bvh.h:203-221).  lh_beam_set_t = the members of ri_beam_t (src/render/beam.h:45-84) those two walks read:
 * org, the four directions SCALED onto the plane at d = 1024 (beam.c:412-432), their cross products (beam.c:446-452), the
 * dominant axis and the direction signs (beam.c:381-403) -- taken as they are, nothing recomputed, so the answer is the
 * reference's for the beam it holds (integration/ri_accel_hip.c copies them out of the ri_beam_t).  invdir, d, t_max,
 * is_tetrahedron and the child beams are not read by either walk (t_max stays RI_INFINITY, beam.c:344). */
typedef struct lh_beam_set {
    double  org[3];
    double  dir[4][3];
    double  normal[4][3];
    int32_t dominant_axis;
    int32_t dirsign[3];
} lh_beam_set_t;

int  lh_accel_beam_visibility_set_host(lh_accel_t *accel, size_t n, const lh_beam_set_t *beams, int32_t *result);

/* ---- the beam-raster path: ri_beam_set + ri_raster_plane_setup + ri_bvh_intersect_beam ----
 * reference: src/render/bvh.c:544-609 (-> :2547-2643, :2315-2426, :2751-2820), src/render/beam.c:469-730,
 * src/render/raster.c:42-147,166-435, src/render/triangle.c:8-68.  The reference never calls this path and left it
 * unfinished; what it COMPUTES is reproduced bit for bit, quirks included (lh_beam.hip lists them): after the call the raster
 * plane's t array holds, per pixel of the window, the ray parameter of the LAST rasterised triangle that covered the pixel
 * in the reference's traversal order, 0.0 elsewhere (u, v, geom, index of ri_raster_plane_t are never written by the
 * reference either).  Like beam visibility it runs on the reference-order tree.
 *   plane:   the raster window shared by the batch -- width x height pixels, frame = du dv dw (raster.h:38), eye =
 *            plane->org, fov in degrees;
 *   corner:  n x 3, the lower-left corner of every beam's window (plane->corner; the testbed shifts it per beam,
 *            simplerender.cpp:703-720);
 *   t_out:   n x height x width doubles; written for status 0 only;
 *   status:  0 traced; 1 nothing done (empty scene or the beam misses the scene box: the reference returns before it clears
 *            the plane, bvh.c:560-563,586-593); LH_BEAM_INVALID where ri_beam_set refuses the beam;
 *   flags:   n x 4 u64 or NULL -- what is UNDEFINED in the reference, reported instead of reproduced: [0] pixel tests outside
 *            the window (the reference writes plane->t[t * width + s] unchecked, raster.c:300-316; here the box is cut to the
 *            window), [1] / [2] the asserts of beam.c:142 / :626 would have fired, [3] triangles rasterised. */
typedef struct lh_raster_plane {
    int32_t width, height;
    double  frame[9];
    double  eye[3];
    double  fov;
} lh_raster_plane_t;

int  lh_accel_beam_raster_host(lh_accel_t *accel, size_t n, const double *org_xyz, const double *corner_dirs_xyz,
                               const double *corner_xyz, const lh_raster_plane_t *plane, double *t_out,
                               int32_t *status, uint64_t *flags);
int  lh_accel_beam_raster_device(lh_accel_t *accel, size_t n, const void *d_org_xyz, const void *d_corner_dirs_xyz,
                                 const void *d_corner_xyz, const lh_raster_plane_t *plane, void *d_t_out,
                                 void *d_status, void *d_flags, void *stream);
/* ... for beams already set up by the caller's ri_beam_set (lh_beam_set_t above); status is never LH_BEAM_INVALID */
int  lh_accel_beam_raster_set_host(lh_accel_t *accel, size_t n, const lh_beam_set_t *beams, const double *corner_xyz,
                                   const lh_raster_plane_t *plane, double *t_out, int32_t *status, uint64_t *flags);

/* whole AO frame into HOST memory: the tile loop of render_frame_controller + bucket_write
 * (src/render/render.c:1168-1207, 919-983) over lh_render_ao_tile.  rgb: height rows of width RGB
 * float triples, top row first (bucket_write's y flip applied) -- what the reference hands its
 * display driver.  tile = tile edge in pixels (0: the largest power of two <= 4096 whose per-tile scratch stays under ~6 GB).
 * stats may be NULL. */
int  lh_render_ao_frame_host(lh_accel_t *accel, const lh_camera_t *cam, int pixel_samples,
                             int gather_nsamples, uint64_t seed, int tile, float *rgb,
                             lh_tile_stats_t *stats);

/* ---- RIB-subset reader + Radiance .hdr writer: `lsh scene.rib` without flex/bison ----
 * reference: the RenderMan front end for the verbs its example scenes use --
 * src/ri/transform.c, context.c, attribute.c, camera.c:209-240,360-438, display.c:70-200,
 * option.c:430-560, src/render/polygon.c:39-262,495-640, src/base/matrix.c, quaternion.c; numbers
 * are C floats as in src/lsh/lexrib.l:213 / parserib.y:119.  The result is what lucille's renderer
 * is handed: the ri_geom_t list (world-space double[4] positions / normals, triangle indices,
 * two_side) in RIB order -- same global primitive ids -- and the camera.  Verbs outside the
 * ray-query path (shaders, lights, colours, quadrics ...) are skipped and counted. */
typedef struct lh_rib_info {
    uint32_t    nmeshes;
    uint64_t    ntriangles;
    lh_camera_t camera;           /* ri_camera_setup (camera.c:209-240) of the parsed state       */
    int         perspective;      /* 0: no Projection "perspective" "fov" seen (reference: ortho)  */
    float       fov;
    int         pixel_samples[2]; /* PixelSamples (context.c:210-222)                              */
    int         gather_nsamples;  /* Option "gather" "nsamples" (option.c:545-549), default 64     */
    int         accel_method;     /* Option "raytrace" "accel_method": 0 grid, 1 bvh, 2 hip        */
    int         nthreads;
    int         world_complete;   /* WorldBegin ... WorldEnd seen                                  */
    uint32_t    nskipped, nrequests;  /* requests outside the ray-query path / all requests      */
    uint32_t    nunknown;             /* of the skipped: not RenderMan requests at all           */
    char        display_name[1024];   /* after display.c's extension rule (".hdr")                */
    char        display_type[64];
} lh_rib_info_t;

int  lh_rib_load(const char *path, lh_rib_scene_t **scene_out);   /* 0 / -1 (lh_rib_last_error) */
void lh_rib_free(lh_rib_scene_t *scene);
const char *lh_rib_last_error(void);
int  lh_rib_info(const lh_rib_scene_t *scene, lh_rib_info_t *info);
/* parse diagnostics, one per line, as `lsh` prints them to stdout ("Unknown RIB command: X") */
const char *lh_rib_messages(const lh_rib_scene_t *scene);
/* borrowed pointers into the scene: positions/normals are npositions x double[4] (normals may be
 * NULL), indices are triangle corners (3 per primitive) */
int  lh_rib_mesh(const lh_rib_scene_t *scene, uint32_t mesh, uint32_t *npositions,
                 const double **positions, uint32_t *nindices, const uint32_t **indices,
                 const double **normals, int *two_side);
/* meshes (+ normals) of a parsed scene into an accelerator, in order; the caller commits */
int  lh_accel_add_rib_scene(lh_accel_t *accel, const lh_rib_scene_t *scene);
/* Radiance RGBE, run-length coded, byte-compatible with the reference's "file" display driver
 * (src/display/hdrdrv.c:38-121, src/imageio/rgbe.c:78-96,118-140,241-345); rgb as above */
int  lh_hdr_write(const char *path, int width, int height, const float *rgb);

/* ---- synthetic workloads (BASELINE configs 3 and 5): input generation only ----
 * One xorshift64 stream (*state; shifts 13/7/17; seed 88172645463325252): triangles first, the ray
 * dump continues it.  positions_xyz: 9 doubles per triangle (packed xyz), indices: identity.
 * lh_synth_tessellate: midpoint subdivision, triangle i -> 4i..4i+3, tri_out holds
 * ntriangles * 4^levels * 9 doubles. */
#define LH_SYNTH_SEED 88172645463325252ULL
void lh_synth_soup_triangles(uint64_t *state, uint32_t ntriangles, double half_extent,
                             double *positions_xyz, uint32_t *indices);
void lh_synth_soup_rays(uint64_t *state, size_t n, double *org_xyz, double *dir_xyz);
/* advance the stream by ndraws uniforms without producing them (a triangle is 12 draws, a ray 5):
 * how a rank that owns a slice of a ray dump reaches its first ray */
void lh_synth_skip(uint64_t *state, uint64_t ndraws);
void lh_synth_tessellate(const double *tri_in, size_t ntriangles, int levels, double *tri_out);

/* copy of the flattened BVH for cross-checks (tests): sizes via lh_accel_info.
 * nodes: nnodes*64 bytes, tri32: ntriangles*48 bytes; either may be NULL. */
int  lh_accel_export(const lh_accel_t *accel, void *nodes, void *tri32);

#ifdef __cplusplus
}
#endif
#endif

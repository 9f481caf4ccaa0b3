/*
 * lh_flatten.hip -- meshes that live on the device (lh_accel_add_mesh_device) -> the 72-byte fp64 triangle records, in primitive-id
 * order, that both device builders read (lh_build.hip, lh_refbuild.hip).  The device-side twin of lh_bvh_flatten (lh_bvh.c;
 * reference: create_triangle_list, src/render/bvh.c:1736-1826: geoms in list order, triangles in index order).
 *
 * A pure bandwidth kernel: 12 bytes of indices read and 72 bytes written per triangle, three dependent vertex gathers.  One lane
 * per (triangle, corner): lane e reads index e of the concatenated index lists (a wave reads 256 contiguous bytes within a mesh)
 * and stores the 24 bytes at 24 e (a wave writes 1536 contiguous bytes).  ONE launch covers every mesh: a lane finds its mesh by
 * a binary search of the first_prim table, narrowed per workgroup to the meshes its 256 corners touch -- a workgroup inside one
 * large mesh does not search at all, a RIB scene of thousands of small meshes searches among the few a workgroup spans.
 *
 * k_gather_attributes is the same walk over the corners for what the meshes carry beside positions (lh_accel_set_normals_device,
 * lh_accel_set_attribute_device): per-vertex values -> the per-primitive arrays the hit epilogue, the AO stage and the path tracer
 * read.  The device-side twin of the loops of host_build (lh_commit.hip) that fill nrm9, attr9, st6 and inside.
 */
#include "lh_internal.h"

/* the mesh holding primitive p: the g in [lo, hi) with first[g] <= p < first[g + 1] (first[lo] <= p < first[hi] on entry; empty
 * meshes repeat their neighbour's entry and are never the answer) */
static __device__ __forceinline__ uint32_t mesh_of_prim(const uint32_t *__restrict__ first, uint32_t lo, uint32_t hi, uint32_t p)
{
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (first[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

/* status[0]: 0, or 1 once a lane has met an index >= npositions; that lane alone then writes [1] mesh, [2] index, [3] npositions */
__global__ __launch_bounds__(256) void k_flatten_meshes(uint32_t ntris, uint32_t nmeshes, const lh_dmesh_desc_t *__restrict__ desc,
                                                        const uint32_t *__restrict__ first, double *__restrict__ tri64,
                                                        uint32_t *__restrict__ status)
{
    __shared__ uint32_t s_g[2];
    const unsigned long long ncorners = 3ull * ntris;
    const unsigned long long e0 = (unsigned long long)blockIdx.x * 256ull, e = e0 + threadIdx.x;
    if (threadIdx.x < 2u) {            /* the meshes of the workgroup's first and last corner */
        const unsigned long long el = threadIdx.x == 0u ? e0 : (e0 + 255ull < ncorners ? e0 + 255ull : ncorners - 1ull);
        s_g[threadIdx.x] = mesh_of_prim(first, 0u, nmeshes, (uint32_t)(el / 3ull));
    }
    __syncthreads();
    if (e >= ncorners) return;
    const uint32_t p = (uint32_t)(e / 3ull);
    const uint32_t g = mesh_of_prim(first, s_g[0], s_g[1] + 1u, p);
    const lh_dmesh_desc_t m = desc[g];
    const uint32_t vi = m.idx[e - 3ull * first[g]];          /* corner e of the scene = index e - 3 first_prim[g] of mesh g */
    if (vi >= m.npos) {                                      /* nothing is addressed with it: the commit reports it */
        if (atomicCAS(&status[0], 0u, 1u) == 0u) { status[1] = g; status[2] = vi; status[3] = m.npos; }
        return;
    }
    const char *v = (const char *)m.pos + (size_t)vi * m.stride;
    double x, y, z;
    if (m.fmt == LH_POS_F32) { const float *f = (const float *)v; x = (double)f[0]; y = (double)f[1]; z = (double)f[2]; }
    else { const double *d = (const double *)v; x = d[0]; y = d[1]; z = d[2]; }
    double *o = tri64 + 3ull * e;
    o[0] = x; o[1] = y; o[2] = z;
}

/* enqueues the launch on `stream`; desc / first (nmeshes descriptors, nmeshes + 1 running triangle counts) and status (4 words,
 * zeroed by the caller) are device memory; ntris in [1, 2^29): 3 ntris corners in 64-bit arithmetic, at most 6.3 M workgroups */
int lh_flatten_launch(uint32_t ntris, uint32_t nmeshes, const lh_dmesh_desc_t *d_desc, const uint32_t *d_first, void *d_tri64,
                      uint32_t *d_status, hipStream_t stream)
{
    if (ntris == 0u || nmeshes == 0u) return 0;
    if (ntris >= (1u << 29)) return fail("lh_flatten_launch: %u triangles (the limit is 2^29)", ntris);
    const unsigned long long nblocks = (3ull * ntris + 255ull) / 256ull;
    hipLaunchKernelGGL(k_flatten_meshes, dim3((unsigned)nblocks), dim3(256), 0, stream, ntris, nmeshes, d_desc, d_first,
                       (double *)d_tri64, d_status);
    HIPCHK(hipGetLastError());
    return 0;
}

static __device__ __forceinline__ double gather_component(const char *v, bool f32, int k)
{
    return f32 ? (double)((const float *)v)[k] : ((const double *)v)[k];
}

/* Per-vertex normals, colours, tangents, binormals and texture coordinates -> the 9- and 6-double-per-primitive arrays, and the
 * `inside` byte.  One launch for every mesh and every kind the scene has; one lane per (triangle, corner): lane e reads index e
 * once and, for each array present, stores that vertex's value at 24 e (xyz; a wave writes 1536 contiguous bytes) or 16 e (st;
 * 1024).  A mesh that lacks a kind another mesh has gets NaN there, the host path's "absent".
 *
 * INVARIANT: launched only after k_flatten_meshes has returned a clean status for the same tables, so every index read here is
 * below its mesh's npositions, and every per-vertex array holds npositions elements (the unshared one: nindices >= 3 ntris,
 * addressed by the corner itself): no lane forms an address from an unchecked index.  Values are not validated: a NaN normal
 * means "no normal" to the consumers, as on the host path. */
__global__ __launch_bounds__(256) void k_gather_attributes(uint32_t ntris, uint32_t nmeshes, const lh_dmesh_desc_t *__restrict__ desc,
                                                           const lh_dmesh_attr_desc_t *__restrict__ attr,
                                                           const uint32_t *__restrict__ first, lh_gather_out_t out)
{
    __shared__ uint32_t s_g[2];
    const unsigned long long ncorners = 3ull * ntris;
    const unsigned long long e0 = (unsigned long long)blockIdx.x * 256ull, e = e0 + threadIdx.x;
    if (threadIdx.x < 2u) {            /* the meshes of the workgroup's first and last corner */
        const unsigned long long el = threadIdx.x == 0u ? e0 : (e0 + 255ull < ncorners ? e0 + 255ull : ncorners - 1ull);
        s_g[threadIdx.x] = mesh_of_prim(first, 0u, nmeshes, (uint32_t)(el / 3ull));
    }
    __syncthreads();
    if (e >= ncorners) return;
    const uint32_t p = (uint32_t)(e / 3ull);
    const uint32_t g = mesh_of_prim(first, s_g[0], s_g[1] + 1u, p);
    const lh_dmesh_attr_desc_t *__restrict__ m = &attr[g];
    const unsigned long long le = e - 3ull * first[g];       /* the corner within its mesh = lucille's prim_index + corner */
    const uint32_t vi = desc[g].idx[le];                     /* < npositions: see INVARIANT */
    const uint32_t f32 = m->f32_mask;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double *const xyz_out[4] = {out.attr9[0], out.attr9[1], out.attr9[2], out.nrm9};
    const int xyz_slot[4] = {0, 1, 2, LH_DATTR_NORMAL};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (!xyz_out[k]) continue;
        const int s = xyz_slot[k];
        double x = nan, y = nan, z = nan;
        const char *d = (const char *)m->data[s];
        if (d) {
            const char *v = d + (size_t)vi * m->stride[s];
            const bool f = (f32 >> s) & 1u;
            x = gather_component(v, f, 0); y = gather_component(v, f, 1); z = gather_component(v, f, 2);
        }
        double *o = xyz_out[k] + 3ull * e;
        o[0] = x; o[1] = y; o[2] = z;
    }
    if (out.st6) {
        double2 st = make_double2(nan, nan);
        const char *sh = (const char *)m->data[3], *un = (const char *)m->data[4];
        if (sh) {                                  /* shared texcoords win over unshared ones */
            const char *v = sh + (size_t)vi * m->stride[3];
            st.x = gather_component(v, (f32 >> 3) & 1u, 0); st.y = gather_component(v, (f32 >> 3) & 1u, 1);
        } else if (un) {                           /* one per index: addressed by the corner, not the vertex */
            const char *v = un + (size_t)le * m->stride[4];
            st.x = gather_component(v, (f32 >> 4) & 1u, 0); st.y = gather_component(v, (f32 >> 4) & 1u, 1);
        }
        *(double2 *)(out.st6 + 2ull * e) = st;     /* 16 bytes at 16 e: aligned, the array comes from hipMalloc */
    }
    if (out.inside && le % 3ull == 0ull)           /* the back faces of a two_side mesh are its second half (prim_index >= nindices / 2) */
        out.inside[p] = (m->two_side && le >= (unsigned long long)(m->nidx / 2u)) ? 1 : 0;
}

/* enqueues the launch on `stream`; the tables are device memory as for lh_flatten_launch, which has run on them with a clean status */
int lh_gather_launch(uint32_t ntris, uint32_t nmeshes, const lh_dmesh_desc_t *d_desc, const lh_dmesh_attr_desc_t *d_attr, const uint32_t *d_first,
                     lh_gather_out_t out, hipStream_t stream)
{
    if (ntris == 0u || nmeshes == 0u) return 0;
    if (ntris >= (1u << 29)) return fail("lh_gather_launch: %u triangles (the limit is 2^29)", ntris);
    const unsigned long long nblocks = (3ull * ntris + 255ull) / 256ull;
    hipLaunchKernelGGL(k_gather_attributes, dim3((unsigned)nblocks), dim3(256), 0, stream, ntris, nmeshes, d_desc, d_attr, d_first, out);
    HIPCHK(hipGetLastError());
    return 0;
}

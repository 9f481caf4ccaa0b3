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

/*
 * lh_render.hip -- the callers on either side of the ray query, batched per tile
 * and kept on the device: camera rays, hit epilogue, ambient-occlusion ray
 * producer and the radiance reduction.
 *
 * Reference (CPU, one pixel / one ray at a time):
 *   subsample + sample_subpixel        src/render/render.c:715-861
 *   ri_camera_get_pos_and_dir          src/ri/camera.c:248-318
 *   ri_intersection_state_build        src/render/intersection_state.c:99-248
 *   ri_ortho_basis                     src/render/reflection.c:311-333
 *   calculate_occlusion,
 *     ri_transport_ambientocclusion    src/transport/ambientocclusion.c:42-151,332-415
 *   render_bucket / bucket_write       src/render/render.c:1107-1166,919-983
 *
 * Wavefront pipeline of one tile (all buffers resident in HBM, no host round trip
 * except one 8-byte hit count):
 *
 *   k_primary_rays  -> [trace closest] -> k_hit_count / k_scan_blocks / k_ao_setup
 *                   -> k_ao_rays -> [trace any] -> k_ao_resolve
 *
 * All geometry arithmetic is fp64 with the reference's operation order and no FMA
 * contraction, so primary rays, P, Ng, Ns and the basis equal the oracle's bits;
 * AO directions use a counter-based RNG by default (the reference's MT19937 stream
 * is order-dependent) or caller-supplied uniforms (parity replay), and the device
 * libm's sin/cos.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/lucille_hip.h"
#include "lh_internal.h"
#include "lh_ao.h"
#include "lh_dirt.h"
#include "lh_env.h"
#include "lh_sky.h"
#include "lh_lights.h"
#include "lh_ptl.h"
#include "lh_area.h"
#include "lh_tex.h"

namespace {

#include "lh_pt.h"
#include "lh_shade.h"

/* the pixels of one device batch: nbands full-rows-of-w bands of band_rows lines each, band b starting at frame line
 * band_y0[b] (or y0 when there is a single band: a plain rectangle).  Pixel index p of the batch: band = p / (w * band_rows),
 * line = (p / w) % band_rows, column = p % w.  A rank's interleaved shards of a frame are ONE such batch: one set of kernel
 * launches -- and one kernel drain, ~1.7 ms on BASELINE config 5 where a few grazing AO rays walk thousands of floor boxes
 * (profiles/README.md r02c) -- per frame instead of one per shard.  Lines >= height (a ragged last band) produce rays that
 * start far outside the scene and miss. */
struct Region {
    int x0, w, band_rows, nbands, height, y0;
    const int *band_y0;
};

/* 32-bit index arithmetic: a batch holds fewer than 2^32 samples (checked by the callers); the 64-bit divisions by run-time values
 * that stood here cost ~100 instructions each, five per thread of k_primary_rays and k_ao_setup */
__device__ __forceinline__ void region_pixel(const Region &rg, uint32_t pix, int &px, int &py)
{
    const uint32_t per = (uint32_t)rg.w * (uint32_t)rg.band_rows;
    const uint32_t band = pix / per, within = pix - band * per;
    const uint32_t line = within / (uint32_t)rg.w;
    px = rg.x0 + (int)(within - line * (uint32_t)rg.w);
    py = (rg.band_y0 ? rg.band_y0[band] : rg.y0) + (int)line;
}

/* radical inverse permutation of init_sigma (render.c:870-917) */
__device__ __forceinline__ unsigned sigma_of(unsigned i, unsigned period)
{
    unsigned digit = period, inverse = 0;
    for (unsigned bits = i; bits; bits >>= 1) { digit >>= 1; if (bits & 1) inverse += digit; }
    return inverse;
}

/* one thread per pixel sub-sample: sample id = ((ly*w + lx)*ys + sy)*xs + sx */
__global__ void k_primary_rays(DevCamera cam, Region rg, int xs, int ys,
                               double *__restrict__ org, double *__restrict__ dir)
{
    LH_NC
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)rg.w * rg.band_rows * rg.nbands * xs * ys;
    if (id >= total) return;
    const uint32_t id32 = (uint32_t)id, pix = id32 / (uint32_t)(xs * ys), sub = id32 - pix * (uint32_t)(xs * ys);
    const int sy = (int)(sub / (uint32_t)xs), sx = (int)(sub - (uint32_t)sy * (uint32_t)xs);
    int px, py;
    region_pixel(rg, pix, px, py);
    if (py >= rg.height) {          /* below the frame (ragged last band): a ray that misses everything */
        org[3 * id] = 1.0e30; org[3 * id + 1] = 1.0e30; org[3 * id + 2] = 1.0e30;
        dir[3 * id] = 1.0; dir[3 * id + 1] = 1.0; dir[3 * id + 2] = 1.0;
        return;
    }
    /* sample_subpixel (render.c:830-861) */
    const unsigned j = (unsigned)sx & ((unsigned)xs - 1), k = (unsigned)sy & ((unsigned)xs - 1);
    double jx = (double)sx + (double)sigma_of(k, (unsigned)xs) / (double)xs;
    double jy = (double)sy + (double)sigma_of(j, (unsigned)ys) / (double)ys;
    jx /= (double)xs; jy /= (double)ys;
    jx += 0.5 / (xs * xs); jy += 0.5 / (ys * ys);
    /* ri_camera_get_pos_and_dir (camera.c:248-318) */
    const double x = (double)(px + jx), y = (double)(py + jy);
    const double W = cam.width, H = cam.height;
    const float sign = cam.rh ? -1.0f : 1.0f;
    double v[4], o[4] = {0.0, 0.0, 0.0, 1.0}, pos[4], dp[4];
    v[0] = (2.0f * x - W) / W; v[1] = (2.0f * y - H) / H; v[2] = sign * cam.flength; v[3] = 1.0;
    if (cam.ortho) { o[0] = v[0]; o[1] = v[1]; v[2] = sign * 1.0; }      /* camera.c:285-301 */
    for (int c = 0; c < 4; c++) {
        pos[c] = 0.0; dp[c] = 0.0;
        for (int r = 0; r < 4; r++) { pos[c] += o[r] * cam.c2w[4 * r + c]; dp[c] += v[r] * cam.c2w[4 * r + c]; }
    }
    double d[3] = {dp[0] - pos[0], dp[1] - pos[1], dp[2] - pos[2]};
    vnormalize(d);
    org[3 * id] = pos[0]; org[3 * id + 1] = pos[1]; org[3 * id + 2] = pos[2];
    dir[3 * id] = d[0]; dir[3 * id + 1] = d[1]; dir[3 * id + 2] = d[2];
}

/* ---- deterministic compaction of the primary hits (sample order) ---------- */
__global__ void k_hit_count(size_t n, const uint32_t *__restrict__ prim, uint32_t *__restrict__ block_counts)
{
    __shared__ uint32_t wsum[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool hit = (i < n) && (prim[i] != LH_MISS_PRIM);
    const unsigned long long m = __ballot(hit);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

/* exclusive scan of block_counts in place (one workgroup); total -> *total_out */
__global__ void k_scan_blocks(uint32_t nblocks, uint32_t *__restrict__ block_counts, unsigned long long *total_out)
{
    __shared__ uint32_t part[1024];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nblocks; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = (i < nblocks) ? block_counts[i] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (uint32_t off = 1; off < 1024; off <<= 1) {
            uint32_t t = (threadIdx.x >= off) ? part[threadIdx.x - off] : 0;
            __syncthreads();
            part[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < nblocks) block_counts[i] = carry + part[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += part[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total_out = carry;
}

struct DevNormals { const double *nrm; };   /* 9 doubles per prim (n0 n1 n2), NaN n0.x => none */

/* the hit epilogue of one AO slot, written once for k_ao_setup (a Region's samples) and k_ao_batch_setup (a caller's batch): the
 * 12-double hit record of `slot` for ray i of the arrays, and the self-primitive bits of the slot's key (its low 34 bits are the caller's).
 * eps: the origin's offset along Ns -- 1e-6 for ambient occlusion (ambientocclusion.c:65-73), the dirt stage's own (lh_dirt.h) */
__device__ __forceinline__ void ao_hit_epilogue(const void *tri64, const double *nrm9,
                                                const double *org, const double *dir,
                                                const uint32_t *prim, const double *t,
                                                const double *u, const double *v, size_t i,
                                                double *hitrec, unsigned long long *slot_key, uint32_t slot, const double eps)
{
    LH_NC
    /* ri_intersection_state_build (intersection_state.c:99-248): P, Ng, Ns */
    const uint32_t p = prim[i];
    const double *tv = (const double *)tri64 + 9 * (size_t)p;
    const double tt = t[i], uu = u[i], vv = v[i];
    double P[3], Ng[3], Ns[3], v01[3], v02[3];
    for (int k = 0; k < 3; k++) P[k] = org[3 * i + k] + dir[3 * i + k] * tt;
    for (int k = 0; k < 3; k++) { v01[k] = tv[3 + k] - tv[k]; v02[k] = tv[6 + k] - tv[k]; }
    vcross(Ng, v01, v02); vnormalize(Ng);
    bool has_n = false;
    if (nrm9) { const double n0x = nrm9[9 * (size_t)p]; has_n = (n0x == n0x); }
    if (has_n) {
        const double *nn = nrm9 + 9 * (size_t)p; const double w = 1.0 - uu - vv;
        for (int k = 0; k < 3; k++) { const double a = nn[k] * w, b = nn[3 + k] * uu, c = nn[6 + k] * vv; Ns[k] = (a + b) + c; }
    } else {
        Ns[0] = Ng[0]; Ns[1] = Ng[1]; Ns[2] = Ng[2];
    }
    /* flat-shaded: the origin triangle cannot occlude its own AO rays (lh_ao.h) -- unless it is degenerate (Ng = 0), or the offset is
     * smaller than the one that argument rests on */
    const bool noself = !has_n && (Ng[0] != 0.0 || Ng[1] != 0.0 || Ng[2] != 0.0) && lh_dirt_selfskip(eps);
    slot_key[slot] |= (unsigned long long)(noself ? p : LH_SLOT_NOSELF) << LH_SLOTKEY_BITS;
    /* ri_ortho_basis(basis, Ns) (reflection.c:311-333) and the offset (ambientocclusion.c:65-73: 1e-6; dirtmap.c:98: 1e-5) */
    double b0[3], b1[3] = {0.0, 0.0, 0.0};
    int ax = 3;
    for (int k = 0; k < 3; k++) if (Ns[k] < 0.6 && Ns[k] > -0.6) { ax = k; break; }
    if (ax >= 3) ax = 0;
    b1[ax] = 1.0;
    vcross(b0, b1, Ns); vnormalize(b0);
    vcross(b1, Ns, b0); vnormalize(b1);
    double *r = hitrec + 12 * (size_t)slot;
    for (int k = 0; k < 3; k++) { r[k] = P[k] + Ns[k] * eps; r[3 + k] = b0[k]; r[6 + k] = b1[k]; r[9 + k] = Ns[k]; }
}

/* one thread per primary sample: slot = exclusive scan of the hit flags; writes the
 * per-hit record {org(3), basis(9)} (12 doubles) and slot_of_sample.  EPS: the offset is the argument (the dirt stage); false: AO's
 * constant 1e-6, the kernel the AO pipeline always ran (the argument cost it two VGPRs) */
template <bool EPS>
__global__ void k_ao_setup(size_t n, const lh_dev_scene_t sc, const double *__restrict__ nrm9,
                           const double *__restrict__ org, const double *__restrict__ dir,
                           const uint32_t *__restrict__ prim, const double *__restrict__ t,
                           const double *__restrict__ u, const double *__restrict__ v,
                           const uint32_t *__restrict__ block_offsets, uint32_t *__restrict__ slot_of_sample,
                           double *__restrict__ hitrec, unsigned long long *__restrict__ slot_key,
                           const Region rg, int spp, int full_width, const double eps)
{
    LH_NC
    __shared__ uint32_t wsum[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool hit = (i < n) && (prim[i] != LH_MISS_PRIM);
    const unsigned long long m = __ballot(hit);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) wsum[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t woff = 0;
    for (int k = 0; k < wv; k++) woff += wsum[k];
    if (i < n) slot_of_sample[i] = LH_MISS_PRIM;
    if (!hit) return;
    const uint32_t slot = block_offsets[blockIdx.x] + woff + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    slot_of_sample[i] = slot;
    {   /* absolute sample key (frame position, not tile position): keeps the built-in
         * RNG independent of how the frame is tiled or sharded */
        int ipx, ipy;
        const uint32_t i32 = (uint32_t)i, ipix = i32 / (uint32_t)spp;
        region_pixel(rg, ipix, ipx, ipy);
        const unsigned long long px = (unsigned long long)ipx, py = (unsigned long long)ipy;
        slot_key[slot] = (py * (unsigned long long)full_width + px) * (unsigned long long)spp + (i32 - ipix * (uint32_t)spp);      /* < 2^34: checked by the caller */
    }

    ao_hit_epilogue(sc.tri64, nrm9, org, dir, prim, t, u, v, i, hitrec, slot_key, slot, EPS ? eps : 1.0e-6);
}

/* counter-based uniforms in [0,1) with 32-bit resolution (like randomMT2's y*2^-32): lh_ao.h */
__device__ __forceinline__ uint32_t mix32(uint64_t x) { return lh_mix32(x); }

/* one thread per AO ray: ray id = slot*N + (j*ntheta + i) (calculate_occlusion's loop order).
 * rnd != NULL: the caller's uniforms (2 per ray), fp64 throughout -- the parity replay of the reference's
 * MT19937 stream.  rnd == NULL: the built-in generator of lh_ao.h -- bit for bit the rays the any-hit kernel
 * generates in its refill when the tile runs fused (this kernel is then only used to show them). */
__device__ __forceinline__ void ao_ray_item(size_t id, size_t nslots, int ntheta, int nphi, unsigned long long seed,
                                            const double *__restrict__ hitrec, const double *__restrict__ rnd /* 2 per ray or NULL */,
                                            const unsigned long long *__restrict__ slot_key, double *__restrict__ org, double *__restrict__ dir)
{
    LH_NC
    const int N = ntheta * nphi;
    if (id >= nslots * (size_t)N) return;
    const size_t slot = id / N; const int r = (int)(id % N);
    const double *h = hitrec + 12 * slot;
    if (!rnd) {
        double ox, oy, oz, dx, dy, dz;
        lh_ao_ray_builtin(h, slot_key[slot], seed, ntheta, nphi, r, ox, oy, oz, dx, dy, dz);
        org[3 * id] = ox; org[3 * id + 1] = oy; org[3 * id + 2] = oz;
        dir[3 * id] = dx; dir[3 * id + 1] = dy; dir[3 * id + 2] = dz;
        return;
    }
    const int i = r % ntheta, j = r / ntheta;
    const double r0 = rnd[2 * id], r1 = rnd[2 * id + 1];
    const double z0 = ((double)(uint32_t)i + r0) / (double)(uint32_t)ntheta;
    const double z1 = ((double)(uint32_t)j + r1) / (double)(uint32_t)nphi;
    const double cos_theta = sqrt(z0), phi = 2.0 * 3.14159265358979323846 * z1;
    double sp, cp;
    sincos(phi, &sp, &cp);
    const double d0 = cp * cos_theta, d1 = sp * cos_theta, d2 = sqrt(1.0 - cos_theta * cos_theta);
    for (int k = 0; k < 3; k++) {
        org[3 * id + k] = h[k];
        dir[3 * id + k] = d0 * h[3 + k] + d1 * h[6 + k] + d2 * h[9 + k];
    }
}

__global__ void k_ao_rays(size_t nslots, int ntheta, int nphi, unsigned long long seed,
                          const double *__restrict__ hitrec, const double *__restrict__ rnd,
                          const unsigned long long *__restrict__ slot_key, double *__restrict__ org, double *__restrict__ dir)
{
    ao_ray_item((size_t)blockIdx.x * blockDim.x + threadIdx.x, nslots, ntheta, nphi, seed, hitrec, rnd, slot_key, org, dir);
}

/* the same rays for a slot count that lives on the device (lh_accel_ao_rays_device reads nothing back): the grid covers the worst
 * case, the threads beyond *nslots_dev x N leave */
__global__ void k_ao_rays_counted(const unsigned long long *__restrict__ nslots_dev, int ntheta, int nphi, unsigned long long seed,
                                  const double *__restrict__ hitrec, const double *__restrict__ rnd,
                                  const unsigned long long *__restrict__ slot_key, double *__restrict__ org, double *__restrict__ dir)
{
    ao_ray_item((size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)*nslots_dev, ntheta, nphi, seed, hitrec, rnd, slot_key, org, dir);
}

/* ---- the material texture of a hit (lh_tex.h) ---- */
typedef lh_tex_args_t TexArgs;          /* lh_internal.h: what the textured resolves and k_tex_batch read; the launchers' callers fill it */

/* texcol of record i (a hit): false = its mesh has no texture (c is not written).  s, t: doubles 18 and 19 of k_state_build */
__device__ __forceinline__ bool tex_color(const TexArgs &tx, size_t i, double c[4])
{
    LH_NC
    const uint32_t p = tx.prim[i];
    const lh_tex_desc_t d = tx.table[tx.prim_mesh[p]];
    if (!d.texels) return false;
    double s = 0.0, t = 0.0;
    if (tx.st6) {
        const double *q = tx.st6 + 6 * (size_t)p;
        if (q[0] == q[0]) lh_tex_st(q, tx.u[i], tx.v[i], &s, &t);
    }
    lh_tex_fetch(d.texels, d.width, d.height, s, t, c);
    return true;
}

/* a workgroup's count into one of the 64 counters at `total`: one atomic per WORKGROUP -- atomics on one address are served one after the other
 * (~5 ns each); one per wave, 262 144 of them on a 4096^2 frame, were 1.2 of the 1.35 ms k_ao_resolve took */
__device__ __forceinline__ void wg_total(unsigned int n, unsigned long long *__restrict__ total)
{
    __shared__ unsigned int wsum[4];
    for (int off = 32; off > 0; off >>= 1) n += (unsigned int)__shfl_xor((int)n, off);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (tot) atomicAdd(total + (blockIdx.x & 63u), (unsigned long long)tot);
    }
}

/* where pixel pix of a batch of h = nbands * band_rows lines goes in rgb: every band is flipped within itself, as a tile is (bucket_write,
 * render.c:962-975: rgb[(h-1-ly)*w + lx]) */
__device__ __forceinline__ float *pixel_out(float *__restrict__ rgb, size_t pix, int w, int band_rows)
{
    const int lx = (int)(pix % w), line = (int)(pix / w), band = line / band_rows, ly = line % band_rows;
    return rgb + 3 * ((size_t)(band * band_rows + (band_rows - 1 - ly)) * w + lx);
}

/* what a hit slot is worth to the thread-per-pixel / thread-per-entry resolves, and the slot's count for the totals: the one expression in which the
 * transports' resolves differ, and so their template parameter.  AO: (N - occluded) / N, from the per-slot count of a fused stage or the N any-hit
 * bytes; dirt: lh_dirt_value over the N bounded t of the slot, in r order, and the bounded hits */
struct AoValue {
    int N; const uint8_t *__restrict__ occ; const unsigned int *__restrict__ occ_count;
    __device__ __forceinline__ double operator()(uint32_t slot, unsigned int &c) const
    {
        if (occ_count) c = occ_count[slot];            /* fused AO stage: occluded rays were counted per slot */
        else {
            const uint8_t *o = occ + (size_t)slot * (size_t)N;
            c = 0;
            for (int r = 0; r < N; r++) if (o[r]) c++;
        }
        const double ns = (double)(uint32_t)N, occlusion = (double)c;
        return 1.0 * (ns - occlusion) / ns;
    }
};
struct DirtValue {
    int N; double near_clip, far_clip; const double *__restrict__ tg;
    __device__ __forceinline__ double operator()(uint32_t slot, unsigned int &c) const
    {
        uint32_t k;
        const double val = lh_dirt_value(tg + (size_t)slot * (size_t)N, N, near_clip, far_clip, &k);
        c = k;
        return val;
    }
};

/* one thread per pixel: accumulates its sub-samples exactly like subsample() (render.c:749-822) and writes like bucket_write (pixel_out); a miss
 * gives 0, a hit its Value.  TEX: value[k] *= texcol[k] where the hit's mesh has a texture (ambientocclusion.c:393-401, dirtmap.c:273-281),
 * accumulated per channel; false: one float to the three channels, the kernels the pipelines ran before textures.  Returns the thread's count */
template <bool TEX, class Value>
__device__ __forceinline__ unsigned int tile_resolve(int w, int h, int band_rows, int xs, int ys, const Value &value, const uint32_t *__restrict__ slot_of_sample,
                                                     float *__restrict__ rgb, const TexArgs *tx)
{
    LH_NC
    const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool inside = pix < (size_t)w * h;
    double accum = 0.0, accum1 = 0.0, accum2 = 0.0;      /* (channels 1 and 2: TEX only) */
    unsigned int n = 0;
    const int S = inside ? xs * ys : 0;
    for (int s = 0; s < S; s++) {
        const uint32_t slot = slot_of_sample[pix * S + s];
        double val = 0.0;
        if (slot != LH_MISS_PRIM) {
            unsigned int c;
            val = value(slot, c);
            n += c;
        }
        if (TEX) {
            double c[4];
            if (slot != LH_MISS_PRIM && tex_color(*tx, pix * S + s, c)) { accum = accum + val * c[0]; accum1 = accum1 + val * c[1]; accum2 = accum2 + val * c[2]; }
            else { accum = accum + val; accum1 = accum1 + val; accum2 = accum2 + val; }
        } else
        accum = accum + val;
    }
    if (inside) {
        float f = (float)(accum * ((double)1.0 / (xs * ys)));
        if (f < 0.0f) f = 0.0f;
        float *o = pixel_out(rgb, pix, w, band_rows);
        o[0] = f; o[1] = f; o[2] = f;
        if (TEX) {
            float f1 = (float)(accum1 * ((double)1.0 / (xs * ys))), f2 = (float)(accum2 * ((double)1.0 / (xs * ys)));
            if (f1 < 0.0f) f1 = 0.0f;
            if (f2 < 0.0f) f2 = 0.0f;
            o[1] = f1; o[2] = f2;
        }
    }
    return n;
}

__global__ void k_ao_resolve(int w, int h, int band_rows, int xs, int ys, int N, const uint32_t *__restrict__ slot_of_sample,
                             const uint8_t *__restrict__ occ, const unsigned int *__restrict__ occ_count,
                             float *__restrict__ rgb, unsigned long long *__restrict__ occ_total)
{
    const unsigned int n = tile_resolve<false>(w, h, band_rows, xs, ys, AoValue{N, occ, occ_count}, slot_of_sample, rgb, NULL);
    if (occ_total) wg_total(n, occ_total);
}

__global__ void k_ao_resolve_tex(int w, int h, int band_rows, int xs, int ys, int N, const uint32_t *__restrict__ slot_of_sample,
                                 const uint8_t *__restrict__ occ, const unsigned int *__restrict__ occ_count,
                                 float *__restrict__ rgb, unsigned long long *__restrict__ occ_total, const TexArgs tx)
{
    const unsigned int n = tile_resolve<true>(w, h, band_rows, xs, ys, AoValue{N, occ, occ_count}, slot_of_sample, rgb, &tx);
    if (occ_total) wg_total(n, occ_total);
}

/* ---- the AO stage for a caller's batch of hit records (lh_accel_ao_device / lh_accel_ao_rays_device) ----------------
 * The samples of a Region become the entries of a list (lh_accel_intersect_device_indexed's: ids in `index` or the identity,
 * `count` on the device or all n_list of them); entry k is traced when k < min(*count, n_list) and its id < n_rays, and is a
 * hit when prim[id] != LH_MISS.  Hit slots number the hits in list order: the same ballot / block-scan compaction as above. */
struct BatchList {
    const uint32_t *index;      /* n_list ids, or NULL: the identity */
    const uint32_t *count;      /* entries to trace (clamped to n_list), or NULL: all */
    uint32_t n_list, n_rays;
};

/* 32-bit index arithmetic: n_list < 2^31 (checked by the callers) */
__device__ __forceinline__ bool batch_entry(const BatchList &bl, uint32_t k, uint32_t &id)
{
    uint32_t lim = bl.n_list;
    if (bl.count) { const uint32_t c = *bl.count; if (c < lim) lim = c; }
    if (k >= lim) return false;
    id = bl.index ? bl.index[k] : k;
    return id < bl.n_rays;
}

__global__ void k_ao_batch_count(const BatchList bl, const uint32_t *__restrict__ prim, uint32_t *__restrict__ block_counts)
{
    __shared__ uint32_t wsum[4];
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    uint32_t id = 0;
    const bool hit = batch_entry(bl, k, id) && (prim[id] != LH_MISS_PRIM);
    const unsigned long long m = __ballot(hit);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

/* k_ao_setup for a batch: one thread per list entry; slot_of_entry[k] = the entry's hit slot or LH_AO_NO_HIT, the hit record and
 * the slot key (the caller's key of the ray -- its id when key is NULL -- in the low 34 bits) through the same epilogue.
 * nslots_out (or NULL): the number of hits as one uint32, for a caller of lh_accel_ao_rays_device.  EPS: as for k_ao_setup */
template <bool EPS>
__global__ void k_ao_batch_setup(const BatchList bl, const lh_dev_scene_t sc, const double *__restrict__ nrm9,
                                 const double *__restrict__ org, const double *__restrict__ dir,
                                 const uint32_t *__restrict__ prim, const double *__restrict__ t,
                                 const double *__restrict__ u, const double *__restrict__ v,
                                 const unsigned long long *__restrict__ key,
                                 const uint32_t *__restrict__ block_offsets, const unsigned long long *__restrict__ total,
                                 uint32_t *__restrict__ slot_of_entry, double *__restrict__ hitrec,
                                 unsigned long long *__restrict__ slot_key, uint32_t *__restrict__ nslots_out, const double eps)
{
    LH_NC
    __shared__ uint32_t wsum[4];
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (nslots_out && k == 0) *nslots_out = (uint32_t)*total;
    uint32_t id = 0;
    const bool hit = batch_entry(bl, k, id) && (prim[id] != LH_MISS_PRIM);
    const unsigned long long m = __ballot(hit);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) wsum[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t woff = 0;
    for (int j = 0; j < wv; j++) woff += wsum[j];
    if (k < bl.n_list) slot_of_entry[k] = LH_AO_NO_HIT;
    if (!hit) return;
    const uint32_t slot = block_offsets[blockIdx.x] + woff + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    slot_of_entry[k] = slot;
    slot_key[slot] = (key ? key[id] : (unsigned long long)id) & LH_SLOTKEY_MASK;
    ao_hit_epilogue(sc.tri64, nrm9, org, dir, prim, t, u, v, (size_t)id, hitrec, slot_key, slot, EPS ? eps : 1.0e-6);
}

/* the resolve of a batch: one thread per list entry, the slot's Value and count -> count_out[id] / value_out[id] (either may be NULL); a traced miss
 * gets LH_AO_NO_HIT / 0.  slot_of_entry NULL: an empty scene, every traced ray is a miss.  The batch's count goes to the 64 counters of total */
template <class Value>
__device__ __forceinline__ void batch_resolve(const BatchList &bl, const Value &value, const uint32_t *__restrict__ slot_of_entry,
                                              uint32_t *__restrict__ count_out, float *__restrict__ value_out, unsigned long long *__restrict__ total)
{
    LH_NC
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    uint32_t id = 0;
    unsigned int n = 0;
    if (batch_entry(bl, k, id)) {
        const uint32_t slot = slot_of_entry ? slot_of_entry[k] : LH_AO_NO_HIT;
        uint32_t c = LH_AO_NO_HIT;
        float val = 0.0f;
        if (slot != LH_AO_NO_HIT) {
            val = (float)value(slot, n);
            c = n;
        }
        if (count_out) count_out[id] = c;
        if (value_out) value_out[id] = val;
    }
    wg_total(n, total);
}

/* ... of the AO stage: occluded_count[id] / radiance[id] */
__global__ void k_ao_batch_resolve(const BatchList bl, int N,
                                   const uint32_t *__restrict__ slot_of_entry, const uint8_t *__restrict__ occ,
                                   const unsigned int *__restrict__ occ_count, uint32_t *__restrict__ occluded_count,
                                   float *__restrict__ radiance, unsigned long long *__restrict__ occ_total)
{
    batch_resolve(bl, AoValue{N, occ, occ_count}, slot_of_entry, occluded_count, radiance, occ_total);
}

/* ---- the dirt stage (lh_dirt.h): the resolves read one double per gather ray -- the t of its bounded closest-hit record, at element
 * slot * N + r -- and apply the rule in r order; whoever traced the rays wrote that array and nothing else ------------------------ */

/* the bound of every gather ray of a materialised dirt stage: far_clip, where the bounded launch reads a bound per ray id */
__global__ void k_dirt_bounds(size_t n, double far_clip, double *__restrict__ bound)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) bound[i] = far_clip;
}

/* k_ao_resolve for the dirt tile: a miss gives 0, a hit its value (ri_transport_dirtmap, dirtmap.c:234-292) */
__global__ void k_dirt_resolve(int w, int h, int band_rows, int xs, int ys, int N, double near_clip, double far_clip,
                               const uint32_t *__restrict__ slot_of_sample, const double *__restrict__ tg,
                               float *__restrict__ rgb, unsigned long long *__restrict__ hit_total)
{
    wg_total(tile_resolve<false>(w, h, band_rows, xs, ys, DirtValue{N, near_clip, far_clip, tg}, slot_of_sample, rgb, NULL), hit_total);
}

__global__ void k_dirt_resolve_tex(int w, int h, int band_rows, int xs, int ys, int N, double near_clip, double far_clip,
                                   const uint32_t *__restrict__ slot_of_sample, const double *__restrict__ tg,
                                   float *__restrict__ rgb, unsigned long long *__restrict__ hit_total, const TexArgs tx)
{
    wg_total(tile_resolve<true>(w, h, band_rows, xs, ys, DirtValue{N, near_clip, far_clip, tg}, slot_of_sample, rgb, &tx), hit_total);
}

/* the fetch alone for a batch of hit records (lh_accel_texture_device): one thread per list entry, 4 doubles at rgba[4 * id] -- texcol, or
 * 1 1 1 1 where the hit's mesh has no texture, or four zeros for a traced miss.  tx.prim NULL: an empty scene, every traced ray is a
 * miss; a primitive id beyond the scene's counts as a miss too */
__global__ void k_tex_batch(const BatchList bl, const TexArgs tx, uint32_t ntris, double *__restrict__ rgba)
{
    LH_NC
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    uint32_t id = 0;
    if (!batch_entry(bl, k, id)) return;
    double c[4] = {0.0, 0.0, 0.0, 0.0};
    const uint32_t p = tx.prim ? tx.prim[id] : LH_MISS_PRIM;
    if (p < ntris && !tex_color(tx, (size_t)id, c)) { c[0] = 1.0; c[1] = 1.0; c[2] = 1.0; c[3] = 1.0; }
    double *o = rgba + 4 * (size_t)id;
    o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; o[3] = c[3];
}

/* k_ao_batch_resolve for the dirt stage: near_hits[id] / value[id] */
__global__ void k_dirt_batch_resolve(const BatchList bl, int N, double near_clip, double far_clip,
                                     const uint32_t *__restrict__ slot_of_entry, const double *__restrict__ tg,
                                     uint32_t *__restrict__ near_hits, float *__restrict__ value, unsigned long long *__restrict__ hit_total)
{
    batch_resolve(bl, DirtValue{N, near_clip, far_clip, tg}, slot_of_entry, near_hits, value, hit_total);
}

/* ---- the environment-lit gather (lh_env.h): the resolves read one byte per gather ray -- its any-hit answer, at element slot * N + r --
 * and, for the rays that are not occluded, fetch the environment in the ray's direction; whoever traced the rays wrote that array -------- */

/* (the environment as a kernel argument, and env_lookup -- env_fetch for a direction nobody checked: lh_shade.h) */

/* what the two resolves share beside their slots: the grid of the hemisphere, the generator's seed, the hit records and keys (the fused stage: the
 * directions are made again by lh_ao_ray_builtin) or the materialised directions (adir != NULL: the same doubles, or the replay's), the bytes */
struct EnvGather {
    int ntheta, nphi; unsigned long long seed;
    const double *hitrec; const unsigned long long *slot_key; const double *adir; const uint8_t *occ;
    double scale; DevEnv env;
};

/* The feature's hot loop, LH_ENV_GROUP lanes per hit slot: lane l takes the rays r = l, l + G, ... of the slot; an open ray costs a generator call
 * (sincos, two square roots), env_fetch's acos and normalisation and four 16-byte texel gathers, an occluded one nothing.  A pass of G rays parks
 * its colours in LDS (12 bytes a lane: component k of lane l is dword 3 l + k, a store banks by 32 dwords per half-wave and 3 is odd, so the 32 lanes
 * of a half hit 32 different banks; 3 KiB a workgroup); lanes
 * 0, 1, 2 of the group then take one channel each and add the pass's open rays in r order -- the order of lh_env_value -- from the group's ballot.
 * Control flow is uniform over the workgroup (N and the sample count are launch constants; a group without a slot runs the passes idle), the LDS
 * hand-over is inside a wave (a group never straddles one): a fence and a wave barrier, no __syncthreads.
 * Returns (lanes 0-2) the channel's sum and (every lane of the group) the occluded count */
#ifndef LH_ENV_GROUP
#define LH_ENV_GROUP 4           /* a power of two from 4 (three channel lanes) to 64; why 4: DESIGN.md 10.0d */
#endif
/* the radiance of an open gather ray, the resolves' one difference and so their template parameter: the accelerator's environment, or the
 * sun-and-sky light (lh_sky.h) -- the sky and its Perez denominators by value in the kernel's arguments (uniform over the launch:
 * scalar loads, nothing to allocate), and one byte per slot, the any-hit answer of the sun's ray (NULL: no sun) */
struct RadEnv {
    const DevEnv &env;
    __device__ __forceinline__ void operator()(double dx, double dy, double dz, float c[3]) const { env_lookup(env, dx, dy, dz, c); }
};
struct RadSky {
    const lh_sky_src_t &s;
    __device__ __forceinline__ void operator()(double dx, double dy, double dz, float c[3]) const { lh_sky_rgb_den(&s.sky, s.den, dx, dy, dz, c); }
};
/* the sun's term of channel lane gl (0-2) of a hit slot: after the last pass, before lh_env_finish */
__device__ __forceinline__ double sky_sun_term(const lh_sky_src_t &s, const uint8_t *__restrict__ sun_occ, uint32_t slot, int gl, double sum)
{
    const float c = gl == 0 ? s.sky.sun_rgb[0] : (gl == 1 ? s.sky.sun_rgb[1] : s.sky.sun_rgb[2]);
    return lh_sky_add_sun(sum, sun_occ[slot] != 0, c);
}
template <class Rad>
__device__ __forceinline__ double env_slot_sum(const EnvGather &gx, const Rad &rad, bool have, uint32_t slot, float (*park)[3], unsigned int &count)
{
    LH_NC
    const int N = gx.ntheta * gx.nphi;
    const int lane = threadIdx.x & 63, gl = lane & (LH_ENV_GROUP - 1), gshift = lane & ~(LH_ENV_GROUP - 1);
    float (*mine)[3] = park + (threadIdx.x & ~(LH_ENV_GROUP - 1));          /* the group's G entries */
    double sum = 0.0;
    count = 0;
    for (int base = 0; base < N; base += LH_ENV_GROUP) {
        const int r = base + gl;
        const bool valid = have && r < N;
        const size_t ray = (size_t)slot * (size_t)N + (size_t)r;
        const bool blocked = valid && gx.occ[ray] != 0;
        const bool open = valid && !blocked;
        if (open) {
            double ox, oy, oz, dx, dy, dz;
            if (gx.adir) { dx = gx.adir[3 * ray]; dy = gx.adir[3 * ray + 1]; dz = gx.adir[3 * ray + 2]; }
            else lh_ao_ray_builtin(gx.hitrec + LH_HITREC_DOUBLES * (size_t)slot, gx.slot_key[slot], gx.seed, gx.ntheta, gx.nphi, r, ox, oy, oz, dx, dy, dz);
            float c[3];
            rad(dx, dy, dz, c);
            mine[gl][0] = c[0]; mine[gl][1] = c[1]; mine[gl][2] = c[2];
        }
        const unsigned long long gmask = LH_ENV_GROUP >= 64 ? ~0ull : ((1ull << (LH_ENV_GROUP & 63)) - 1ull);
        const unsigned long long m_open = (__ballot(open) >> gshift) & gmask;
        count += (unsigned int)__popcll((__ballot(blocked) >> gshift) & gmask);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (gl < 3) for (unsigned long long m = m_open; m != 0ull; m &= m - 1ull) sum = lh_env_add(sum, mine[__ffsll(m) - 1][gl]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    return sum;
}

/* k_ao_resolve for the environment gather's tile, a group of lanes per pixel: a miss gives 0 (ambientocclusion.c:407-411), a hit the three floats of
 * lh_env_value; sub-samples accumulate per channel and are written as ao_resolve does.  TEX: times the texture of the hit's mesh, as ao_resolve */
template <bool TEX, class Rad>
__device__ __forceinline__ void env_resolve(int w, int h, int band_rows, int xs, int ys, const EnvGather &gx, const Rad &rad, const uint32_t *__restrict__ slot_of_sample,
                                            float *__restrict__ rgb, unsigned long long *__restrict__ occ_total, const TexArgs *tx,
                                            const lh_sky_src_t *sky = NULL, const uint8_t *__restrict__ sun_occ = NULL)
{
    LH_NC
    __shared__ float park[256][3];
    const size_t pix = (size_t)blockIdx.x * (256 / LH_ENV_GROUP) + (threadIdx.x / LH_ENV_GROUP);
    const int gl = threadIdx.x & (LH_ENV_GROUP - 1);
    const bool inside = pix < (size_t)w * h;
    const int S = xs * ys, N = gx.ntheta * gx.nphi;
    double accum = 0.0;          /* lanes 0-2: the pixel's channel */
    unsigned int nocc = 0;
    for (int s = 0; s < S; s++) {
        const uint32_t slot = inside ? slot_of_sample[pix * S + s] : LH_MISS_PRIM;
        const bool hit = slot != LH_MISS_PRIM;
        unsigned int c;
        double sum = env_slot_sum(gx, rad, hit, slot, park, c);
        if (gl == 0) nocc += c;
        double val = 0.0;
        if (sun_occ && hit && gl < 3) sum = sky_sun_term(*sky, sun_occ, slot, gl, sum);
        if (hit && gl < 3) val = (double)lh_env_finish(gx.scale, sum, N);
        if (TEX) {
            double tc[4];
            if (hit && gl < 3 && tex_color(*tx, pix * S + s, tc)) val = val * (gl == 0 ? tc[0] : (gl == 1 ? tc[1] : tc[2]));
        }
        accum = accum + val;
    }
    if (inside && gl < 3) {
        float f = (float)(accum * ((double)1.0 / (xs * ys)));
        if (f < 0.0f) f = 0.0f;
        pixel_out(rgb, pix, w, band_rows)[gl] = f;
    }
    wg_total(nocc, occ_total);
}

__global__ __launch_bounds__(256) void k_env_resolve(int w, int h, int band_rows, int xs, int ys, const EnvGather gx, const uint32_t *__restrict__ slot_of_sample,
                                                     float *__restrict__ rgb, unsigned long long *__restrict__ occ_total)
{
    env_resolve<false>(w, h, band_rows, xs, ys, gx, RadEnv{gx.env}, slot_of_sample, rgb, occ_total, NULL);
}

/* ... under the sun-and-sky light: no texture multiply (ambientocclusion.c:369-375) */
__global__ __launch_bounds__(256) void k_sky_resolve(int w, int h, int band_rows, int xs, int ys, const EnvGather gx, const lh_sky_src_t sky,
                                                     const uint8_t *__restrict__ sun_occ, const uint32_t *__restrict__ slot_of_sample,
                                                     float *__restrict__ rgb, unsigned long long *__restrict__ occ_total)
{
    env_resolve<false>(w, h, band_rows, xs, ys, gx, RadSky{sky}, slot_of_sample, rgb, occ_total, NULL, &sky, sun_occ);
}

__global__ __launch_bounds__(256) void k_env_resolve_tex(int w, int h, int band_rows, int xs, int ys, const EnvGather gx, const uint32_t *__restrict__ slot_of_sample,
                                                         float *__restrict__ rgb, unsigned long long *__restrict__ occ_total, const TexArgs tx)
{
    env_resolve<true>(w, h, band_rows, xs, ys, gx, RadEnv{gx.env}, slot_of_sample, rgb, occ_total, &tx);
}

/* k_ao_batch_resolve for the environment gather, a group of lanes per list entry: occluded_count[id] / rgb[3 id ..] (either may be NULL); a traced
 * miss gets LH_AO_NO_HIT and three zeros.  slot_of_entry NULL: an empty scene, every traced ray is a miss */
template <class Rad>
__device__ __forceinline__ void env_batch_resolve(const BatchList &bl, const EnvGather &gx, const Rad &rad, const uint32_t *__restrict__ slot_of_entry,
                                                  uint32_t *__restrict__ occluded_count, float *__restrict__ rgb,
                                                  unsigned long long *__restrict__ occ_total, const lh_sky_src_t *sky = NULL,
                                                  const uint8_t *__restrict__ sun_occ = NULL)
{
    LH_NC
    __shared__ float park[256][3];
    const uint32_t k = blockIdx.x * (256u / LH_ENV_GROUP) + threadIdx.x / LH_ENV_GROUP;
    const int gl = threadIdx.x & (LH_ENV_GROUP - 1);
    uint32_t id = 0;
    const bool traced = batch_entry(bl, k, id);
    const uint32_t slot = (traced && slot_of_entry) ? slot_of_entry[k] : LH_AO_NO_HIT;
    const bool hit = slot != LH_AO_NO_HIT;
    unsigned int c;
    double sum = env_slot_sum(gx, rad, hit, slot, park, c);
    if (sun_occ && hit && gl < 3) sum = sky_sun_term(*sky, sun_occ, slot, gl, sum);
    if (traced) {
        if (occluded_count && gl == 0) occluded_count[id] = hit ? c : LH_AO_NO_HIT;
        if (rgb && gl < 3) rgb[3 * (size_t)id + gl] = hit ? lh_env_finish(gx.scale, sum, gx.ntheta * gx.nphi) : 0.0f;
    }
    wg_total((hit && gl == 0) ? c : 0u, occ_total);
}

__global__ __launch_bounds__(256) void k_env_batch_resolve(const BatchList bl, const EnvGather gx, const uint32_t *__restrict__ slot_of_entry,
                                                           uint32_t *__restrict__ occluded_count, float *__restrict__ rgb,
                                                           unsigned long long *__restrict__ occ_total)
{
    env_batch_resolve(bl, gx, RadEnv{gx.env}, slot_of_entry, occluded_count, rgb, occ_total);
}

__global__ __launch_bounds__(256) void k_sky_batch_resolve(const BatchList bl, const EnvGather gx, const lh_sky_src_t sky, const uint8_t *__restrict__ sun_occ,
                                                           const uint32_t *__restrict__ slot_of_entry, uint32_t *__restrict__ occluded_count,
                                                           float *__restrict__ rgb, unsigned long long *__restrict__ occ_total)
{
    env_batch_resolve(bl, gx, RadSky{sky}, slot_of_entry, occluded_count, rgb, occ_total, &sky, sun_occ);
}

/* the fetch alone (lh_accel_environment_device): one thread per direction */
__global__ void k_env_batch(size_t n, const DevEnv env, const double *__restrict__ dir, float *__restrict__ rgb)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float c[3];
    env_lookup(env, dir[3 * i], dir[3 * i + 1], dir[3 * i + 2], c);
    rgb[3 * i] = c[0]; rgb[3 * i + 1] = c[1]; rgb[3 * i + 2] = c[2];
}

/* ... of the sky (lh_accel_sky_device): no index is made of a direction, so whatever it holds reaches a colour, not an address */
__global__ void k_sky_batch(size_t n, const lh_sky_src_t sky, const double *__restrict__ dir, float *__restrict__ rgb)
{
    LH_NC
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float c[3];
    lh_sky_rgb_den(&sky.sky, sky.den, dir[3 * i], dir[3 * i + 1], dir[3 * i + 2], c);
    rgb[3 * i] = c[0]; rgb[3 * i + 1] = c[1]; rgb[3 * i + 2] = c[2];
}

/* the sun's shadow rays, one per hit slot: the gather's origin P + eps Ns (the hit record's first three doubles) along the light's direction.
 * nslots_dev (or NULL): the slot count where it lives on the device, nslots then its upper bound.  A plain any-hit launch answers them: no slot
 * key, no self-primitive skip -- a sun behind the surface meets the hit's own triangle, and the reference counts that as shadow */
__global__ void k_sun_rays(size_t nslots, const unsigned long long *__restrict__ nslots_dev, const double *__restrict__ hitrec,
                           double sx, double sy, double sz, double *__restrict__ org, double *__restrict__ dir)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (nslots_dev && (size_t)*nslots_dev < nslots) nslots = (size_t)*nslots_dev;
    if (i >= nslots) return;
    const double *h = hitrec + LH_HITREC_DOUBLES * i;
    org[3 * i] = h[0]; org[3 * i + 1] = h[1]; org[3 * i + 2] = h[2];
    dir[3 * i] = sx; dir[3 * i + 1] = sy; dir[3 * i + 2] = sz;
}

/* ---- direct light (lh_lights.h): the resolves read one byte per shadow ray -- its bounded any-hit answer, at element slot * L + l -- make the
 * item's ray and weight again from the hit record and the light table and add the visible lights in list order; whoever traced the rays wrote that
 * array.  The table is a kernel argument by value: the resolves index it uniformly (scalar loads), the ray maker per thread ------------------------ */

/* the shadow rays and bounds of a materialised stage, and of lh_accel_light_rays_device: one thread per item, ray (slot, l) at element slot * L + l;
 * the bound of an item that is not traced is 0.0 (a dead bound: the bounded launch answers 0 for it, the byte a fused stage stores).  nslots_dev (or
 * NULL): the slot count where it lives on the device, nslots then its upper bound */
__global__ void k_light_rays(size_t nslots, const unsigned long long *__restrict__ nslots_dev, int L, const double *__restrict__ hitrec,
                             double *__restrict__ org, double *__restrict__ dir, double *__restrict__ tmax, const lh_light_tab_t tab)
{
    LH_NC
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (nslots_dev && (size_t)*nslots_dev < nslots) nslots = (size_t)*nslots_dev;
    if (id >= nslots * (size_t)L) return;
    const size_t slot = id / (size_t)L; const int l = (int)(id - slot * (size_t)L);
    const double *h = hitrec + LH_HITREC_DOUBLES * slot;
    const double O[3] = {h[0], h[1], h[2]}, Ns[3] = {h[9], h[10], h[11]};
    double d[3], w;
    const double tm = lh_light_item(O, Ns, tab.l + l, d, &w);
    org[3 * id] = O[0]; org[3 * id + 1] = O[1]; org[3 * id + 2] = O[2];
    dir[3 * id] = d[0]; dir[3 * id + 1] = d[1]; dir[3 * id + 2] = d[2];
    tmax[id] = tm;
}

/* what the two resolves share: the list's length, the hit records, the bytes */
struct LightGather { int L; const double *hitrec; const uint8_t *occ; };

/* the mask and value of a hit slot, and how many of its L items have their bit clear */
struct light_slot {
    const LightGather &g; const lh_light_tab_t &tab;
    __device__ __forceinline__ uint32_t operator()(uint32_t slot, float val[3], unsigned int &dark) const
    {
        LH_NC
        const double *h = g.hitrec + LH_HITREC_DOUBLES * (size_t)slot;
        const double O[3] = {h[0], h[1], h[2]}, Ns[3] = {h[9], h[10], h[11]};
        const uint32_t mask = lh_lights_value(O, Ns, tab.l, g.L, g.occ + (size_t)slot * (size_t)g.L, val);
        dark = (unsigned int)(g.L - __popc(mask));
        return mask;
    }
};

/* the resolves of an item kind.  Slot: "mask, value and closed count of a hit slot" over the kind's gather and its table, which stay the kernel's
 * by-value arguments (light_slot, area_slot).
 * k_ao_resolve for an item kind's tile, a thread per pixel: a miss gives 0, a hit the three floats of its slot; sub-samples are widened, added per
 * channel in sample order and written as env_resolve does.  No texture multiply (the reference's sun branch fetches none) */
template <class Slot>
__device__ __forceinline__ void item_resolve(int w, int h, int band_rows, int xs, int ys, const Slot &at, const uint32_t *__restrict__ slot_of_sample,
                                             float *__restrict__ rgb, unsigned long long *__restrict__ dark_total)
{
    LH_NC
    const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool inside = pix < (size_t)w * h;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    unsigned int n = 0;
    const int S = inside ? xs * ys : 0;
    for (int s = 0; s < S; s++) {
        const uint32_t slot = slot_of_sample[pix * S + s];
        float val[3] = {0.0f, 0.0f, 0.0f};
        if (slot != LH_MISS_PRIM) { unsigned int c; (void)at(slot, val, c); n += c; }
        a0 = a0 + (double)val[0]; a1 = a1 + (double)val[1]; a2 = a2 + (double)val[2];
    }
    if (inside) {
        const double inv = (double)1.0 / (xs * ys);
        float f0 = (float)(a0 * inv), f1 = (float)(a1 * inv), f2 = (float)(a2 * inv);
        if (f0 < 0.0f) f0 = 0.0f;
        if (f1 < 0.0f) f1 = 0.0f;
        if (f2 < 0.0f) f2 = 0.0f;
        float *o = pixel_out(rgb, pix, w, band_rows);
        o[0] = f0; o[1] = f1; o[2] = f2;
    }
    wg_total(n, dark_total);
}

/* k_ao_batch_resolve for an item kind, a thread per list entry: visible[id] / rgb[3 id ..] (either may be NULL); a traced miss gets LH_AO_NO_HIT and
 * three zeros.  slot_of_entry NULL: an empty scene, every traced ray is a miss */
template <class Slot>
__device__ __forceinline__ void item_batch_resolve(const BatchList &bl, const Slot &at, const uint32_t *__restrict__ slot_of_entry, uint32_t *__restrict__ visible,
                                                   float *__restrict__ rgb, unsigned long long *__restrict__ dark_total)
{
    LH_NC
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    uint32_t id = 0;
    unsigned int n = 0;
    if (batch_entry(bl, k, id)) {
        const uint32_t slot = slot_of_entry ? slot_of_entry[k] : LH_AO_NO_HIT;
        uint32_t mask = LH_AO_NO_HIT;
        float val[3] = {0.0f, 0.0f, 0.0f};
        if (slot != LH_AO_NO_HIT) mask = at(slot, val, n);
        if (visible) visible[id] = mask;
        if (rgb) { rgb[3 * (size_t)id] = val[0]; rgb[3 * (size_t)id + 1] = val[1]; rgb[3 * (size_t)id + 2] = val[2]; }
    }
    wg_total(n, dark_total);
}

__global__ __launch_bounds__(256) void k_light_resolve(int w, int h, int band_rows, int xs, int ys, const LightGather g, const uint32_t *__restrict__ slot_of_sample,
                                                       float *__restrict__ rgb, unsigned long long *__restrict__ dark_total, const lh_light_tab_t tab)
{
    item_resolve(w, h, band_rows, xs, ys, light_slot{g, tab}, slot_of_sample, rgb, dark_total);
}

__global__ __launch_bounds__(256) void k_light_batch_resolve(const BatchList bl, const LightGather g, const uint32_t *__restrict__ slot_of_entry,
                                                             uint32_t *__restrict__ visible, float *__restrict__ rgb,
                                                             unsigned long long *__restrict__ dark_total, const lh_light_tab_t tab)
{
    item_batch_resolve(bl, light_slot{g, tab}, slot_of_entry, visible, rgb, dark_total);
}

/* ---- area lights (lh_area.h): the light stage's shape with S samples per light -- one byte per item at element (slot * L + l) * S + s; the resolves make every
 * item's uniforms, sample and weight again (replayed uniforms: read again) and average over the samples.  The table of lights, the emitter table's address, S, the
 * bound and the uniforms' address are a kernel argument by value ------------------------------------------------------------------------------------------ */

/* the rays, bounds and weights of a materialised stage, and of lh_accel_area_light_rays_device: one thread per item; the bound of an item that is not traced is
 * 0.0; weight (or NULL): the item's w.  nslots_dev (or NULL): the slot count where it lives on the device, nslots then its upper bound */
__global__ void k_area_rays(size_t nslots, const unsigned long long *__restrict__ nslots_dev, unsigned long long seed, const double *__restrict__ hitrec,
                            const unsigned long long *__restrict__ slot_key, double *__restrict__ org, double *__restrict__ dir, double *__restrict__ tmax,
                            double *__restrict__ weight, const lh_area_tab_t tab)
{
    LH_NC
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t S = (size_t)tab.S, LS = (size_t)tab.L * S;
    if (nslots_dev && (size_t)*nslots_dev < nslots) nslots = (size_t)*nslots_dev;
    if (id >= nslots * LS) return;
    const size_t slot = id / LS, r = id - slot * LS; const int l = (int)(r / S), sm = (int)(r - (size_t)l * S);
    const double *h = hitrec + LH_HITREC_DOUBLES * slot;
    const double O[3] = {h[0], h[1], h[2]}, Ns[3] = {h[9], h[10], h[11]};
    double x[3], d[3], w;
    lh_area_item_uniforms(tab.uniforms ? tab.uniforms + 3 * LS * slot : NULL, slot_key[slot], seed, tab.L, tab.S, l, sm, x);
    const double tm = lh_area_item(O, Ns, tab.l + l, tab.emitters, x, tab.bound, d, &w);
    org[3 * id] = O[0]; org[3 * id + 1] = O[1]; org[3 * id + 2] = O[2];
    dir[3 * id] = d[0]; dir[3 * id + 1] = d[1]; dir[3 * id + 2] = d[2];
    tmax[id] = tm;
    if (weight) weight[id] = w;
}

/* what the two resolves share: the hit records, the keys, the seed, the bytes */
struct AreaGather { const double *hitrec; const unsigned long long *key; unsigned long long seed; const uint8_t *occ; };

/* the mask and value of a hit slot, and how many of its L S items are not open */
struct area_slot {
    const AreaGather &g; const lh_area_tab_t &tab;
    __device__ __forceinline__ uint32_t operator()(uint32_t slot, float val[3], unsigned int &closed) const
    {
        LH_NC
        const size_t LS = (size_t)tab.L * (size_t)tab.S;
        const double *h = g.hitrec + LH_HITREC_DOUBLES * (size_t)slot;
        const double O[3] = {h[0], h[1], h[2]}, Ns[3] = {h[9], h[10], h[11]};
        return lh_area_value(O, Ns, tab.l, tab.L, tab.S, tab.emitters, tab.bound, tab.uniforms ? tab.uniforms + 3 * LS * (size_t)slot : NULL, g.key[slot], g.seed,
                             g.occ + (size_t)slot * LS, val, &closed);
    }
};

__global__ __launch_bounds__(256) void k_area_resolve(int w, int h, int band_rows, int xs, int ys, const AreaGather g, const uint32_t *__restrict__ slot_of_sample,
                                                      float *__restrict__ rgb, unsigned long long *__restrict__ dark_total, const lh_area_tab_t tab)
{
    item_resolve(w, h, band_rows, xs, ys, area_slot{g, tab}, slot_of_sample, rgb, dark_total);
}

__global__ __launch_bounds__(256) void k_area_batch_resolve(const BatchList bl, const AreaGather g, const uint32_t *__restrict__ slot_of_entry,
                                                            uint32_t *__restrict__ visible, float *__restrict__ rgb,
                                                            unsigned long long *__restrict__ dark_total, const lh_area_tab_t tab)
{
    item_batch_resolve(bl, area_slot{g, tab}, slot_of_entry, visible, rgb, dark_total);
}


/* ---- the whole hit epilogue for a batch of hit records --------------------------------------
 * ri_intersection_state_build (intersection_state.c:99-248), every member a shader reads: P, Ng, Ns, tangent,
 * binormal, colour, st, I (normalised direction), inside.  Attributes are per-primitive SoA arrays in
 * primitive-id order (9 doubles = 3 corners x xyz; st: 6 doubles; first value NaN = the mesh has none):
 * one thread per ray, LH_STATE_DOUBLES per record, misses are left untouched. */
__global__ void k_state_build(size_t n, const lh_dev_scene_t sc, const double *__restrict__ nrm9, const double *__restrict__ col9,
                              const double *__restrict__ tan9, const double *__restrict__ bin9, const double *__restrict__ st6,
                              const uint8_t *__restrict__ inside_of_prim,
                              const double *__restrict__ org, const double *__restrict__ dir, const uint32_t *__restrict__ prim,
                              const double *__restrict__ t, const double *__restrict__ u, const double *__restrict__ v,
                              double *__restrict__ state)
{
    LH_NC
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = prim[i];
    if (p == LH_MISS_PRIM) return;
    const double tt = t[i], uu = u[i], vv = v[i], w = 1.0 - uu - vv;
    double *o = state + LH_STATE_DOUBLES * i;
    double P[3], Ng[3], Ns[3], I[3];
    /* P, Ng, Ns, I: the part a transport of its own shares (lh_shade.h; k_whitted_bounce) */
    const bool has_n = state_core<true>(sc.tri64, nrm9, p, org + 3 * i, dir + 3 * i, tt, uu, vv, P, Ng, Ns, I);
    bool has_tb = false;
    if (has_n && tan9 && bin9) { const double x = tan9[9 * (size_t)p], y = bin9[9 * (size_t)p]; has_tb = (x == x) && (y == y); }
#define LH_LERP9(A, dst) { const double *q_ = (A) + 9 * (size_t)p; \
        for (int k = 0; k < 3; k++) { const double a_ = q_[k] * w, b_ = q_[3 + k] * uu, c_ = q_[6 + k] * vv; (dst)[k] = (a_ + b_) + c_; } }
    for (int k = 0; k < 3; k++) { o[k] = P[k]; o[3 + k] = Ng[k]; o[6 + k] = Ns[k]; }
    if (has_tb) { LH_LERP9(tan9, o + 9) LH_LERP9(bin9, o + 12) }
    else {
        /* ri_ortho_basis(tmpbasis, Ng) (reflection.c:311-333) */
        double b0[3], b1[3] = {0.0, 0.0, 0.0};
        int ax = 3;
        for (int k = 0; k < 3; k++) if (Ng[k] < 0.6 && Ng[k] > -0.6) { ax = k; break; }
        if (ax >= 3) ax = 0;
        b1[ax] = 1.0;
        vcross(b0, b1, Ng); vnormalize(b0);
        vcross(b1, Ng, b0); vnormalize(b1);
        for (int k = 0; k < 3; k++) { o[9 + k] = b0[k]; o[12 + k] = b1[k]; }
    }
    bool has_c = false, has_st = false;
    if (col9) { const double x = col9[9 * (size_t)p]; has_c = (x == x); }
    if (has_c) LH_LERP9(col9, o + 15) else { o[15] = 1.0; o[16] = 1.0; o[17] = 1.0; }
    if (st6) { const double x = st6[6 * (size_t)p]; has_st = (x == x); }
    if (has_st) {
        /* lerp_uv (intersection_state.c:58-76): (1-u-v) st0 + u st1 + v st2 */
        const double *q = st6 + 6 * (size_t)p;
        o[18] = (w * q[0] + uu * q[2]) + vv * q[4];
        o[19] = (w * q[1] + uu * q[3]) + vv * q[5];
    } else { o[18] = 0.0; o[19] = 0.0; }
    for (int k = 0; k < 3; k++) o[20 + k] = I[k];
    o[23] = (inside_of_prim && inside_of_prim[p]) ? 1.0 : 0.0;
#undef LH_LERP9
}

/* ------------------------------------------------------------------------------------ */
/* wavefront path tracer (BASELINE config 4)                                */
/*                                                                                       */
/* The reference's Kajiya path tracer (src/transport/pathtrace.c) is dead code that no     */
/* longer compiles; what is kept is its documented algorithm (pathtrace.c:189-314,407-537) */
/* re-expressed as closest-hit batches:                                                    */
/*   camera sample through a random sub-pixel position (sample_pixel :316-352);            */
/*   miss -> the IBL radiance in the ray's direction (ri_texture_ibl_fetch, texture.c:     */
/*   238-276: angular map, bilinear) or a constant environment;                            */
/*   hit  -> Russian roulette on d + s + t = the averages of the material's kd, ks, kt     */
/*   (russian_roulette :407-430), reflection type D / S / T drawn in those proportions     */
/*   (sample_reflection_type :432-459), next direction: cosine-weighted about the normal   */
/*   (sample_cosweight :500-531), mirror reflection (ri_reflect) or refraction with the    */
/*   material's ior, entering / leaving tracked per path, total internal reflection turns  */
/*   T into S (sample_outdir :461-498, ri_refract reflection.c:69-128); throughput *=      */
/*   reflectance x the interpolated vertex colour (brdf :533-565), to a vertex limit.      */
/* Two departures, both stated in DESIGN.md: (1) the reference multiplies the BRDF value    */
/* (kd / pi ...) without the cosine / pdf factor and never compensates the roulette: the    */
/* default here is the unbiased estimator of the same sampling scheme (a furnace renders    */
/* white), LH_PT_REFERENCE_WEIGHTS reproduces the reference's factors; (2) its final        */
/* "connect" step (one more sampled direction + visibility ray, light_sample :354-382) is   */
/* what the extension ray already is in wavefront form: a path that leaves the scene        */
/* collects the environment in the direction it left.  Parity for this row is at the        */
/* ri_raytrace level (every bounce goes through the closest-hit kernel and fp64 resolve).   */
/* ------------------------------------------------------------------------------------ */

/* After the closest-hit launch of bounce `depth`: the live paths are DECIDED (k_pt_decide) and the survivors SCATTERED
 * (k_pt_scatter).  Round 2 ran decide -> flag count -> scan -> emit with the survivor count read back by the host before the
 * next launch (110 dependent launches and 28 host round trips per 64-sample pass); rounds 3-4 ran ONE kernel per bounce, a
 * workgroup deciding 2048 consecutive paths, listing its survivors in LDS and scattering them -- at the scatter's 136-146
 * VGPRs and 96 bytes of scratch: three waves per SIMD, every one of them waiting on its loads 61-74 % of the time, the decision
 * loop one dependent load chain per item (profiles/r05_pmc_pt_summary.txt: 31 ms for a 2^30-path pass's first bounce with the
 * vector pipes 37 % busy).  Round 5 splits the two halves at the place where their needs differ:
 *   k_pt_decide  -- a streaming pass at eight waves per SIMD: a workgroup takes LH_PT_ITEMS x 256 consecutive paths, loads their
 *     hit words (and, for the misses, throughputs) in one batch, decides them (miss -> radiance = throughput x environment, the
 *     path ends; hit -> vertex limit and Russian roulette on d + s + t, pathtrace.c:407-430 -> ends with radiance 0, or goes
 *     on), reserves the survivors' slots with one atomic on counts[depth + 1] and writes each survivor's SOURCE INDEX into its
 *     slot of the next bounce's path-word array, in path order within the workgroup;
 *   k_pt_scatter -- one thread per survivor slot j: source index i = path_of2[j], hit epilogue, lobe, next ray, throughput,
 *     written once into slot j (the path word over the source index it has just read).
 * The launch's own path count is counts[depth], left there by the previous bounce: nothing comes back to the host inside a
 * pass.  Every path writes its radiance exactly once (where it ends), so the buffer needs no clearing.  Slot order across
 * workgroups depends on scheduling; a path's arithmetic does not (keys are (pixel, sample, bounce)): the frame is the same. */
#define LH_PT_ITEMS 8
struct PtPass {
    DevMaterial override_mat; DevEnv env;
    const PtCamSrc *cam;                 /* bounce 0: the pass's rays are the camera rays, regenerated from the path id */
    unsigned long long seed;
    int use_override, ref_weights, depth, max_depth, s0, spp, x0, y0, w, band_rows, band_stride, full_width;
    PtDivs dv;                           /* divisions by spp, w, band_rows as multiplications (lh_pt.h) */
};

/* PROBE: the environment is a light probe (a miss evaluates it in the path's direction: fp64 acos / sqrt / divisions, kept out of the
 * constant-environment instantiation, whose decision loop is unrolled over its batch).
 * A workgroup's span is LH_PT_ROUNDS batches of LH_PT_ITEMS x 256 paths behind ONE atomic on the survivor count: every workgroup of
 * every launch adds to the same word, and same-address atomics retire one every ~20 ns -- at 2048 paths an atomic a 2^30-path
 * pass's first decision took 6.0 ms for its 13 GB; at 8192 the atomics are a quarter of that. */
#define LH_PT_ROUNDS 4

/* A path's radiance goes into its pixel's accumulator where the path ends -- three 64-bit FIXED-POINT sums per pixel of the pass
 * (32 fraction bits; a term clamped to +-2^18: the 2^12 terms of a pixel that lh_tile.hip allows in one pass -- its samples; in a lit pass, lh_ptl.h, its samples x the bounces, each entry of which may add a term -- stay below 2^62) -- instead of into a 12-byte record per path that a resolve pass sums afterwards (rounds 2-4): those records
 * were written where the paths ended, a few of every 128-byte line per bounce (6.7 + 5.6 + ... GB of partial-line writes and
 * 12.9 GB read back per 2^30-path pass, 12.9 GB of HBM held).  Integer sums do not depend on the order of their terms: a pixel
 * is the same whatever the slot order, tiling or sharding, bit for bit, as before.  Lanes of a wave hold consecutive slots,
 * i.e. runs of paths of the same pixel: the runs are summed across the wave first (a segmented scan over run numbers), one
 * atomic per run and channel. */
#define LH_PT_FIX_CLAMP 262144.0f
__device__ __forceinline__ unsigned long long pt_fix(float r)
{
    r = fminf(fmaxf(r, -LH_PT_FIX_CLAMP), LH_PT_FIX_CLAMP);          /* (a NaN never gets here: pt_accumulate drops it) */
    float fl = floorf(r), fr = r - fl;          /* fr is exact in fp32 -- except for a tiny negative r (-1e-10: floor -1, r + 1 rounds to 1.0f) */
    if (fr >= 1.0f) { fr = 0.0f; fl += 1.0f; }  /* ... which is the carry: without it (uint32_t)(1.0f * 2^32) is out of range */
    const uint32_t lo = (uint32_t)(fr * 4294967296.0f);
    return ((unsigned long long)(long long)(int)fl << 32) | (unsigned long long)lo;
}

__device__ __forceinline__ void pt_accumulate(unsigned long long *__restrict__ accum, uint32_t pix, bool ends, float r0, float r1, float r2, int lane)
{
    const bool v0 = ends && r0 == r0 && r0 != 0.0f, v1 = ends && r1 == r1 && r1 != 0.0f, v2 = ends && r2 == r2 && r2 != 0.0f;      /* a NaN channel adds nothing */
    if (__ballot(v0 | v1 | v2) == 0ull) return;                        /* wave-uniform: nothing ends here with light */
    unsigned long long a = v0 ? pt_fix(r0) : 0ull, b = v1 ? pt_fix(r1) : 0ull, c = v2 ? pt_fix(r2) : 0ull;
    /* run number: the pixel may come back later in the wave (two workgroups' survivors of one pixel with a third's between) */
    const uint32_t before = (uint32_t)__shfl_up((int)pix, 1);
    const unsigned long long heads = __ballot(lane == 0 || before != pix);
    const uint32_t run = (uint32_t)__popcll(heads & ((2ull << lane) - 1ull));
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t ru = (uint32_t)__shfl_up((int)run, off);
        const unsigned long long au = __shfl_up(a, off), bu = __shfl_up(b, off), cu = __shfl_up(c, off);
        if (lane >= off && ru == run) { a += au; b += bu; c += cu; }
    }
    const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
    if (last && (a | b | c) != 0ull) {
        unsigned long long *o = accum + 3 * (size_t)pix;
        if (a) atomicAdd(o, a);
        if (b) atomicAdd(o + 1, b);
        if (c) atomicAdd(o + 2, c);
    }
}

/* the same when every path that ends here with light carries the SAME radiance (camera rays that leave the scene under a constant
 * environment -- half of a frame's paths): a run's sum is its count x that value, counted from the wave's ballots, no scan */
__device__ __forceinline__ void pt_accumulate_uniform(unsigned long long *__restrict__ accum, uint32_t pix, bool ends, const float e[3], int lane)
{
    const unsigned long long mm = __ballot(ends);
    if (mm == 0ull) return;
    const uint32_t before = (uint32_t)__shfl_up((int)pix, 1);
    const unsigned long long heads = __ballot(lane == 0 || before != pix);
    const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
    if (last) {
        const unsigned long long upto = (2ull << lane) - 1ull;
        const int start = 63 - __clzll((long long)(heads & upto));                    /* bit `lane`'s run begins at its nearest head below */
        const unsigned long long cnt = (unsigned long long)__popcll(mm & upto & ~((1ull << start) - 1ull));
        if (cnt) {
            unsigned long long *o = accum + 3 * (size_t)pix;
            for (int c = 0; c < 3; c++) if (e[c] == e[c] && e[c] != 0.0f) atomicAdd(o + c, cnt * pt_fix(e[c]));
        }
    }
}

template <bool FIRST, bool PROBE>
__global__ __launch_bounds__(256) void k_pt_decide(const PtPass ps, const uint32_t *__restrict__ prim_mesh, const DevMaterial *__restrict__ materials,
                                                   uint32_t *__restrict__ counts, const double *__restrict__ dir, const uint32_t *__restrict__ prim,
                                                   const uint32_t *__restrict__ path_of, const float *__restrict__ thr, unsigned long long *__restrict__ accum,
                                                   uint32_t *__restrict__ src_of)
{
    LH_NC
    constexpr int NB = LH_PT_ROUNDS * LH_PT_ITEMS * 4;             /* ballots of a span: (round, item, wave) */
    __shared__ unsigned long long sbal[NB];
    __shared__ uint32_t soff[NB];
    __shared__ uint32_t gbase;
    const uint32_t n = counts[ps.depth];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t batch = 256u * LH_PT_ITEMS, span = batch * LH_PT_ROUNDS;
    for (uint32_t base = blockIdx.x * span; base < n; base += gridDim.x * span) {      /* n < 2^31: no wrap */
#pragma unroll 1
        for (int r = 0; r < LH_PT_ROUNDS; r++) {
            const uint32_t b0 = base + (uint32_t)r * batch;
            /* the batch's loads first, all of them in flight together: hit words, path words, the misses' throughputs */
            uint32_t pr[LH_PT_ITEMS], pw[LH_PT_ITEMS];
            float g0[LH_PT_ITEMS], g1[LH_PT_ITEMS], g2[LH_PT_ITEMS];
#pragma unroll
            for (int k = 0; k < LH_PT_ITEMS; k++) {
                const uint32_t i = b0 + (uint32_t)k * 256u + threadIdx.x;
                pr[k] = i < n ? prim[i] : 0u;
                pw[k] = FIRST ? i : (i < n ? path_of[i] : 0u);
            }
#pragma unroll
            for (int k = 0; k < LH_PT_ITEMS; k++) {
                const uint32_t i = b0 + (uint32_t)k * 256u + threadIdx.x;
                g0[k] = 1.0f; g1[k] = 1.0f; g2[k] = 1.0f;
                if (!FIRST && i < n && pr[k] == LH_MISS_PRIM) { g0[k] = thr[3 * (size_t)i]; g1[k] = thr[3 * (size_t)i + 1]; g2[k] = thr[3 * (size_t)i + 2]; }
            }
#pragma unroll
            for (int k = 0; k < LH_PT_ITEMS; k++) {
                const uint32_t i = b0 + (uint32_t)k * 256u + threadIdx.x;
                bool go = false;
                const uint32_t path = pw[k] & ~LH_PT_INTERIOR;
                float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
                if (i < n) {
                    const uint32_t p = pr[k];
                    if (p == LH_MISS_PRIM) {
                        float e[3];
                        if (PROBE) {
                            double o[3], d[3];
                            if (FIRST) pt_camera_ray(ps.cam, i, o, d);
                            else { d[0] = dir[3 * (size_t)i]; d[1] = dir[3 * (size_t)i + 1]; d[2] = dir[3 * (size_t)i + 2]; }
                            env_fetch(ps.env, d[0], d[1], d[2], e);
                        } else { e[0] = ps.env.rgb[0]; e[1] = ps.env.rgb[1]; e[2] = ps.env.rgb[2]; }
                        if (FIRST) { r0 = e[0]; r1 = e[1]; r2 = e[2]; }
                        else { r0 = g0[k] * e[0]; r1 = g1[k] * e[1]; r2 = g2[k] * e[2]; }
                    } else {
                        const double ksum = ps.use_override ? ps.override_mat.asum9 : materials[prim_mesh[p]].asum9;
                        go = pt_survives(ksum, pt_key(ps.seed, path, ps.spp, ps.s0, ps.x0, ps.y0, ps.w, ps.band_rows, ps.band_stride, ps.dv, ps.full_width, ps.depth), ps.depth, ps.max_depth);
                    }
                }
                /* a path the roulette ended adds nothing */
                if (FIRST && !PROBE) pt_accumulate_uniform(accum, lh_div(path, ps.dv.spp), i < n && pr[k] == LH_MISS_PRIM, ps.env.rgb, lane);
                else pt_accumulate(accum, lh_div(path, ps.dv.spp), i < n && !go, r0, r1, r2, lane);
                const unsigned long long m = __ballot(go);
                if (lane == 0) sbal[(r * LH_PT_ITEMS + k) * 4 + wv] = m;
            }
        }
        __syncthreads();
        /* NB counts -> exclusive offsets in path order (round, item, wave), by the first wave: two entries a lane */
        if (wv == 0) {
            static_assert(NB == 128, "two ballots a lane");
            const uint32_t c0 = (uint32_t)__popcll(sbal[2 * lane]), c1 = (uint32_t)__popcll(sbal[2 * lane + 1]);
            uint32_t incl = c0 + c1;
            for (int off = 1; off < 64; off <<= 1) { const uint32_t up = (uint32_t)__shfl_up((int)incl, off); if (lane >= off) incl += up; }
            soff[2 * lane] = incl - c0 - c1; soff[2 * lane + 1] = incl - c1;
            if (lane == 63) gbase = incl ? atomicAdd(&counts[ps.depth + 1], incl) : 0u;
        }
        __syncthreads();
        const uint32_t g = gbase;
#pragma unroll 4
        for (int q = 0; q < LH_PT_ROUNDS * LH_PT_ITEMS; q++) {
            const unsigned long long m = sbal[q * 4 + wv];
            if ((m >> lane) & 1ull) src_of[g + soff[q * 4 + wv] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = base + (uint32_t)q * 256u + threadIdx.x;
        }
        __syncthreads();
    }
}

template <bool FIRST>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 8))) void k_pt_scatter(const PtPass ps, const lh_dev_scene_t sc, const double *__restrict__ nrm9,
                                                    const double *__restrict__ col9, const uint32_t *__restrict__ prim_mesh,
                                                    const DevMaterial *__restrict__ materials, const uint32_t *__restrict__ counts,
                                                    const double *__restrict__ org, const double *__restrict__ dir,
                                                    const uint32_t *__restrict__ prim, const double *__restrict__ t,
                                                    const double *__restrict__ u, const double *__restrict__ v,
                                                    const uint32_t *__restrict__ path_of, const float *__restrict__ thr,
                                                    double *__restrict__ org2, double *__restrict__ dir2,
                                                    uint32_t *path_of2 /* in: the survivor's source index; out: its path word */, float *__restrict__ thr2)
{
    LH_NC
    const uint32_t n2 = counts[ps.depth + 1];
#pragma unroll 1
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < n2; j += gridDim.x * 256u) {
        const uint32_t i = path_of2[j];
        const uint32_t pword = FIRST ? i : path_of[i];
        const uint32_t path = pword & ~LH_PT_INTERIOR;
        const uint32_t p = prim[i];
        const double tt = t[i], uu = u[i], vv = v[i];
        float G[3] = {1.0f, 1.0f, 1.0f};
        if (!FIRST) { G[0] = thr[3 * (size_t)i]; G[1] = thr[3 * (size_t)i + 1]; G[2] = thr[3 * (size_t)i + 2]; }
        double Or[3], D[3];
        if (FIRST) pt_camera_ray(ps.cam, i, Or, D);
        else {
            Or[0] = org[3 * (size_t)i]; Or[1] = org[3 * (size_t)i + 1]; Or[2] = org[3 * (size_t)i + 2];
            D[0] = dir[3 * (size_t)i]; D[1] = dir[3 * (size_t)i + 1]; D[2] = dir[3 * (size_t)i + 2];
        }
        const uint64_t key = pt_key(ps.seed, path, ps.spp, ps.s0, ps.x0, ps.y0, ps.w, ps.band_rows, ps.band_stride, ps.dv, ps.full_width, ps.depth);
        /* field by field: a whole-struct copy from one of two places keeps the record in scratch (96 bytes a lane, and the lobe's
         * reflectance then read from it by a run-time offset) */
        DevMaterial M;
#define LH_MFIELDS LH_MF(kd[0]) LH_MF(kd[1]) LH_MF(kd[2]) LH_MF(ks[0]) LH_MF(ks[1]) LH_MF(ks[2]) LH_MF(kt[0]) LH_MF(kt[1]) LH_MF(kt[2]) LH_MF(ior) \
                   LH_MF(ad) LH_MF(as) LH_MF(at) LH_MF(asum9) LH_MF(wd) LH_MF(ws) LH_MF(wt)
        M.pad = 0.0f;
        if (ps.use_override) {
#define LH_MF(x) M.x = ps.override_mat.x;
            LH_MFIELDS
#undef LH_MF
        } else {
            const DevMaterial *mp = materials + prim_mesh[p];
#define LH_MF(x) M.x = mp->x;
            LH_MFIELDS
#undef LH_MF
        }
#undef LH_MFIELDS
        double o2[3], O[3]; float G2[3]; uint32_t pw2;
        pt_scatter(sc, nrm9, col9, M, ps.ref_weights, key, p, pword, Or, D, tt, uu, vv, G, o2, O, G2, pw2);
        for (int c = 0; c < 3; c++) { thr2[3 * (size_t)j + c] = G2[c]; org2[3 * (size_t)j + c] = o2[c]; dir2[3 * (size_t)j + c] = O[c]; }
        path_of2[j] = pw2;
    }
}

/* counts[0] = the pass's paths, counts[1 ..] = 0; the pass's camera-ray source into device memory */
__global__ void k_pt_begin(uint32_t *counts, uint32_t paths, int nentries, const PtCamSrc src, PtCamSrc *dst)
{
    for (int i = threadIdx.x; i < nentries; i += blockDim.x) counts[i] = i == 0 ? paths : 0u;
    if (threadIdx.x == 0) *dst = src;
}

/* per pixel: add the mean of this pass's samples -- the pixel's three fixed-point sums (pt_accumulate) as floats x 1 / spp_total --
 * and leave the sums zero for the next pass.  (Rounds 2-4 summed 12-byte per-path records here, staged through LDS: 3.3 ms of a
 * 2^30-path pass.) */
__global__ __launch_bounds__(256) void k_pt_resolve(int w, int h, int band_rows, float inv_total_spp, unsigned long long *__restrict__ accum, float *__restrict__ rgb)
{
    const size_t npix = (size_t)w * h, pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= npix) return;
    float sum[3];
    for (int c = 0; c < 3; c++) {
        const long long v = (long long)accum[3 * pix + c];
        accum[3 * pix + c] = 0ull;
        sum[c] = (float)((double)v * 2.3283064365386963e-10);
    }
    /* every band is written in image orientation (its first frame line last); a tile is one band */
    const int lx = (int)(pix % w), ly = (int)(pix / w), band = ly / band_rows;
    float *o = rgb + 3 * ((size_t)(band * band_rows + (band_rows - 1 - (ly - band * band_rows))) * w + lx);
    o[0] += sum[0] * inv_total_spp; o[1] += sum[1] * inv_total_spp; o[2] += sum[2] * inv_total_spp;
}

/* ---- direct light at the path vertices (lh_ptl.h) and the path-vertex sink --------------------------------------------------------------
 * Between the closest-hit launch of bounce `depth` and its shading pass, for a caller with lights or a sink (lh_tile.hip pt_tile): the light
 * stage of a caller's batch answers `value` for the bounce's entries, k_pt_direct turns it into the hits' r and adds that to their pixels,
 * k_pt_sink hands the entries out.  Bounce 0 has no ray in memory (the closest-hit walk makes the camera rays in its refill): the stage and
 * the sink read them from the arrays k_pt_camera_rays fills.  With area lights the area stage answers a second `value`, keyed per entry by
 * k_pt_area_keys; k_pt_value_add folds the two where a pass has both kinds. */

/* the pass's camera rays, pt_camera_ray per path id */
__global__ __launch_bounds__(256) void k_pt_camera_rays(uint32_t n, const PtCamSrc *__restrict__ cam, double *__restrict__ org, double *__restrict__ dir)
{
    LH_NC
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        double o[3], d[3];
        pt_camera_ray(cam, i, o, d);
        for (int c = 0; c < 3; c++) { org[3 * (size_t)i + c] = o[c]; dir[3 * (size_t)i + c] = d[c]; }
    }
}

/* what the two kernels read of a pass */
struct PtLit { float okd[3]; int use_override, depth; LhDiv spp; };

/* one streaming pass over the first counts[depth] entries: r of every hit by the rule into its pixel's sums; with `keep` r goes back into
 * `value` (three zeros for a miss) for the sink to hand out.  pt_accumulate is wave-wide: the loop's bounds are the workgroup's, every lane
 * reaches it in every iteration, an entry beyond the count or a miss with ends = false */
template <bool FIRST>
__global__ __launch_bounds__(256) void k_pt_direct(const PtLit ps, const double *__restrict__ col9, const uint32_t *__restrict__ prim_mesh,
                                                   const DevMaterial *__restrict__ materials, const uint32_t *__restrict__ counts,
                                                   const uint32_t *__restrict__ prim, const double *__restrict__ u, const double *__restrict__ v,
                                                   const uint32_t *__restrict__ path_of, const float *__restrict__ thr, float *__restrict__ value,
                                                   int keep, unsigned long long *__restrict__ accum)
{
    LH_NC
    const uint32_t n = counts[ps.depth];
    const int lane = threadIdx.x & 63;
    for (uint32_t base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u) {      /* n <= 2^30: no wrap */
        const uint32_t i = base + threadIdx.x;
        const bool in = i < n;
        const uint32_t p = in ? prim[i] : LH_MISS_PRIM;
        const uint32_t path = (FIRST ? i : (in ? path_of[i] : 0u)) & ~LH_PT_INTERIOR;
        const bool hit = p != LH_MISS_PRIM;
        float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
        if (hit) {
            float G0 = 1.0f, G1 = 1.0f, G2 = 1.0f;
            if (!FIRST) { G0 = thr[3 * (size_t)i]; G1 = thr[3 * (size_t)i + 1]; G2 = thr[3 * (size_t)i + 2]; }
            float k0 = ps.okd[0], k1 = ps.okd[1], k2 = ps.okd[2];
            if (!ps.use_override) { const DevMaterial *mp = materials + prim_mesh[p]; k0 = mp->kd[0]; k1 = mp->kd[1]; k2 = mp->kd[2]; }
            float c0 = 1.0f, c1 = 1.0f, c2 = 1.0f;
            if (col9) {
                const double *cc = col9 + 9 * (size_t)p;
                if (cc[0] == cc[0]) {
                    const double uu = u[i], vv = v[i], wgt = 1.0 - uu - vv;
                    c0 = lh_ptl_colour(cc[0], cc[3], cc[6], wgt, uu, vv);
                    c1 = lh_ptl_colour(cc[1], cc[4], cc[7], wgt, uu, vv);
                    c2 = lh_ptl_colour(cc[2], cc[5], cc[8], wgt, uu, vv);
                }
            }
            r0 = lh_ptl_direct(G0, k0, c0, value[3 * (size_t)i]);
            r1 = lh_ptl_direct(G1, k1, c1, value[3 * (size_t)i + 1]);
            r2 = lh_ptl_direct(G2, k2, c2, value[3 * (size_t)i + 2]);
        }
        if (keep && in) { value[3 * (size_t)i] = r0; value[3 * (size_t)i + 1] = r1; value[3 * (size_t)i + 2] = r2; }
        pt_accumulate(accum, lh_div(path, ps.spp), hit, r0, r1, r2, lane);
    }
}

/* a pass with both kinds of light (lh_ptl.h): `value` holds the delta stage's answer per entry, `area` the area stage's; value_k = delta_k + area_k
 * becomes the entry's one value, in place, before k_pt_direct reads it.  One streaming pass over counts[depth] entries, three floats each; a miss's
 * slots hold what the stages left there and nobody reads them */
__global__ __launch_bounds__(256) void k_pt_value_add(int depth, const uint32_t *__restrict__ counts, float *__restrict__ value, const float *__restrict__ area)
{
    LH_NC
    const uint32_t n = counts[depth];
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u)
        for (int c = 0; c < 3; c++) value[3 * (size_t)i + c] = lh_ptl_value(value[3 * (size_t)i + c], area[3 * (size_t)i + c]);
}

/* the keys of bounce `depth`'s entries for the area stage's generator (lh_ptl.h): one streaming pass over counts[depth] entries, path word ->
 * (pixel of the pass, sample) -> frame pixel (pt_pixel) -> lh_ptl_area_key, one 8-byte store per entry.  cam: the pass as k_pt_begin wrote it */
template <bool FIRST>
__global__ __launch_bounds__(256) void k_pt_area_keys(int depth, int spp_total, const PtCamSrc *__restrict__ cam, const uint32_t *__restrict__ counts,
                                                      const uint32_t *__restrict__ path_of, unsigned long long *__restrict__ key)
{
    const uint32_t n = counts[depth];
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t path = (FIRST ? i : path_of[i]) & ~LH_PT_INTERIOR;
        const uint32_t pix = lh_div(path, cam->dv.spp);
        int px, py;
        pt_pixel(pix, cam->x0, cam->y0, cam->w, cam->band_rows, cam->band_stride, cam->dv, px, py);
        key[i] = lh_ptl_area_key(px, py, cam->cam.width, spp_total, cam->s0, (int)(path - pix * (uint32_t)cam->spp));
    }
}

/* the caller's arrays (lh_pt_sink_t), each may be NULL */
struct PtSinkOut { uint32_t *path, *depth; double *org, *dir; uint32_t *prim; double *t, *u, *v; float *thr, *direct; unsigned long long capacity; };

/* bounce `depth`'s entries, misses included, behind those of the bounces before it: entry i at record counts[0] + .. + counts[depth - 1] + i,
 * the slot order of the bounce; a record at or beyond the capacity is not written.  direct (or NULL: no lights): what k_pt_direct kept */
template <bool FIRST>
__global__ __launch_bounds__(256) void k_pt_sink(int depth, const uint32_t *__restrict__ counts, const double *__restrict__ org, const double *__restrict__ dir,
                                                 const uint32_t *__restrict__ prim, const double *__restrict__ t, const double *__restrict__ u,
                                                 const double *__restrict__ v, const uint32_t *__restrict__ path_of, const float *__restrict__ thr,
                                                 const float *__restrict__ direct, const PtSinkOut o)
{
    __shared__ unsigned long long sfirst;
    if (threadIdx.x < 64) {          /* the block's own sum of the earlier bounces' counts, by its first wave */
        unsigned long long sum = 0ull;
        for (int k = (int)threadIdx.x; k < depth; k += 64) sum += counts[k];
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if (threadIdx.x == 0) sfirst = sum;
    }
    __syncthreads();
    const unsigned long long first = sfirst;
    const uint32_t n = counts[depth];
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const unsigned long long r = first + i;
        if (r >= o.capacity) continue;
        if (o.path) o.path[r] = (FIRST ? i : path_of[i]) & ~LH_PT_INTERIOR;
        if (o.depth) o.depth[r] = (uint32_t)depth;
        if (o.org) for (int c = 0; c < 3; c++) o.org[3 * r + c] = org[3 * (size_t)i + c];
        if (o.dir) for (int c = 0; c < 3; c++) o.dir[3 * r + c] = dir[3 * (size_t)i + c];
        if (o.prim) o.prim[r] = prim[i];
        if (o.t) o.t[r] = t[i];
        if (o.u) o.u[r] = u[i];
        if (o.v) o.v[r] = v[i];
        if (o.thr) for (int c = 0; c < 3; c++) o.thr[3 * r + c] = FIRST ? 1.0f : thr[3 * (size_t)i + c];
        if (o.direct) for (int c = 0; c < 3; c++) o.direct[3 * r + c] = (direct && prim[i] != LH_MISS_PRIM) ? direct[3 * (size_t)i + c] : 0.0f;
    }
}

} /* namespace */

/* ---- host side -------------------------------------------------------------- */

static Region make_region(int x0, int w, int nbands, int band_rows, const int *d_band_y0, int y0, int height)
{
    Region rg; rg.x0 = x0; rg.w = w; rg.band_rows = band_rows; rg.nbands = nbands; rg.height = height; rg.y0 = y0; rg.band_y0 = d_band_y0;
    return rg;
}

/* d_band_y0 NULL: one band starting at y0 (a rectangle); height_limit: lines at or beyond it produce missing rays
 * (pass INT_MAX-like for "no limit": the plain rectangle entry points never clip) */
extern "C" int lh_render_launch_primary_region(const lh_camera_t *cam, int x0, int w, int nbands, int band_rows, const int *d_band_y0,
                                               int y0, int height_limit, int xs, int ys, double *d_org, double *d_dir, void *stream)
{
    DevCamera c;
    for (int i = 0; i < 16; i++) c.c2w[i] = cam->cam2world[i];
    c.flength = cam->flength; c.width = cam->width; c.height = cam->height; c.rh = cam->rh; c.ortho = cam->ortho;
    const size_t total = (size_t)w * band_rows * nbands * xs * ys;
    if (total == 0) return 0;
    hipLaunchKernelGGL(k_primary_rays, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       c, make_region(x0, w, nbands, band_rows, d_band_y0, y0, height_limit), xs, ys, d_org, d_dir);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int lh_render_launch_primary(const lh_camera_t *cam, int x0, int y0, int w, int h, int xs, int ys,
                                        double *d_org, double *d_dir, void *stream)
{
    return lh_render_launch_primary_region(cam, x0, w, 1, h, NULL, y0, 0x7fffffff, xs, ys, d_org, d_dir, stream);
}

extern "C" int lh_render_launch_compact(const lh_dev_scene_t *sc, const double *d_nrm9, size_t n, const double *d_org,
                                        const double *d_dir, const uint32_t *d_prim, const double *d_t,
                                        const double *d_u, const double *d_v, uint32_t *d_block_counts,
                                        uint32_t *d_slot_of_sample, double *d_hitrec,
                                        unsigned long long *d_slot_key, int x0, int w, int nbands, int band_rows,
                                        const int *d_band_y0, int y0, int spp, int full_width,
                                        unsigned long long *d_total, double eps, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return 0;
    const unsigned nb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_hit_count, dim3(nb), dim3(256), 0, s, n, d_prim, d_block_counts);
    hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, s, nb, d_block_counts, d_total);
    hipLaunchKernelGGL(eps == 1.0e-6 ? k_ao_setup<false> : k_ao_setup<true>, dim3(nb), dim3(256), 0, s, n, *sc, d_nrm9, d_org, d_dir, d_prim, d_t, d_u, d_v,
                       d_block_counts, d_slot_of_sample, d_hitrec, d_slot_key,
                       make_region(x0, w, nbands, band_rows, d_band_y0, y0, 0x7fffffff), spp, full_width, eps);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int lh_render_launch_ao_rays(size_t nslots, int ntheta, int nphi, unsigned long long seed,
                                        const double *d_hitrec, const double *d_rnd,
                                        const unsigned long long *d_slot_key, double *d_org, double *d_dir, void *stream)
{
    const size_t total = nslots * (size_t)(ntheta * nphi);
    if (total == 0) return 0;
    hipLaunchKernelGGL(k_ao_rays, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       nslots, ntheta, nphi, seed, d_hitrec, d_rnd, d_slot_key, d_org, d_dir);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* nslots_max: the bound the arrays were sized for; the kernel reads the count at d_nslots */
extern "C" int lh_render_launch_ao_rays_counted(size_t nslots_max, const unsigned long long *d_nslots, int ntheta, int nphi,
                                                unsigned long long seed, const double *d_hitrec, const double *d_rnd,
                                                const unsigned long long *d_slot_key, double *d_org, double *d_dir, void *stream)
{
    const size_t total = nslots_max * (size_t)(ntheta * nphi), nb = (total + 255) / 256;
    if (total == 0) return 0;
    if (nb > 0x7fffffffu) return -1;
    hipLaunchKernelGGL(k_ao_rays_counted, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream,
                       d_nslots, ntheta, nphi, seed, d_hitrec, d_rnd, d_slot_key, d_org, d_dir);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* the environment gather's resolves -- a group of LH_ENV_GROUP lanes per pixel / list entry -- read the stage through an EnvGather.  adir: the
 * materialised directions, or NULL: the fused stage (the directions are made again from the hit records and keys).  Under a sky the environment is none */
static EnvGather env_gather(const lh_gather_left_t &g)
{
    const lh_env_src_t none = {{0.0f, 0.0f, 0.0f}, NULL, 0, 0};
    EnvGather gx;
    gx.ntheta = g.ntheta; gx.nphi = g.nphi; gx.seed = g.seed; gx.hitrec = g.hitrec; gx.slot_key = g.key; gx.adir = g.adir; gx.occ = g.occ;
    gx.scale = g.scale; gx.env = env_of(g.sky ? none : *g.env);
    return gx;
}

/* a call's n lights (HOST memory) as the kernels take them; -1: no table, or a count outside 1 .. LH_LIGHTS_MAX */
static int light_tab(const lh_light_t *lights, int n, lh_light_tab_t *tab)
{
    if (!lights || n < 1 || n > LH_LIGHTS_MAX) return -1;
    memset(tab, 0, sizeof(*tab));
    memcpy(tab->l, lights, sizeof(lh_light_t) * (size_t)n);
    return 0;
}

/* the resolve of a tile: what the stage left (g, by its kind and light) into the region's pixels (to).  to->tex NULL: no mesh has a texture -- the
 * kernel and the arguments of every frame before textures; the sun-and-sky gather has no texture multiply (ambientocclusion.c:369-375) */
extern "C" int lh_render_launch_tile_resolve(const lh_resolve_tile_t *to, const lh_gather_left_t *g, void *stream)
{
    const int w = to->w, h = to->h, band_rows = to->band_rows, xs = to->xs, ys = to->ys, N = g->ntheta * g->nphi;
    const size_t total = (size_t)w * h, per = g->kind == LH_GATHER_ENV ? 256 / LH_ENV_GROUP : 256, nb = (total + per - 1) / per;
    hipStream_t s = (hipStream_t)stream;
    lh_light_tab_t tab;
    if (total == 0) return 0;
    if (nb > 0x7fffffffu) return -1;
    const dim3 grid((unsigned)nb), block(256);
    switch (g->kind) {
    case LH_GATHER_AO:
        if (to->tex) hipLaunchKernelGGL(k_ao_resolve_tex, grid, block, 0, s, w, h, band_rows, xs, ys, N, to->slot_of_sample, g->occ, g->occ_count, to->rgb, g->total, *to->tex);
        else hipLaunchKernelGGL(k_ao_resolve, grid, block, 0, s, w, h, band_rows, xs, ys, N, to->slot_of_sample, g->occ, g->occ_count, to->rgb, g->total);
        break;
    case LH_GATHER_DIRT:
        if (to->tex) hipLaunchKernelGGL(k_dirt_resolve_tex, grid, block, 0, s, w, h, band_rows, xs, ys, N, g->near_clip, g->far_clip, to->slot_of_sample, g->t, to->rgb, g->total, *to->tex);
        else hipLaunchKernelGGL(k_dirt_resolve, grid, block, 0, s, w, h, band_rows, xs, ys, N, g->near_clip, g->far_clip, to->slot_of_sample, g->t, to->rgb, g->total);
        break;
    case LH_GATHER_ENV:
        if (g->sky) hipLaunchKernelGGL(k_sky_resolve, grid, block, 0, s, w, h, band_rows, xs, ys, env_gather(*g), *g->sky, g->sun_occ, to->slot_of_sample, to->rgb, g->total);
        else if (to->tex) hipLaunchKernelGGL(k_env_resolve_tex, grid, block, 0, s, w, h, band_rows, xs, ys, env_gather(*g), to->slot_of_sample, to->rgb, g->total, *to->tex);
        else hipLaunchKernelGGL(k_env_resolve, grid, block, 0, s, w, h, band_rows, xs, ys, env_gather(*g), to->slot_of_sample, to->rgb, g->total);
        break;
    case LH_GATHER_LIGHT:
        if (light_tab(g->lights, N, &tab) != 0) return -1;
        hipLaunchKernelGGL(k_light_resolve, grid, block, 0, s, w, h, band_rows, xs, ys, LightGather{N, g->hitrec, g->occ}, to->slot_of_sample, to->rgb, g->total, tab);
        break;
    case LH_GATHER_AREA:
        if (!g->area || g->area->L != g->nphi || g->area->S != g->ntheta) return -1;
        hipLaunchKernelGGL(k_area_resolve, grid, block, 0, s, w, h, band_rows, xs, ys, AreaGather{g->hitrec, g->key, g->seed, g->occ}, to->slot_of_sample, to->rgb,
                           g->total, *g->area);
        break;
    default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* ... and of a batch: into the two per-ray outputs of the list's rays (either may be NULL; slot_of_entry NULL: an empty scene) */
extern "C" int lh_render_launch_list_resolve(const lh_resolve_list_t *to, const lh_gather_left_t *g, void *stream)
{
    if (to->n_list == 0) return 0;
    if (to->n_list >= ((size_t)1 << 31) || to->n_rays >= ((size_t)1 << 31)) return -1;
    const BatchList bl = {to->index, to->count, (uint32_t)to->n_list, (uint32_t)to->n_rays};
    const size_t per = g->kind == LH_GATHER_ENV ? 256 / LH_ENV_GROUP : 256;
    const dim3 grid((unsigned)((to->n_list + per - 1) / per)), block(256);
    const int N = g->ntheta * g->nphi;
    hipStream_t s = (hipStream_t)stream;
    lh_light_tab_t tab;
    switch (g->kind) {
    case LH_GATHER_AO:
        hipLaunchKernelGGL(k_ao_batch_resolve, grid, block, 0, s, bl, N, to->slot_of_entry, g->occ, g->occ_count, to->count_out, to->value_out, g->total);
        break;
    case LH_GATHER_DIRT:
        hipLaunchKernelGGL(k_dirt_batch_resolve, grid, block, 0, s, bl, N, g->near_clip, g->far_clip, to->slot_of_entry, g->t, to->count_out, to->value_out, g->total);
        break;
    case LH_GATHER_ENV:
        if (g->sky) hipLaunchKernelGGL(k_sky_batch_resolve, grid, block, 0, s, bl, env_gather(*g), *g->sky, g->sun_occ, to->slot_of_entry, to->count_out, to->value_out, g->total);
        else hipLaunchKernelGGL(k_env_batch_resolve, grid, block, 0, s, bl, env_gather(*g), to->slot_of_entry, to->count_out, to->value_out, g->total);
        break;
    case LH_GATHER_LIGHT:
        if (light_tab(g->lights, N, &tab) != 0) return -1;
        hipLaunchKernelGGL(k_light_batch_resolve, grid, block, 0, s, bl, LightGather{N, g->hitrec, g->occ}, to->slot_of_entry, to->count_out, to->value_out, g->total, tab);
        break;
    case LH_GATHER_AREA:
        if (!g->area || g->area->L != g->nphi || g->area->S != g->ntheta) return -1;
        hipLaunchKernelGGL(k_area_batch_resolve, grid, block, 0, s, bl, AreaGather{g->hitrec, g->key, g->seed, g->occ}, to->slot_of_entry, to->count_out,
                           to->value_out, g->total, *g->area);
        break;
    default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int lh_render_launch_tex_batch(size_t n_list, size_t n_rays, const uint32_t *d_index, const uint32_t *d_count,
                                          const lh_tex_args_t *tex, uint32_t ntris, double *d_rgba, void *stream)
{
    if (n_list == 0) return 0;
    if (n_list >= ((size_t)1 << 31) || n_rays >= ((size_t)1 << 31)) return -1;
    const BatchList bl = {d_index, d_count, (uint32_t)n_list, (uint32_t)n_rays};
    hipLaunchKernelGGL(k_tex_batch, dim3((unsigned)((n_list + 255) / 256)), dim3(256), 0, (hipStream_t)stream, bl, *tex, ntris, d_rgba);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* the compaction of a batch's hits (list-aware k_hit_count, k_scan_blocks, k_ao_batch_setup); d_total: the number of hits (64 bits,
 * where lh_launch_trace_gather reads it); d_nslots32 (or NULL): the same as one uint32 */
extern "C" int lh_render_launch_batch_compact(const lh_dev_scene_t *sc, const double *d_nrm9, size_t n_list, size_t n_rays,
                                              const uint32_t *d_index, const uint32_t *d_count, const double *d_org, const double *d_dir,
                                              const uint32_t *d_prim, const double *d_t, const double *d_u, const double *d_v,
                                              const unsigned long long *d_key, uint32_t *d_block_counts, uint32_t *d_slot_of_entry,
                                              double *d_hitrec, unsigned long long *d_slot_key, unsigned long long *d_total,
                                              uint32_t *d_nslots32, double eps, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (n_list == 0 || n_list >= ((size_t)1 << 31) || n_rays >= ((size_t)1 << 31)) return n_list == 0 ? 0 : -1;
    const unsigned nb = (unsigned)((n_list + 255) / 256);
    const BatchList bl = {d_index, d_count, (uint32_t)n_list, (uint32_t)n_rays};
    hipLaunchKernelGGL(k_ao_batch_count, dim3(nb), dim3(256), 0, s, bl, d_prim, d_block_counts);
    hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, s, nb, d_block_counts, d_total);
    hipLaunchKernelGGL(eps == 1.0e-6 ? k_ao_batch_setup<false> : k_ao_batch_setup<true>, dim3(nb), dim3(256), 0, s, bl, *sc, d_nrm9, d_org, d_dir, d_prim, d_t, d_u, d_v, d_key,
                       d_block_counts, d_total, d_slot_of_entry, d_hitrec, d_slot_key, d_nslots32, eps);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* the bound array of a materialised dirt stage; the fetches alone of the sky and of the environment; the sun's rays */
extern "C" int lh_render_launch_dirt_bounds(size_t n, double far_clip, double *d_bound, void *stream)
{
    if (n == 0) return 0;
    if ((n + 255) / 256 > 0x7fffffffu) return -1;
    hipLaunchKernelGGL(k_dirt_bounds, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, far_clip, d_bound);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int lh_render_launch_sky_fetch(size_t n, const lh_sky_src_t *sky, const double *d_dir, float *d_rgb, void *stream)
{
    if (n == 0) return 0;
    if ((n + 255) / 256 > 0x7fffffffu) return -1;
    hipLaunchKernelGGL(k_sky_batch, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, *sky, d_dir, d_rgb);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int lh_render_launch_sun_rays(size_t nslots, const unsigned long long *d_nslots, const double *d_hitrec, const double sun_dir[3],
                                         double *d_org, double *d_dir, void *stream)
{
    if (nslots == 0) return 0;
    if ((nslots + 255) / 256 > 0x7fffffffu) return -1;
    hipLaunchKernelGGL(k_sun_rays, dim3((unsigned)((nslots + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nslots, d_nslots, d_hitrec,
                       sun_dir[0], sun_dir[1], sun_dir[2], d_org, d_dir);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* the shadow rays and bounds of nslots hit records to the n lights of a HOST table (d_nslots or NULL: the slot count on the device, nslots its upper bound) */
extern "C" int lh_render_launch_light_rays(size_t nslots, const unsigned long long *d_nslots, const lh_light_t *lights, int n, const double *d_hitrec,
                                           double *d_org, double *d_dir, double *d_tmax, void *stream)
{
    lh_light_tab_t tab;
    if (nslots == 0) return 0;
    if (light_tab(lights, n, &tab) != 0) return -1;
    const size_t items = nslots * (size_t)n;
    if ((items + 255) / 256 > 0x7fffffffu) return -1;
    hipLaunchKernelGGL(k_light_rays, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nslots, d_nslots, n, d_hitrec, d_org, d_dir, d_tmax, tab);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* the rays, bounds and weights (d_weight or NULL) of nslots hit records' area-light items (d_nslots or NULL: the slot count on the device, nslots its upper bound) */
extern "C" int lh_render_launch_area_rays(size_t nslots, const unsigned long long *d_nslots, const lh_area_tab_t *area, unsigned long long seed,
                                          const double *d_hitrec, const unsigned long long *d_slot_key, double *d_org, double *d_dir, double *d_tmax,
                                          double *d_weight, void *stream)
{
    if (nslots == 0) return 0;
    if (!area || area->L < 1 || area->L > LH_AREA_LIGHTS_MAX || area->S < 1 || area->S > LH_AREA_SAMPLES_MAX || !area->emitters) return -1;
    const size_t items = nslots * (size_t)area->L * (size_t)area->S;
    if ((items + 255) / 256 > 0x7fffffffu) return -1;
    hipLaunchKernelGGL(k_area_rays, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nslots, d_nslots, seed, d_hitrec, d_slot_key,
                       d_org, d_dir, d_tmax, d_weight, *area);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int lh_render_launch_env_fetch(size_t n, const lh_env_src_t *env, const double *d_dir, float *d_rgb, void *stream)
{
    if (n == 0) return 0;
    if ((n + 255) / 256 > 0x7fffffffu) return -1;
    hipLaunchKernelGGL(k_env_batch, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, env_of(*env), d_dir, d_rgb);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* lh_material_t -> the device record (lh_pt.h: + channel averages, 1 / P(lobe)) */
static void pack_material(const lh_material_t *m, DevMaterial *d)
{
    memset(d, 0, sizeof(*d));
    for (int k = 0; k < 3; k++) { d->kd[k] = m->kd[k]; d->ks[k] = m->ks[k]; d->kt[k] = m->kt[k]; }
    d->ior = m->ior;
    d->ad = ((double)m->kd[0] + m->kd[1] + m->kd[2]) / 3.0; d->as = ((double)m->ks[0] + m->ks[1] + m->ks[2]) / 3.0;
    d->at = ((double)m->kt[0] + m->kt[1] + m->kt[2]) / 3.0;
    d->asum9 = ((double)m->kd[0] + m->kd[1] + m->kd[2] + m->ks[0] + m->ks[1] + m->ks[2] + m->kt[0] + m->kt[1] + m->kt[2]) / 3.0;
    d->wd = (float)(1.0 / d->ad); d->ws = (float)(1.0 / d->as); d->wt = (float)(1.0 / d->at);
}
extern "C" size_t lh_pt_material_bytes(void) { return sizeof(DevMaterial); }
extern "C" void lh_pt_material_pack(const lh_material_t *m, void *out) { pack_material(m, (DevMaterial *)out); }

/* start of a pass: counts[0] = its paths, the camera-ray source (PtCamSrc) into d_cam */
extern "C" int lh_pt_launch_begin(const lh_camera_t *cam, int x0, int y0, int w, int h, int band_rows, int band_stride, int spp, int s0,
                                  unsigned long long seed, void *d_cam, uint32_t *d_counts, int ncounts, void *stream)
{
    PtCamSrc c;
    memset(&c, 0, sizeof(c));
    for (int i = 0; i < 16; i++) c.cam.c2w[i] = cam->cam2world[i];
    c.cam.flength = cam->flength; c.cam.width = cam->width; c.cam.height = cam->height; c.cam.rh = cam->rh; c.cam.ortho = cam->ortho;
    c.seed = seed; c.x0 = x0; c.y0 = y0; c.w = w; c.spp = spp; c.s0 = s0; c.band_rows = band_rows; c.band_stride = band_stride;
    c.dv.spp = lh_div_make((uint32_t)spp); c.dv.w = lh_div_make((uint32_t)w); c.dv.rows = lh_div_make((uint32_t)band_rows);
    const size_t total = (size_t)w * h * spp;
    hipLaunchKernelGGL(k_pt_begin, dim3(1), dim3(256), 0, (hipStream_t)stream, d_counts, (uint32_t)total, ncounts, c, (PtCamSrc *)d_cam);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" size_t lh_pt_cam_bytes(void) { return sizeof(PtCamSrc); }

/* the shading pass of bounce `depth` over counts[depth] paths (at most n_max); survivors are counted into counts[depth + 1] */
extern "C" int lh_pt_launch_shade(size_t n_max, const lh_dev_scene_t *sc, const double *d_nrm9, const double *d_col9,
                                  const uint32_t *d_prim_mesh, const void *d_materials, const lh_material_t *override_mat,
                                  const float env_rgb[3], const void *d_env_map, int env_w, int env_h, int ref_weights,
                                  int depth, int max_depth, unsigned long long seed, int s0, int spp, int x0, int y0, int w,
                                  int band_rows, int band_stride, int full_width, const void *d_cam, uint32_t *d_counts, const double *d_org, const double *d_dir, const uint32_t *d_prim,
                                  const double *d_t, const double *d_u, const double *d_v, const uint32_t *d_path_of,
                                  const float *d_thr, unsigned long long *d_accum, double *d_org2, double *d_dir2, uint32_t *d_path_of2,
                                  float *d_thr2, int ncus, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (n_max == 0) return 0;
    PtPass ps;
    memset(&ps, 0, sizeof(ps));
    if (override_mat) pack_material(override_mat, &ps.override_mat);
    ps.env.rgb[0] = env_rgb[0]; ps.env.rgb[1] = env_rgb[1]; ps.env.rgb[2] = env_rgb[2];
    ps.env.map = (const float4 *)d_env_map; ps.env.w = env_w; ps.env.h = env_h;
    ps.cam = (const PtCamSrc *)d_cam;
    ps.seed = seed; ps.use_override = override_mat != NULL; ps.ref_weights = ref_weights; ps.depth = depth; ps.max_depth = max_depth;
    ps.s0 = s0; ps.spp = spp; ps.x0 = x0; ps.y0 = y0; ps.w = w; ps.band_rows = band_rows; ps.band_stride = band_stride; ps.full_width = full_width;
    ps.dv.spp = lh_div_make((uint32_t)spp); ps.dv.w = lh_div_make((uint32_t)w); ps.dv.rows = lh_div_make((uint32_t)band_rows);
    const size_t spans = (n_max + 256 * LH_PT_ITEMS * LH_PT_ROUNDS - 1) / (256 * LH_PT_ITEMS * LH_PT_ROUNDS);
    const size_t cus = (size_t)(ncus > 0 ? ncus : 256);
    const unsigned nb = (unsigned)(spans < cus * 16 ? spans : cus * 16);                    /* decide: 2 x the eight resident workgroups of a CU */
    const size_t blocks = (n_max + 255) / 256;
    const unsigned ns = (unsigned)(blocks < cus * 16 ? blocks : cus * 16);                  /* scatter: grid-stride over the survivors counted by then */
    if (depth == 0) {
        if (d_env_map)
            hipLaunchKernelGGL((k_pt_decide<true, true>), dim3(nb), dim3(256), 0, s, ps, d_prim_mesh, (const DevMaterial *)d_materials, d_counts, d_dir, d_prim,
                               d_path_of, d_thr, d_accum, d_path_of2);
        else
            hipLaunchKernelGGL((k_pt_decide<true, false>), dim3(nb), dim3(256), 0, s, ps, d_prim_mesh, (const DevMaterial *)d_materials, d_counts, d_dir, d_prim,
                               d_path_of, d_thr, d_accum, d_path_of2);
        hipLaunchKernelGGL((k_pt_scatter<true>), dim3(ns), dim3(256), 0, s, ps, *sc, d_nrm9, d_col9, d_prim_mesh, (const DevMaterial *)d_materials,
                           (const uint32_t *)d_counts, d_org, d_dir, d_prim, d_t, d_u, d_v, d_path_of, d_thr, d_org2, d_dir2, d_path_of2, d_thr2);
    } else {
        if (d_env_map)
            hipLaunchKernelGGL((k_pt_decide<false, true>), dim3(nb), dim3(256), 0, s, ps, d_prim_mesh, (const DevMaterial *)d_materials, d_counts, d_dir, d_prim,
                               d_path_of, d_thr, d_accum, d_path_of2);
        else
            hipLaunchKernelGGL((k_pt_decide<false, false>), dim3(nb), dim3(256), 0, s, ps, d_prim_mesh, (const DevMaterial *)d_materials, d_counts, d_dir, d_prim,
                               d_path_of, d_thr, d_accum, d_path_of2);
        hipLaunchKernelGGL((k_pt_scatter<false>), dim3(ns), dim3(256), 0, s, ps, *sc, d_nrm9, d_col9, d_prim_mesh, (const DevMaterial *)d_materials,
                           (const uint32_t *)d_counts, d_org, d_dir, d_prim, d_t, d_u, d_v, d_path_of, d_thr, d_org2, d_dir2, d_path_of2, d_thr2);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* streaming grids of the lit pass's kernels: a workgroup per 256 entries of the upper bound, at most 16 per compute unit */
static unsigned pt_lit_grid(size_t n_max, int ncus)
{
    const size_t blocks = (n_max + 255) / 256, cus = (size_t)(ncus > 0 ? ncus : 256);
    return (unsigned)(blocks < cus * 16 ? blocks : cus * 16);
}

/* the camera rays of the pass (d_cam: what lh_pt_launch_begin wrote) into d_org / d_dir */
extern "C" int lh_pt_launch_camera_rays(size_t n, const void *d_cam, double *d_org, double *d_dir, int ncus, void *stream)
{
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_pt_camera_rays, dim3(pt_lit_grid(n, ncus)), dim3(256), 0, (hipStream_t)stream, (uint32_t)n, (const PtCamSrc *)d_cam, d_org, d_dir);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* the direct light of bounce `depth` (lh_ptl.h) over counts[depth] entries (at most n_max): d_value holds the light stage's answer per entry and,
 * with keep, r afterwards */
extern "C" int lh_pt_launch_direct(size_t n_max, const double *d_col9, const uint32_t *d_prim_mesh, const void *d_materials,
                                   const lh_material_t *override_mat, int depth, int spp, const uint32_t *d_counts, const uint32_t *d_prim,
                                   const double *d_u, const double *d_v, const uint32_t *d_path_of, const float *d_thr, float *d_value, int keep,
                                   unsigned long long *d_accum, int ncus, void *stream)
{
    if (n_max == 0) return 0;
    PtLit ps;
    memset(&ps, 0, sizeof(ps));
    if (override_mat) for (int k = 0; k < 3; k++) ps.okd[k] = override_mat->kd[k];
    ps.use_override = override_mat != NULL; ps.depth = depth; ps.spp = lh_div_make((uint32_t)spp);
    const dim3 grid(pt_lit_grid(n_max, ncus));
    if (depth == 0)
        hipLaunchKernelGGL((k_pt_direct<true>), grid, dim3(256), 0, (hipStream_t)stream, ps, d_col9, d_prim_mesh, (const DevMaterial *)d_materials, d_counts,
                           d_prim, d_u, d_v, d_path_of, d_thr, d_value, keep, d_accum);
    else
        hipLaunchKernelGGL((k_pt_direct<false>), grid, dim3(256), 0, (hipStream_t)stream, ps, d_col9, d_prim_mesh, (const DevMaterial *)d_materials, d_counts,
                           d_prim, d_u, d_v, d_path_of, d_thr, d_value, keep, d_accum);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* the area stage's keys of bounce `depth` (lh_ptl.h) for counts[depth] entries (at most n_max) into d_key; d_cam: what lh_pt_launch_begin wrote */
extern "C" int lh_pt_launch_area_keys(size_t n_max, int depth, int spp_total, const void *d_cam, const uint32_t *d_counts, const uint32_t *d_path_of,
                                      unsigned long long *d_key, int ncus, void *stream)
{
    if (n_max == 0) return 0;
    const dim3 grid(pt_lit_grid(n_max, ncus));
    if (depth == 0)
        hipLaunchKernelGGL((k_pt_area_keys<true>), grid, dim3(256), 0, (hipStream_t)stream, depth, spp_total, (const PtCamSrc *)d_cam, d_counts, d_path_of, d_key);
    else
        hipLaunchKernelGGL((k_pt_area_keys<false>), grid, dim3(256), 0, (hipStream_t)stream, depth, spp_total, (const PtCamSrc *)d_cam, d_counts, d_path_of, d_key);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* both kinds of light: d_value (the delta stage's answer) += d_area (the area stage's) over counts[depth] entries, before lh_pt_launch_direct */
extern "C" int lh_pt_launch_value_add(size_t n_max, int depth, const uint32_t *d_counts, float *d_value, const float *d_area, int ncus, void *stream)
{
    if (n_max == 0) return 0;
    hipLaunchKernelGGL(k_pt_value_add, dim3(pt_lit_grid(n_max, ncus)), dim3(256), 0, (hipStream_t)stream, depth, d_counts, d_value, d_area);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* bounce `depth`'s entries into the caller's sink; d_direct: what lh_pt_launch_direct kept, or NULL (no lights) */
extern "C" int lh_pt_launch_sink(size_t n_max, int depth, const uint32_t *d_counts, const double *d_org, const double *d_dir, const uint32_t *d_prim,
                                 const double *d_t, const double *d_u, const double *d_v, const uint32_t *d_path_of, const float *d_thr,
                                 const float *d_direct, const lh_pt_sink_t *sink, int ncus, void *stream)
{
    if (n_max == 0) return 0;
    const PtSinkOut o = {(uint32_t *)sink->d_path, (uint32_t *)sink->d_depth, (double *)sink->d_org, (double *)sink->d_dir, (uint32_t *)sink->d_prim,
                         (double *)sink->d_t, (double *)sink->d_u, (double *)sink->d_v, (float *)sink->d_thr, (float *)sink->d_direct,
                         (unsigned long long)sink->capacity};
    const dim3 grid(pt_lit_grid(n_max, ncus));
    if (depth == 0)
        hipLaunchKernelGGL((k_pt_sink<true>), grid, dim3(256), 0, (hipStream_t)stream, depth, d_counts, d_org, d_dir, d_prim, d_t, d_u, d_v, d_path_of, d_thr, d_direct, o);
    else
        hipLaunchKernelGGL((k_pt_sink<false>), grid, dim3(256), 0, (hipStream_t)stream, depth, d_counts, d_org, d_dir, d_prim, d_t, d_u, d_v, d_path_of, d_thr, d_direct, o);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int lh_pt_launch_resolve(int w, int h, int band_rows, float inv_total_spp, unsigned long long *d_accum, float *d_rgb, void *stream)
{
    const size_t total = (size_t)w * h;
    if (total == 0) return 0;
    hipLaunchKernelGGL(k_pt_resolve, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       w, h, band_rows, inv_total_spp, d_accum, d_rgb);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int lh_render_launch_state_build(size_t n, const lh_dev_scene_t *sc, const double *d_nrm9, const double *d_col9,
                                            const double *d_tan9, const double *d_bin9, const double *d_st6, const uint8_t *d_inside,
                                            const double *d_org, const double *d_dir, const uint32_t *d_prim, const double *d_t,
                                            const double *d_u, const double *d_v, double *d_state, void *stream)
{
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_state_build, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, *sc, d_nrm9, d_col9,
                       d_tan9, d_bin9, d_st6, d_inside, d_org, d_dir, d_prim, d_t, d_u, d_v, d_state);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

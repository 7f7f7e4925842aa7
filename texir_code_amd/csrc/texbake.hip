// The radiance atlas and the index texture from calibrated panoramas (no reference counterpart for the selection: the reference's private capture pipeline
// writes 0.png; tools/trans_hdr_tex.py:16-61 repackHDRTexture only gathers the panoramas' pixels through its codes, and utils/Pano2Cube.py:57-82 fixes which
// panorama pixel a direction reads).  For every listed texel: among the views that the texel faces, whose panorama pixel is valid and that see it
// un-occluded, the one with the largest cosine over squared distance; an exact tie goes to the lowest view id.  include/texir_hip.h (texir_atlas_bake) states
// the rule, the float32 operation sequence and its rounding bound; this file follows that text operation by operation (contraction off).
//
// One lane is one listed texel, 64 per wave over the caller's id list (Morton order: 64 neighbouring texels looking at ONE camera are the most coherent ray
// bundle the traversal gets).  The views are walked in ascending order by the whole wave; the view's matrix and position are wave-uniform (scalar) loads.
// A lane traces a view only when it faces it, its pixel is valid and its score beats the lane's best so far (views come in ascending order, so a tie never
// replaces an earlier view: the lowest id keeps it); a view no lane of the wave needs is skipped by ballot.  The segment test is ONE closest-hit query
// (device_common.h trace_closest<false, kLstk, WIDTH>, the single-ray kernels' shared form) with org = pos, dir = camera - pos: the view is occluded iff the closest hit has t < 1.
// ANY (texir_atlas_bake_any): the same question put to trace_occluded<kLstk, WIDTH>(..., 0, 1), which stops at the first accepted triangle: the same
// answer per pair (see there), hence the same view, pix, rgb and counts, bit for bit.
// The outcome per texel is a pure function of the inputs: no atomics on results, nothing depends on the list's order or the launch shape.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace texir {

// every product, sum and quotient below is its own rounded float32 operation: the header states the arithmetic and the tests restate it
#pragma clang fp contract(off)

constexpr float kPi32 = 3.14159274101257324f, kHalfPi32 = 1.57079637050628662f;

// the pixel rule: t = W (p, 1) -> (row, col) of an h x w equirectangular panorama; false when |t| is zero or not finite
__device__ __forceinline__ bool pano_pixel(const float* __restrict__ Wm, float px, float py, float pz, int h, int w, int& row, int& col)
{
    const float tx = ((Wm[0] * px + Wm[1] * py) + Wm[2] * pz) + Wm[3];
    const float ty = ((Wm[4] * px + Wm[5] * py) + Wm[6] * pz) + Wm[7];
    const float tz = ((Wm[8] * px + Wm[9] * py) + Wm[10] * pz) + Wm[11];
    const float r2 = (tx * tx + ty * ty) + tz * tz;
    if (!(r2 > 0.f) || !finite32(r2)) return false;
    const float r = sqrtf(r2);
    const float az = atan2f(tx, tz);
    const float q = fminf(fmaxf(ty / r, -1.f), 1.f);
    const float el = asinf(q);
    const float x = ((az / kPi32 + 1.f) * 0.5f) * (float)w;
    const float y = ((1.f - el / kHalfPi32) * 0.5f) * (float)h;
    col = (int)fminf(fmaxf(floorf(x), 0.f), (float)(w - 1));
    row = (int)fminf(fmaxf(floorf(y), 0.f), (float)(h - 1));
    return true;
}

template <int WIDTH, bool ANY>
__global__ __launch_bounds__(kBlock) void atlas_bake_kernel(SceneDev sc, const float* __restrict__ pos, const float* __restrict__ nrm, const int32_t* __restrict__ ids,
                                                            int64_t n, int64_t Nt, const float* __restrict__ cams, const float* __restrict__ cam_pos,
                                                            const uint32_t* __restrict__ panos, const uint8_t* __restrict__ valid, int K, int h, int w, float cos_min,
                                                            int32_t* __restrict__ view, int32_t* __restrict__ pix, uint32_t* __restrict__ rgb,
                                                            unsigned long long* __restrict__ stats)
{
    uint32_t cn = 0, ct = 0;
    uint32_t n_facing = 0, n_traced = 0, n_visible = 0, n_assigned = 0;
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n; base += (int64_t)gridDim.x * kBlock) {
        const int64_t i = base + threadIdx.x;
        int64_t tex = i < n ? (ids ? (int64_t)ids[i] : i) : -1;
        if (tex >= Nt) tex = -1;                                           // an id outside the atlas is not a texel: nothing is read or written for it
        const bool live = tex >= 0;
        float px = 0.f, py = 0.f, pz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
        if (live) {
            px = pos[3 * tex]; py = pos[3 * tex + 1]; pz = pos[3 * tex + 2];
            nx = nrm[3 * tex]; ny = nrm[3 * tex + 1]; nz = nrm[3 * tex + 2];
        }
        int best_k = -1, best_row = 0, best_col = 0;
        float best_s = 0.f;
        for (int k = 0; k < K; k++) {
            const float* Wm = cams + 12 * (size_t)k;                       // wave-uniform: scalar loads
            const float cx = cam_pos[3 * (size_t)k], cy = cam_pos[3 * (size_t)k + 1], cz = cam_pos[3 * (size_t)k + 2];
            const float dx = cx - px, dy = cy - py, dz = cz - pz;
            const float dd = (dx * dx + dy * dy) + dz * dz;
            const float nd = (nx * dx + ny * dy) + nz * dz;
            const float len = sqrtf(dd);
            bool need = live && dd > 0.f && nd > cos_min * len;
            int row = 0, col = 0;
            float s = 0.f;
            if (need) {
                n_facing++;
                need = pano_pixel(Wm, px, py, pz, h, w, row, col);
                if (need && valid) need = valid[((size_t)k * h + row) * w + col] != 0;
                s = nd / (dd * len);
                need = need && (best_k < 0 || s > best_s);
            }
            if (!__any(need)) continue;                                    // no lane of the wave needs this view
            if (need) {
                n_traced++;
                bool occluded;
                if constexpr (ANY) occluded = trace_occluded<kLstk, WIDTH>(sc, px, py, pz, dx, dy, dz, 0.f, 1.f);
                else {
                    const Hit hit = trace_closest<false, kLstk, WIDTH>(sc, px, py, pz, dx, dy, dz, cn, ct);
                    occluded = hit.slot >= 0 && hit.t < 1.f;
                }
                if (!occluded) {
                    n_visible++;
                    best_k = k; best_s = s; best_row = row; best_col = col;
                }
            }
        }
        if (live) {
            uint32_t r = 0u, g = 0u, b = 0u;
            if (best_k >= 0) {
                const size_t o = 3 * (((size_t)best_k * h + best_row) * w + best_col);
                r = panos[o]; g = panos[o + 1]; b = panos[o + 2];           // the pixel's bits as they are
                n_assigned++;
            }
            view[tex] = best_k;
            pix[2 * tex] = best_row; pix[2 * tex + 1] = best_col;
            rgb[3 * tex] = r; rgb[3 * tex + 1] = g; rgb[3 * tex + 2] = b;
        }
    }
    if (stats) {
        const unsigned long long a = wave_sum_u64(n_facing), b = wave_sum_u64(n_traced), c = wave_sum_u64(n_visible), d = wave_sum_u64(n_assigned);
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(stats, a); atomicAdd(stats + 1, b); atomicAdd(stats + 2, c); atomicAdd(stats + 3, d);
        }
    }
}

// the four repack*Texture gathers (tools/trans_hdr_tex.py:16-216) on the device: out[t] = imgs[view[t], pix[t]] for the listed texels, zeros where view < 0
__global__ __launch_bounds__(256) void atlas_gather_kernel(const int32_t* __restrict__ view, const int32_t* __restrict__ pix, const int32_t* __restrict__ ids, int64_t n,
                                                           int64_t Nt, const uint32_t* __restrict__ imgs, int K, int h, int w, int C, uint32_t* __restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t tex = ids ? (int64_t)ids[i] : i;
        if (tex < 0 || tex >= Nt) continue;
        const int v = view[tex], row = pix[2 * tex], col = pix[2 * tex + 1];
        const bool ok = v >= 0 && v < K && row >= 0 && row < h && col >= 0 && col < w;       // (codes are the caller's data: never read outside the images)
        const size_t o = (size_t)C * (((size_t)(ok ? v : 0) * h + (ok ? row : 0)) * w + (ok ? col : 0));
        for (int c = 0; c < C; c++) out[(size_t)C * tex + c] = ok ? imgs[o + c] : 0u;
    }
}

hipError_t launch_atlas_bake(const SceneDev& sc, const float* pos, const float* nrm, const int32_t* ids, int64_t n, int64_t Nt, const float* cams, const float* cam_pos,
                             const float* panos, const uint8_t* valid, int K, int h, int w, float cos_min, int32_t* view, int32_t* pix, float* rgb,
                             unsigned long long* stats, hipStream_t st, bool any)
{
    if (n <= 0) return hipSuccess;
    const dim3 grid(grid_capped(kBlock, n));
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, st, sc, pos, nrm, ids, n, Nt, cams, cam_pos, (const uint32_t*)panos, valid, K, h, w, cos_min, view, pix,
                           (uint32_t*)rgb, stats);
    };
    if (sc.nodes4) { if (any) go(atlas_bake_kernel<4, true>); else go(atlas_bake_kernel<4, false>); }
    else { if (any) go(atlas_bake_kernel<2, true>); else go(atlas_bake_kernel<2, false>); }
    return hipGetLastError();
}

hipError_t launch_atlas_gather(const int32_t* view, const int32_t* pix, const int32_t* ids, int64_t n, int64_t Nt, const float* imgs, int K, int h, int w, int C,
                               float* out, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(atlas_gather_kernel, dim3(grid_capped(256, n)), dim3(256), 0, st, view, pix, ids, n, Nt, (const uint32_t*)imgs, K, h, w, C, (uint32_t*)out);
    return hipGetLastError();
}

}  // namespace texir

// Several radiance textures in one traced IrT pass (include/texir_hip.h texir_irt_multi states the rule; this file follows it).
//
// The rays of irt_group_kernel<false, 4, 6> (kernels.hip) -- one texel per lane, one sample per pass, the same direction cells in the same order, the same
// closest-hit query -- are traced ONCE; the hit shader computes the footprint of shade_hit (device_common.h) and then, per texture k, the bilinear sum of
// the caller's texture k over that footprint: the float32 expression shade_hit evaluates on a scene whose texture is T_k.  So out[k] is bit for bit what
// texir_irt_generate in its 64-texel form writes after set_texture(T_k) -- K passes for the price of one traversal, and the scene's own texture (and its
// layout) is neither read nor touched.  irt_split_kernel (irtsplit.hip) is the special case T_k = tex * [label == k].
//
// The K textures arrive interleaved per texel, [Ht][Wt][K][3]: a row's two taps are 2 * K * 12 contiguous bytes (192 B at K = 8, two to three 128-byte
// lines), where K planes would touch 2 * K lines.
//
// A wave owns 64 consecutive ids of the caller's (Morton-ordered) list; a chunk is 64 texels x one part of the passes.  Chunks are dealt statically: wave w
// of the grid takes chunks w, w + waves, ... -- no work counter, no wave waits on another, every loop is bounded by N, the chunk count or the traversal's
// own bounds.  The partial sums go to partial[part][k][i][3] and irt_combine_kernel (kernels.hip) adds them in part order, so the result is a pure function of the
// inputs: list order, list cuts, launch shape and stream do not change a bit.
//
// The accumulators are registers under static indexing (loops over KMAX are unrolled; K is wave-uniform, so `q < K` is a scalar branch and textures
// q >= K are not read); the only private memory is the traversal's own overflow stack.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env.h"
#include "kernels.h"

namespace texir {

constexpr int kMultiMaxTextures = 8;

// waves per SIMD the kernel is compiled for: irt_split_kernel's (3 accumulators per texture on top of irt_group_kernel's 64 registers at 8 waves)
template <int KMAX> struct MultiWaves { static constexpr int value = KMAX <= 2 ? 6 : (KMAX <= 4 ? 5 : 4); };

// ------------------------------------------------------------------------------------------------
// hit shader: shade_hit's footprint, then one bilinear sum per texture -- separately rounded operations, as in device_common.h
// (multi_footprint repeats the first lines of shade_hit, as split_footprint does; what keeps the texts equal is the bit-identity tests of
// tests/test_gpu_irt_multi.py)
// ------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)

struct MultiTaps {
    float w00, w10, w01, w11;
    size_t o00, o10, o01, o11;       // texel offsets of the four taps in a row-major [Ht][Wt] image
};

__device__ __forceinline__ MultiTaps multi_footprint(const SceneDev& sc, int tri_slot, float bu, float bv)
{
    float u = fminf(fmaxf(bu, 0.f), 1.f), v = fminf(fmaxf(bv, 0.f), 1.f);      // :250 np.clip
    float4 a, b;
    tri_uvs(sc, tri_slot, a, b);
    float w = 1.0f - u - v;
    float gx = a.x * w + a.z * u + b.x * v;
    float gy = a.y * w + a.w * u + b.y * v;
    gx = gx * 2.f - 1.f;                  // :262
    gy = -(1.f - gy * 2.f);               // :263
    float x = ((gx + 1.f) * (float)sc.Wt - 1.f) * 0.5f, y = ((gy + 1.f) * (float)sc.Ht - 1.f) * 0.5f;
    x = fminf(fmaxf(x, 0.f), (float)(sc.Wt - 1)); y = fminf(fmaxf(y, 0.f), (float)(sc.Ht - 1));
    float x0f = floorf(x), y0f = floorf(y);
    int x0 = (int)x0f, y0 = (int)y0f;
    float wx1 = x - x0f, wx0 = 1.f - wx1, wy1 = y - y0f, wy0 = 1.f - wy1;
    int x1 = min(x0 + 1, sc.Wt - 1), y1 = min(y0 + 1, sc.Ht - 1);
    MultiTaps t;
    t.w00 = wx0 * wy0;
    t.w10 = (x0 + 1 < sc.Wt) ? wx1 * wy0 : 0.f;
    t.w01 = (y0 + 1 < sc.Ht) ? wx0 * wy1 : 0.f;
    t.w11 = (x0 + 1 < sc.Wt && y0 + 1 < sc.Ht) ? wx1 * wy1 : 0.f;
    t.o00 = (size_t)y0 * sc.Wt + x0; t.o10 = (size_t)y0 * sc.Wt + x1;
    t.o01 = (size_t)y1 * sc.Wt + x0; t.o11 = (size_t)y1 * sc.Wt + x1;
    return t;
}

// the bilinear sum of one channel of one texture
__device__ __forceinline__ float multi_tap_sum(const MultiTaps& t, float v00, float v10, float v01, float v11)
{
    float acc = v00 * t.w00;
    acc += v10 * t.w10;
    acc += v01 * t.w01;
    acc += v11 * t.w11;
    return acc;
}

#pragma clang fp contract(fast)

template <int KMAX>
__global__ __launch_bounds__(kBlock, MultiWaves<KMAX>::value) void irt_multi_kernel(SceneDev sc, const float* __restrict__ tex, const float* __restrict__ pos,
                                                                                   const float* __restrict__ nrm, const float* __restrict__ shift,
                                                                                   const int32_t* __restrict__ ids, int64_t n_ids, int N, int log2N, int mode, int K,
                                                                                   float* __restrict__ partial, int log2parts)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (wave-uniform: the chunk loop and the pass loop stay scalar)
    const int64_t gw = (int64_t)blockIdx.x * (kBlock / 64) + wave, nw = (int64_t)gridDim.x * (kBlock / 64);
    uint32_t cn = 0, ct = 0;
    const int part_cells = N >> log2parts;
    const size_t texel_floats = (size_t)3 * K;       // floats of one texel of the interleaved buffer
    // the cell order of irt_group_kernel with one sample per texel per pass (device_common.h wedge_cell)
    const int cell_bits = log2N < 0 ? 0 : log2N, bphi = (cell_bits + 1) >> 1, bth = cell_bits - bphi;
    const int64_t n_groups = (n_ids + 63) / 64;
    const int64_t n_chunks = n_groups << log2parts;
    for (int64_t chunk = gw; chunk < n_chunks; chunk += nw) {
        const int part = (int)(chunk & ((1ll << log2parts) - 1ll));
        const int64_t k = (chunk >> log2parts) * 64 + lane;
        const bool live = k < n_ids;
        const int64_t t = live ? (ids ? (int64_t)ids[k] : k) : 0;
        const Texel x = load_texel(pos, nrm, shift, t);
        const Frame f = make_frame(x.nx, x.ny, x.nz);
        float acc[KMAX][3];
#pragma unroll
        for (int q = 0; q < KMAX; q++) { acc[q][0] = 0.f; acc[q][1] = 0.f; acc[q][2] = 0.f; }
        for (int Lc = part * part_cells; Lc < (part + 1) * part_cells; Lc++) {
            const int J = log2N >= 0 ? wedge_cell(Lc, bphi, bth) : Lc;
            if (live) {
                // (N not a power of two: natural sample order)
                const uint32_t i = log2N < 0 ? (uint32_t)J : sample_index_m(cell_to_pass_m((uint32_t)J, x.sh0, x.sh1, log2N, 0), 0u, log2N, 0);
                float d[3];
                texel_sample_dir(mode, i, (uint32_t)N, x.sh0, x.sh1, f, d);
                const float ndl = fminf(fmaxf(x.nx * d[0] + x.ny * d[1] + x.nz * d[2], 0.f), 1.f);       // :170, RAW normal
                Hit h = trace_closest<false, kGroupLstk, 4>(sc, x.px, x.py, x.pz, d[0], d[1], d[2], cn, ct, nullptr);
                if (h.slot >= 0 && h.t > 1e-4f) {          // tracer_o3d_irt.py:248
                    const MultiTaps tp = multi_footprint(sc, h.slot, h.u, h.v);
                    const float* p00 = tex + tp.o00 * texel_floats;
                    const float* p10 = tex + tp.o10 * texel_floats;
                    const float* p01 = tex + tp.o01 * texel_floats;
                    const float* p11 = tex + tp.o11 * texel_floats;
#pragma unroll
                    for (int q = 0; q < KMAX; q++) {
                        if (q < K) {
#pragma unroll
                            for (int c = 0; c < 3; c++) {
                                const float L = multi_tap_sum(tp, p00[3 * q + c], p10[3 * q + c], p01[3 * q + c], p11[3 * q + c]);
                                acc[q][c] += L * ndl;
                            }
                        }
                    }
                }
            }
        }
        if (live) {
#pragma unroll
            for (int q = 0; q < KMAX; q++) {
                if (q < K) {
                    float* o = partial + (((int64_t)part * K + q) * n_ids + k) * 3;
                    o[0] = acc[q][0]; o[1] = acc[q][1]; o[2] = acc[q][2];
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// launcher
// ------------------------------------------------------------------------------------------------

// parts per texel of the 64-texel plan, as irt_plan takes them (launch_util.h irt_log2parts)
static int irt_multi_log2parts(int N) { return irt_log2parts(N, env().irt_min_part_cells, env().irt_log2parts_cap); }

size_t irt_multi_workspace_bytes(int64_t n_ids, int N, int K)
{
    if (n_ids <= 0 || N <= 0 || K < 1 || K > kMultiMaxTextures) return 0;
    return (sizeof(float) * 3 * (size_t)n_ids * (size_t)K) << irt_multi_log2parts(N);
}

template <int KMAX>
static void multi_launch(const SceneDev& sc, const float* tex, const float* pos, const float* nrm, const float* shift, const int32_t* ids, int64_t n_ids, int N, int l2,
                         int mode, int K, float* partial, int log2parts, hipStream_t st)
{
    const int grid = persistent_grid(irt_multi_kernel<KMAX>, ((n_ids + 63) / 64) << log2parts, kBlock);      // a wave per chunk, at most the resident ones
    hipLaunchKernelGGL((irt_multi_kernel<KMAX>), dim3(grid), dim3(kBlock), 0, st, sc, tex, pos, nrm, shift, ids, n_ids, N, l2, mode, K, partial, log2parts);
}

hipError_t launch_irt_multi(const SceneDev& sc, const float* tex, const float* pos, const float* nrm, const float* shift, const int32_t* ids, int64_t n_ids, int64_t Nt,
                            int N, int mode, int K, float* out, float* partial, hipStream_t st)
{
    if (n_ids <= 0) return hipSuccess;
    const bool pow2 = (N & (N - 1)) == 0;
    const int l2 = pow2 ? ilog2_exact(N) : -1;
    const int log2parts = irt_multi_log2parts(N);
    if (K <= 2) multi_launch<2>(sc, tex, pos, nrm, shift, ids, n_ids, N, l2, mode, K, partial, log2parts, st);
    else if (K <= 4) multi_launch<4>(sc, tex, pos, nrm, shift, ids, n_ids, N, l2, mode, K, partial, log2parts, st);
    else multi_launch<8>(sc, tex, pos, nrm, shift, ids, n_ids, N, l2, mode, K, partial, log2parts, st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_irt_combine(partial, ids, n_ids, Nt, K, 1 << log2parts, N, 2.f, out, st);
}

}  // namespace texir

// Irradiance split by source label: per-class IrT in one traced pass (include/texir_hip.h texir_irt_split states the rule; this file follows it).
//
// The rays of irt_group_kernel<false, 4, 6> (kernels.hip) -- one texel per lane, one sample per pass, the same direction cells in the same order, the same
// closest-hit query -- are traced ONCE; the hit shader computes the footprint of shade_hit (device_common.h) and then, per class k, the bilinear sum over the
// taps whose LABEL is k (every other tap counts as +0.0f): the float32 expression shade_hit evaluates on the texture tex * [label == k].  Adding +0 changes no
// float, so out[k] is bit for bit what texir_irt_generate in its 64-texel form writes for that masked texture -- K passes for the price of one traversal.
//
// A wave owns 64 consecutive ids of the caller's (Morton-ordered) list; a chunk is 64 texels x one part of the passes.  Chunks are dealt statically: wave w
// of the grid takes chunks w, w + waves, ... -- no work counter, no wave waits on another, every loop is bounded by N, the chunk count or the traversal's
// own bounds.  The partial sums go to partial[part][k][i][3] and irt_combine_kernel (kernels.hip) adds them in part order, so the result is a pure function of the
// inputs: list order, list cuts, launch shape and stream do not change a bit.
//
// The class accumulators are registers under static indexing (loops over KMAX are unrolled, the class of a tap is applied by selects); the only private
// memory is the traversal's own overflow stack.  The taps are read from the row-major master copy of the radiance texture (the floats every layout of the
// hit shader's copy holds); the four label bytes of a footprint are two rows of two adjacent bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env.h"
#include "kernels.h"

namespace texir {

// (the traversal's template arguments are irt_group_kernel's on the 4-wide tree: device_common.h kGroupLstk)
constexpr int kSplitMaxClasses = 8;

// waves per SIMD the kernel is compiled for: 3 accumulators per class on top of irt_group_kernel's 64 registers at 8 waves
template <int KMAX> struct SplitWaves { static constexpr int value = KMAX <= 2 ? 6 : (KMAX <= 4 ? 5 : 4); };

// ------------------------------------------------------------------------------------------------
// hit shader: shade_hit's footprint, then one bilinear sum per class -- separately rounded operations, as in device_common.h
// (split_footprint repeats the first lines of shade_hit; what keeps the two texts equal is the bit-identity tests of tests/test_gpu_irt_split.py)
// ------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)

struct SplitTaps {
    float w00, w10, w01, w11;
    int l00, l10, l01, l11;          // labels of the four taps
    size_t o00, o10, o01, o11;       // texel offsets of the four taps in the row-major texture
};

__device__ __forceinline__ SplitTaps split_footprint(const SceneDev& sc, const uint8_t* __restrict__ labels, int tri_slot, float bu, float bv)
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
    SplitTaps t;
    t.w00 = wx0 * wy0;
    t.w10 = (x0 + 1 < sc.Wt) ? wx1 * wy0 : 0.f;
    t.w01 = (y0 + 1 < sc.Ht) ? wx0 * wy1 : 0.f;
    t.w11 = (x0 + 1 < sc.Wt && y0 + 1 < sc.Ht) ? wx1 * wy1 : 0.f;
    t.o00 = (size_t)y0 * sc.Wt + x0; t.o10 = (size_t)y0 * sc.Wt + x1;
    t.o01 = (size_t)y1 * sc.Wt + x0; t.o11 = (size_t)y1 * sc.Wt + x1;
    t.l00 = labels[t.o00]; t.l10 = labels[t.o10]; t.l01 = labels[t.o01]; t.l11 = labels[t.o11];
    return t;
}

// class k's bilinear sum of one channel: taps of another class are +0.0f
__device__ __forceinline__ float split_class_sum(const SplitTaps& t, int k, float v00, float v10, float v01, float v11)
{
    float acc = (t.l00 == k ? v00 : 0.f) * t.w00;
    acc += (t.l10 == k ? v10 : 0.f) * t.w10;
    acc += (t.l01 == k ? v01 : 0.f) * t.w01;
    acc += (t.l11 == k ? v11 : 0.f) * t.w11;
    return acc;
}

#pragma clang fp contract(fast)

template <int KMAX, bool UNIT>
__global__ __launch_bounds__(kBlock, SplitWaves<KMAX>::value) void irt_split_kernel(SceneDev sc, const float* __restrict__ tex, const uint8_t* __restrict__ labels,
                                                                                   const float* __restrict__ pos, const float* __restrict__ nrm,
                                                                                   const float* __restrict__ shift, const int32_t* __restrict__ ids, int64_t n_ids,
                                                                                   int N, int log2N, int mode, int K, float* __restrict__ partial, int log2parts)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (wave-uniform: the chunk loop and the pass loop stay scalar)
    const int64_t gw = (int64_t)blockIdx.x * (kBlock / 64) + wave, nw = (int64_t)gridDim.x * (kBlock / 64);
    uint32_t cn = 0, ct = 0;
    const int part_cells = N >> log2parts;
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
                    const SplitTaps tp = split_footprint(sc, labels, h.slot, h.u, h.v);
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        float v00 = 1.0f, v10 = 1.0f, v01 = 1.0f, v11 = 1.0f;
                        if constexpr (!UNIT) { v00 = tex[3 * tp.o00 + c]; v10 = tex[3 * tp.o10 + c]; v01 = tex[3 * tp.o01 + c]; v11 = tex[3 * tp.o11 + c]; }
#pragma unroll
                        for (int q = 0; q < KMAX; q++) {
                            const float L = split_class_sum(tp, q, v00, v10, v01, v11);
                            acc[q][c] += L * ndl;
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
static int irt_split_log2parts(int N) { return irt_log2parts(N, env().irt_min_part_cells, env().irt_log2parts_cap); }

size_t irt_split_workspace_bytes(int64_t n_ids, int N, int K)
{
    if (n_ids <= 0 || N <= 0 || K < 1 || K > kSplitMaxClasses) return 0;
    return (sizeof(float) * 3 * (size_t)n_ids * (size_t)K) << irt_split_log2parts(N);
}

template <int KMAX, bool UNIT>
static void split_launch(const SceneDev& sc, const float* tex, const uint8_t* labels, const float* pos, const float* nrm, const float* shift, const int32_t* ids,
                         int64_t n_ids, int N, int l2, int mode, int K, float* partial, int log2parts, hipStream_t st)
{
    const int grid = persistent_grid(irt_split_kernel<KMAX, UNIT>, ((n_ids + 63) / 64) << log2parts, kBlock);      // a wave per chunk, at most the resident ones
    hipLaunchKernelGGL((irt_split_kernel<KMAX, UNIT>), dim3(grid), dim3(kBlock), 0, st, sc, tex, labels, pos, nrm, shift, ids, n_ids, N, l2, mode, K, partial, log2parts);
}

hipError_t launch_irt_split(const SceneDev& sc, const float* tex_row_major, const uint8_t* labels, const float* pos, const float* nrm, const float* shift,
                            const int32_t* ids, int64_t n_ids, int64_t Nt, int N, int mode, int K, int unit, float* out, float* partial, hipStream_t st)
{
    if (n_ids <= 0) return hipSuccess;
    const bool pow2 = (N & (N - 1)) == 0;
    const int l2 = pow2 ? ilog2_exact(N) : -1;
    const int log2parts = irt_split_log2parts(N);
#define TEXIR_SPLIT(KMAX) { if (unit) split_launch<KMAX, true>(sc, tex_row_major, labels, pos, nrm, shift, ids, n_ids, N, l2, mode, K, partial, log2parts, st); \
                            else split_launch<KMAX, false>(sc, tex_row_major, labels, pos, nrm, shift, ids, n_ids, N, l2, mode, K, partial, log2parts, st); }
    if (K <= 2) TEXIR_SPLIT(2)
    else if (K <= 4) TEXIR_SPLIT(4)
    else TEXIR_SPLIT(8)
#undef TEXIR_SPLIT
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_irt_combine(partial, ids, n_ids, Nt, K, 1 << log2parts, N, 2.f, out, st);
}

}  // namespace texir

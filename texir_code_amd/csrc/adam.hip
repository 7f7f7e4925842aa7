// The optimiser kernels of libtexir_hip.so:
//   adam_kernel        torch.optim.Adam step fused with the trainer's post-step clamp (train_material.py:448-458).
//   adam_tex_*         the same step over a texture, fused with the last folds of the mip backward and with level 1 of the next forward's mip stack
//                      (single-texture and batched launches, material.hip has the kernels in front of and behind them).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env.h"
#include "kernels.h"

namespace texir {

// ------------------------------------------------------------------------------------------------------------------
// torch.optim.Adam (no amsgrad / weight decay / maximize), same operation order as torch's single-tensor path, fused
// with the trainer's clamp (materials_r in [1e-2, 0.8], materials_a >= 0; train_material.py:458,592-593)
// ------------------------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)
// one Adam update with explicitly placed roundings (shared by both optimiser kernels so that they agree bit for bit):
//   exp_avg.lerp_(grad, 1 - beta1); exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2); param.addcdiv_(exp_avg, denom, value = -step_size)
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float beta1, float beta2, float eps, float step_size,
                                            float bc2_sqrt, float lo, float hi)
{
    const float mi = __builtin_fmaf(g - m, 1.f - beta1, m);
    const float vi = __builtin_fmaf(g * g, 1.f - beta2, v * beta2);
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    const float pi = __builtin_fmaf(mi / denom, -step_size, p);
    m = mi; v = vi; p = fminf(fmaxf(pi, lo), hi);
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                   int64_t n, float beta1, float beta2, float eps, float step_size, float bc2_sqrt,
                                                   float lo, float hi, const float* __restrict__ hyp)
{
    if (hyp) { step_size = hyp[0]; bc2_sqrt = hyp[1]; }          // device-resident step size / bias correction (adam_tick_kernel): hipGraph replays
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        adam_update(p[i], g[i], m[i], v[i], beta1, beta2, eps, step_size, bc2_sqrt, lo, hi);
    }
}
#pragma clang fp contract(fast)

// Adam over a texture [H,W,C] whose gradient is level 0 + 0.25 * (level-1 gradient of the 2x2 block): the last fold of the mip
// backward happens here, while the gradient is read anyway (saves one read-modify-write of the finest level per step).
// Same arithmetic as mip_fold_kernel followed by adam_kernel, bit for bit.
//   * l0_mask (one bit per texel, nullable): g holds valid values only at the texels whose bit is set (the texels a cached view's
//     tap lists write -- the buffer is never zero-filled); every other texel's level-0 gradient is zero;
//   * g == nullptr: the level-0 part of the gradient is identically zero (no pixel of the step sampled mip level 0 -- the usual
//     case for 4k textures seen through 128^2 cube faces), so it is neither zero-filled nor read (fma(0.25, g1, 0) is the same float);
//   * mip1 != nullptr: the thread also writes the 2x2 average of the UPDATED texels = level 1 of the next forward's mip stack
//     (same expression as the mip build), which removes the build's pass over the whole level-0 texture.
template <int C>
__global__ __launch_bounds__(256) void adam_tex_kernel(float* __restrict__ p, const float* __restrict__ g, const uint32_t* __restrict__ l0_mask,
                                                       const float* __restrict__ g1, const float* __restrict__ g2, float* __restrict__ m, float* __restrict__ v, float* __restrict__ mip1,
                                                       int H, int W, float beta1, float beta2, float eps, float step_size, float bc2_sqrt, float lo, float hi, const float* __restrict__ hyp,
                                                       const uint32_t* __restrict__ g1_mask /* nullable: see adam_tex_vec_body */)
{
    if (hyp) { step_size = hyp[0]; bc2_sqrt = hyp[1]; }
    // one thread per (2x2 block column, channel): t = bx * C + ch.  Its level-1 element and its g1 element sit at index t of the
    // half-resolution row (perfectly coalesced); its four texture elements are rows 2by / 2by+1 at bx * 2C + ch and + C (the two
    // loads of a row together cover the row densely, every 128-byte line is fetched once).
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int Wh = W >> 1, Hh = H >> 1;
    if (t >= Wh * C) return;
    const int bx = t / C, ch = t - bx * C;
    const int e0 = bx * 2 * C + ch;
    for (int by = blockIdx.y; by < Hh; by += gridDim.y) {
        float g1c = 0.f;                                             // (g1 == nullptr: no tap of the view touches level 1, its direct gradient is identically zero)
        if (g1) {
            bool has = true;
            if (g1_mask) { const size_t tt = (size_t)by * Wh + bx; has = (g1_mask[tt >> 5] >> (tt & 31)) & 1u; }
            if (has) g1c = g1[(size_t)by * Wh * C + t];
        }
        if (g2) g1c = __builtin_fmaf(0.25f, g2[((size_t)(by >> 1) * (Wh >> 1) + (bx >> 1)) * C + ch], g1c);      // the fold level 2 -> level 1, taken over as well
        float acc = 0.f;
#pragma unroll
        for (int r = 0; r < 2; r++) {
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const size_t i = (size_t)(2 * by + r) * W * C + e0 + q * C;
                float g0 = 0.f;
                if (g) {
                    // level-0 gradient: dense (no mask), or only where this view's tap lists wrote one (bit of the texel set)
                    const size_t texel = (size_t)(2 * by + r) * W + 2 * bx + q;
                    if (!l0_mask || ((l0_mask[texel >> 5] >> (texel & 31)) & 1u)) g0 = g[i];
                }
                const float gi = __builtin_fmaf(0.25f, g1c, g0);
                float pi = p[i], mi = m[i], vi = v[i];
                adam_update(pi, gi, mi, vi, beta1, beta2, eps, step_size, bc2_sqrt, lo, hi);
                p[i] = pi; m[i] = mi; v[i] = vi;
                acc = (r == 0 && q == 0) ? pi : acc + pi;           // ((a + b) + c) + d, the mip build's order
            }
        }
        if (mip1) mip1[(size_t)by * Wh * C + t] = 0.25f * acc;
    }
}

// floats of a row pair one block of adam_tex_vec_kernel owns: the largest multiple of BOTH 2C (no 2x2 texel block straddles two blocks) and 32
// (a block's segment starts and ends on a 128-byte line: with 1020 floats per block -- the largest multiple of 6 -- every segment boundary of
// the 3-channel texture split a line between two blocks, i.e. two CUs / XCDs each wrote part of it) that fits 256 threads x one float4
constexpr int adam_vec_epb(int C) { return C == 3 ? 960 : (1024 / (2 * C)) * (2 * C); }

// The same step with 16-byte accesses: a block owns EPB consecutive floats of a row pair (adam_vec_epb, so
// that no 2x2 texel block straddles two blocks), every thread one float4 of each row; the level-1 gradient segment and the updated
// texels go through LDS so that the level-1 texels come out in the mip build's own summation order ((p00 + p01) + p10) + p11.
// Needs W*C % 4 == 0 (16-byte aligned rows); launch_adam_tex falls back to adam_tex_kernel otherwise.  Identical bits.
// Waves per SIMD the step is compiled for: 94 VGPRs, no scratch (unbounded: 116 = 4 waves; 6: 24 bytes of scratch).  Alone the launch takes the same
// time at 4 / 5 / 6; inside the step 5 was 10 us ahead of 4.
constexpr int kAdamWaves = 5;
// The step's loads and stores of texels and moments carry the non-temporal hint.  Measured (profiles/r04/adam_batch_probe_s15.txt): 310 -> 283 us per
// launch over both 4k textures, 5.5 -> 6.0 TB/s; loads or stores alone: a third of it each.
typedef float texir_vf4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 adam_ld4(const float* __restrict__ q)
{
    const texir_vf4 t = __builtin_nontemporal_load(reinterpret_cast<const texir_vf4*>(q));
    return make_float4(t.x, t.y, t.z, t.w);
}
__device__ __forceinline__ void adam_st4(float* __restrict__ q, float a, float b, float c, float d)
{
    texir_vf4 t; t.x = a; t.y = b; t.z = c; t.w = d;
    __builtin_nontemporal_store(t, reinterpret_cast<texir_vf4*>(q));
}

//   * g1_mask (nullable, only together with g2): the level-1 stack is a never-cleared buffer; its texels carry this step's values only where the view's tap
//     lists wrote them (bit by * W/2 + x of the mask -- level 1 leads the `rest` stack, so this is the stack's own mask), all others count as zero and
//     are not read.
template <int C>
__device__ __forceinline__ void adam_tex_vec_body(float* __restrict__ p, const float* __restrict__ g, const uint32_t* __restrict__ l0_mask,
                                                  const float* __restrict__ g1, const uint32_t* __restrict__ g1_mask, const float* __restrict__ g2,
                                                  float* __restrict__ m, float* __restrict__ v, float* __restrict__ mip1,
                                                  int H, int W, float beta1, float beta2, float eps, float step_size, float bc2_sqrt, float lo, float hi,
                                                  int bx, int by0, int gy, float* __restrict__ g1s /* LDS [EPB / 2] */, float (*ps)[adam_vec_epb(C)] /* LDS [2][EPB] */)
{
    constexpr int EPB = adam_vec_epb(C);
    const int row_elems = W * C, Wh = W >> 1, Hh = H >> 1;
    const int e_base = bx * EPB;
    const int n_here = min(EPB, row_elems - e_base);                 // multiple of 2C and of 4
    const int j4 = threadIdx.x * 4;
    const bool act = j4 < n_here;
    const int h_base = e_base / 2, n_half = n_here / 2;              // this block's segment of the half-resolution row
    for (int by = by0; by < Hh; by += gy) {
        // The thread's own texels, moments and level-0 gradient (or the mask bits that say where it is valid) FIRST: these loads depend on nothing, and
        // issued here they are in flight while the level-1 segment is staged (mask word -> value -> level-2 value: up to three dependent round trips
        // that the barrier below would otherwise put in front of them).
        float4 pv[2], mv[2], vv[2], gv[2];
        uint32_t l0bits = 0;                                        // bit r * 4 + q: element q of row r has a level-0 gradient to read
        if (act) {
#pragma unroll
            for (int r = 0; r < 2; r++) {
                const size_t i = (size_t)(2 * by + r) * row_elems + e_base + j4;
                pv[r] = adam_ld4(p + i); mv[r] = adam_ld4(m + i); vv[r] = adam_ld4(v + i);
                if (g && !l0_mask) gv[r] = *reinterpret_cast<const float4*>(g + i);
                if (g && l0_mask) {
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const size_t texel = (size_t)(2 * by + r) * W + (e_base / C) + (j4 + q) / C;
                        l0bits |= ((l0_mask[texel >> 5] >> (texel & 31)) & 1u) << (r * 4 + q);
                    }
                }
            }
        }
        for (int k = threadIdx.x; k < n_half; k += 256) {
            const int txh = (h_base + k) / C, ch = (h_base + k) - txh * C;
            // (the level-2 value is loaded before the mask word is tested: it does not depend on it)
            const float x2 = g2 ? g2[((size_t)(by >> 1) * (Wh >> 1) + (txh >> 1)) * C + ch] : 0.f;
            float x = 0.f;                                          // (g1 == nullptr: level-1 direct gradient identically zero -- not read)
            if (g1) {
                bool has = true;
                if (g1_mask) { const size_t t = (size_t)by * Wh + txh; has = (g1_mask[t >> 5] >> (t & 31)) & 1u; }
                if (has) x = g1[(size_t)by * Wh * C + h_base + k];
            }
            if (g2) x = __builtin_fmaf(0.25f, x2, x);               // the fold level 2 -> level 1, taken over as well (same fma as mip_pyr_fold_kernel's)
            g1s[k] = x;
        }
        __syncthreads();
        if (act) {
#pragma unroll
            for (int r = 0; r < 2; r++) {
                const size_t i = (size_t)(2 * by + r) * row_elems + e_base + j4;
                float pe[4] = {pv[r].x, pv[r].y, pv[r].z, pv[r].w}, me[4] = {mv[r].x, mv[r].y, mv[r].z, mv[r].w}, ve[4] = {vv[r].x, vv[r].y, vv[r].z, vv[r].w};
                const float ge[4] = {gv[r].x, gv[r].y, gv[r].z, gv[r].w};
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int el = j4 + q;                           // element inside the block's segment
                    const int tx = el / C, ch = el - tx * C;
                    float g0 = 0.f;
                    if (g) {
                        // dense level-0 gradient (read above), or only where this view's tap lists wrote one (bit of the texel set: rare)
                        if (!l0_mask) g0 = ge[q];
                        else if ((l0bits >> (r * 4 + q)) & 1u) g0 = g[i + q];
                    }
                    const float gi = __builtin_fmaf(0.25f, g1s[(tx >> 1) * C + ch], g0);
                    adam_update(pe[q], gi, me[q], ve[q], beta1, beta2, eps, step_size, bc2_sqrt, lo, hi);
                    ps[r][el] = pe[q];
                }
                adam_st4(p + i, pe[0], pe[1], pe[2], pe[3]);
                adam_st4(m + i, me[0], me[1], me[2], me[3]);
                adam_st4(v + i, ve[0], ve[1], ve[2], ve[3]);
            }
        }
        __syncthreads();
        if (mip1) {
            for (int k = threadIdx.x; k < n_half; k += 256) {
                const int txh = k / C, ch = k - txh * C;
                const int a = (2 * txh) * C + ch;
                mip1[(size_t)by * Wh * C + h_base + k] = 0.25f * (ps[0][a] + ps[0][a + C] + ps[1][a] + ps[1][a + C]);
            }
        }
        // (the next iteration's first barrier orders these LDS reads before the rewrite of ps; g1s is rewritten before it, and nobody
        // reads g1s after the barrier above)
    }
}

template <int C>
__global__ __launch_bounds__(256, kAdamWaves) void adam_tex_vec_kernel(float* __restrict__ p, const float* __restrict__ g, const uint32_t* __restrict__ l0_mask,
                                                           const float* __restrict__ g1, const float* __restrict__ g2, float* __restrict__ m, float* __restrict__ v, float* __restrict__ mip1,
                                                           int H, int W, float beta1, float beta2, float eps, float step_size, float bc2_sqrt, float lo, float hi, const float* __restrict__ hyp)
{
    if (hyp) { step_size = hyp[0]; bc2_sqrt = hyp[1]; }
    constexpr int EPB = adam_vec_epb(C);
    __shared__ float g1s[EPB / 2];
    __shared__ float ps[2][EPB];
    adam_tex_vec_body<C>(p, g, l0_mask, g1, nullptr, g2, m, v, mip1, H, W, beta1, beta2, eps, step_size, bc2_sqrt, lo, hi, blockIdx.x, blockIdx.y, gridDim.y, g1s, ps);
}

// step size and bias correction of torch.optim.Adam's single-tensor path from (lr, step), in double; hyp != nullptr: the kernels read the pair from device
// memory instead (adam_tick_kernel) and these defaults are not used
struct AdamHyper { float step_size = 0.f, bc2_sqrt = 1.f; };

static AdamHyper adam_hyper(float lr, float beta1, float beta2, int step, const float* hyp)
{
    AdamHyper h;
    if (!hyp) {
        double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
        h.step_size = (float)((double)lr / bc1);
        h.bc2_sqrt = (float)sqrt(bc2);
    }
    return h;
}

// the 16-byte form needs 16-byte aligned rows (TEXIR_ADAM_SCALAR: the parity tests' reference kernel)
static bool adam_vec_ok(int W, int C) { return (W * C) % 4 == 0 && !env().adam_scalar; }

// grid of the 16-byte form over one texture: its row segments of adam_vec_epb(C) floats x its row pairs, at most 2048 (the blocks stride over the rest)
static dim3 adam_vec_grid(int H, int W, int C)
{
    const int epb = adam_vec_epb(C);
    dim3 grid((W * C + epb - 1) / epb, (H >> 1) > 2048 ? 2048 : (H >> 1));
    if (const int v = env().adam_grid_y; v >= 1 && v < (int)grid.y) grid.y = v;      // (probe: fewer, longer blocks leave wave slots to a concurrent kernel)
    return grid;
}

// scalar form (reference kernel of the parity tests, or rows that are not 16-byte aligned)
static void launch_adam_tex_scalar(const texir_adam_tex_job& q, AdamHyper h, hipStream_t st)
{
    dim3 grid(((q.W >> 1) * q.C + 255) / 256, (q.H >> 1) > 4096 ? 4096 : (q.H >> 1));
    with_channels(q.C, [&](auto c) {
        hipLaunchKernelGGL(adam_tex_kernel<decltype(c)::value>, grid, dim3(256), 0, st, q.param, q.grad, q.grad_mask, q.grad_level1, q.grad_level2, q.exp_avg, q.exp_avg_sq,
                           q.mip_level1, q.H, q.W, q.beta1, q.beta2, q.eps, h.step_size, h.bc2_sqrt, q.clamp_lo, q.clamp_hi, q.hyper, q.level1_mask);
    });
}

// one texture (q.level1_mask: a field of the batched step alone, null here); q.hyper == nullptr: the step size and bias correction of (lr, step)
hipError_t launch_adam_tex(const texir_adam_tex_job& q, float lr, int step, hipStream_t st)
{
    const AdamHyper h = adam_hyper(lr, q.beta1, q.beta2, step, q.hyper);
    if (adam_vec_ok(q.W, q.C)) {
        with_channels(q.C, [&](auto c) {
            hipLaunchKernelGGL(adam_tex_vec_kernel<decltype(c)::value>, adam_vec_grid(q.H, q.W, q.C), dim3(256), 0, st, q.param, q.grad, q.grad_mask, q.grad_level1, q.grad_level2,
                               q.exp_avg, q.exp_avg_sq, q.mip_level1, q.H, q.W, q.beta1, q.beta2, q.eps, h.step_size, h.bc2_sqrt, q.clamp_lo, q.clamp_hi, q.hyper);
        });
    } else launch_adam_tex_scalar(q, h, st);
    return hipGetLastError();
}

// One thread per parameter record: advances the step count and derives the step size / bias correction the Adam kernels read, in
// double precision with the same expressions the host path uses (torch.optim.Adam's single-tensor path): a captured hipGraph that
// contains this launch followed by the Adam kernels needs no host argument per replay.
//   state [n][4] doubles: step count, lr, beta1, beta2      hyper [n][2] floats: lr / (1 - beta1^step), sqrt(1 - beta2^step)
__global__ void adam_tick_kernel(double* __restrict__ state, float* __restrict__ hyper, int n, unsigned long long mask)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !((mask >> i) & 1ull)) return;
    double* s = state + 4 * i;
    const double step = s[0] + 1.0;
    s[0] = step;
    const double bc1 = 1.0 - pow(s[2], step), bc2 = 1.0 - pow(s[3], step);
    hyper[2 * i] = (float)(s[1] / bc1);
    hyper[2 * i + 1] = (float)sqrt(bc2);
}

hipError_t launch_adam_tick(double* state, float* hyper, int n, unsigned long long mask, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(64), 0, st, state, hyper, n, mask);
    return hipGetLastError();
}

hipError_t launch_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, int step,
                       float lo, float hi, const float* hyp, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    const AdamHyper h = adam_hyper(lr, beta1, beta2, step, hyp);
    hipLaunchKernelGGL(adam_kernel, dim3(grid_capped(256 * 4, n, 4096)), dim3(256), 0, st, p, g, m, v, n, beta1, beta2, eps, h.step_size, h.bc2_sqrt, lo, hi, hyp);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------
// The batched step (include/texir_hip.h, "batched forms"; material.hip has the other kinds): one launch for up to TEXIR_MAX_BATCH textures, the job body is
// the single-texture kernel's own (adam_tex_vec_body), so every job's result keeps its bits.
// ------------------------------------------------------------------------------------------------------------------
struct AdamTexJob { float* p; const float* g; const uint32_t* l0_mask; const float* g1; const uint32_t* g1_mask; const float* g2; float* m; float* v; float* mip1;
                    int H, W, C; float beta1, beta2, eps, lo, hi; const float* hyp; int first, gy; };
struct AdamTexBatch { int n; AdamTexJob j[kMaxBatch]; };

// grid.x = the jobs' row segments side by side, grid.y = the largest row-pair stride of the batch (a job with fewer rows leaves the surplus rows idle)
// CSET: bit C-1 set for every channel count that occurs in the batch -- the other bodies are not compiled in (the kernel's register count is the largest of
// its bodies': 92 VGPRs with all four, 64 with the albedo + roughness pair)
template <int CSET>
__global__ __launch_bounds__(256, kAdamWaves) void adam_tex_vec_batch_kernel(AdamTexBatch b)
{
    __shared__ float g1s[512];
    __shared__ float ps[2 * 1024];
    const AdamTexJob& J = b.j[job_of_block(b, blockIdx.x)];
    if ((int)blockIdx.y >= J.gy) return;
    const float step_size = J.hyp[0], bc2_sqrt = J.hyp[1];
    const int bx = blockIdx.x - J.first;
#define TEXIR_ADAM_BODY(CC)                                                                                                                                   \
    if constexpr ((CSET >> (CC - 1)) & 1)                                                                                                                     \
        if (J.C == CC) {                                                                                                                                      \
            adam_tex_vec_body<CC>(J.p, J.g, J.l0_mask, J.g1, J.g1_mask, J.g2, J.m, J.v, J.mip1, J.H, J.W, J.beta1, J.beta2, J.eps, step_size, bc2_sqrt, J.lo, \
                                  J.hi, bx, blockIdx.y, J.gy, g1s, reinterpret_cast<float (*)[adam_vec_epb(CC)]>(ps));                                        \
            return;                                                                                                                                           \
        }
    TEXIR_ADAM_BODY(1) TEXIR_ADAM_BODY(2) TEXIR_ADAM_BODY(3) TEXIR_ADAM_BODY(4)
#undef TEXIR_ADAM_BODY
}

hipError_t launch_adam_tex_batch(const texir_adam_tex_job* jobs, int n, hipStream_t st)
{
    bool vec = true;
    for (int k = 0; k < n; k++) vec = vec && adam_vec_ok(jobs[k].W, jobs[k].C);
    if (!vec) {
        for (int k = 0; k < n; k++) launch_adam_tex_scalar(jobs[k], AdamHyper{}, st);      // one launch per job
        return hipGetLastError();
    }
    AdamTexBatch ab; ab.n = n;
    int gx = 0, gy = 1, cset = 0;
    for (int k = 0; k < n; k++) {
        const texir_adam_tex_job& q = jobs[k];
        AdamTexJob& J = ab.j[k];
        J.p = q.param; J.g = q.grad; J.l0_mask = q.grad_mask; J.g1 = q.grad_level1; J.g1_mask = q.level1_mask; J.g2 = q.grad_level2; J.m = q.exp_avg; J.v = q.exp_avg_sq; J.mip1 = q.mip_level1;
        J.H = q.H; J.W = q.W; J.C = q.C; J.beta1 = q.beta1; J.beta2 = q.beta2; J.eps = q.eps; J.lo = q.clamp_lo; J.hi = q.clamp_hi; J.hyp = q.hyper;
        const dim3 grid = adam_vec_grid(q.H, q.W, q.C);
        J.first = gx; J.gy = (int)grid.y;
        gx += (int)grid.x;
        if (J.gy > gy) gy = J.gy;
        cset |= 1 << (q.C - 1);
    }
    if (cset == 0b0001) hipLaunchKernelGGL(adam_tex_vec_batch_kernel<0b0001>, dim3(gx, gy), dim3(256), 0, st, ab);
    else if (cset == 0b0100) hipLaunchKernelGGL(adam_tex_vec_batch_kernel<0b0100>, dim3(gx, gy), dim3(256), 0, st, ab);
    else if (cset == 0b0101) hipLaunchKernelGGL(adam_tex_vec_batch_kernel<0b0101>, dim3(gx, gy), dim3(256), 0, st, ab);
    else hipLaunchKernelGGL(adam_tex_vec_batch_kernel<0b1111>, dim3(gx, gy), dim3(256), 0, st, ab);
    return hipGetLastError();
}

}  // namespace texir

// The texture side of libtexir_hip.so (gbuffer.hip: the cube G-buffer the fetches read their uvs from; adam.hip: the optimiser step that consumes the gradients):
//   mip_build / tex_fetch_fwd / tex_fetch_bwd / mip_fold
//                      nvdiffrast `texture` semantics restated (mat_nvdiffrast.py:131-139): 'linear' = bilinear with wrap,
//                      'linear-mipmap-linear' = 2x2-box mip stack, LOD = log2 of the major axis of the uv_da footprint in
//                      texels, clamped to [0, max level], trilinear; backward scatters into every touched mip and folds
//                      the stack down to level 0.   (nvdiffrast is un-vendored: parity unpinned, see DESIGN.md.)
//   tex_taps / tex_gather
//                      the atomics-free backward for fixed (uv, uv_da); grad_add_masked: a sparse level-0 gradient added to a dense one.
//   *_batch_kernel     one launch per kind of kernel for up to TEXIR_MAX_BATCH textures.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env.h"
#include "kernels.h"

namespace texir {

// ------------------------------------------------------------------------------------------------------------------
// mip stack + texture fetch
// ------------------------------------------------------------------------------------------------------------------
// Level 0 IS the caller's texture (no copy); levels 1.. live in a separate "rest" buffer: level l at rest + off[l].
struct MipDesc { int H, W, C, levels; int64_t off[16]; };

static MipDesc make_desc(int H, int W, int C, int levels)
{
    MipDesc d; d.H = H; d.W = W; d.C = C; d.levels = levels;
    int64_t o = 0;
    d.off[0] = 0;
    for (int l = 1; l < 16; l++) { d.off[l] = o; if (l < levels) o += (int64_t)(H >> l) * (W >> l) * C; }
    return d;
}

int mip_levels(int H, int W, int max_mip_level)
{
    int l = 1;   // level 0
    while (l <= max_mip_level && l < 16 && ((H >> (l - 1)) % 2 == 0) && ((W >> (l - 1)) % 2 == 0) && (H >> l) >= 1 && (W >> l) >= 1) l++;
    return l;
}

// elements of levels 1 .. levels-1 (the "rest" buffer); at least 1 so that callers can always allocate
int64_t mip_total_elems(int H, int W, int C, int levels)
{
    int64_t o = 0;
    for (int l = 1; l < levels; l++) o += (int64_t)(H >> l) * (W >> l) * C;
    return o > 0 ? o : 1;
}

// one thread per output float; rows come from blockIdx.y, so the index math is 32-bit with a compile-time C (no 64-bit div/mod)
// and consecutive lanes read consecutive floats of the two source rows
template <int C>
__global__ __launch_bounds__(256) void mip_down_kernel(const float* __restrict__ src, float* __restrict__ dst, int Hd, int Wd)
{
    const int e = blockIdx.x * 256 + threadIdx.x;           // element inside an output row: texel * C + channel
    if (e >= Wd * C) return;
    const int tx = e / C, ch = e - tx * C;
    for (int y = blockIdx.y; y < Hd; y += gridDim.y) {
        const float* r0 = src + ((size_t)(2 * y) * (2 * Wd) + 2 * tx) * C + ch;
        const float* r1 = r0 + (size_t)(2 * Wd) * C;
        dst[(size_t)y * Wd * C + e] = 0.25f * (r0[0] + r0[C] + r1[0] + r1[C]);
    }
}

// all remaining (small) levels in one single-block launch: level l from level l-1, block barrier in between
__device__ __forceinline__ void mip_down_tail_body(float* __restrict__ rest, const MipDesc& d, int l_begin)
{
    for (int l = l_begin; l < d.levels; l++) {
        const int Hd = d.H >> l, Wd = d.W >> l, C = d.C, Ws = Wd * 2;
        const float* src = rest + d.off[l - 1];
        float* dst = rest + d.off[l];
        const int n = Hd * Wd * C;
        for (int g = threadIdx.x; g < n; g += 1024) {
            int ch = g % C, t = g / C, x = t % Wd, y = t / Wd;
            const float* s = src + ((2 * y) * Ws + 2 * x) * C + ch;
            dst[g] = 0.25f * (s[0] + s[C] + s[Ws * C] + s[Ws * C + C]);
        }
        __threadfence_block();
        __syncthreads();
    }
}

__global__ __launch_bounds__(1024) void mip_down_tail_kernel(float* __restrict__ rest, MipDesc d, int l_begin) { mip_down_tail_body(rest, d, l_begin); }

// fold: grad[l-1][2y+a][2x+b] += 0.25 * grad[l][y][x].  One thread per FINE float (coalesced read-modify-write of the fine row),
// rows from blockIdx.y, 32-bit index math with compile-time C.
template <int C>
__global__ __launch_bounds__(256) void mip_fold_kernel(float* __restrict__ fine, const float* __restrict__ coarse, int Hf, int Wf)
{
    const int e = blockIdx.x * 256 + threadIdx.x;           // element inside a fine row
    if (e >= Wf * C) return;
    const int tx = e / C, ch = e - tx * C;
    for (int y = blockIdx.y; y < Hf; y += gridDim.y)
        fine[(size_t)y * Wf * C + e] = __builtin_fmaf(0.25f, coarse[((size_t)(y >> 1) * (Wf >> 1) + (tx >> 1)) * C + ch], fine[(size_t)y * Wf * C + e]);
}

__global__ __launch_bounds__(1024) void mip_fold_tail_kernel(float* __restrict__ rest, MipDesc d, int l_end /* fold levels-1 .. l_end+1 into l_end */)
{
    for (int l = d.levels - 1; l > l_end; l--) {
        const int Hf = d.H >> (l - 1), Wf = d.W >> (l - 1), C = d.C;
        float* fine = rest + d.off[l - 1];
        const float* coarse = rest + d.off[l];
        const int n = Hf * Wf * C;
        for (int g = threadIdx.x; g < n; g += 1024) {
            int ch = g % C, t = g / C, x = t % Wf, y = t / Wf;
            fine[g] += 0.25f * coarse[((y >> 1) * (Wf >> 1) + (x >> 1)) * C + ch];
        }
        __threadfence_block();
        __syncthreads();
    }
}


// Several mip levels per launch.  A block owns a 32x32-texel tile of the SOURCE level s and produces its 16x16 / 8x8 / ... / 1x1
// descendants (levels s+1 .. s+5) through LDS; the levels above (at most 32^2 texels) are left to the single-block tail kernel.
// Same arithmetic as one mip_down_kernel launch per level (0.25 * (((a + b) + c) + d)), so the stack is bit-identical.
template <int C>
__device__ __forceinline__ void mip_pyr_down_body(const float* __restrict__ src, float* __restrict__ rest, const MipDesc& d, int s, int n_out, int bid,
                                                  float (*buf)[16 * 16 * C] /* LDS: 2 x 16*16*C floats */)
{
    const int Hs = d.H >> s, Ws = d.W >> s;
    const int tiles_x = (Ws + 31) / 32;
    const int ty = bid / tiles_x, tx = bid - ty * tiles_x;
    // level s+1: 16x16 outputs straight from global memory, one thread per output texel
    {
        const int oy = threadIdx.x >> 4, ox = threadIdx.x & 15;
        const int Y = ty * 16 + oy, X = tx * 16 + ox, Hd = Hs >> 1, Wd = Ws >> 1;
        if (Y < Hd && X < Wd) {
            const float* r0 = src + ((size_t)(2 * Y) * Ws + 2 * X) * C;
            const float* r1 = r0 + (size_t)Ws * C;
            float* o = rest + d.off[s + 1] + ((size_t)Y * Wd + X) * C;
#pragma unroll
            for (int c = 0; c < C; c++) { const float v = 0.25f * (r0[c] + r0[C + c] + r1[c] + r1[C + c]); o[c] = v; buf[0][(oy * 16 + ox) * C + c] = v; }
        }
    }
    int cur = 0;
    for (int k = 2; k <= n_out; k++) {
        __syncthreads();
        const int n = 32 >> k;                                  // outputs per tile side at level s+k
        const int Hd = Hs >> k, Wd = Ws >> k;
        if ((int)threadIdx.x < n * n) {
            const int oy = threadIdx.x / n, ox = threadIdx.x - oy * n;
            const int Y = ty * n + oy, X = tx * n + ox;
            if (Y < Hd && X < Wd) {
                const float* b = buf[cur] + ((2 * oy) * (2 * n) + 2 * ox) * C;
                float* o = rest + d.off[s + k] + ((size_t)Y * Wd + X) * C;
#pragma unroll
                for (int c = 0; c < C; c++) { const float v = 0.25f * (b[c] + b[C + c] + b[2 * n * C + c] + b[2 * n * C + C + c]); o[c] = v; buf[cur ^ 1][(oy * n + ox) * C + c] = v; }
            }
        }
        cur ^= 1;
    }
}

template <int C>
__global__ __launch_bounds__(256) void mip_pyr_down_kernel(const float* __restrict__ src, float* __restrict__ rest, MipDesc d, int s, int n_out)
{
    __shared__ float buf[2][16 * 16 * C];
    mip_pyr_down_body<C>(src, rest, d, s, n_out, blockIdx.x, buf);
}

// The folds of a whole gradient stack in one launch: level f (the finest one to fold INTO) += 0.25 * level f+1 += 0.25 * level f+2 ...
// A block owns a 32x32 tile of level f.  It first walks its chain of ancestors down from the top level (one texel per level: the
// same fused multiply-adds the level-by-level kernels perform on those texels), then folds its own sub-pyramid (levels f+5 .. f+1)
// through LDS and finally read-modify-writes its tile of level f.  Only level f is written back: nothing reads the coarser
// gradient levels afterwards.  Bit-identical to mip_fold_tail_kernel + one mip_fold_kernel launch per level.
// `mask` (nullable): one bit per texel of the `rest` stack (bit t & 31 of word t >> 5, t = d.off[l] / C + y * W_l + x).  With a mask the stack is NEVER
// cleared between steps: only the texels a view's tap lists wrote this step (their bit is set) hold values, every other texel counts as zero --
// reads of levels f+1 .. top go through the mask, and level f itself is WRITTEN (own masked value + a quarter of the parent) instead of
// read-modify-written.  Same floats as folding a zero-filled stack.
template <int C>
__device__ __forceinline__ float rest_read(const float* __restrict__ rest, const uint32_t* __restrict__ mask, int64_t off, int64_t texel, int c)
{
    // (the value is loaded whether its bit is set or not and SELECTED afterwards: a branch on the mask word would put every value load behind its own
    // mask load -- a block of the fold issues ~20 of these per thread, and as dependent round trips they were the whole launch, 23 us.  What an unset
    // texel holds is never used in arithmetic.)
    const float val = rest[off + texel * C + c];
    if (mask) {
        const int64_t t = off / C + texel;
        return ((mask[t >> 5] >> (t & 31)) & 1u) ? val : 0.f;
    }
    return val;
}

// The tile of a stack with at least five levels above f whose level f is made of whole 32 x 32 tiles with 16-byte aligned rows (every texture that matters): the
// same fused multiply-adds as the general body below, but
//   * EVERY global load of the tile -- the ancestors' texels, the tile's own texels of levels f+4 .. f+1 and of level f, through the mask where there is one --
//     is issued before the first barrier (the general form walks the levels with a load + barrier each);
//   * level f, where the bytes are, moves as float4: C loads and C stores per thread instead of 4C.  On gfx9 a store holds its address / data registers until it
//     completes, and the compiler reuses them for the next one: the twelve scalar stores of the 3-channel tile ran as twelve dependent round trips (an
//     `s_waitcnt vmcnt(0)` in front of each, see the ISA) -- 17 us for 12 MB against 8 us for the 1-channel texture's 4 MB.
template <int C>
__device__ __forceinline__ void mip_pyr_fold_tile5(float* __restrict__ fine_base, const float* __restrict__ rest, const MipDesc& d, int f,
                                                   const uint32_t* __restrict__ mask, int ty, int tx, float (*buf)[16 * 16 * C])
{
    const int tid = threadIdx.x, top = d.levels - 1;
    const int Wf = d.W >> f;
    const bool masked_f = mask != nullptr && f >= 1;
    // element i of the tile's n x n x C block of level f+k (n = 32 >> k, k = 1 .. 4): channel, texel inside the level, in bounds?
    auto locate = [&](int k, int i, int& c, int& ox, int& oy, int64_t& texel) -> bool {
        const int n = 32 >> k, Hl = d.H >> (f + k), Wl = d.W >> (f + k);
        c = i % C; const int t = i / C; ox = t % n; oy = t / n;
        const int Y = ty * n + oy, X = tx * n + ox;
        texel = (int64_t)Y * Wl + X;
        return i < n * n * C && Y < Hl && X < Wl;
    };
    auto load = [&](int k, int i) -> float {
        int c, ox, oy; int64_t texel;
        return locate(k, i, c, ox, oy, texel) ? rest_read<C>(rest, mask, d.off[f + k], texel, c) : 0.f;
    };
    // ---- all loads ----
    // (ancestors: thread j * C + c holds the tile's texel of level top - j, channel c; they meet in LDS below)
    float anc = 0.f;
    if (tid < 16 * C) {
        const int j = tid / C, l = top - j;
        if (l >= f + 5) {
            const int sh = l - f - 5;                           // tile coordinate -> texel of level l (tile = 32 texels of level f = 1 texel of level f+5)
            anc = rest_read<C>(rest, mask, d.off[l], (int64_t)(ty >> sh) * (d.W >> l) + (tx >> sh), tid - j * C);
        }
    }
    const float l4 = load(4, tid), l3 = load(3, tid), l2 = load(2, tid);
    float l1[C];
#pragma unroll
    for (int j = 0; j < C; j++) l1[j] = load(1, tid + 256 * j);
    // level f: the tile is 32 rows of 32 * C floats = 8 * C float4; thread tid owns float4 number tid + 256 * j (j < C) of the tile
    float4 own[C];
    uint32_t ownbits = 0xffffu;                                  // bit 4 * j + m: element m of float4 j holds a value of this step (mask)
    const int64_t f_off = d.off[f] / C;
#pragma unroll
    for (int j = 0; j < C; j++) {
        const int q = tid + 256 * j, row = q / (8 * C), e0 = (q - row * (8 * C)) * 4;
        const int64_t texel0 = (int64_t)(ty * 32 + row) * Wf + tx * 32;
        own[j] = *reinterpret_cast<const float4*>(fine_base + texel0 * C + e0);
        if (masked_f) {
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const int64_t tt = f_off + texel0 + (e0 + m) / C;
                if (!((mask[tt >> 5] >> (tt & 31)) & 1u)) ownbits &= ~(1u << (4 * j + m));
            }
        }
    }
    // ---- the chain, top down ----
    if (tid < 16 * C) buf[1][tid] = anc;
    __syncthreads();
    if (tid < C) {
        float acc = buf[1][tid];
        for (int j = 1; j < 16; j++) if (top - j >= f + 5) acc = __builtin_fmaf(0.25f, acc, buf[1][j * C + tid]);
        buf[0][tid] = acc;                                       // folded level f+5: the tile's one texel there
    }
    int cur = 0;
    auto fold_level = [&](int k, int i, float val) {
        int c, ox, oy; int64_t texel;
        const int n = 32 >> k;
        if (i < n * n * C) {
            const bool in = locate(k, i, c, ox, oy, texel);
            buf[cur ^ 1][i] = in ? __builtin_fmaf(0.25f, buf[cur][((oy >> 1) * (n >> 1) + (ox >> 1)) * C + c], val) : 0.f;
        }
    };
    __syncthreads(); fold_level(4, tid, l4); cur ^= 1;
    __syncthreads(); fold_level(3, tid, l3); cur ^= 1;
    __syncthreads(); fold_level(2, tid, l2); cur ^= 1;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < C; j++) fold_level(1, tid + 256 * j, l1[j]);
    cur ^= 1;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < C; j++) {
        const int q = tid + 256 * j, row = q / (8 * C), e0 = (q - row * (8 * C)) * 4;
        const int64_t texel0 = (int64_t)(ty * 32 + row) * Wf + tx * 32;
        const float o4[4] = {own[j].x, own[j].y, own[j].z, own[j].w};
        float r4[4];
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const int ox = (e0 + m) / C, c = (e0 + m) - ox * C;
            const float mine = ((ownbits >> (4 * j + m)) & 1u) ? o4[m] : 0.f;
            r4[m] = __builtin_fmaf(0.25f, buf[cur][((row >> 1) * 16 + (ox >> 1)) * C + c], mine);
        }
        *reinterpret_cast<float4*>(fine_base + texel0 * C + e0) = make_float4(r4[0], r4[1], r4[2], r4[3]);
    }
}

template <int C>
__device__ __forceinline__ void mip_pyr_fold_body(float* __restrict__ fine_base /* level f */, const float* __restrict__ rest, const MipDesc& d, int f,
                                                  const uint32_t* __restrict__ mask, int bid, float (*buf)[16 * 16 * C])
{
    const int Hf = d.H >> f, Wf = d.W >> f;
    const int tiles_x = (Wf + 31) / 32;
    const int ty = bid / tiles_x, tx = bid - ty * tiles_x;
    const int top = d.levels - 1;
    const int K = min(5, top - f);                              // levels f+1 .. f+K live inside the tile
    // (whole tiles, 16-byte aligned rows and level base: the float4 form)
    if (K == 5 && (Hf & 31) == 0 && (Wf & 31) == 0 && ((uintptr_t)fine_base & 15) == 0) { mip_pyr_fold_tile5<C>(fine_base, rest, d, f, mask, ty, tx, buf); return; }
    // ancestors: levels top .. f+K (one texel each for this tile), folded from the top down by the first C threads
    if (K == 5 && (int)threadIdx.x < C) {
        const int c = threadIdx.x;
        // (all the loads first -- they are independent -- then the dependent chain of fused multiply-adds)
        float gl[16];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int l = top - j;
            gl[j] = 0.f;
            if (l >= f + 5) {
                const int sh = l - f - 5;                       // tile coordinate -> texel of level l (tile = 32 texels of level f = 1 texel of level f+5)
                gl[j] = rest_read<C>(rest, mask, d.off[l], (int64_t)(ty >> sh) * (d.W >> l) + (tx >> sh), c);
            }
        }
        float acc = gl[0];
#pragma unroll
        for (int j = 1; j < 16; j++) if (top - j >= f + 5) acc = __builtin_fmaf(0.25f, acc, gl[j]);
        buf[0][c] = acc;                                         // folded level f+5: the tile's one texel there
    }
    // (K < 5 only for stacks with fewer than six levels above f: then level f+K is the top level and the tile covers all of it)
    int cur = 0;
    if (K < 5) {
        __syncthreads();
        const int n = 32 >> K, Hl = d.H >> (f + K), Wl = d.W >> (f + K);
        for (int i = threadIdx.x; i < n * n * C; i += 256) {
            const int c = i % C, t = i / C, ox = t % n, oy = t / n;
            const int Y = ty * n + oy, X = tx * n + ox;
            buf[1][i] = (Y < Hl && X < Wl) ? rest_read<C>(rest, mask, d.off[f + K], (int64_t)Y * Wl + X, c) : 0.f;
        }
        cur = 1;
    }
    for (int k = K - 1; k >= 1; k--) {
        __syncthreads();
        const int n = 32 >> k, Hl = d.H >> (f + k), Wl = d.W >> (f + k);
        for (int i = threadIdx.x; i < n * n * C; i += 256) {
            const int c = i % C, t = i / C, ox = t % n, oy = t / n;
            const int Y = ty * n + oy, X = tx * n + ox;
            float v = 0.f;
            if (Y < Hl && X < Wl) v = __builtin_fmaf(0.25f, buf[cur][((oy >> 1) * (n >> 1) + (ox >> 1)) * C + c], rest_read<C>(rest, mask, d.off[f + k], (int64_t)Y * Wl + X, c));
            buf[cur ^ 1][i] = v;
        }
        cur ^= 1;
    }
    __syncthreads();
    // level f: 32x32 texels, read-modify-write -- or, under a mask, a plain write (when K == 0 there is nothing above f: the launcher does not call us)
    const bool masked_f = mask != nullptr && f >= 1;                    // (level 0 is not part of the `rest` stack: never masked)
    for (int i = threadIdx.x; i < 32 * 32 * C; i += 256) {
        const int c = i % C, t = i / C, ox = t & 31, oy = t >> 5;
        const int Y = ty * 32 + oy, X = tx * 32 + ox;
        if (Y < Hf && X < Wf) {
            float* o = fine_base + ((size_t)Y * Wf + X) * C + c;
            float own = *o;
            if (masked_f) {
                const int64_t tt = d.off[f] / C + (int64_t)Y * Wf + X;
                own = ((mask[tt >> 5] >> (tt & 31)) & 1u) ? own : 0.f;
            }
            *o = __builtin_fmaf(0.25f, buf[cur][((oy >> 1) * 16 + (ox >> 1)) * C + c], own);
        }
    }
}

template <int C>
__global__ __launch_bounds__(256) void mip_pyr_fold_kernel(float* __restrict__ fine_base /* level f */, const float* __restrict__ rest, MipDesc d, int f)
{
    __shared__ float buf[2][16 * 16 * C];
    mip_pyr_fold_body<C>(fine_base, rest, d, f, nullptr, blockIdx.x, buf);
}

__device__ __forceinline__ float mip_level_from_da(float4 da, int W, int H, int maxl)
{
    float dsdx = da.x * (float)W, dsdy = da.y * (float)W, dtdx = da.z * (float)H, dtdy = da.w * (float)H;
    float A = dsdx * dsdx + dtdx * dtdx, B = dsdy * dsdy + dtdy * dtdy, Cc = dsdx * dsdy + dtdx * dtdy;
    float l2b = 0.5f * (A + B), l2n = 0.25f * (A - B) * (A - B) + Cc * Cc;
    float major = l2b + sqrtf(l2n);
    float lv = 0.5f * log2f(major);
    return fminf(fmaxf(lv, 0.f), (float)maxl);       // log2(0) = -inf clamps to 0
}

struct Tap { int64_t i00, i10, i01, i11; float w00, w10, w01, w11; };

__device__ __forceinline__ Tap bilinear_wrap(float u, float v, int W, int H)
{
    u = u - floorf(u); v = v - floorf(v);                      // boundary_mode='wrap'
    float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;
    float x0f = floorf(x), y0f = floorf(y);
    float fx = x - x0f, fy = y - y0f;
    int x0 = (int)x0f, y0 = (int)y0f, x1 = x0 + 1, y1 = y0 + 1;
    if (x0 < 0) x0 += W;
    if (y0 < 0) y0 += H;
    if (x1 >= W) x1 -= W;
    if (y1 >= H) y1 -= H;
    Tap t;
    t.i00 = (int64_t)y0 * W + x0; t.i10 = (int64_t)y0 * W + x1; t.i01 = (int64_t)y1 * W + x0; t.i11 = (int64_t)y1 * W + x1;
    t.w00 = (1.f - fx) * (1.f - fy); t.w10 = fx * (1.f - fy); t.w01 = (1.f - fx) * fy; t.w11 = fx * fy;
    return t;
}

template <bool BWD>
__device__ __forceinline__ void tex_fetch_body(float* __restrict__ lvl0, float* __restrict__ rest, const MipDesc& d, const float* __restrict__ uv,
                                               const float* __restrict__ uvda, int trilinear, int64_t P, float* __restrict__ io, int bid, int nb)
{
    const int C = d.C;
    for (int64_t p = (int64_t)bid * 256 + threadIdx.x; p < P; p += (int64_t)nb * 256) {
        const float u = uv[2 * p], v = uv[2 * p + 1];
        int l0 = 0, l1 = 0; float f = 0.f;
        if (trilinear && d.levels > 1) {
            float4 da = *reinterpret_cast<const float4*>(uvda + 4 * p);
            float lv = mip_level_from_da(da, d.W, d.H, d.levels - 1);
            l0 = (int)floorf(lv); l1 = min(l0 + 1, d.levels - 1); f = lv - (float)l0;
        }
        float out[4] = {0.f, 0.f, 0.f, 0.f};
        for (int pass = 0; pass < 2; pass++) {
            const int l = pass ? l1 : l0;
            const float wl = pass ? f : 1.f - f;
            if (wl == 0.f) continue;
            Tap t = bilinear_wrap(u, v, d.W >> l, d.H >> l);
            float* base = l == 0 ? lvl0 : rest + d.off[l];
            for (int ch = 0; ch < C; ch++) {
                if (BWD) {
                    float g = io[(int64_t)C * p + ch] * wl;
                    if (g != 0.f) {
                        atomicAdd(base + t.i00 * C + ch, g * t.w00); atomicAdd(base + t.i10 * C + ch, g * t.w10);
                        atomicAdd(base + t.i01 * C + ch, g * t.w01); atomicAdd(base + t.i11 * C + ch, g * t.w11);
                    }
                } else {
                    out[ch] += wl * (base[t.i00 * C + ch] * t.w00 + base[t.i10 * C + ch] * t.w10 + base[t.i01 * C + ch] * t.w01 + base[t.i11 * C + ch] * t.w11);
                }
            }
        }
        if (!BWD) for (int ch = 0; ch < C; ch++) io[(int64_t)C * p + ch] = out[ch];
    }
}

template <bool BWD>
__global__ __launch_bounds__(256) void tex_fetch_kernel(float* __restrict__ lvl0, float* __restrict__ rest, MipDesc d, const float* __restrict__ uv,
                                                        const float* __restrict__ uvda, int trilinear, int64_t P, float* __restrict__ io)
{
    tex_fetch_body<BWD>(lvl0, rest, d, uv, uvda, trilinear, P, io, blockIdx.x, gridDim.x);
}

constexpr int kTailElems = 16 * 16 * 4;     // levels with at most this many elements are handled by the single-block tail kernels (measured: 64^2 1.36, 32^2 1.31, 16^2 1.29, 8^2 1.29, none 1.31 ms per material step)

static int tail_begin(const MipDesc& d)
{
    int l = 1;
    while (l < d.levels && (int64_t)(d.H >> l) * (d.W >> l) * d.C > kTailElems) l++;
    return l < 2 ? 2 : l;        // first level produced by the tail kernel (level 1 always comes from the separate level-0 pointer)
}

static void launch_down(const float* src, float* dst, int Hd, int Wd, int C, hipStream_t st)
{
    dim3 grid((Wd * C + 255) / 256, Hd > 4096 ? 4096 : Hd);
    with_channels(C, [&](auto c) { hipLaunchKernelGGL(mip_down_kernel<decltype(c)::value>, grid, dim3(256), 0, st, src, dst, Hd, Wd); });
}

static void launch_fold(float* fine, const float* coarse, int Hf, int Wf, int C, hipStream_t st)
{
    dim3 grid((Wf * C + 255) / 256, Hf > 4096 ? 4096 : Hf);
    with_channels(C, [&](auto c) { hipLaunchKernelGGL(mip_fold_kernel<decltype(c)::value>, grid, dim3(256), 0, st, fine, coarse, Hf, Wf); });
}

// ---- atomics-free texture backward for FIXED (uv, uv_da): the taps of a view never change, so they are enumerated once, sorted by
// texel on the host side (torch.sort) and replayed as a gather: one thread per touched texel sums its (pixel, weight) list in a fixed
// order -- deterministic, and ~10x faster than the float-atomic scatter of tex_fetch_kernel<true>.
// key = unified texel index over [level 0 | levels 1.. in `rest` order]; skipped taps (blend weight 0) get key -1.
__global__ __launch_bounds__(256) void tex_taps_kernel(MipDesc d, const float* __restrict__ uv, const float* __restrict__ uvda, int trilinear,
                                                       int64_t P, long long* __restrict__ keys, float* __restrict__ weights)
{
    const int64_t n0 = (int64_t)d.H * d.W;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) {
        const float u = uv[2 * p], v = uv[2 * p + 1];
        int l0 = 0, l1 = 0; float f = 0.f;
        if (trilinear && d.levels > 1) {
            float4 da = *reinterpret_cast<const float4*>(uvda + 4 * p);
            float lv = mip_level_from_da(da, d.W, d.H, d.levels - 1);
            l0 = (int)floorf(lv); l1 = min(l0 + 1, d.levels - 1); f = lv - (float)l0;
        }
        for (int pass = 0; pass < 2; pass++) {
            const int l = pass ? l1 : l0;
            const float wl = pass ? f : 1.f - f;
            long long* k = keys + 8 * p + 4 * pass;
            float* w = weights + 8 * p + 4 * pass;
            if (wl == 0.f) { k[0] = k[1] = k[2] = k[3] = -1; w[0] = w[1] = w[2] = w[3] = 0.f; continue; }
            Tap t = bilinear_wrap(u, v, d.W >> l, d.H >> l);
            const int64_t base = l == 0 ? 0 : n0 + d.off[l] / d.C;
            k[0] = base + t.i00; k[1] = base + t.i10; k[2] = base + t.i01; k[3] = base + t.i11;
            w[0] = wl * t.w00; w[1] = wl * t.w10; w[2] = wl * t.w01; w[3] = wl * t.w11;
        }
    }
}

template <int C>
__device__ __forceinline__ void tex_gather_body(float* __restrict__ lvl0, float* __restrict__ rest, int64_t n0, const long long* __restrict__ seg_key,
                                                const int* __restrict__ seg_start, const int* __restrict__ seg_count, int n_seg,
                                                const int* __restrict__ pix, const float* __restrict__ w, const float* __restrict__ d_out, int bid, int nb,
                                                const float* __restrict__ d_out2 = nullptr /* a second gradient of the same fetch output, added on the fly */)
{
    constexpr int R = 8;                                         // taps per round
    for (int s = bid * 256 + threadIdx.x; s < n_seg; s += nb * 256) {
        const long long key = seg_key[s];
        const int b = seg_start[s], e = b + seg_count[s];    // (all three loads before the first branch: one round trip, not three)
        if (key < n0 && !lvl0) continue;                     // (caller passed no level-0 buffer: it promised that no list samples level 0)
        float acc[C];
        for (int c = 0; c < C; c++) acc[c] = 0.f;
        // The launch lasts as long as its LONGEST list (one thread per touched texel; median 2 taps, 99.9 % below 40, a few coarse-level texels near 100 --
        // profiles/r04/tap_level_probe.txt), and a tap is two dependent loads (index + weight, then the gathered gradient).  Eight taps' loads are in flight per
        // round (a short tail re-reads the last tap), and the next round's indices and weights are requested BEFORE this round's gradient values are consumed:
        // one round trip per eight taps instead of two per four.  The fused multiply-adds stay in list order, one per real tap: the sum keeps its bits.
        int pp[R]; float ww[R];
#pragma unroll
        for (int k = 0; k < R; k++) { const int ik = min(b + k, e - 1); pp[k] = pix[ik]; ww[k] = w[ik]; }
        for (int i = b; i < e; i += R) {
            const int n = e - i;                                   // taps of this round: R, or fewer in the last one
            float v[R][C];
#pragma unroll
            for (int k = 0; k < R; k++)
#pragma unroll
                for (int c = 0; c < C; c++) v[k][c] = d_out[(int64_t)pp[k] * C + c];
            // (two consumers of one fetch output -- the specular term and the loss both read the roughness -- send two gradients: their sum, the float
            // autograd's add kernel would have written, is formed here instead)
            if (d_out2) {
#pragma unroll
                for (int k = 0; k < R; k++)
#pragma unroll
                    for (int c = 0; c < C; c++) v[k][c] += d_out2[(int64_t)pp[k] * C + c];
            }
            float wc[R];
#pragma unroll
            for (int k = 0; k < R; k++) wc[k] = ww[k];
            if (i + R < e) {
#pragma unroll
                for (int k = 0; k < R; k++) { const int ik = min(i + R + k, e - 1); pp[k] = pix[ik]; ww[k] = w[ik]; }
            }
#pragma unroll
            for (int c = 0; c < C; c++) {
                float a = acc[c];
#pragma unroll
                for (int k = 0; k < R; k++) if (k < n) a = __builtin_fmaf(v[k][c], wc[k], a);
                acc[c] = a;
            }
        }
        float* o = key < n0 ? lvl0 + key * C : rest + (key - n0) * C;
        for (int c = 0; c < C; c++) o[c] = acc[c];
    }
}

template <int C>
__global__ __launch_bounds__(256) void tex_gather_kernel(float* __restrict__ lvl0, float* __restrict__ rest, int64_t n0, const long long* __restrict__ seg_key,
                                                         const int* __restrict__ seg_start, const int* __restrict__ seg_count, int n_seg,
                                                         const int* __restrict__ pix, const float* __restrict__ w, const float* __restrict__ d_out)
{
    tex_gather_body<C>(lvl0, rest, n0, seg_key, seg_start, seg_count, n_seg, pix, w, d_out, blockIdx.x, gridDim.x);
}

// blocks of the pyramid kernels (build and fold) over level l: one per 32x32-texel tile
static int pyr_blocks(const MipDesc& d, int l) { return (((d.H >> l) + 31) / 32) * (((d.W >> l) + 31) / 32); }

// One pyramid launch builds at most five levels above its source level s; the single-block tail kernel makes the rest, from level `tail` on.
struct PyrPlan { int n_out, tail; };
static PyrPlan pyr_plan(int levels, int s)
{
    const int n_out = (levels - 1 - s) < 5 ? (levels - 1 - s) : 5;
    return {n_out, s + n_out + 1};
}

// builds levels from_level+1 .. levels-1 into `rest`; from_level = 0: from the caller's level-0 texture, = 1: level 1 is already
// in `rest` (the fused optimiser wrote it while it updated the texture, texir_adam_step_tex)
// TEXIR_MIP_PER_LEVEL=1 keeps the first implementation (one launch per level) alive: the parity tests run both and demand identical bits
static bool mip_per_level() { return env().mip_per_level != 0; }

hipError_t launch_mip_build(const float* tex, float* rest, int H, int W, int C, int levels, int from_level, hipStream_t st)
{
    if (levels <= 1 + from_level) return hipSuccess;
    MipDesc d = make_desc(H, W, C, levels);
    if (mip_per_level()) {
        const int lt = tail_begin(d);
        for (int l = 1 + from_level; l < lt && l < levels; l++) {
            const float* src_l = l == 1 ? tex : rest + d.off[l - 1];
            launch_down(src_l, rest + d.off[l], H >> l, W >> l, C, st);
        }
        if (lt < levels) hipLaunchKernelGGL(mip_down_tail_kernel, dim3(1), dim3(1024), 0, st, rest, d, lt);
        return hipGetLastError();
    }
    const int s_lvl = from_level;
    const PyrPlan pl = pyr_plan(levels, s_lvl);
    const float* src = s_lvl == 0 ? tex : rest + d.off[s_lvl];
    with_channels(C, [&](auto c) {
        hipLaunchKernelGGL(mip_pyr_down_kernel<decltype(c)::value>, dim3(pyr_blocks(d, s_lvl)), dim3(256), 0, st, src, rest, d, s_lvl, pl.n_out);
    });
    // (the levels above the pyramid: a last-block-finishes fusion was measured -- 16 384 same-address atomics cost 0.5 ms against this 5 us launch)
    if (pl.tail < levels) hipLaunchKernelGGL(mip_down_tail_kernel, dim3(1), dim3(1024), 0, st, rest, d, pl.tail);
    return hipGetLastError();
}

hipError_t launch_tex_taps(int H, int W, int C, int levels, const float* uv, const float* uvda, int trilinear, int64_t P, long long* keys,
                           float* weights, hipStream_t st)
{
    if (P <= 0) return hipSuccess;
    MipDesc d = make_desc(H, W, C, levels);
    hipLaunchKernelGGL(tex_taps_kernel, dim3(grid_capped(256, P, 4096)), dim3(256), 0, st, d, uv, uvda, trilinear, P, keys, weights);
    return hipGetLastError();
}

static void launch_folds(float* d_tex, float* grad_rest, const MipDesc& d, int f, hipStream_t st)
{
    // one launch folds the whole stack into level f (1: level 1 stays un-folded into level 0 -- texir_adam_step_tex adds
    // 0.25 * level 1 while it reads the gradient; 2: level 2 stays un-folded into level 1 as well, the optimiser step takes both folds over)
    if (d.levels - 1 - f < 1) return;
    if (mip_per_level()) {
        const int lt = tail_begin(d);
        // small levels: levels-1 .. lt folded down to level lt-1 inside one block
        if (lt < d.levels) hipLaunchKernelGGL(mip_fold_tail_kernel, dim3(1), dim3(1024), 0, st, grad_rest, d, lt - 1 > f ? lt - 1 : f);
        for (int l = (lt < d.levels ? lt : d.levels) - 1; l >= 1 + f; l--) {
            float* fine_l = l == 1 ? d_tex : grad_rest + d.off[l - 1];
            launch_fold(fine_l, grad_rest + d.off[l], d.H >> (l - 1), d.W >> (l - 1), d.C, st);
        }
        return;
    }
    float* fine = f == 0 ? d_tex : grad_rest + d.off[f];
    with_channels(d.C, [&](auto c) { hipLaunchKernelGGL(mip_pyr_fold_kernel<decltype(c)::value>, dim3(pyr_blocks(d, f)), dim3(256), 0, st, fine, grad_rest, d, f); });
}

// d_tex and grad_rest zero on entry; gather of the sorted tap lists, then the same folds as launch_tex_fetch_bwd (rest_mask, d_out2: the batched launch alone)
hipError_t launch_tex_gather_bwd(const texir_tex_gather_job& q, hipStream_t st)
{
    MipDesc d = make_desc(q.H, q.W, q.C, q.levels);
    const int64_t n0 = (int64_t)q.H * q.W;
    if (q.n_seg > 0) {
        dim3 grid(grid_capped(256, q.n_seg, 4096));
        with_channels(q.C, [&](auto c) {
            hipLaunchKernelGGL(tex_gather_kernel<decltype(c)::value>, grid, dim3(256), 0, st, q.d_tex, q.grad_rest, n0, (const long long*)q.seg_key, q.seg_start, q.seg_count, q.n_seg,
                               q.pix, q.weights, q.d_out);
        });
    }
    if (q.filter_mode && q.levels > 1) launch_folds(q.d_tex, q.grad_rest, d, q.defer_last_fold, st);
    return hipGetLastError();
}

// (the fetch alone: q.build_from is the batched launch's)
hipError_t launch_tex_fetch(const texir_tex_fetch_job& q, hipStream_t st)
{
    if (q.P <= 0) return hipSuccess;
    MipDesc d = make_desc(q.H, q.W, q.C, q.levels);
    hipLaunchKernelGGL(tex_fetch_kernel<false>, dim3(grid_capped(256, q.P, 4096)), dim3(256), 0, st, const_cast<float*>(q.tex), q.mips_rest, d, q.uv, q.uv_da, q.filter_mode, q.P, q.out);
    return hipGetLastError();
}

// d_tex [H,W,C] and grad_rest [mip_total_elems] must be zero on entry; on return d_tex holds d loss / d texture
hipError_t launch_tex_fetch_bwd(float* d_tex, float* grad_rest, int H, int W, int C, int levels, const float* uv, const float* uvda, int trilinear,
                                int64_t P, const float* d_out, int fold_to_level, hipStream_t st)
{
    MipDesc d = make_desc(H, W, C, levels);
    if (P > 0)
        hipLaunchKernelGGL(tex_fetch_kernel<true>, dim3(grid_capped(256, P, 4096)), dim3(256), 0, st, d_tex, grad_rest, d, uv, uvda, trilinear, P, const_cast<float*>(d_out));
    if (trilinear && levels > 1) launch_folds(d_tex, grad_rest, d, fold_to_level, st);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------
// Batched launches (include/texir_hip.h, "batched forms"): one launch per KIND of kernel for up to TEXIR_MAX_BATCH textures.  A step over the
// albedo and the roughness texture is latency-bound in these kernels (5 ... 20 us each, the launch-to-launch floor is ~4.7 us): dealing the
// blocks of ONE grid to the jobs removes a launch per kind and lets the short jobs hide in the long ones' tails.  The job bodies are the
// single-texture kernels' own (…_body above), so every job's result keeps its bits.
// ------------------------------------------------------------------------------------------------------------------
struct PyrDownJob { const float* src; float* rest; MipDesc d; int s, n_out, first; };
struct PyrDownBatch { int n; PyrDownJob j[kMaxBatch]; };
struct TailJob { float* rest; MipDesc d; int l_begin; };
struct TailBatch { int n; TailJob j[kMaxBatch]; };
struct FetchJob { float* lvl0; float* rest; MipDesc d; const float* uv; const float* uvda; int trilinear; int64_t P; float* out; int first, nb; };
struct FetchBatch { int n; FetchJob j[kMaxBatch]; };
struct GatherJob { float* lvl0; float* rest; int64_t n0; const long long* seg_key; const int* seg_start; const int* seg_count; int n_seg; const int* pix; const float* w;
                   const float* d_out; const float* d_out2; int C, first, nb; };
struct GatherBatch { int n; GatherJob j[kMaxBatch]; };
struct FoldJob { float* fine; const float* rest; MipDesc d; int f; const uint32_t* mask; int first; };
struct FoldBatch { int n; FoldJob j[kMaxBatch]; };

__global__ __launch_bounds__(256) void mip_pyr_down_batch_kernel(PyrDownBatch b)
{
    __shared__ float smem[2 * 16 * 16 * 4];
    const PyrDownJob& J = b.j[job_of_block(b, blockIdx.x)];
    const int bid = blockIdx.x - J.first;
    with_channels(J.d.C, [&](auto c) {
        constexpr int C = decltype(c)::value;
        mip_pyr_down_body<C>(J.src, J.rest, J.d, J.s, J.n_out, bid, reinterpret_cast<float (*)[16 * 16 * C]>(smem));
    });
}

__global__ __launch_bounds__(1024) void mip_down_tail_batch_kernel(TailBatch b)
{
    const TailJob& J = b.j[blockIdx.x];
    mip_down_tail_body(J.rest, J.d, J.l_begin);
}

__global__ __launch_bounds__(256) void tex_fetch_batch_kernel(FetchBatch b)
{
    const FetchJob& J = b.j[job_of_block(b, blockIdx.x)];
    tex_fetch_body<false>(J.lvl0, J.rest, J.d, J.uv, J.uvda, J.trilinear, J.P, J.out, blockIdx.x - J.first, J.nb);
}

__global__ __launch_bounds__(256) void tex_gather_batch_kernel(GatherBatch b)
{
    const GatherJob& J = b.j[job_of_block(b, blockIdx.x)];
    const int bid = blockIdx.x - J.first;
    with_channels(J.C, [&](auto c) {
        tex_gather_body<decltype(c)::value>(J.lvl0, J.rest, J.n0, J.seg_key, J.seg_start, J.seg_count, J.n_seg, J.pix, J.w, J.d_out, bid, J.nb, J.d_out2);
    });
}

__global__ __launch_bounds__(256) void mip_pyr_fold_batch_kernel(FoldBatch b)
{
    __shared__ float smem[2 * 16 * 16 * 4];
    const FoldJob& J = b.j[job_of_block(b, blockIdx.x)];
    const int bid = blockIdx.x - J.first;
    // (written out: through with_channels this one kernel comes out as other code -- the same 8263 instructions, other registers -- and the batched fold is measured as it is)
    switch (J.d.C) {
        case 1: mip_pyr_fold_body<1>(J.fine, J.rest, J.d, J.f, J.mask, bid, reinterpret_cast<float (*)[16 * 16 * 1]>(smem)); break;
        case 2: mip_pyr_fold_body<2>(J.fine, J.rest, J.d, J.f, J.mask, bid, reinterpret_cast<float (*)[16 * 16 * 2]>(smem)); break;
        case 3: mip_pyr_fold_body<3>(J.fine, J.rest, J.d, J.f, J.mask, bid, reinterpret_cast<float (*)[16 * 16 * 3]>(smem)); break;
        default: mip_pyr_fold_body<4>(J.fine, J.rest, J.d, J.f, J.mask, bid, reinterpret_cast<float (*)[16 * 16 * 4]>(smem)); break;
    }
}

// g[t][c] += (bit t of mask) ? g0[t][c] : 0 -- the sparse level-0 gradient (valid under the view's tap mask only) folded into a DENSE level-0 gradient that another
// fetch of the same texture produced in the same backward pass (stage 1: the un-mipmapped roughness fetch is dense, the trilinear one sparse).  One pass; the
// torch form it replaces (shift, and, bool, where, add_ over the whole texture: five launches, 130 us at 4096^2) computed the same sums in the same order.
__global__ __launch_bounds__(256) void grad_add_masked_kernel(float* __restrict__ g, const float* __restrict__ g0, const uint32_t* __restrict__ mask, int64_t n_texels, int C)
{
    const int64_t n = n_texels * C;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t t = i / C;
        const bool on = (mask[t >> 5] >> (t & 31)) & 1u;
        if (on) g[i] = g[i] + g0[i];                                 // (a texel whose bit is clear keeps its bits: -0 + 0 would turn a negative zero over)
    }
}

hipError_t launch_grad_add_masked(float* g, const float* g0, const uint32_t* mask, int64_t n_texels, int C, hipStream_t st)
{
    hipLaunchKernelGGL(grad_add_masked_kernel, dim3(grid_capped(256 * 4, n_texels * C, 4096)), dim3(256), 0, st, g, g0, mask, n_texels, C);
    return hipGetLastError();
}

hipError_t launch_tex_fetch_batch(const texir_tex_fetch_job* jobs, int n, hipStream_t st)
{
    // the reference form (one launch per level, TEXIR_MIP_PER_LEVEL=1) stays a sequence of single launches
    if (mip_per_level() || n == 1) {
        for (const texir_tex_fetch_job* q = jobs; q < jobs + n; q++)
            if (hipError_t e = q->build_from < 0 ? hipSuccess : launch_mip_build(q->tex, q->mips_rest, q->H, q->W, q->C, q->levels, q->build_from, st); e != hipSuccess) return e;
        for (int k = 0; k < n; k++)
            if (hipError_t e = launch_tex_fetch(jobs[k], st); e != hipSuccess) return e;
        return hipSuccess;
    }
    PyrDownBatch pb; pb.n = 0;
    TailBatch tb; tb.n = 0;
    int blocks = 0;
    for (int k = 0; k < n; k++) {
        const texir_tex_fetch_job& q = jobs[k];
        if (q.build_from < 0 || q.levels <= 1 + q.build_from) continue;
        MipDesc d = make_desc(q.H, q.W, q.C, q.levels);
        const int s_lvl = q.build_from;
        const PyrPlan pl = pyr_plan(q.levels, s_lvl);
        PyrDownJob& J = pb.j[pb.n++];
        J.src = s_lvl == 0 ? q.tex : q.mips_rest + d.off[s_lvl]; J.rest = q.mips_rest; J.d = d; J.s = s_lvl; J.n_out = pl.n_out; J.first = blocks;
        blocks += pyr_blocks(d, s_lvl);
        if (pl.tail < q.levels) { TailJob& T = tb.j[tb.n++]; T.rest = q.mips_rest; T.d = d; T.l_begin = pl.tail; }
    }
    if (pb.n > 0) hipLaunchKernelGGL(mip_pyr_down_batch_kernel, dim3(blocks), dim3(256), 0, st, pb);
    if (tb.n > 0) hipLaunchKernelGGL(mip_down_tail_batch_kernel, dim3(tb.n), dim3(1024), 0, st, tb);
    FetchBatch fb; fb.n = 0;
    blocks = 0;
    for (int k = 0; k < n; k++) {
        const texir_tex_fetch_job& q = jobs[k];
        if (q.P <= 0) continue;
        FetchJob& J = fb.j[fb.n++];
        J.lvl0 = const_cast<float*>(q.tex); J.rest = q.mips_rest; J.d = make_desc(q.H, q.W, q.C, q.levels); J.uv = q.uv; J.uvda = q.uv_da; J.trilinear = q.filter_mode; J.P = q.P; J.out = q.out;
        J.first = blocks; J.nb = grid_capped(256, q.P, 4096);
        blocks += J.nb;
    }
    if (fb.n > 0) hipLaunchKernelGGL(tex_fetch_batch_kernel, dim3(blocks), dim3(256), 0, st, fb);
    return hipGetLastError();
}

hipError_t launch_tex_gather_bwd_batch(const texir_tex_gather_job* jobs, int n, hipStream_t st)
{
    if (mip_per_level()) {
        for (int k = 0; k < n; k++)
            if (hipError_t e = launch_tex_gather_bwd(jobs[k], st); e != hipSuccess) return e;
        return hipSuccess;
    }
    GatherBatch gb; gb.n = 0;
    int blocks = 0;
    for (int k = 0; k < n; k++) {
        const texir_tex_gather_job& q = jobs[k];
        if (q.n_seg <= 0) continue;
        GatherJob& J = gb.j[gb.n++];
        J.lvl0 = q.d_tex; J.rest = q.grad_rest; J.n0 = (int64_t)q.H * q.W; J.seg_key = (const long long*)q.seg_key; J.seg_start = q.seg_start; J.seg_count = q.seg_count; J.n_seg = q.n_seg;
        J.pix = q.pix; J.w = q.weights; J.d_out = q.d_out; J.d_out2 = q.d_out2; J.C = q.C; J.first = blocks; J.nb = grid_capped(256, q.n_seg, 4096);
        blocks += J.nb;
    }
    if (gb.n > 0) hipLaunchKernelGGL(tex_gather_batch_kernel, dim3(blocks), dim3(256), 0, st, gb);
    FoldBatch fb; fb.n = 0;
    blocks = 0;
    for (int k = 0; k < n; k++) {
        const texir_tex_gather_job& q = jobs[k];
        const int f = q.defer_last_fold;
        if (!(q.filter_mode == 1 && q.levels > 1) || q.levels - 1 - f < 1) continue;
        FoldJob& J = fb.j[fb.n++];
        J.d = make_desc(q.H, q.W, q.C, q.levels);
        J.fine = f == 0 ? q.d_tex : q.grad_rest + J.d.off[f]; J.rest = q.grad_rest; J.f = f; J.mask = q.rest_mask; J.first = blocks;
        blocks += pyr_blocks(J.d, f);
    }
    if (fb.n > 0) hipLaunchKernelGGL(mip_pyr_fold_batch_kernel, dim3(blocks), dim3(256), 0, st, fb);
    return hipGetLastError();
}

}  // namespace texir

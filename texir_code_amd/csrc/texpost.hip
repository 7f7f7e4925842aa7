// The asset step between the two stages (tools/padding_texture.py:49-87): every zero texel of the irradiance texture takes the value of its nearest
// non-zero texel, then the texture is denoised.  The reference does the first with scipy's Euclidean distance transform + grid_sample on the CPU and the
// second by piping the file through the Open Image Denoise binary; here both are kernels on the device texture the IrT stage has just produced.
//
// (a)+(b) texpost_column_kernel, texpost_fill_kernel: exact nearest-valid-texel transform and its application.
//   A texel is a hole when c0 + c1 + c2 (float32, in that order) == 0.0 (padding_texture.py:54-56).
//   Phase 1, one lane per column (lanes along x: coalesced): g[y][x] = the non-hole row of column x nearest to y, -1 when the column has none.  A downward
//   sweep carries the last non-hole row above, an upward sweep the next one below; on equal distance the UPPER row wins.
//   Phase 2, one lane per texel: the squared distance to the nearest non-hole texel of column x' is (x - x')^2 + (g[y][x'] - y)^2, so the lane walks
//   outwards, dx = 0, 1, 2, ... (column x - dx, then column x + dx), keeps the best exact integer squared distance and stops once dx^2 >= best: no column
//   further out can be strictly nearer.  That is the same minimisation Meijster's second phase performs with a lower envelope, done by direct search: the
//   walk of a hole is as long as the hole is deep (tens of texels in an atlas) and a non-hole texel stops at once.  There is NO window: a texel whose
//   nearest source is W - 1 columns away walks W - 1 columns.  The worst case -- one valid texel in a 4096^2 image -- is 2 x 4096 cached, lane-coalesced
//   loads per texel.
//   TIE RULE (deterministic, independent of the launch configuration): among the texels at minimal squared distance the one met FIRST wins, in the order
//   column x; x - 1, x + 1; x - 2, x + 2; ... and, inside one column, the upper of two equidistant rows.
//   All distances are int32: H, W <= 16384 keeps 2 * 16384^2 below 2^31.
//
// (c) atrous_kernel: the fused form of tools.denoise_atrous -- an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) on log(1 + x), one launch
//   per pass, the 25 taps in the torch loop's order (dy outer, dx inner) with separately rounded float ops, optional normal / position guides.
//   Between passes the buffers hold log-domain colours, which are never negative; the sign bit of channel 0 carries "this texel is a hole" from the
//   first pass (which sees the image) to the later ones, so a tap costs one texel read, not one of the colour and one of the image.
//   Two forms with identical bits: taps as plain global loads (coalesced across lanes), or from an LDS tile of 32 x 8 texels + a 2 * step halo
//   (planar, one float plane per channel: lanes read consecutive words, no bank conflicts).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env.h"
#include "kernels.h"

namespace texir {

// the torch path evaluates every product, difference and sum of these formulas as its own rounded float op
#pragma clang fp contract(off)

constexpr int kPB = 256;
constexpr int kCB = 64;                  // phase 1 has only W lanes of work: one wave per block spreads them over W / 64 compute units

template <int C>
__device__ __forceinline__ bool texel_is_hole(const float* __restrict__ p)
{
    float s = p[0];
#pragma unroll
    for (int c = 1; c < C; c++) s = s + p[c];
    return s == 0.0f;
}

// phase 1: one lane per column
template <int C>
__global__ __launch_bounds__(kCB) void texpost_column_kernel(const float* __restrict__ img, int H, int W, int32_t* __restrict__ g)
{
    const int x = blockIdx.x * kCB + threadIdx.x;
    if (x >= W) return;
    int last = -1;
    for (int y = 0; y < H; y++) {
        const size_t t = (size_t)y * W + x;
        if (!texel_is_hole<C>(img + t * C)) last = y;
        g[t] = last;
    }
    int next = -1;
    for (int y = H - 1; y >= 0; y--) {
        const size_t t = (size_t)y * W + x;
        const int up = g[t];
        if (up == y) { next = y; continue; }
        if (next >= 0 && (up < 0 || next - y < y - up)) g[t] = next;      // strictly nearer below; equal distance keeps the upper row
    }
}

// phase 2 + apply: one lane per texel
template <int C>
__global__ __launch_bounds__(kPB) void texpost_fill_kernel(const float* __restrict__ img, int H, int W, const int32_t* __restrict__ g,
                                                           const int32_t* __restrict__ row_map, const int32_t* __restrict__ col_map,
                                                           float* __restrict__ out, int32_t* __restrict__ src)
{
    const int x = blockIdx.x * kPB + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const int32_t* __restrict__ grow = g + (size_t)y * W;
    const size_t t = (size_t)y * W + x;
    int best = 0x7fffffff, br = -1, bc = -1;
    {
        const int r = grow[x];
        if (r >= 0) { best = (r - y) * (r - y); br = r; bc = x; }
    }
    for (int dx = 1; dx < W; dx++) {
        const int d0 = dx * dx;
        if (d0 >= best) break;
        const int xl = x - dx, xr = x + dx;
        if (xl < 0 && xr >= W) break;
        if (xl >= 0) {
            const int r = grow[xl];
            if (r >= 0) { const int d = d0 + (r - y) * (r - y); if (d < best) { best = d; br = r; bc = xl; } }
        }
        if (xr < W) {
            const int r = grow[xr];
            if (r >= 0) { const int d = d0 + (r - y) * (r - y); if (d < best) { best = d; br = r; bc = xr; } }
        }
    }
    const int s = br < 0 ? -1 : br * W + bc;
    if (src) src[t] = s;
    float v[C];
    if (s < 0 || (size_t)s == t) {                    // a non-hole keeps its bits; so does every texel of an image without a non-hole
#pragma unroll
        for (int c = 0; c < C; c++) v[c] = img[t * C + c];
    } else {
        int rr = br, cc = bc;
        if (row_map) { rr = row_map[br]; cc = col_map[bc]; }          // `reference`: what grid_sample(nearest, align_corners=False) reads for (br, bc)
        const bool ok = rr >= 0 && cc >= 0;
        const size_t q = ok ? (size_t)rr * W + cc : 0;
#pragma unroll
        for (int c = 0; c < C; c++) v[c] = ok ? img[q * C + c] : 0.0f;
    }
#pragma unroll
    for (int c = 0; c < C; c++) out[t * C + c] = v[c];
}

size_t texpost_pad_workspace_bytes(int H, int W) { return (size_t)H * W * sizeof(int32_t); }

hipError_t launch_texture_pad(const float* img, int H, int W, int C, const int32_t* row_map, const int32_t* col_map, float* out, int32_t* src,
                              void* workspace, hipStream_t st)
{
    int32_t* g = (int32_t*)workspace;
    const dim3 gc((W + kCB - 1) / kCB), gf((W + kPB - 1) / kPB, H);
#define TEXPOST_PAD(C_)                                                                                         \
    case C_:                                                                                                    \
        texpost_column_kernel<C_><<<gc, kCB, 0, st>>>(img, H, W, g);                                            \
        texpost_fill_kernel<C_><<<gf, kPB, 0, st>>>(img, H, W, g, row_map, col_map, out, src);                  \
        break;
    switch (C) { TEXPOST_PAD(1) TEXPOST_PAD(2) TEXPOST_PAD(3) TEXPOST_PAD(4) default: return hipErrorInvalidValue; }
#undef TEXPOST_PAD
    return hipGetLastError();
}

// ---- (c) --------------------------------------------------------------------------------------------------------------------------------------------

constexpr int kTX = 32, kTY = 8;              // texels per block (both forms)
constexpr int kMaxLdsStep = 4;                // largest hole size the LDS tile is built for: (32 + 16) x (8 + 16) texels, 10 planes = 45 KB

struct AtrousArgs {
    const float* in;            // pass 0: the image; later: log-domain colours, sign bit of channel 0 set on holes
    const float* nrm;           // nullable guides [H,W,3]
    const float* pos;
    float* out;
    int H, W, step;
    float s2c, s2n, s2p;        // sigma^2 of this pass (colour: already halved per pass); guides: 0 = term off
};

__device__ __forceinline__ bool sign_set(float v) { return (__float_as_uint(v) >> 31) != 0; }

// one texel as the filter sees it: log-domain colour + validity
template <bool FIRST>
__device__ __forceinline__ void decode_texel(float r0, float r1, float r2, float c[3], bool& valid)
{
    if (FIRST) {
        valid = ((r0 + r1) + r2) != 0.0f;
        c[0] = log1pf(fmaxf(r0, 0.0f)); c[1] = log1pf(fmaxf(r1, 0.0f)); c[2] = log1pf(fmaxf(r2, 0.0f));
    } else {
        valid = !sign_set(r0);
        c[0] = fabsf(r0); c[1] = r1; c[2] = r2;
    }
}

template <bool FIRST, bool LAST, bool GUIDED, bool LDS>
__global__ __launch_bounds__(kTX* kTY) void atrous_kernel(AtrousArgs a)
{
    extern __shared__ float tile[];
    const int step = a.step, H = a.H, W = a.W;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int x0 = blockIdx.x * kTX, y0 = blockIdx.y * kTY;
    const int x = x0 + tx, y = y0 + ty;
    const int halo = 2 * step, pw = kTX + 2 * halo, ph = kTY + 2 * halo, plane = pw * ph;
    // planes of the tile: c0 c1 c2 valid [n0 n1 n2 p0 p1 p2]

    if (LDS) {
        for (int i = ty * kTX + tx; i < plane; i += kTX * kTY) {
            const int ly = i / pw, lx = i - ly * pw;
            const int gy = y0 + ly - halo, gx = x0 + lx - halo;
            const int cy = min(max(gy, 0), H - 1), cx = min(max(gx, 0), W - 1);          // replicate border (colour, guides)
            const size_t q = ((size_t)cy * W + cx) * 3;
            float c[3]; bool v;
            decode_texel<FIRST>(a.in[q], a.in[q + 1], a.in[q + 2], c, v);
            tile[i] = c[0]; tile[plane + i] = c[1]; tile[2 * plane + i] = c[2];
            tile[3 * plane + i] = (v && gy == cy && gx == cx) ? 1.0f : 0.0f;             // validity is zero outside the image
            if (GUIDED) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    tile[(4 + k) * plane + i] = a.nrm ? a.nrm[q + k] : 0.0f;
                    tile[(7 + k) * plane + i] = a.pos ? a.pos[q + k] : 0.0f;
                }
            }
        }
        __syncthreads();
    }
    if (x >= W || y >= H) return;

    const size_t t = ((size_t)y * W + x) * 3;
    float c[3]; bool valid;
    decode_texel<FIRST>(a.in[t], a.in[t + 1], a.in[t + 2], c, valid);
    float res[3] = {c[0], c[1], c[2]};
    if (valid) {
        float n[3] = {0.f, 0.f, 0.f}, p[3] = {0.f, 0.f, 0.f};
        if (GUIDED) {
#pragma unroll
            for (int k = 0; k < 3; k++) { if (a.nrm) n[k] = a.nrm[t + k]; if (a.pos) p[k] = a.pos[t + k]; }
        }
        const float k1[5] = {1.0f / 16.0f, 4.0f / 16.0f, 6.0f / 16.0f, 4.0f / 16.0f, 1.0f / 16.0f};
        float acc[3] = {0.f, 0.f, 0.f}, wsum = 0.f;
#pragma unroll
        for (int dy = 0; dy < 5; dy++) {
#pragma unroll
            for (int dx = 0; dx < 5; dx++) {
                const int gy = y + (dy - 2) * step, gx = x + (dx - 2) * step;
                float q[3], qn[3], qp[3]; bool qv;
                if (LDS) {
                    const int i = (ty + dy * step) * pw + tx + dx * step;
                    q[0] = tile[i]; q[1] = tile[plane + i]; q[2] = tile[2 * plane + i];
                    qv = tile[3 * plane + i] != 0.0f;
                    if (GUIDED) {
#pragma unroll
                        for (int k = 0; k < 3; k++) { qn[k] = tile[(4 + k) * plane + i]; qp[k] = tile[(7 + k) * plane + i]; }
                    }
                } else {
                    qv = gy >= 0 && gy < H && gx >= 0 && gx < W;
                    if (!qv) continue;                  // weight 0: the torch loop adds +0 here
                    const size_t u = ((size_t)gy * W + gx) * 3;
                    decode_texel<FIRST>(a.in[u], a.in[u + 1], a.in[u + 2], q, qv);
                    if (GUIDED) {
#pragma unroll
                        for (int k = 0; k < 3; k++) { qn[k] = a.nrm ? a.nrm[u + k] : 0.0f; qp[k] = a.pos ? a.pos[u + k] : 0.0f; }
                    }
                }
                if (!qv) continue;
                const float d0 = q[0] - c[0], d1 = q[1] - c[1], d2 = q[2] - c[2];
                float e = ((d0 * d0 + d1 * d1) + d2 * d2) / a.s2c;
                if (GUIDED) {
                    if (a.s2n > 0.0f) { const float m0 = qn[0] - n[0], m1 = qn[1] - n[1], m2 = qn[2] - n[2]; e = e + ((m0 * m0 + m1 * m1) + m2 * m2) / a.s2n; }
                    if (a.s2p > 0.0f) { const float m0 = qp[0] - p[0], m1 = qp[1] - p[1], m2 = qp[2] - p[2]; e = e + ((m0 * m0 + m1 * m1) + m2 * m2) / a.s2p; }
                }
                const float w = (k1[dy] * k1[dx]) * expf(-e);
                acc[0] = acc[0] + q[0] * w; acc[1] = acc[1] + q[1] * w; acc[2] = acc[2] + q[2] * w;
                wsum = wsum + w;
            }
        }
        const float den = fmaxf(wsum, 1e-20f);
        res[0] = acc[0] / den; res[1] = acc[1] / den; res[2] = acc[2] / den;
    }
    if (LAST) {
        a.out[t] = valid ? expm1f(res[0]) : 0.0f; a.out[t + 1] = valid ? expm1f(res[1]) : 0.0f; a.out[t + 2] = valid ? expm1f(res[2]) : 0.0f;
    } else {
        a.out[t] = valid ? res[0] : -res[0]; a.out[t + 1] = res[1]; a.out[t + 2] = res[2];       // (res[0] >= 0: -res[0] sets the sign bit, -0.0 included)
    }
}

// how many of the first passes read their taps from the LDS tile (TEXIR_ATROUS_LDS_PASSES).  Default: every pass the tile is built for (hole sizes 1, 2, 4).
// Measured at 4096^2: each of the three is faster from LDS -- the first by far, because the global-load form evaluates log1p once
// per TAP and the tile once per texel; from hole size 8 on the halo (2 * 16 texels around a 32 x 8 tile) outgrows the tile and the taps are global loads.
int atrous_lds_passes()
{
    const int e = env().atrous_lds_passes;
    return e < 0 ? 3 : e;
}

template <bool GUIDED>
static void atrous_pass(const AtrousArgs& a, bool first, bool last, bool lds, hipStream_t st)
{
    const dim3 grid((a.W + kTX - 1) / kTX, (a.H + kTY - 1) / kTY), block(kTX, kTY);
    const int halo = 2 * a.step;
    const size_t sh = lds ? (size_t)(kTX + 2 * halo) * (kTY + 2 * halo) * (GUIDED ? 10 : 4) * sizeof(float) : 0;
#define ATROUS(F, L)                                                                         \
    do {                                                                                     \
        if (lds) atrous_kernel<F, L, GUIDED, true><<<grid, block, sh, st>>>(a);              \
        else atrous_kernel<F, L, GUIDED, false><<<grid, block, 0, st>>>(a);                  \
    } while (0)
    if (first && last) ATROUS(true, true);
    else if (first) ATROUS(true, false);
    else if (last) ATROUS(false, true);
    else ATROUS(false, false);
#undef ATROUS
}

hipError_t launch_texture_denoise(const float* img, int H, int W, const float* nrm, const float* pos, int iterations, float sigma_c, float sigma_n,
                                  float sigma_p, float* tmp, float* out, hipStream_t st)
{
    const bool guided = (nrm && sigma_n > 0.0f) || (pos && sigma_p > 0.0f);
    const int n_lds = atrous_lds_passes();
    for (int it = 0; it < iterations; it++) {
        AtrousArgs a{};
        // ping-pong so that the last pass lands in `out`
        float* dst = ((iterations - 1 - it) & 1) ? tmp : out;
        a.in = it == 0 ? img : (dst == out ? tmp : out);
        a.out = dst;
        a.nrm = (nrm && sigma_n > 0.0f) ? nrm : nullptr;
        a.pos = (pos && sigma_p > 0.0f) ? pos : nullptr;
        a.H = H; a.W = W; a.step = 1 << it;
        // (sigma_c * 0.5 ** it) ** 2 as the torch path forms it: in double, rounded to float32 when it meets the tensor
        const double sc = (double)sigma_c * (1.0 / (double)(1 << it));
        a.s2c = (float)(sc * sc);
        a.s2n = (float)((double)sigma_n * (double)sigma_n);
        a.s2p = (float)((double)sigma_p * (double)sigma_p);
        const bool lds = it < n_lds && a.step <= kMaxLdsStep;
        if (guided) atrous_pass<true>(a, it == 0, it == iterations - 1, lds, st);
        else atrous_pass<false>(a, it == 0, it == iterations - 1, lds, st);
    }
    return hipGetLastError();
}

}  // namespace texir

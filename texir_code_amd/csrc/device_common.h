// Device-side building blocks shared by the gfx950 kernels: Hammersley/Cranley-Patterson sampling,
// local frames, hemisphere/GGX directions (utils/sample_util.py:28-146), per-lane BVH2 traversal
// with an LDS-resident stack and its build configuration, the query_irf hit shader
// (models/tracer_o3d_irt.py:248-267), the sample order of the multi-texel IrT kernels and wave reductions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "bvh_build.h"

namespace texir {

struct SceneDev {
    const float4* nodes4;  // GpuNode4 as 4 x 16 B (4-wide quantised tree; null when the scene was built binary-only)
    const float4* nodes4f; // GpuNode4F (float child planes of the same tree, index for index) -- read through the scalar cache by wave-uniform
                           // node steps; null = every node step per lane (TEXIR_UNIFORM_FLOAT=0)
    const float4* nodes;   // GpuNode as 4 x float4
    const float4* tris;    // GpuTri as kTriQuads x float4, by leaf-order slot
    const float4* quads;   // GpuQuad as 3 x float4, by record (what the 4-wide tree's leaves name; record r owns slots 2 r, 2 r + 1)
    const float4* uvs;     // GpuTriUV as 2 x float4
    const float* tex;      // [Ht,Wt,3] row-major (layout 0), or the retiled copy the hit shader reads (layouts 1, 2: see shade_hit)
    int Ht, Wt;
    int tex_layout;        // 0 row-major; 1 = 8x8-texel tiles of 12-byte texels; 2 = overlapping 3x3 tiles at stride 2, one 128-byte line each;
                           // 3, 4 = 4-byte shared-exponent texels (pack_texel), overlapping 5x5 tiles at stride 4 / 8x4 tiles at stride 7x3, one line each
    int tiles_x;           // tiles per tile row (layouts 1, 2)
    int sched_weight;      // phase scheduler of trace_closest: weight of the lanes at inner nodes (2; 1 for scenes whose node steps run less than ~60 % full: texir_scene_tune measures it once per scene)
};

// the hit shader's view of a scene (shade_hit): irt_group_kernel's fixed form fills it from its kernel arguments at the hit
struct ShadeDev { const float4* uvs; const float* tex; int Ht, Wt, tiles_x; };

constexpr int kBlock = 256;          // 4 waves
constexpr int kLdsStack = 24;        // default: entries per lane kept in LDS (24 KiB per block)
constexpr int kSentinel = 0x7FFFFFFF;
constexpr int kStackCap = 96;        // LDS part + private overflow; the host checks the tree's worst case against it

// ------------------------------------------------------------------------------------------------
// build configuration of the traversal, shared by every tracing kernel (kernels.hip, gbuffer.hip, texbake.hip, irtsplit.hip, irtlight.hip)
// ------------------------------------------------------------------------------------------------
// Occupancy.  Round 1 (4-byte stack entries): 5 waves / 24 entries 13.85, 6 / 24 14.79, 7 / 16 15.11, 8 / 16 15.06 Grays/s (c4).  Round 2, after the
// scalar node path took the L1 off the critical path (8-byte entries): 6 waves / 12 entries 15.01, 7 / 11 15.82, 8 / 10 15.87 (c2: 16.30, 17.11, 17.40;
// c4_scan: 4.98, 5.31, 5.54): 8 waves per SIMD = 64 VGPRs (the compiler parks the per-texel frame and the ray's shear rows in scratch across the
// traversal loop) and a 10-entry LDS stack.
// Stack entries are 8 bytes (child code + the child's entry distance, see trace_core): 10 x 2 KiB = 20 KiB per block, 8 blocks = all 160 KiB of a CU.
constexpr int kGroupLstk = 10;                          // the IrT kernels (irt_kernel, irt_group_kernel, irt_stream_kernel, irt_split_kernel)
constexpr int kGroupWaves = 8;
constexpr int kLstk = kLdsStack / 2;                    // the single-ray tracing kernels: 24 KiB of stack per block

// ------------------------------------------------------------------------------------------------
// sampling -- kept free of fused multiply-adds so that it tracks the reference's separately rounded
// float32 torch ops (utils/sample_util.py) as closely as the libm differences allow
// ------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)

// sample_util.py:41  float32(double(i)/double(N)).  For N = 2^k (and i < 2^24) the quotient is exact in float32, so the
// multiply by the exact reciprocal gives the identical value without a float64 division.
// (a caller that knows N = 2^k <= 2^24 at compile time takes the product alone, on its own exact 1 / N: texel_sample_dir<MODE>(i, inv_n, ...))
__device__ __forceinline__ float ham0(uint32_t i, uint32_t N)
{
    if ((N & (N - 1u)) == 0u && i < (1u << 24)) return (float)i * (1.0f / (float)N);
    return (float)((double)i / (double)N);
}
// :28-38  float32(double(bitrev(i)) * 2^-32): scaling by a power of two commutes with the rounding to 24 bits
__device__ __forceinline__ float ham1(uint32_t i) { return __uint2float_rn(__brev(i)) * 2.3283064365386963e-10f; }

__device__ __forceinline__ float shift_wrap_clamp(float s, float shift)
{
    s = s + shift;                       // :103
    if (s > 1.f) s = s - 1.f;            // :104-105 (strict >)
    if (s < 0.f) s = s + 1.f;            // :106-107
    return fminf(fmaxf(s, 1e-6f), (float)(1.0 - 1e-6));   // :108
}

struct Frame { float n[3], U[3], V[3]; };

__device__ __forceinline__ Frame make_frame(float nx, float ny, float nz)
{
    Frame f;
    // :84 axis choice on the RAW normal; :86-91 x/(|x|+1e-6)
    float ax = 1.f, ay = 0.f;
    if (fabsf(nx) > 0.99f) { ax = 0.f; ay = 1.f; }
    float ln = sqrtf(nx * nx + ny * ny + nz * nz) + 1e-6f;
    f.n[0] = nx / ln; f.n[1] = ny / ln; f.n[2] = nz / ln;
    float c0 = ay * f.n[2] - 0.f * f.n[1], c1 = 0.f * f.n[0] - ax * f.n[2], c2 = ax * f.n[1] - ay * f.n[0];
    float lc = sqrtf(c0 * c0 + c1 * c1 + c2 * c2) + 1e-6f;
    f.U[0] = c0 / lc; f.U[1] = c1 / lc; f.U[2] = c2 / lc;
    float e0 = f.n[1] * f.U[2] - f.n[2] * f.U[1], e1 = f.n[2] * f.U[0] - f.n[0] * f.U[2], e2 = f.n[0] * f.U[1] - f.n[1] * f.U[0];
    float le = sqrtf(e0 * e0 + e1 * e1 + e2 * e2) + 1e-6f;
    f.V[0] = e0 / le; f.V[1] = e1 / le; f.V[2] = e2 / le;
    return f;
}

// cos/sin of the polar angle for the three modes (:115-143).  MODE >= 0: the mode is the caller's compile-time constant (`mode` is not read) and only
// its arm is compiled -- the arm's expressions are the run-time form's
template <int MODE = -1>
__device__ __forceinline__ void polar(int mode, float s0, float rough, float& ct, float& st)
{
    if constexpr (MODE == 0) { ct = 1.0f - s0; st = sqrtf(1.0f - ct * ct); return; }
    else if constexpr (MODE == 1) { ct = sqrtf(1.0f - s0); st = sqrtf(1.0f - ct * ct); return; }
    else if constexpr (MODE >= 2) mode = MODE;
    if (mode == 0) { ct = 1.0f - s0; st = sqrtf(1.0f - ct * ct); }
    else if (mode == 1) { ct = sqrtf(1.0f - s0); st = sqrtf(1.0f - ct * ct); }
    else {
        float a = rough * rough;
        ct = sqrtf((1.0f - s0) / (1.0f + (a * a - 1.f) * s0));
        ct = fminf(fmaxf(ct, -1.0f + 1e-6f), 1.0f - 1e-6f);
        st = fminf(fmaxf(sqrtf(1.0f - ct * ct), -1.0f + 1e-6f), 1.0f - 1e-6f);
    }
}

// (sin / cos of phi from libm's sincosf, ~70 instructions: the form that is pinned at 5e-6 on the reference's own directions)
template <int MODE = -1>
__device__ __forceinline__ void sample_dir(int mode, float s0, float s1, float rough, const Frame& f, float* L)
{
    float ct, st;
    polar<MODE>(mode, s0, rough, ct, st);
    float sp, cp;
    float phi = 6.283185307179586f * s1 - 3.141592653589793f;
    sincosf(phi, &sp, &cp);
    sp = sp * st; cp = -(cp * st);
    for (int a = 0; a < 3; a++) L[a] = f.V[a] * sp + f.n[a] * ct + f.U[a] * cp;
}

// What the IrT kernels read of texel t: position, RAW normal, the two Cranley-Patterson shifts
struct Texel { float px, py, pz, nx, ny, nz, sh0, sh1; };
__device__ __forceinline__ Texel load_texel(const float* __restrict__ pos, const float* __restrict__ nrm, const float* __restrict__ shift, int64_t t)
{
    Texel x;
    x.px = pos[3 * t]; x.py = pos[3 * t + 1]; x.pz = pos[3 * t + 2];
    x.nx = nrm[3 * t]; x.ny = nrm[3 * t + 1]; x.nz = nrm[3 * t + 2];
    x.sh0 = shift[2 * t]; x.sh1 = shift[2 * t + 1];
    return x;
}

// direction of sample i of N of a texel with shifts (sh0, sh1) and frame f, as the IrT kernels take it (no roughness: modes 0, 1)
__device__ __forceinline__ void texel_sample_dir(int mode, uint32_t i, uint32_t N, float sh0, float sh1, const Frame& f, float* d)
{
    const float s0 = shift_wrap_clamp(ham0(i, N), sh0);
    const float s1 = shift_wrap_clamp(ham1(i), sh1);
    sample_dir(mode, s0, s1, 0.f, f, d);
}
// ... for N = 2^k <= 2^24 and a compile-time MODE, on the caller's inv_n = 1 / N (exact): ham0's product, the same bits
template <int MODE>
__device__ __forceinline__ void texel_sample_dir(uint32_t i, float inv_n, float sh0, float sh1, const Frame& f, float* d)
{
    static_assert(MODE == 0 || MODE == 1, "the IrT kernels' modes");
    const float s0 = shift_wrap_clamp((float)i * inv_n, sh0);
    const float s1 = shift_wrap_clamp(ham1(i), sh1);
    sample_dir<MODE>(MODE, s0, s1, 0.f, f, d);
}

// corner uvs of the triangle in leaf slot `slot`: a = (uv0, uv1), b = (uv2, -, -)
// (SC: SceneDev, or any view of it that has `uvs`)
template <typename SC>
__device__ __forceinline__ void tri_uvs(const SC& sc, int slot, float4& a, float4& b)
{
    // one 32-byte record per quad record: (q0, q1), (q2, q3); the even slot is triangle (q0, q1, q2), the odd one (q3, q2, q1)  (bvh_build.h)
    const size_t rec = (size_t)(slot >> 1);
    const float4 A = sc.uvs[2 * rec], B = sc.uvs[2 * rec + 1];
    const bool odd = (slot & 1) != 0;
    a = odd ? make_float4(B.z, B.w, B.x, B.y) : A;
    b = odd ? make_float4(A.z, A.w, 0.f, 0.f) : B;
}
// ... for irt_group_kernel's fixed form: both halves of the record loaded at once.  Left to the compiler the select by parity becomes a load of the middle
// 16 bytes, a wait, a branch and two more loads -- one dependent memory round trip more than the data needs.  The empty asm names all eight words, so
// both 16-byte loads are issued unconditionally in front of one wait; the values selected are the same.  c4 1342.0 -> 1336.6 ms (profiles/r11).
__device__ __forceinline__ void tri_uvs(const ShadeDev& sc, int slot, float4& a, float4& b)
{
    const size_t rec = (size_t)(slot >> 1);
    float4 A = sc.uvs[2 * rec], B = sc.uvs[2 * rec + 1];
    asm volatile("" : "+v"(A.x), "+v"(A.y), "+v"(A.z), "+v"(A.w), "+v"(B.x), "+v"(B.y), "+v"(B.z), "+v"(B.w));
    const bool odd = (slot & 1) != 0;
    a = odd ? make_float4(B.z, B.w, B.x, B.y) : A;
    b = odd ? make_float4(A.z, A.w, 0.f, 0.f) : B;
}
// primitive id (row of the caller's index array) of the triangle in leaf slot `slot`
__device__ __forceinline__ uint32_t tri_prim(const SceneDev& sc, int slot) { return __float_as_uint(sc.tris[3 * (size_t)slot].w); }

// ------------------------------------------------------------------------------------------------
// 4-byte texels (texture layouts 3, 4).  The reference's radiance texture is an RGBE file times 2^hdr_exposure
// (tracer_o3d_irt.py:77-81): every texel is three 8-bit integers times ONE power of two.  Such a texel is stored as
// m_r | m_g << 8 | m_b << 16 | E << 24 with value_c = m_c * 2^(E - 127) -- E is the float exponent field of the scale itself, so the decode
// is one shift + mask for the scale, v_cvt_f32_ubyte{0,1,2} and three multiplications by a power of two: the IDENTICAL float32 values
// (m <= 255 times a normal power of two is exact), hence bit-identical bilinear sums.  pack_texel says whether a float triple has this form.
// ------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ bool pack_texel(uint32_t br, uint32_t bg, uint32_t bb, uint32_t& word)
{
    const uint32_t b[3] = {br, bg, bb};
    int t[3]; uint32_t odd[3];
    int k = 1 << 30;
    for (int c = 0; c < 3; c++) {
        if (b[c] == 0u) { t[c] = 1 << 30; odd[c] = 0u; continue; }           // +0.0
        const uint32_t ex = b[c] >> 23;                                       // sign bit set -> ex > 254 below
        if (ex < 1u || ex > 254u) return false;                               // negative (incl. -0.0), subnormal, inf, nan
        uint32_t m = (b[c] & 0x7FFFFFu) | 0x800000u;
        int tz = 0;
        while (!(m & 1u)) { m >>= 1; tz++; }                                  // <= 23 rounds
        odd[c] = m; t[c] = (int)ex - 150 + tz;                                // value = odd * 2^t
        k = t[c] < k ? t[c] : k;
    }
    if (k == (1 << 30)) { word = 0u; return true; }                           // black texel
    const int E = k + 127;
    if (E < 1 || E > 254) return false;
    uint32_t w = (uint32_t)E << 24;
    for (int c = 0; c < 3; c++) {
        if (odd[c] == 0u) continue;
        const int sh = t[c] - k;
        if (sh > 7) return false;
        const uint32_t m = odd[c] << sh;
        if (m > 255u) return false;
        w |= m << (8 * c);
    }
    word = w;
    return true;
}

__device__ __forceinline__ void unpack_texel(uint32_t q, float& r, float& g, float& b)
{
    const float scale = __uint_as_float((q >> 1) & 0x7F800000u);
    r = (float)(q & 0xFFu) * scale; g = (float)((q >> 8) & 0xFFu) * scale; b = (float)((q >> 16) & 0xFFu) * scale;
}

// ------------------------------------------------------------------------------------------------
// hit shader: query_irf post-intersection math (tracer_o3d_irt.py:248-267)
// ------------------------------------------------------------------------------------------------
// LAYOUT >= 0: the texture layout is the caller's compile-time constant (sc.tex_layout is not read) and only its arm is compiled.  SC: SceneDev, or a view
// of it that has uvs, tex, Ht, Wt, tiles_x (ShadeDev: what irt_group_kernel's fixed form re-reads from its kernel arguments per hit)
template <int LAYOUT = -1, typename SC = SceneDev>
__device__ __forceinline__ void shade_hit(const SC& sc, int tri_slot, float bu, float bv, float* rgb)
{
    float u = fminf(fmaxf(bu, 0.f), 1.f), v = fminf(fmaxf(bv, 0.f), 1.f);      // :250 np.clip
    float4 a, b;
    tri_uvs(sc, tri_slot, a, b);
    float w = 1.0f - u - v;
    // :260 (float64 in the reference; float32 here -- <=1e-7 in uv, far below a texel)
    float gx = a.x * w + a.z * u + b.x * v;
    float gy = a.y * w + a.w * u + b.y * v;
    gx = gx * 2.f - 1.f;                  // :262
    gy = -(1.f - gy * 2.f);               // :263
    // F.grid_sample(bilinear, border, align_corners=False) (:265)
    float x = ((gx + 1.f) * (float)sc.Wt - 1.f) * 0.5f, y = ((gy + 1.f) * (float)sc.Ht - 1.f) * 0.5f;
    x = fminf(fmaxf(x, 0.f), (float)(sc.Wt - 1)); y = fminf(fmaxf(y, 0.f), (float)(sc.Ht - 1));
    float x0f = floorf(x), y0f = floorf(y);
    int x0 = (int)x0f, y0 = (int)y0f;
    float wx1 = x - x0f, wx0 = 1.f - wx1, wy1 = y - y0f, wy0 = 1.f - wy1;
    int x1 = min(x0 + 1, sc.Wt - 1), y1 = min(y0 + 1, sc.Ht - 1);
    // out-of-range neighbours carry weight exactly 0 after the border clamp, so clamping their index is exact
    float w00 = wx0 * wy0, w10 = (x0 + 1 < sc.Wt) ? wx1 * wy0 : 0.f, w01 = (y0 + 1 < sc.Ht) ? wx0 * wy1 : 0.f,
          w11 = (x0 + 1 < sc.Wt && y0 + 1 < sc.Ht) ? wx1 * wy1 : 0.f;
    // Where the four taps live.  The values read are the same in every layout (the retiled copies hold the identical floats), so
    // the result is bit-identical; what changes is how many 128-byte lines a fetch touches: row-major 2 rows 12*Wt bytes apart
    // (2.4 lines on average), layout 2 exactly one line (any 2x2 footprint lies inside the 3x3 tile of (x0/2, y0/2)).
    int layout;
    if constexpr (LAYOUT >= 0) layout = LAYOUT; else layout = sc.tex_layout;
    if (layout >= 3) {
        // one 128-byte line of 4-byte texels holds the whole footprint: two adjacent-dword loads
        const uint32_t* t;
        int pitch;
        if (layout == 3) {
            t = (const uint32_t*)sc.tex + ((size_t)(y0 >> 2) * sc.tiles_x + (x0 >> 2)) * 32 + ((y0 & 3) * 5 + (x0 & 3));
            pitch = 5;
        } else {
            const int tx = (int)__umulhi((uint32_t)x0, 0x24924925u), ty = (int)__umulhi((uint32_t)y0, 0x55555556u);      // x0 / 7, y0 / 3 (exact below 2^17; the host checks the size)
            t = (const uint32_t*)sc.tex + ((size_t)ty * sc.tiles_x + tx) * 32 + ((y0 - 3 * ty) * 8 + (x0 - 7 * tx));
            pitch = 8;
        }
        const uint32_t q00 = t[0], q10 = t[1], q01 = t[pitch], q11 = t[pitch + 1];
        float a[3], b[3], c[3], d[3];
        unpack_texel(q00, a[0], a[1], a[2]); unpack_texel(q10, b[0], b[1], b[2]);
        unpack_texel(q01, c[0], c[1], c[2]); unpack_texel(q11, d[0], d[1], d[2]);
        for (int ch = 0; ch < 3; ch++) {
            float acc = a[ch] * w00;
            acc += b[ch] * w10;
            acc += c[ch] * w01;
            acc += d[ch] * w11;
            rgb[ch] = acc;
        }
        return;
    }
    const float *p00, *p10, *p01, *p11;
    if (layout == 2) {
        const float* t = sc.tex + ((size_t)(y0 >> 1) * sc.tiles_x + (x0 >> 1)) * 32 + ((y0 & 1) * 3 + (x0 & 1)) * 3;
        p00 = t; p10 = t + 3; p01 = t + 9; p11 = t + 12;
    } else if (layout == 1) {
        auto at = [&](int x, int y) { return sc.tex + (((size_t)(y >> 3) * sc.tiles_x + (x >> 3)) * 64 + ((y & 7) * 8 + (x & 7))) * 3; };
        p00 = at(x0, y0); p10 = at(x1, y0); p01 = at(x0, y1); p11 = at(x1, y1);
    } else {
        p00 = sc.tex + ((size_t)y0 * sc.Wt + x0) * 3;
        p10 = sc.tex + ((size_t)y0 * sc.Wt + x1) * 3;
        p01 = sc.tex + ((size_t)y1 * sc.Wt + x0) * 3;
        p11 = sc.tex + ((size_t)y1 * sc.Wt + x1) * 3;
    }
    for (int c = 0; c < 3; c++) {
        float acc = p00[c] * w00;
        acc += p10[c] * w10;
        acc += p01[c] * w01;
        acc += p11[c] * w11;
        rgb[c] = acc;
    }
}

// Watertight triangle test (Woop, Benthin, Wald: "Watertight Ray/Triangle Intersection", JCGT 2013 -- the algorithm class Embree's
// robust mode stands for; Open3D's RaycastingScene is an Embree scene): the triangle's vertices are moved to the ray's origin and
// sheared so that the ray becomes the +z axis; what is left is a 2D point-in-triangle test of the origin.  A vertex's sheared
// coordinates depend on the vertex and the ray only, so every triangle sharing it sees the same numbers, and the three edge
// functions  C.x*B.y - C.y*B.x  are evaluated with EXACT signs: products and difference rounded separately (rounding is monotonic:
// the sign of the rounded difference is right unless it is 0), and an exact-zero result is resolved by the error terms of the two
// products (fma(a, b, -fl(a*b)) is exact).  The set of triangles that accept a ray is therefore exactly the set whose sheared
// (rounded) 2D image contains the origin, edges and vertices included: a closed mesh cannot leak.
// Returns U, V, W (weights of v0, v1, v2 before normalisation) and whether the origin is inside (all signs agree, zeros count as inside).
__device__ __forceinline__ float edge2_exact(float bx, float by, float cx, float cy)
{
    const float p = cx * by, q = cy * bx;
    float r = p - q;
    if (r == 0.f) r = __builtin_fmaf(cx, by, -p) - __builtin_fmaf(cy, bx, -q);
    return r;
}

#pragma clang fp contract(fast)

// ------------------------------------------------------------------------------------------------
// closest-hit traversal, one ray per lane.  Stack: LSTK entries per lane in LDS laid out
// [entry][thread] (conflict-free ds_read/write), deeper entries in a private overflow array.  While the stacks of a wave's lanes stay inside the
// LDS part, a pop that culls reads the top entry whole and then two entries per LDS round trip (pop_lds).
// Returns hit triangle slot (leaf order) or -1; t in units of |dir| (Embree semantics: t > 0).
// ------------------------------------------------------------------------------------------------
struct Hit { float t, u, v; int slot; };

// TEXIR_CHAIN_PROBE (measurement build only, tools/chain_probe.sh; 0 = shipped): the wave reads the shader clock (s_memtime) around every wave-level step of
// trace_core -- per-lane (vector) node step, wave-uniform (scalar-cache) node step, leaf step -- and the kernel around the trace, the hit shader and the whole
// pass; cycles and step counts per kind go to stats[8...] (kernels.hip irt_probe_flush).  Summed over the resident waves these cycles ARE the kernel's duration
// (a wave is always in exactly one of the measured regions or in the scheduler between them), which is what bench.py's `roofline.limits.chain` is built from.
#ifndef TEXIR_CHAIN_PROBE
#define TEXIR_CHAIN_PROBE 0
#endif
// A clock read is not free: s_memtime goes through the scalar memory path and its result is waited for (a first probe build that read it around EVERY step
// ran 3.9x slower than the shipped kernel and measured mostly itself).  The build therefore COUNTS every step (one scalar add) but TIMES only every
// kProbeEvery-th wave-level step of a wave, and times an empty region right after each timed step (`null`): mean(step) - mean(null) is the step's duration
// under the load of seven undisturbed neighbour waves.
#if TEXIR_CHAIN_PROBE
__device__ __forceinline__ uint32_t probe_clock() { return (uint32_t)__builtin_amdgcn_s_memtime(); }
// wave-uniform accumulate (keeps the counter in an SGPR)
__device__ __forceinline__ void probe_add(uint32_t& acc, uint32_t x) { acc = (uint32_t)__builtin_amdgcn_readfirstlane((int)(acc + x)); }
#ifndef TEXIR_PROBE_EVERY
#define TEXIR_PROBE_EVERY 32
#endif
constexpr uint32_t kProbeEvery = TEXIR_PROBE_EVERY;
#endif
// wave_iters[2 + ...]: steps, timed steps, cycles of timed steps -- of per-lane node steps, wave-uniform node steps, leaf steps; then timed empty regions, their cycles
constexpr int kProbeSlots = 11;

// How the wave shares its issue slots between lanes that hold an inner node and lanes that hold a leaf: per step, ballot + population
// count of both kinds of lanes and the body with more lanes waiting runs; node lanes count w-fold (a leaf step -- 1 or 2 watertight triangle
// tests and the culling pop -- costs ~1.5 node steps, and on coherent scenes leaf lanes arrive in bursts that are worth a short wait).
// Every lane performs exactly the same node visits, triangle tests and stack operations in the same order as under any other schedule
// (the schedule only decides WHEN a lane's next step issues), so hits do not depend on it, bit for bit.
//   What it replaced was a "while-while" loop -- node steps until NO lane holds an inner node, then leaf steps until NO lane holds a leaf.
// There one lane on a long run of inner nodes keeps 63 lanes waiting at their leaves: on cluttered scenes the wave executes 2.8x the node
// steps of its average ray (c4_scan: 55 wave-level node steps per pass for 19.7 per ray, of which only 30 are the slowest lane's).
// CPU replay of the kernel's schedule (tools/bvh_sim.cpp): c4_scan 55.3 -> 36.8 (w = 1) / 40.6 (w = 2) wave-level node steps per pass,
// c4 19.5 -> 17.6 / 17.8.  Measured (profiles/r03/ab_tables.txt; Grays/s, while-while = 1): w = 1: c4_scan 1.28, c4 0.98 (the leaf
// batches get smaller: wave-level triangle steps 5.2 -> 7.1); w = 2: c4_scan 1.24, c4 1.00; w = 3: 1.19, 1.00.
// w comes with the scene (SceneDev::sched_weight): kSchedNodeWeight = 2 unless texir_scene_tune has measured that the scene's node steps
// run less than 60 % full (cluttered scenes), then 1.
constexpr int kSchedNodeWeight = 2;
// wave_iters[kWiCulled / kWiOverflow] (STATS; per LANE, unlike the wave-level slots before them): stats[6] and stats[7] of include/texir_hip.h
constexpr int kWiCulled = 2 + kProbeSlots, kWiOverflow = 3 + kProbeSlots, kWiSlots = 4 + kProbeSlots;

// Culling: a stack entry also carries the child's entry distance, and an entry whose distance is not below the closest hit found
// since it was pushed is dropped when it is popped (it cannot contain a closer hit: same result, bit for bit) instead of
// costing a node fetch + a full node step that finds all four children behind the hit.  Entries are 8 bytes (one
// ds_write_b64 / ds_read_b64, conflict-free in the [entry][thread] layout), so a kernel keeps LSTK * 2 KiB of LDS per block.

// trace_core is the traversal; trace_closest (one ray per lane, run to completion), trace_stream (lanes take their NEXT ray while the others
// are still under way: compaction by refill, see there) and trace_occluded (any hit inside a segment, see there) are its three drivers.
// ANY: the any-hit form.  h.t starts at the segment's far end `t_start` instead of +inf -- the box tests, the culling pops and the leaf's t < h.t then
// apply the far bound as they apply a closest hit -- a triangle is accepted beyond `t_near` instead of beyond 0, and a lane that has accepted one empties
// its stack at the end of that leaf: the pop that ends the leaf finds nothing and the lane is finished, nothing is drained.  The accept test is the one
// expression of the closest-hit form: a triangle's t and its inside test do not depend on h.t.
struct NoNext { };
// HAVE_F: the caller guarantees sc.nodes4f (the float node copy) is present, so `agree` does not test the pointer
template <bool STATS, int LSTK, int WIDTH, bool STREAM, bool ANY, typename Next, bool HAVE_F = false>
__device__ __forceinline__ Hit trace_core(const SceneDev& sc, float ox, float oy, float oz, float dx, float dy, float dz,
                                          uint32_t& n_nodes, uint32_t& n_tris, uint32_t* wave_iters, int refill_at, Next&& next, float t_start, float t_near)
{
    static_assert(!(ANY && STREAM), "the any-hit form runs one ray per lane to completion");
    typedef int2 Entry;                  // (child code, the child's entry distance)
    // what the traversal keeps of a ray (set by begin_ray; a streamed lane overwrites them when it takes its next ray)
    float idx, idy, idz, oodx, oody, oodz;
    uint32_t lon;
    // The ray-space shear of the watertight test: kz = dominant axis of the direction, (k1, k2) = the two axes that follow it cyclically;
    // a vertex A (relative to the origin) maps to x' = A[k1] - Sx A[kz], y' = A[k2] - Sy A[kz], z' = Sz A[kz], which sends d to (0, 0, 1).
    // (Woop et al. swap k1 / k2 for d[kz] < 0 to keep the winding: that negates U, V, W and their sum EXACTLY and changes neither the accept test --
    // no two signs differ -- nor t, u, v; it is left out.)  What a ray carries into the leaf steps is (kz, Sx, Sy, Sz): 4 registers instead of the
    // 9 of three general matrix rows.  When the rays of the wave share kz (one ~3-degree direction cell: they do unless the cell straddles a
    // |dx| = |dy|-like plane) the leaf step runs a body specialised for that axis -- 3 sub + 2 fma + 1 mul per vertex, no component selects; the
    // per-lane body selects the components and then evaluates the SAME expressions, so a ray's hit does not depend on its wave's company.
    int kz; float Sx, Sy, Sz;
    auto begin_ray = [&]() __attribute__((always_inline)) {
        const float ooeps = 8.271806e-25f;  // 2^-80
        idx = __builtin_amdgcn_rcpf(fabsf(dx) > ooeps ? dx : copysignf(ooeps, dx));
        idy = __builtin_amdgcn_rcpf(fabsf(dy) > ooeps ? dy : copysignf(ooeps, dy));
        idz = __builtin_amdgcn_rcpf(fabsf(dz) > ooeps ? dz : copysignf(ooeps, dz));
        oodx = ox * idx; oody = oy * idy; oodz = oz * idz;
        // the ray's octant (bit a: negative direction along axis a), wave-uniform when the rays' signs agree: it names the body of a wave-uniform node step
        lon = (idx < 0.f ? 1u : 0u) | (idy < 0.f ? 2u : 0u) | (idz < 0.f ? 4u : 0u);
        const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
        kz = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
        const float dkz = kz == 0 ? dx : (kz == 1 ? dy : dz);
        const float dk1 = kz == 0 ? dy : (kz == 1 ? dz : dx), dk2 = kz == 0 ? dz : (kz == 1 ? dx : dy);
        Sz = __builtin_amdgcn_rcpf(dkz); Sx = dk1 * Sz; Sy = dk2 * Sz;
    };
    if constexpr (!STREAM) begin_ray();
    else { idx = idy = idz = oodx = oody = oodz = 0.f; lon = 0u; kz = 0; Sx = Sy = Sz = 0.f; }
    // what the lanes of the wave agree on (decided per ray batch; a streamed wave decides again after every refill, over the lanes that hold a ray)
    uint32_t son; bool signs_uniform;
    int kz0; bool kz_uniform;
    // (`has`: this lane holds a ray under way -- always, except in a streamed wave)
    auto agree = [&](bool has) __attribute__((always_inline)) {
        if constexpr (STREAM) {
            const unsigned long long m = __ballot(has);
            const int src = m ? __ffsll((long long)m) - 1 : 0;
            son = (uint32_t)__builtin_amdgcn_readlane((int)lon, src);
            signs_uniform = WIDTH == 4 && (HAVE_F || sc.nodes4f != nullptr) && !__any(has && lon != son);
            kz0 = __builtin_amdgcn_readlane(kz, src);
            kz_uniform = !__any(has && kz != kz0);
        } else {
            son = (uint32_t)__builtin_amdgcn_readfirstlane((int)lon);
            signs_uniform = WIDTH == 4 && (HAVE_F || sc.nodes4f != nullptr) && !__any(lon != son);
            kz0 = __builtin_amdgcn_readfirstlane(kz);
            kz_uniform = !__any(kz != kz0);
        }
    };
    agree(true);
    Hit h;
    h.t = t_start; h.u = 0.f; h.v = 0.f; h.slot = -1;
    const float t_accept = ANY ? t_near : 0.f;                 // a triangle is accepted beyond it
    int node = STREAM ? kSentinel : 0;                       // (a streamed lane gets its first ray from `next` like every later one)
    auto first_active = [&]() -> bool { unsigned long long m = __ballot(1); return (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1; };
    // the traversal stack: LSTK entries per lane in LDS ([entry][thread]), deeper ones private.  The stack pointer is kept as
    // the LDS address of the next free entry (push = ds_write + one add, no index scaling in the node step).
    __shared__ Entry lds_all[LSTK * kBlock];
    Entry ovf[kStackCap - LSTK];
    Entry* const base = lds_all + threadIdx.x;
    Entry* const lim = base + LSTK * kBlock;
    Entry* top = base;
    auto make = [](int code, float tn) -> Entry { return make_int2(code, __float_as_int(tn)); };
    // (STATS, per lane: entries dropped by culling; pushes and pops that went through the private overflow array)
    auto count_culled = [&](uint32_t n) __attribute__((always_inline)) { if constexpr (STATS) { if (wave_iters) wave_iters[kWiCulled] += n; } };
    auto count_ovf = [&]() __attribute__((always_inline)) { if constexpr (STATS) { if (wave_iters && top >= lim) wave_iters[kWiOverflow]++; } };
    // LDS part and private overflow are kept in separate, wave-uniformly guarded code paths: the overflow is almost never
    // touched (depth > LSTK), and hipcc must not merge the two address spaces into one flat access
    auto push = [&](int code, float tn) {
        const Entry x = make(code, tn);
        if (top < lim) *top = x;
        if (__any(top >= lim)) { if (top >= lim) ovf[(top - lim) / kBlock] = x; }
        count_ovf();
        top += kBlock;
    };
    auto pop = [&]() -> int {
        for (;;) {
            if (top == base) return kSentinel;
            top -= kBlock;
            Entry v = *(top < lim ? top : lim - kBlock);
            if (__any(top >= lim)) { Entry b = ovf[top >= lim ? (top - lim) / kBlock : 0]; v = top >= lim ? b : v; }
            count_ovf();
            if (__int_as_float(v.y) < h.t) return v.x;
            count_culled(1u);                                  // behind the closest hit, drop it
        }
    };
    // The culling pop with every entry of the lane in LDS (the caller's wave-uniform guard).  Once a ray has found its hit most of its stack is dead, and the
    // whole wave waits while one lane drains it.  The top entry is read whole (code and distance: one round trip for a pop that visits); behind it the
    // entries are examined TWO per round trip: the two entries below `top` lie kBlock * 8 bytes apart (one ds_read2st64_b64), and the upper one is looked at
    // first, as a loop over single entries would -- the same entries are dropped and the same one is visited.  With one entry left the pair is (slot 0,
    // slot 1) and slot 1 -- free space inside the lane's column, never an address below `base` -- is ignored.
    auto pop_lds = [&]() __attribute__((always_inline)) -> int {
        static_assert(LSTK >= 2, "the paired read needs two LDS slots per lane");
        // (the read is issued for every lane, from slot 0 where the stack is empty, instead of inside an exec-mask region of its own; the wave-uniform test
        // repeats the callers' guard -- with it irt_group_kernel keeps its 800 bytes of scratch per lane, without it the register allocator takes 816)
        Entry e0 = Entry();
        if (!__any(top > lim)) e0 = *(top == base ? base : top - kBlock);
        if (top == base) return kSentinel;
        top -= kBlock;
        if (__int_as_float(e0.y) < h.t) return e0.x;
        count_culled(1u);
        int n = kSentinel;
        // (one exit, selects inside: the two loads are issued together and unconditionally -- the empty asm keeps the compiler from splitting them into
        // a distance read, a branch and a code read per entry)
        bool more = top != base;
        while (more) {
            const bool two = top != base + kBlock;
            Entry* const lo = two ? top - 2 * kBlock : base;
            Entry el = lo[0], eu = lo[kBlock];
            asm volatile("" : "+v"(el.x), "+v"(el.y), "+v"(eu.x), "+v"(eu.y));
            const bool au = two & (__int_as_float(eu.y) < h.t), al = __int_as_float(el.y) < h.t;
            count_culled(au ? 0u : (two ? 1u : 0u) + (al ? 0u : 1u));
            top = au ? top - kBlock : lo;
            n = au ? eu.x : (al ? el.x : n);
            more = !(au | al) & (top != base);
        }
        return n;
    };

#if TEXIR_CHAIN_PROBE
    bool probe_scalar_path = false;
    uint32_t pn_nv = 0, pt_nv = 0, pc_nv = 0, pn_ns = 0, pt_ns = 0, pc_ns = 0, pn_lf = 0, pt_lf = 0, pc_lf = 0, pt_null = 0, pc_null = 0, probe_tick = 0;
#endif
    // ---- one node step of the 4-wide tree: four box tests, sort, push the far children, descend into the nearest ----
    auto node_step4 = [&]() __attribute__((always_inline)) {
        float key[4]; int code[4];
        // The box tests on per-lane node words (vector loads of the 64-byte quantised node): the ray's direction signs decide once
        // per node (for all four children at a time: the bytes stay packed) which of the lo/hi planes is the entry and which the exit
        // plane; the cell size is folded into the reciprocal direction, the node origin into the offset.
        auto box4 = [&](uint32_t q0x, uint32_t q0y, uint32_t q0z, uint32_t q0w, uint32_t q1x, uint32_t q1y, uint32_t q1z, uint32_t q1w,
                        uint32_t q2x, uint32_t q2y, uint32_t q2z, uint32_t q2w) __attribute__((always_inline)) {
            const float sx = __uint_as_float(q0w) * idx, sy = __uint_as_float(q2z) * idy, sz = __uint_as_float(q2w) * idz;
            const float bx = __uint_as_float(q0x) * idx - oodx, by = __uint_as_float(q0y) * idy - oody, bz = __uint_as_float(q0z) * idz - oodz;
            const uint32_t nx_ = idx < 0.f ? q1w : q1x, fx_ = idx < 0.f ? q1x : q1w;
            const uint32_t ny_ = idy < 0.f ? q2x : q1y, fy_ = idy < 0.f ? q1y : q2x;
            const uint32_t nz_ = idz < 0.f ? q2y : q1z, fz_ = idz < 0.f ? q1z : q2y;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int sh = 8 * k;
                float nxt = (float)((nx_ >> sh) & 255u) * sx + bx, fxt = (float)((fx_ >> sh) & 255u) * sx + bx;
                float nyt = (float)((ny_ >> sh) & 255u) * sy + by, fyt = (float)((fy_ >> sh) & 255u) * sy + by;
                float nzt = (float)((nz_ >> sh) & 255u) * sz + bz, fzt = (float)((fz_ >> sh) & 255u) * sz + bz;
                float tn = fmaxf(fmaxf(nxt, nyt), fmaxf(nzt, 0.f));
                float tf = fminf(fminf(fxt, fyt), fminf(fzt, h.t));
                // (unused slots: inverted box, and if ever entered they lead to a degenerate dummy triangle -- no test needed here)
                key[k] = tn <= tf ? tn : __builtin_inff();
            }
        };
        // Wave-uniform steps (the rays of a pass leave neighbouring points in nearly the same direction and walk the upper levels
        // together: 45 % of the wave-level node steps on c4): a vector fetch costs the L1 64 lanes x 64 bytes whether or not the lanes
        // agree (tools/tcp_node.hip: 60 clocks per wave fetch from 1 to 16 distinct nodes); the scalar path costs it nothing.  When the
        // wave's rays also share their direction signs (a pass is one ~2.5 degree direction cell: they do unless the cell straddles an
        // axis plane), the step reads the FLOAT planes of the node (GpuNode4F) through the scalar cache: no byte -> float conversion
        // (24 per step), no sign select, no origin / cell-size set-up.
        //   The node is fetched by three loads at fixed offsets from ONE base address: the x and y plane arrays (64 B, s_load_dwordx16), the z plane
        // arrays (32 B, x8) and the child codes (16 B, x4).  Which array of an axis is the near one is the octant's business, and the octant is the
        // wave's (`son`): one body per octant picks its planes at compile time, and the branch to it runs while the loads are in flight.  (Round 2-6
        // form: six 16-byte loads through per-axis near / far offsets plus one for the codes -- each a 64-bit address sum of its own, the offsets
        // parked in VGPR lanes under the kernel's SGPR pressure and read back by v_readlane, all on the step's dependent chain.)
        const int n0 = __builtin_amdgcn_readfirstlane(node);
#if TEXIR_CHAIN_PROBE
        probe_scalar_path = signs_uniform && !__any(node != n0);
#endif
        if (signs_uniform && !__any(node != n0)) {
            typedef float F16 __attribute__((ext_vector_type(16)));
            typedef float F8 __attribute__((ext_vector_type(8)));
            typedef int32_t I4 __attribute__((ext_vector_type(4)));
            const char __attribute__((address_space(4)))* const nb =
                (const char __attribute__((address_space(4)))*)(reinterpret_cast<const char*>(sc.nodes4f) + ((uint32_t)n0 << 7));
            const F16 pxy = *(const F16 __attribute__((address_space(4)))*)nb;           // lo.x, hi.x, lo.y, hi.y
            const F8 pz = *(const F8 __attribute__((address_space(4)))*)(nb + 64u);      // lo.z, hi.z
            const I4 ch = *(const I4 __attribute__((address_space(4)))*)(nb + 96u);
            auto body = [&](auto OCT) __attribute__((always_inline)) {
                constexpr int o = decltype(OCT)::value;
                constexpr int nx = (o & 1) ? 4 : 0, ny = (o & 2) ? 12 : 8, nz = (o & 4) ? 4 : 0;       // near arrays; the far one is the other of the pair (^ 4)
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const float nxt = pxy[nx + k] * idx - oodx, fxt = pxy[(nx ^ 4) + k] * idx - oodx;
                    const float nyt = pxy[ny + k] * idy - oody, fyt = pxy[(ny ^ 4) + k] * idy - oody;
                    const float nzt = pz[nz + k] * idz - oodz, fzt = pz[(nz ^ 4) + k] * idz - oodz;
                    const float tn = fmaxf(fmaxf(nxt, nyt), fmaxf(nzt, 0.f)), tf = fminf(fminf(fxt, fyt), fminf(fzt, h.t));
                    key[k] = tn <= tf ? tn : __builtin_inff();
                }
            };
            // (each case ends in a distinct empty asm statement: without it the compiler merges the eight bodies back into one that indexes the loaded
            // planes by run-time octant -- index moves, spills -- undoing the specialisation)
            switch (son) {
                case 0: body(std::integral_constant<int, 0>{}); asm volatile("; octant 0"); break;
                case 1: body(std::integral_constant<int, 1>{}); asm volatile("; octant 1"); break;
                case 2: body(std::integral_constant<int, 2>{}); asm volatile("; octant 2"); break;
                case 3: body(std::integral_constant<int, 3>{}); asm volatile("; octant 3"); break;
                case 4: body(std::integral_constant<int, 4>{}); asm volatile("; octant 4"); break;
                case 5: body(std::integral_constant<int, 5>{}); asm volatile("; octant 5"); break;
                case 6: body(std::integral_constant<int, 6>{}); asm volatile("; octant 6"); break;
                default: body(std::integral_constant<int, 7>{}); asm volatile("; octant 7"); break;
            }
            code[0] = ch.x; code[1] = ch.y; code[2] = ch.z; code[3] = ch.w;
        } else {
            // (uniform base + 32-bit byte offset: one VALU op of address arithmetic, saddr-form loads)
            const uint4* np = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(sc.nodes4) + ((uint32_t)node << 6));
            const uint4 v0 = np[0], v1 = np[1], v2 = np[2], v3 = np[3];
            box4(v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w);
            code[0] = (int)v3.x; code[1] = (int)v3.y; code[2] = (int)v3.z; code[3] = (int)v3.w;
        }
        if (STATS) { n_nodes++; if (wave_iters && first_active()) wave_iters[0]++; }
        // sort the four (key, code) pairs ascending: 5-comparator network
#define TEXIR_CSWAP(a, b) { bool s_ = key[b] < key[a]; float ka = s_ ? key[b] : key[a], kb = s_ ? key[a] : key[b]; int ca = s_ ? code[b] : code[a], cb = s_ ? code[a] : code[b]; key[a] = ka; key[b] = kb; code[a] = ca; code[b] = cb; }
        TEXIR_CSWAP(0, 1) TEXIR_CSWAP(2, 3) TEXIR_CSWAP(0, 2) TEXIR_CSWAP(1, 3) TEXIR_CSWAP(1, 2)
#undef TEXIR_CSWAP
        const float inf = __builtin_inff();
        if (!__any(top + 3 * kBlock > lim)) {
            // common case (one wave-uniform test per node): the whole update stays inside the LDS part of the stack
            if (key[3] < inf) { *top = make(code[3], key[3]); top += kBlock; }
            if (key[2] < inf) { *top = make(code[2], key[2]); top += kBlock; }
            if (key[1] < inf) { *top = make(code[1], key[1]); top += kBlock; }
            if (key[0] < inf) node = code[0];
            else node = pop_lds();
        } else {
            if (key[3] < inf) push(code[3], key[3]);
            if (key[2] < inf) push(code[2], key[2]);
            if (key[1] < inf) push(code[1], key[1]);
            node = key[0] < inf ? code[0] : pop();
        }
    };

    // ---- one node step of the binary tree (scenes too deep for the wide tree's stack bound, TEXIR_BVH_WIDTH=2) ----
    auto node_step2 = [&]() __attribute__((always_inline)) {
        const float4* np = sc.nodes + 4 * (size_t)node;
        float4 n0 = np[0], n1 = np[1], n2 = np[2];
        int2 ch = *reinterpret_cast<const int2*>(np + 3);
        if (STATS) { n_nodes++; if (wave_iters && first_active()) wave_iters[0]++; }
        float c0lox = n0.x * idx - oodx, c0hix = n0.y * idx - oodx, c0loy = n0.z * idy - oody, c0hiy = n0.w * idy - oody;
        float c0loz = n2.x * idz - oodz, c0hiz = n2.y * idz - oodz;
        float c1lox = n1.x * idx - oodx, c1hix = n1.y * idx - oodx, c1loy = n1.z * idy - oody, c1hiy = n1.w * idy - oody;
        float c1loz = n2.z * idz - oodz, c1hiz = n2.w * idz - oodz;
        float t0n = fmaxf(fmaxf(fminf(c0lox, c0hix), fminf(c0loy, c0hiy)), fmaxf(fminf(c0loz, c0hiz), 0.f));
        float t0f = fminf(fminf(fmaxf(c0lox, c0hix), fmaxf(c0loy, c0hiy)), fminf(fmaxf(c0loz, c0hiz), h.t));
        float t1n = fmaxf(fmaxf(fminf(c1lox, c1hix), fminf(c1loy, c1hiy)), fmaxf(fminf(c1loz, c1hiz), 0.f));
        float t1f = fminf(fminf(fmaxf(c1lox, c1hix), fmaxf(c1loy, c1hiy)), fminf(fmaxf(c1loz, c1hiz), h.t));
        bool h0 = t0n <= t0f, h1 = t1n <= t1f;
        if (h0 && h1) {
            bool swp = t1n < t0n;
            int nearc = swp ? ch.y : ch.x, farc = swp ? ch.x : ch.y;
            push(farc, swp ? t0n : t1n);
            node = nearc;
        } else if (h0) node = ch.x;
        else if (h1) node = ch.y;
        else node = pop();
    };

    // ---- one leaf: test its triangles, then pop (the pop drops what this leaf's hit has just put out of reach) ----
    // KZ = std::integral_constant<int, 0 | 1 | 2>: the wave's common dominant axis; -1: per lane
    auto leaf_body = [&](auto KZ) __attribute__((always_inline)) {
        constexpr int kzc = decltype(KZ)::value;
        const uint32_t code = ~(uint32_t)node;
        // the pop that ends the leaf: the two-per-round-trip form unless some lane's stack reaches into the private overflow part (wave-uniform test)
        auto leaf_pop = [&]() __attribute__((always_inline)) -> int {
            if (!__any(top > lim)) return pop_lds();
            return pop();
        };
        if constexpr (WIDTH == 4) {
            // Quad records (bvh_build.h): three 16-byte words hold the four vertices of two triangles that share the edge (q1, q2): triangle 0 = (q0, q1, q2),
            // triangle 1 = (q3, q2, q1).  Four vertices are sheared instead of six, five edge functions evaluated instead of six -- the shared edge's value
            // for triangle 1 is triangle 0's negated (edge2_exact is antisymmetric bit for bit) -- and each triangle then goes through exactly the
            // arithmetic of the single-triangle test below, in its stored corner order.
            const int first = (int)(code >> 3), cnt = (int)(code & 7u) + 1;
            for (int r = first; r < first + cnt; r++) {
                const float4* qp = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(sc.quads) + (uint32_t)r * 48u);
                const float4 w0 = qp[0], w1 = qp[1], w2 = qp[2];
                if (STATS) { n_tris += 2; if (wave_iters && first_active()) wave_iters[1]++; }
                auto shear = [&](float p0, float p1, float p2, float& X, float& Y, float& Z) __attribute__((always_inline)) {
                    const float q0 = p0 - ox, q1 = p1 - oy, q2 = p2 - oz;
                    float qz, qx, qy;
                    if constexpr (kzc == 0) { qz = q0; qx = q1; qy = q2; }
                    else if constexpr (kzc == 1) { qz = q1; qx = q2; qy = q0; }
                    else if constexpr (kzc == 2) { qz = q2; qx = q0; qy = q1; }
                    else { qz = kz == 0 ? q0 : (kz == 1 ? q1 : q2); qx = kz == 0 ? q1 : (kz == 1 ? q2 : q0); qy = kz == 0 ? q2 : (kz == 1 ? q0 : q1); }
                    X = __builtin_fmaf(-Sx, qz, qx); Y = __builtin_fmaf(-Sy, qz, qy); Z = Sz * qz;
                };
                float X0, Y0, Z0, X1, Y1, Z1, X2, Y2, Z2, X3, Y3, Z3;
                shear(w0.x, w0.y, w0.z, X0, Y0, Z0); shear(w0.w, w1.x, w1.y, X1, Y1, Z1); shear(w1.z, w1.w, w2.x, X2, Y2, Z2); shear(w2.y, w2.z, w2.w, X3, Y3, Z3);
                const float E12 = edge2_exact(X1, Y1, X2, Y2);
                auto accept = [&](float U, float V, float W, float Az, float Bz, float Cz, int slot) __attribute__((always_inline)) {
                    const float mn = fminf(fminf(U, V), W), mxw = fmaxf(fmaxf(U, V), W);
                    const float det = U + V + W;
                    const float inv = __builtin_amdgcn_rcpf(det);
                    const float t = (U * Az + V * Bz + W * Cz) * inv;
                    const float u = V * inv, v = W * inv;
                    const bool ok = !((mn < 0.f) & (mxw > 0.f)) & (det != 0.f) & (t > t_accept) & (t < h.t);
                    if (ok) { h.t = t; h.u = u; h.v = v; h.slot = slot; }
                };
                // triangle 0 = (A, B, C) = (q0, q1, q2): U = e(B, C), V = e(C, A), W = e(A, B)
                accept(E12, edge2_exact(X2, Y2, X0, Y0), edge2_exact(X0, Y0, X1, Y1), Z0, Z1, Z2, 2 * r);
                // triangle 1 = (A, B, C) = (q3, q2, q1): U = e(q2, q1) = -e(q1, q2), V = e(q1, q3), W = e(q3, q2)
                accept(-E12, edge2_exact(X1, Y1, X3, Y3), edge2_exact(X3, Y3, X2, Y2), Z3, Z2, Z1, 2 * r + 1);
            }
            if constexpr (ANY) { if (h.slot >= 0) top = base; }          // occluded: the lane's stack is dropped whole, the pop below returns the sentinel
            node = leaf_pop();
            return;
        }
        // the binary tree's leaves name triangle slots
        const int first = (int)(code >> 3), cnt = (int)(code & 7u) + 1;
        for (int i = first; i < first + cnt; i++) {
            const float4* tp = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(sc.tris) + (uint32_t)i * (uint32_t)(16 * kTriQuads));
            float4 v0 = tp[0], e1 = tp[1], e2 = tp[2];
            if (STATS) { n_tris++; if (wave_iters && first_active()) wave_iters[1]++; }
            // (tp[1], tp[2] hold the vertices v1, v2 here, not edges.)  Shear the three vertices into ray space ...
            auto shear = [&](float p0, float p1, float p2, float& X, float& Y, float& Z) __attribute__((always_inline)) {
                const float q0 = p0 - ox, q1 = p1 - oy, q2 = p2 - oz;
                float qz, qx, qy;
                if constexpr (kzc == 0) { qz = q0; qx = q1; qy = q2; }
                else if constexpr (kzc == 1) { qz = q1; qx = q2; qy = q0; }
                else if constexpr (kzc == 2) { qz = q2; qx = q0; qy = q1; }
                else { qz = kz == 0 ? q0 : (kz == 1 ? q1 : q2); qx = kz == 0 ? q1 : (kz == 1 ? q2 : q0); qy = kz == 0 ? q2 : (kz == 1 ? q0 : q1); }
                X = __builtin_fmaf(-Sx, qz, qx); Y = __builtin_fmaf(-Sy, qz, qy); Z = Sz * qz;
            };
            float Ax, Ay, Az, Bx, By, Bz, Cx, Cy, Cz;
            shear(v0.x, v0.y, v0.z, Ax, Ay, Az); shear(e1.x, e1.y, e1.z, Bx, By, Bz); shear(e2.x, e2.y, e2.z, Cx, Cy, Cz);
            // ... 2D edge functions with exact signs (edge2_exact): U, V, W = unnormalised weights of v0, v1, v2
            const float U = edge2_exact(Bx, By, Cx, Cy), V = edge2_exact(Cx, Cy, Ax, Ay), W = edge2_exact(Ax, Ay, Bx, By);
            const float mn = fminf(fminf(U, V), W), mxw = fmaxf(fmaxf(U, V), W);
            const float det = U + V + W;
            const float inv = __builtin_amdgcn_rcpf(det);
            const float t = (U * Az + V * Bz + W * Cz) * inv;
            const float u = V * inv, v = W * inv;
            // inside <=> no two of the signs differ (zeros -- the origin exactly on an edge or vertex -- count as inside for BOTH neighbours)
            const bool ok = !((mn < 0.f) & (mxw > 0.f)) & (det != 0.f) & (t > t_accept) & (t < h.t);
            if (ok) { h.t = t; h.u = u; h.v = v; h.slot = i; }
        }
        if constexpr (ANY) { if (h.slot >= 0) top = base; }
        node = leaf_pop();
    };
    auto leaf_step = [&]() __attribute__((always_inline)) {
        if (kz_uniform) {
            if (kz0 == 0) leaf_body(std::integral_constant<int, 0>{});
            else if (kz0 == 1) leaf_body(std::integral_constant<int, 1>{});
            else leaf_body(std::integral_constant<int, 2>{});
        } else leaf_body(std::integral_constant<int, -1>{});
    };
    auto node_step = [&]() __attribute__((always_inline)) { if constexpr (WIDTH == 4) node_step4(); else node_step2(); };

    const int sched_w = sc.sched_weight > 0 ? sc.sched_weight : kSchedNodeWeight;      // (wave-uniform: an SGPR)
    if constexpr (STREAM) {
        // Compaction by refill (SURVEY / north_star: "wavefront ballot / prefix-sum ray compaction").  A lane whose ray is finished does not wait for
        // the slowest ray of the batch: once `refill_at` lanes of the wave are idle (ballot + s_bcnt1) they hand their hit to `next`, which shades and
        // accumulates it and gives the lane its NEXT ray (the caller's next direction cell of the same texel) -- the wave stays full while rays of
        // very different lengths pass through it.  next(finished, h, dx, dy, dz) -> true if the lane has a new ray in (dx, dy, dz).
        // Every ray still performs exactly the same node visits and triangle tests, and a lane accumulates its samples in its own cell order: the
        // sums are the same bits as the lock-step kernel's.
        bool holds = false;                                  // this lane holds a finished ray that has not been handed over yet
        bool more = true;                                    // `next` may still have rays for this lane
        for (;;) {
            const bool at_node = (uint32_t)node < (uint32_t)kSentinel;
            const unsigned long long m_node = __ballot(at_node), m_leaf = __ballot(node < 0);
            const bool idle = node == kSentinel && (holds || more);
            const unsigned long long m_idle = __ballot(idle);
            const bool drained = !(m_node | m_leaf);
            if (drained && !m_idle) break;
            if (drained || __popcll(m_idle) >= refill_at) {
                if (idle) {
                    const bool got = next(holds, h, dx, dy, dz);
                    holds = got; more = got;
                    if (got) { begin_ray(); h.t = __builtin_inff(); h.u = 0.f; h.v = 0.f; h.slot = -1; node = 0; top = base; }
                }
                agree(node != kSentinel);                    // (over the lanes that hold a ray now; lanes without one take part in no step)
                continue;
            }
            if (sched_w * __popcll(m_node) >= __popcll(m_leaf)) { if (at_node) node_step(); }
            else if (node < 0) leaf_step();
        }
        return h;
    } else {
    for (;;) {
        const bool at_node = (uint32_t)node < (uint32_t)kSentinel;        // an inner node (>= 0 and not the sentinel)
        const unsigned long long m_node = __ballot(at_node), m_leaf = __ballot(node < 0);
        if (!(m_node | m_leaf)) break;
#if TEXIR_CHAIN_PROBE
        probe_add(probe_tick, 1u);
        const bool timed = (probe_tick & (kProbeEvery - 1u)) == 0u;              // wave-uniform
        uint32_t c0 = 0;
        if (timed) c0 = probe_clock();
        if (sched_w * __popcll(m_node) >= __popcll(m_leaf)) {
            if (at_node) node_step();
            const bool scalar = __ballot(at_node && probe_scalar_path) != 0ull;
            if (scalar) probe_add(pn_ns, 1u); else probe_add(pn_nv, 1u);
            if (timed) {
                const uint32_t dt = probe_clock() - c0;
                if (scalar) { probe_add(pc_ns, dt); probe_add(pt_ns, 1u); } else { probe_add(pc_nv, dt); probe_add(pt_nv, 1u); }
            }
        } else {
            if (node < 0) leaf_step();
            probe_add(pn_lf, 1u);
            if (timed) { probe_add(pc_lf, probe_clock() - c0); probe_add(pt_lf, 1u); }
        }
        if (timed) { const uint32_t n0 = probe_clock(); probe_add(pc_null, probe_clock() - n0); probe_add(pt_null, 1u); }
#else
        if (sched_w * __popcll(m_node) >= __popcll(m_leaf)) { if (at_node) node_step(); }
        else if (node < 0) leaf_step();
#endif
    }
#if TEXIR_CHAIN_PROBE
    if (wave_iters) {
        const uint32_t v[kProbeSlots] = {pn_nv, pt_nv, pc_nv, pn_ns, pt_ns, pc_ns, pn_lf, pt_lf, pc_lf, pt_null, pc_null};
        for (int q = 0; q < kProbeSlots; q++) probe_add(wave_iters[2 + q], v[q]);
    }
#endif
    return h;
    }
}

// closest hit of one ray per lane, run to completion (all lanes of the wave enter and leave together).  One instance per kernel: it
// owns the LDS part of the stacks.  STATS: n_nodes / n_tris count this lane's node fetches and triangle tests; wave_iters[0/1] (if
// given) count, on the first active lane, how many times the wave executed the node-step and the triangle-test bodies.
template <bool STATS, int LSTK = kLdsStack, int WIDTH = 2, bool HAVE_F = false>
__device__ __forceinline__ Hit trace_closest(const SceneDev& sc, float ox, float oy, float oz, float dx, float dy, float dz,
                                             uint32_t& n_nodes, uint32_t& n_tris, uint32_t* wave_iters = nullptr)
{
    return trace_core<STATS, LSTK, WIDTH, false, false, NoNext, HAVE_F>(sc, ox, oy, oz, dx, dy, dz, n_nodes, n_tris, wave_iters, 64, NoNext{}, __builtin_inff(), 0.f);
}

// Streamed form: every ray of the lane, the first one included, comes from `next`, which is called for the idle lanes once `refill_at` of them have
// gathered (or the wave has run dry): next(finished, hit, dx, dy, dz) first consumes the finished ray's hit (finished = false on a lane's first call),
// then returns true with the lane's next direction, or false when the lane has no ray left.
template <bool STATS, int LSTK, int WIDTH, typename Next>
__device__ __forceinline__ void trace_stream(const SceneDev& sc, float ox, float oy, float oz, uint32_t& n_nodes, uint32_t& n_tris, uint32_t* wave_iters,
                                             int refill_at, Next&& next)
{
    (void)trace_core<STATS, LSTK, WIDTH, true, false>(sc, ox, oy, oz, 0.f, 0.f, 0.f, n_nodes, n_tris, wave_iters, refill_at, next, __builtin_inff(), 0.f);
}

// Any hit inside a segment, one ray per lane, run to completion: true iff some triangle passes the leaf test above with t_near < t < t_far, t the float32 t
// that test computes (include/texir_hip.h, texir_trace_occluded, states the rule).  At t_near = 0 this is the answer of `trace_closest(...).t < t_far`, bit for
// bit: a box's computed entry distance is never above the computed t of a triangle inside it (what the culling pops already rely on), so a walk that starts with
// h.t = t_far never culls a box that holds an accepted triangle with t < t_far, and "the closest accepted t is below t_far" says the same as "an accepted
// triangle with t < t_far exists".  A lane stops at the end of the first leaf that accepts a triangle; a segment without one walks the boxes it crosses up
// to t_far, in no particular need of their order.  t_far = NaN or <= t_near accepts nothing; a zero or non-finite direction accepts nothing (as closest hit).
// One instance per kernel, like trace_closest: it owns the LDS part of the stacks.
template <int LSTK, int WIDTH>
__device__ __forceinline__ bool trace_occluded(const SceneDev& sc, float ox, float oy, float oz, float dx, float dy, float dz, float t_near, float t_far)
{
    uint32_t cn = 0, ct = 0;
    return trace_core<false, LSTK, WIDTH, false, true>(sc, ox, oy, oz, dx, dy, dz, cn, ct, nullptr, 64, NoNext{}, t_far, t_near).slot >= 0;
}

__device__ __forceinline__ float wave_sum(float x)
{
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
// (counters: a lane's 32-bit count widened before the sum, so the wave's total cannot wrap)
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long x)
{
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// neither inf nor nan
__device__ __forceinline__ bool finite32(float x) { return x - x == 0.f; }

// The IrT estimator's scale of a summed texel: sum * 2 * np.pi / N (tracer_o3d_irt.py:171); `two` = 1 for the cosine estimator, sum * np.pi / N
// (mat_nvdiffrast.py:256-257).  Three separately rounded operations, in this order, wherever a kernel finishes a texel.
__device__ __forceinline__ float irt_scale(float acc, float two, int N) { return ((acc * two) * 3.141592653589793f) / (float)N; }

// The wave's next ticket of a work counter: lane 0 takes it, every lane gets it (two readfirstlane: the ticket stays wave-uniform, in SGPRs).
// Persistent waves pull chunks from a counter: a chunk is milliseconds of work, so a static round-robin would leave the slowest wave's surplus (the sum of
// its chunk-time deviations) as an idle tail.
__device__ __forceinline__ unsigned long long wave_take(unsigned long long* counter, int lane)
{
    unsigned long long x = 0;
    if (lane == 0) x = atomicAdd(counter, 1ull);
    return ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(x >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
}

// ------------------------------------------------------------------------------------------------
// sample order of the multi-texel IrT kernels (irt_group_kernel, irt_stream_kernel, irt_split_kernel).  A wave traces GRP neighbouring texels at
// once: lane group g (64/GRP lanes) belongs to texel g and all groups take, in the same pass, the lattice cell of THEIR texel that lies nearest to one
// absolute direction cell J (cell_to_pass_m).  The 64 rays of a pass then span 1/(32*GRP) of the hemisphere instead of 1/32 (for N = 2048) and start
// within a few millimetres of each other: their traversals stay together much longer, which is what an issue-bound SIMT traversal needs.
// Every sample of every texel is still traced exactly once (J -> cell is a bijection for a fixed shift).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t sample_index_m(uint32_t cell, uint32_t sub, int log2N, int log2m)
{
    int cells = log2N - log2m;
    int bphi = (cells + 1) >> 1, bth = cells - bphi;
    uint32_t low = cell & ((1u << bphi) - 1u);
    uint32_t th = bth ? (cell >> bphi) : 0u;
    return (th << (log2N - bth)) | (sub << bphi) | low;
}

__device__ __forceinline__ uint32_t cell_to_pass_m(uint32_t J, float sh0, float sh1, int log2N, int log2m)
{
    int cells = log2N - log2m;
    int bphi = (cells + 1) >> 1, bth = cells - bphi;
    uint32_t nphi = 1u << bphi, nth = 1u << bth;
    uint32_t Jphi = J & (nphi - 1u), Jth = J >> bphi;
    uint32_t dphi = (uint32_t)(sh1 * (float)nphi + 0.5f), dth = (uint32_t)(sh0 * (float)nth + 0.5f);
    uint32_t phibin = (Jphi + nphi - (dphi & (nphi - 1u))) & (nphi - 1u);
    uint32_t th = (Jth + nth - (dth & (nth - 1u))) & (nth - 1u);
    uint32_t low = bphi ? (__brev(phibin) >> (32 - bphi)) : 0u;
    return (th << bphi) | low;
}

// The direction cell J of the Lc-th cell a texel's passes walk; bphi / bth = the azimuth / elevation bits of the cell index.  The
// cells are walked azimuth-major (all elevations of one azimuth bin, then the next bin), so a part -- a contiguous range of Lc -- is an azimuthal WEDGE of
// the hemisphere (N = 2048: 2 of the 64 azimuth bins = 5.6 degrees, all 32 elevations) instead of a full ring of one elevation.  The rays of a wedge leave
// a surface patch towards one side of the room: what they touch deep in the tree, their triangles and their radiance-texture lines are shared by the
// chunks of neighbouring wedges.  (irt_stream_kernel's `next` keeps this expression as text: see there.)
__device__ __forceinline__ int wedge_cell(int Lc, int bphi, int bth)
{
    return ((Lc & ((1 << bth) - 1)) << bphi) | (Lc >> bth);
}

}  // namespace texir

// The shadow an inserted emitter's BODY casts on the captured light, per texel (include/texir_hip.h texir_irt_shadow states the rule, the float32 operation
// sequence of the body tests and its rounding bound; this file follows that text operation by operation, contraction off for the body tests).
//
// The samples, rays, n.l and closest hits are those of irt_group_kernel<false, 4, 6> (kernels.hip) -- one texel per lane, one sample per pass, the same
// direction cells in the same order.  Per pass a lane computes its direction and n.l, then meets the K analytic bodies (parallelograms, two-sided here, and
// solid balls).  A lane whose ray meets no body does NOT trace; a pass in which no lane's ray meets a body is skipped by ballot: the pass costs what the
// bodies' solid angle costs, not what irt_generate costs.  A lane that meets one traces the scene (trace_closest<false, kGroupLstk, 4>), and where the
// accepted hit lies behind a body it shades it from the scene's own texture (shade_hit, any layout) and adds L * ndl to every SET of bodies whose mask meets
// the mask of bodies in front of the hit: a set is evaluated from the per-ray mask, so overlapping bodies are a union, not a sum.
//
// The K records are device data (a replayed graph sees moved bodies): once per chunk lane k of the wave loads, validates and prepares record k -- m = a x b
// and the reciprocal basis of a quad, r^2 of a sphere -- and the pass loop reads the prepared words across the wave (v_readlane: scalars, no LDS, no
// memory).  A chunk is 64 consecutive listed texels x one part of the passes, dealt statically as irt_multi_kernel deals them; the partial sums go to
// partial[part][set][i][3] and irt_combine_kernel adds them in part order: a pure function of the inputs, no atomics on results, no work counter.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env.h"
#include "kernels.h"

namespace texir {

constexpr int kShadowMaxBodies = 8, kShadowMaxSets = 8;
constexpr float kFourPiB = 12.5663709640502930f;      // the float32 neighbour of 4 pi (texir_irt_lights' validity rule of a sphere)

// waves per SIMD the kernel is compiled for: 12 prepared words and 8 distances on top of irt_multi_kernel's accumulators
template <int MMAX> struct ShadowWaves { static constexpr int value = MMAX <= 2 ? 5 : 4; };

// ------------------------------------------------------------------------------------------------
// the body tests: every product, sum and quotient is its own rounded float32 operation (the header states the arithmetic and the tests restate it)
// ------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)

// what lane k keeps of record k: p = the quad's corner or the sphere's centre; quad: m = a x b, ua, vb the reciprocal basis (h = u a + v b -> u = h . ua,
// v = h . vb; speclight.hip's expressions, repeated here: sharing them through a header would re-schedule that file's kernels); sphere: m[0] = r * r
struct Body {
    float p[3], m[3], ua[3], vb[3];
    bool quad, sphere;
};

__device__ __forceinline__ Body body_prepare(const float* __restrict__ L /*the lane's record, null: none*/)
{
    Body B = {};
    if (!L) return B;
    const float kind = L[0];
    const float cx = L[1], cy = L[2], cz = L[3], ax = L[4], ay = L[5], az = L[6], bx = L[7], by = L[8], bz = L[9];
    const bool quad = kind == 0.f, sphere = kind == 1.f;
    bool valid = finite32(cx) && finite32(cy) && finite32(cz) && finite32(ax);
    B.p[0] = cx; B.p[1] = cy; B.p[2] = cz;
    if (quad) {
        const float mx = ay * bz - az * by;
        const float my = az * bx - ax * bz;
        const float mz = ax * by - ay * bx;
        valid = valid && finite32(mx) && finite32(my) && finite32(mz) && finite32(ay) && finite32(az) && finite32(bx) && finite32(by) && finite32(bz) &&
                (mx != 0.f || my != 0.f || mz != 0.f);
        const float mm = (mx * mx + my * my) + mz * mz;
        valid = valid && finite32(mm) && mm > 0.f;             // (|m|^2 outside float32: no coordinates, the body never blocks)
        B.m[0] = mx; B.m[1] = my; B.m[2] = mz;
        B.ua[0] = (by * mz - bz * my) / mm; B.ua[1] = (bz * mx - bx * mz) / mm; B.ua[2] = (bx * my - by * mx) / mm;
        B.vb[0] = (my * az - mz * ay) / mm; B.vb[1] = (mz * ax - mx * az) / mm; B.vb[2] = (mx * ay - my * ax) / mm;
    } else if (sphere) {
        const float w = (kFourPiB * ax) * ax;
        valid = valid && ax > 0.f && finite32(w);
        B.m[0] = ax * ax;
    } else valid = false;
    B.quad = valid && quad;
    B.sphere = valid && sphere;
    return B;
}

// the ray (x, d) against a parallelogram, two-sided: t in units of |d|
__device__ __forceinline__ bool quad_meets(float ox, float oy, float oz, float mx, float my, float mz, float uax, float uay, float uaz, float vbx, float vby, float vbz,
                                           float px, float py, float pz, float dx, float dy, float dz, float* tb)
{
    const float den = (mx * dx + my * dy) + mz * dz;
    const float qx = ox - px, qy = oy - py, qz = oz - pz;
    const float num = (mx * qx + my * qy) + mz * qz;
    const float t = num / den;
    const float hx = t * dx - qx, hy = t * dy - qy, hz = t * dz - qz;
    const float u = (hx * uax + hy * uay) + hz * uaz, v = (hx * vbx + hy * vby) + hz * vbz;
    *tb = t;
    return den != 0.f && finite32(t) && t > 0.f && u >= 0.f && u <= 1.f && v >= 0.f && v <= 1.f;
}

// the ray (x, d) against a solid ball: the entry distance, 0 from inside
__device__ __forceinline__ bool ball_meets(float cx, float cy, float cz, float rr, float px, float py, float pz, float dx, float dy, float dz, float* tb)
{
    const float ox = cx - px, oy = cy - py, oz = cz - pz;
    const float b = (ox * dx + oy * dy) + oz * dz;
    const float dd = (dx * dx + dy * dy) + dz * dz;
    const float cc = ((ox * ox + oy * oy) + oz * oz) - rr;
    const float disc = b * b - dd * cc;
    if (!(disc >= 0.f)) return false;
    const float s = b + sqrtf(disc);
    const float far = s / dd;
    if (!(far > 0.f)) return false;
    *tb = cc <= 0.f ? 0.f : cc / s;
    return true;
}

#pragma clang fp contract(fast)

// word `v` of the record lane k prepared, as a wave-uniform value
__device__ __forceinline__ float lane_word(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }

template <int MMAX>
__global__ __launch_bounds__(kBlock, ShadowWaves<MMAX>::value) void irt_shadow_kernel(SceneDev sc, const float* __restrict__ pos, const float* __restrict__ nrm,
                                                                                     const float* __restrict__ shift, const int32_t* __restrict__ ids, int64_t n_ids, int N,
                                                                                     int log2N, int mode, const float* __restrict__ bodies, int K,
                                                                                     const uint32_t* __restrict__ sets, int M, float* __restrict__ partial, int log2parts,
                                                                                     unsigned long long* __restrict__ stats)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (wave-uniform: the chunk loop and the pass loop stay scalar)
    const int64_t gw = (int64_t)blockIdx.x * (kBlock / 64) + wave, nw = (int64_t)gridDim.x * (kBlock / 64);
    uint32_t cn = 0, ct = 0;
    unsigned long long n_traced = 0, n_blocked = 0;
    const int part_cells = N >> log2parts;
    // the cell order of irt_group_kernel with one sample per texel per pass (device_common.h wedge_cell)
    const int cell_bits = log2N < 0 ? 0 : log2N, bphi = (cell_bits + 1) >> 1, bth = cell_bits - bphi;
    const int64_t n_groups = (n_ids + 63) / 64;
    const int64_t n_chunks = n_groups << log2parts;
    // the sets: wave-uniform (scalar) loads; bits at or above K name no body
    const uint32_t body_bits = (1u << K) - 1u;
    uint32_t set_mask[MMAX];
#pragma unroll
    for (int q = 0; q < MMAX; q++) set_mask[q] = q < M ? (sets[q] & body_bits) : 0u;
    for (int64_t chunk = gw; chunk < n_chunks; chunk += nw) {
        const int part = (int)(chunk & ((1ll << log2parts) - 1ll));
        const int64_t k = (chunk >> log2parts) * 64 + lane;
        const bool live = k < n_ids;
        const int64_t t = live ? (ids ? (int64_t)ids[k] : k) : 0;
        const Texel x = load_texel(pos, nrm, shift, t);
        const Frame f = make_frame(x.nx, x.ny, x.nz);
        // the records: device data the host never saw.  Lane j < K reads, validates and prepares record j; everything is decided here.
        const Body B = body_prepare(lane < K ? bodies + 16 * (size_t)lane : nullptr);
        const uint32_t quads = (uint32_t)__ballot(B.quad), balls = (uint32_t)__ballot(B.sphere);
        float acc[MMAX][3];
#pragma unroll
        for (int q = 0; q < MMAX; q++) { acc[q][0] = 0.f; acc[q][1] = 0.f; acc[q][2] = 0.f; }
        uint32_t c_traced = 0, c_blocked = 0;
        if (quads | balls) {                                                // (wave-uniform; no valid body: nothing is met, the sums stay +0)
            for (int Lc = part * part_cells; Lc < (part + 1) * part_cells; Lc++) {
                const int J = log2N >= 0 ? wedge_cell(Lc, bphi, bth) : Lc;
                // (N not a power of two: natural sample order)
                const uint32_t i = log2N < 0 ? (uint32_t)J : sample_index_m(cell_to_pass_m((uint32_t)J, x.sh0, x.sh1, log2N, 0), 0u, log2N, 0);
                float d[3];
                texel_sample_dir(mode, i, (uint32_t)N, x.sh0, x.sh1, f, d);
                const float ndl = fminf(fmaxf(x.nx * d[0] + x.ny * d[1] + x.nz * d[2], 0.f), 1.f);       // :170, RAW normal
                uint32_t met = 0;
                float tb[kShadowMaxBodies];
#pragma unroll
                for (int j = 0; j < kShadowMaxBodies; j++) {
                    tb[j] = 0.f;
                    if ((quads >> j) & 1u) {                                // (wave-uniform)
                        float tq;
                        if (quad_meets(lane_word(B.p[0], j), lane_word(B.p[1], j), lane_word(B.p[2], j), lane_word(B.m[0], j), lane_word(B.m[1], j), lane_word(B.m[2], j),
                                       lane_word(B.ua[0], j), lane_word(B.ua[1], j), lane_word(B.ua[2], j), lane_word(B.vb[0], j), lane_word(B.vb[1], j),
                                       lane_word(B.vb[2], j), x.px, x.py, x.pz, d[0], d[1], d[2], &tq)) {
                            met |= 1u << j;
                            tb[j] = tq;
                        }
                    } else if ((balls >> j) & 1u) {
                        float tq;
                        if (ball_meets(lane_word(B.p[0], j), lane_word(B.p[1], j), lane_word(B.p[2], j), lane_word(B.m[0], j), x.px, x.py, x.pz, d[0], d[1], d[2], &tq)) {
                            met |= 1u << j;
                            tb[j] = tq;
                        }
                    }
                }
                if (!live) met = 0;
                if (!__any(met != 0)) continue;                             // no lane's ray meets a body: the pass is skipped
                if (met) {
                    c_traced++;
                    Hit h = trace_closest<false, kGroupLstk, 4>(sc, x.px, x.py, x.pz, d[0], d[1], d[2], cn, ct, nullptr);
                    if (h.slot >= 0 && h.t > 1e-4f) {          // tracer_o3d_irt.py:248
                        uint32_t front = 0;                     // the bodies the ray enters before the scene's surface
#pragma unroll
                        for (int j = 0; j < kShadowMaxBodies; j++)
                            if (((met >> j) & 1u) && tb[j] < h.t) front |= 1u << j;
                        if (front) {
                            c_blocked++;
                            float L[3];
                            shade_hit(sc, h.slot, h.u, h.v, L);
#pragma unroll
                            for (int q = 0; q < MMAX; q++) {
                                if (set_mask[q] & front) { acc[q][0] += L[0] * ndl; acc[q][1] += L[1] * ndl; acc[q][2] += L[2] * ndl; }
                            }
                        }
                    }
                }
            }
        }
        if (live) {
#pragma unroll
            for (int q = 0; q < MMAX; q++) {
                if (q < M) {
                    float* o = partial + (((int64_t)part * M + q) * n_ids + k) * 3;
                    o[0] = acc[q][0]; o[1] = acc[q][1]; o[2] = acc[q][2];
                }
            }
        }
        n_traced += c_traced; n_blocked += c_blocked;
    }
    if (stats) {
        const unsigned long long a = wave_sum_u64(n_traced), b = wave_sum_u64(n_blocked);
        if (lane == 0) { atomicAdd(stats, a); atomicAdd(stats + 1, b); }
    }
}

// ------------------------------------------------------------------------------------------------
// launcher
// ------------------------------------------------------------------------------------------------

// parts per texel of the 64-texel plan, as irt_plan takes them (launch_util.h irt_log2parts)
static int irt_shadow_log2parts(int N) { return irt_log2parts(N, env().irt_min_part_cells, env().irt_log2parts_cap); }

size_t irt_shadow_workspace_bytes(int64_t n_ids, int N, int M)
{
    if (n_ids <= 0 || N <= 0 || M < 1 || M > kShadowMaxSets) return 0;
    return (sizeof(float) * 3 * (size_t)n_ids * (size_t)M) << irt_shadow_log2parts(N);
}

template <int MMAX>
static void shadow_launch(const SceneDev& sc, const float* pos, const float* nrm, const float* shift, const int32_t* ids, int64_t n_ids, int N, int l2, int mode,
                          const float* bodies, int K, const uint32_t* sets, int M, float* partial, int log2parts, unsigned long long* stats, hipStream_t st)
{
    const int grid = persistent_grid(irt_shadow_kernel<MMAX>, ((n_ids + 63) / 64) << log2parts, kBlock);      // a wave per chunk, at most the resident ones
    hipLaunchKernelGGL((irt_shadow_kernel<MMAX>), dim3(grid), dim3(kBlock), 0, st, sc, pos, nrm, shift, ids, n_ids, N, l2, mode, bodies, K, sets, M, partial, log2parts,
                       stats);
}

hipError_t launch_irt_shadow(const SceneDev& sc, const float* pos, const float* nrm, const float* shift, const int32_t* ids, int64_t n_ids, int64_t Nt, int N, int mode,
                             const float* bodies, int K, const uint32_t* sets, int M, float* out, unsigned long long* stats, float* partial, hipStream_t st)
{
    if (n_ids <= 0) return hipSuccess;
    const bool pow2 = (N & (N - 1)) == 0;
    const int l2 = pow2 ? ilog2_exact(N) : -1;
    const int log2parts = irt_shadow_log2parts(N);
    if (M <= 2) shadow_launch<2>(sc, pos, nrm, shift, ids, n_ids, N, l2, mode, bodies, K, sets, M, partial, log2parts, stats, st);
    else if (M <= 4) shadow_launch<4>(sc, pos, nrm, shift, ids, n_ids, N, l2, mode, bodies, K, sets, M, partial, log2parts, stats, st);
    else shadow_launch<8>(sc, pos, nrm, shift, ids, n_ids, N, l2, mode, bodies, K, sets, M, partial, log2parts, stats, st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_irt_combine(partial, ids, n_ids, Nt, M, 1 << log2parts, N, 2.f, out, st);
}

}  // namespace texir

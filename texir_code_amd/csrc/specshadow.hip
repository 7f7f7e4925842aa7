// The shadow inserted emitters' BODIES and inserted triangle-mesh OBJECTS cast in the SPECULAR term of the captured light, per pixel (include/texir_hip.h
// texir_spec_shadow states the rule; the body tests are texir_irt_shadow's float32 operation sequence, the object-space ray and the box prefilter are
// texir_irt_shadow_mesh's; this file follows those texts operation by operation, contraction off for the body tests, the ray transform and the box test).
//
// The samples, rays, weights and closest hits are those of spec_kernel<false, 4> (kernels.hip), and so is the lane assignment: lpp lanes per pixel, 64 / lpp
// pixels per wave, lane sl of a pixel takes the samples q * lpp + sl in ascending pass q, the xor butterfly over the pixel's lanes, acc / S.  Where every
// accepted sample of a pixel is blocked the sum is spec_kernel's own, addition by addition.
//
// Per pass a lane runs spec_sample, meets the Kb analytic bodies (parallelograms, two-sided here, and solid balls) and the padded boxes of the J instances.
// A lane whose ray meets neither traces nothing; a pass in which no lane meets anything is skipped by ballot.  The others walk ONE traversal instance --
// trace_core<false, kLstk, 4, false, false>, the instantiation trace_closest<false, kLstk, 4> is -- in a wave-uniform loop over {scene, instance 0, ...,
// instance J - 1}: the SceneDev is chosen by a scalar, so the kernel owns one LDS stack and one private overflow array.  The scene comes first: its accepted
// closest hit t_s decides the bodies (t_b < t_s) and is the far bound an instance's walk STARTS with (irtshadowmesh.hip: slot >= 0 is then the blocked bit).
// B = body bits | instance bits << 8; a set is evaluated from the per-ray mask, so overlapping bodies and instances are a union, not a sum.
//
// The records, matrices and sets are device data (a replayed graph sees them moved): once per pixel group lane k prepares record k and lane j loads and
// validates matrix j; the box of instance j is parked in lane j once per kernel; the pass loop reads the words across the wave (v_readlane).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env.h"
#include "kernels.h"
#include "mesh_instance.h"
#include "spec_sample.h"

namespace texir {

constexpr int kSpecShadowMaxBodies = 8;
constexpr float kFourPiSS = 12.5663709640502930f;      // the float32 neighbour of 4 pi (texir_irt_lights' validity rule of a sphere)

// ------------------------------------------------------------------------------------------------
// the body tests: every product, sum and quotient is its own rounded float32 operation (irtshadow.hip's expressions, repeated here: sharing them through
// a header would re-schedule that file's kernels)
// ------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)

// what lane k keeps of record k: p = the quad's corner or the sphere's centre; quad: m = a x b, ua, vb the reciprocal basis; sphere: m[0] = r * r
struct SsBody {
    float p[3], m[3], ua[3], vb[3];
    bool quad, sphere;
};

__device__ __forceinline__ SsBody ss_body_prepare(const float* __restrict__ L /*the lane's record, null: none*/)
{
    SsBody B = {};
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
        const float w = (kFourPiSS * ax) * ax;
        valid = valid && ax > 0.f && finite32(w);
        B.m[0] = ax * ax;
    } else valid = false;
    B.quad = valid && quad;
    B.sphere = valid && sphere;
    return B;
}

// the ray (x, d) against a parallelogram, two-sided: t in units of |d|
__device__ __forceinline__ bool ss_quad_meets(float ox, float oy, float oz, float mx, float my, float mz, float uax, float uay, float uaz, float vbx, float vby, float vbz,
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
__device__ __forceinline__ bool ss_ball_meets(float cx, float cy, float cz, float rr, float px, float py, float pz, float dx, float dy, float dz, float* tb)
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
__device__ __forceinline__ float ss_lane_word(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }

// MMAX: the sets a lane carries accumulators for (3 * MMAX registers), 2 / 4 / 8 as irt_shadow_kernel splits them
template <int MMAX>
__global__ __launch_bounds__(kBlock) void spec_shadow_kernel(SceneDev sc, const float* __restrict__ normal, const float* __restrict__ rough,
                                                             const float* __restrict__ points, const float* __restrict__ cam, const float* __restrict__ shift,
                                                             const int32_t* __restrict__ ids, int64_t n, int64_t P, int S, int lpp, float ceps,
                                                             const float* __restrict__ bodies, int Kb, MeshOccluders occ, const float* __restrict__ world_to_obj, int J,
                                                             const uint32_t* __restrict__ sets, int M, int prefilter, float* __restrict__ out,
                                                             unsigned long long* __restrict__ stats)
{
    // spec_kernel's lane assignment
    const int lane = threadIdx.x & 63;
    const int ppw = 64 / lpp;                              // pixels per wave
    const int sub = lane / lpp, sl = lane % lpp;
    const int64_t gw = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * kBlock) >> 6;
    const float cx = cam[0], cy = cam[1], cz = cam[2];
    const int passes = (S + lpp - 1) / lpp;
    unsigned long long n_traced = 0, n_queries = 0, n_blocked = 0;
    // the sets: wave-uniform (scalar) loads; bit k = body k, bit 8 + j = instance j, everything else names nothing
    const uint32_t named = ((1u << Kb) - 1u) | (((1u << J) - 1u) << 8);
    uint32_t set_mask[MMAX];
#pragma unroll
    for (int q = 0; q < MMAX; q++) set_mask[q] = q < M ? (sets[q] & named) : 0u;
    MeshParked inst;
    mesh_park_boxes(inst, occ, lane);
    for (int64_t base = gw * ppw; base < n; base += nw * ppw) {
        const int64_t k = base + sub;
        int64_t p = k < n ? (ids ? (int64_t)ids[k] : k) : -1;
        if (p >= P) p = -1;                                                 // an id outside [0, P) is not a pixel: nothing is read or written for it
        const bool live = p >= 0;
        float nx = 0, ny = 0, nz = 0, r = 0.1f, ox = 0, oy = 0, oz = 0, vx = 0, vy = 0, vz = 0, sh0 = 0, sh1 = 0;
        if (live) {
            nx = normal[3 * p]; ny = normal[3 * p + 1]; nz = normal[3 * p + 2];
            r = rough[p];
            ox = points[3 * p]; oy = points[3 * p + 1]; oz = points[3 * p + 2];
            sh0 = shift[2 * p]; sh1 = shift[2 * p + 1];
            // F.normalize(cam - p, eps=1e-4)  (mat_nvdiffrast.py:218), spec_kernel's expression
            vx = cx - ox; vy = cy - oy; vz = cz - oz;
            float lv = fmaxf(sqrtf(vx * vx + vy * vy + vz * vz), 1e-4f);
            vx /= lv; vy /= lv; vz /= lv;
        }
        const Frame f = make_frame(nx, ny, nz);
        // the records and the matrices: device data the host never saw.  Lane k < Kb prepares record k, lane j < J loads and validates matrix j.
        const SsBody B = ss_body_prepare(lane < Kb ? bodies + 16 * (size_t)lane : nullptr);
        const uint32_t quads = (uint32_t)__ballot(B.quad), balls = (uint32_t)__ballot(B.sphere);
        mesh_park_matrices(inst, world_to_obj, J, lane);
        float acc[MMAX][3];
#pragma unroll
        for (int q = 0; q < MMAX; q++) { acc[q][0] = 0.f; acc[q][1] = 0.f; acc[q][2] = 0.f; }
        uint32_t c_traced = 0, c_queries = 0, c_blocked = 0;
        if (quads | balls | inst.valid) {                                   // (wave-uniform; no valid body or instance: nothing is met, the sums stay +0)
            for (int q = 0; q < passes; q++) {
                const int i = q * lpp + sl;
                const bool active = live && i < S;
                const float s0 = shift_wrap_clamp(ham0((uint32_t)i, (uint32_t)S), sh0);
                const float s1 = shift_wrap_clamp(ham1((uint32_t)i), sh1);
                const SpecSample ss = spec_sample(f, nx, ny, nz, vx, vy, vz, r, s0, s1, ceps);
                const float w = ss.w.v;
                const float d[3] = {ss.l[0], ss.l[1], ss.l[2]};
                // the bodies the ray meets, with their entry distances
                uint32_t met_b = 0;
                float tb[kSpecShadowMaxBodies];
#pragma unroll
                for (int j = 0; j < kSpecShadowMaxBodies; j++) {
                    tb[j] = 0.f;
                    if ((quads >> j) & 1u) {                                // (wave-uniform)
                        float tq;
                        if (ss_quad_meets(ss_lane_word(B.p[0], j), ss_lane_word(B.p[1], j), ss_lane_word(B.p[2], j), ss_lane_word(B.m[0], j), ss_lane_word(B.m[1], j),
                                          ss_lane_word(B.m[2], j), ss_lane_word(B.ua[0], j), ss_lane_word(B.ua[1], j), ss_lane_word(B.ua[2], j), ss_lane_word(B.vb[0], j),
                                          ss_lane_word(B.vb[1], j), ss_lane_word(B.vb[2], j), ox, oy, oz, d[0], d[1], d[2], &tq)) {
                            met_b |= 1u << j;
                            tb[j] = tq;
                        }
                    } else if ((balls >> j) & 1u) {
                        float tq;
                        if (ss_ball_meets(ss_lane_word(B.p[0], j), ss_lane_word(B.p[1], j), ss_lane_word(B.p[2], j), ss_lane_word(B.m[0], j), ox, oy, oz, d[0], d[1], d[2],
                                          &tq)) {
                            met_b |= 1u << j;
                            tb[j] = tq;
                        }
                    }
                }
                // the instances whose box the object-space ray meets (prefilter off: every valid one)
                uint32_t met_i = 0;
                if (inst.valid) met_i = prefilter ? mesh_boxes_met(inst, ox, oy, oz, d[0], d[1], d[2]) : inst.valid;      // (wave-uniform condition)
                if (!active) { met_b = 0; met_i = 0; }
                if (!__any((met_b | met_i) != 0)) continue;                 // no lane's ray meets a body or a box: the pass is skipped
                // one traversal instance, a wave-uniform loop over {scene, instance 0, ...}: s = 0 the scene's closest hit, s = j + 1 instance j inside (0, t_s)
                Hit hs;
                hs.t = 0.f; hs.u = 0.f; hs.v = 0.f; hs.slot = -1;
                bool accepted = false;
                uint32_t front_b = 0, front_i = 0, ask_i = 0;
#pragma clang loop unroll(disable)
                for (int s = 0; s <= J; s++) {
                    const int j = s > 0 ? s - 1 : 0;                        // (wave-uniform)
                    if (s > 0 && !((inst.valid >> j) & 1u)) continue;
                    const bool need = s == 0 ? (met_b | met_i) != 0 : ((ask_i >> j) & 1u) != 0;
                    if (!__any(need)) continue;
                    SceneDev cur = sc;
                    float o2[3] = {ox, oy, oz}, d2[3] = {d[0], d[1], d[2]}, t_start = __builtin_inff();
                    if (s > 0) {
                        cur.nodes4 = occ.nodes4[j]; cur.nodes4f = occ.nodes4f[j]; cur.quads = occ.quads[j];
                        mesh_ray(inst, j, ox, oy, oz, d[0], d[1], d[2], o2, d2);
                        t_start = hs.t;
                    }
                    if (need) {
                        uint32_t cn = 0, ct = 0;
                        const Hit h = trace_core<false, kLstk, 4, false, false>(cur, o2[0], o2[1], o2[2], d2[0], d2[1], d2[2], cn, ct, nullptr, 64, NoNext{}, t_start, 0.f);
                        if (s == 0) {
                            c_traced++;
                            hs = h;
                            accepted = h.slot >= 0 && h.t > 1e-4f;          // spec_kernel's acceptance test
                            if (accepted) {
                                // the bodies the ray enters before the scene's surface
#pragma unroll
                                for (int b = 0; b < kSpecShadowMaxBodies; b++)
                                    if (((met_b >> b) & 1u) && tb[b] < h.t) front_b |= 1u << b;
                                // the instances still to be asked: all that were met -- unless a body already blocks the sample: then only those that can
                                // still add it to a set the bodies have not added it to (the others change no bit of out and not the blocked count)
                                ask_i = met_i;
                                if (front_b) {
                                    uint32_t open = 0;
#pragma unroll
                                    for (int m = 0; m < MMAX; m++)
                                        if (!(set_mask[m] & front_b)) open |= set_mask[m] >> 8;
                                    ask_i &= open;
                                }
                            }
                        } else {
                            c_queries++;
                            if (h.slot >= 0) front_i |= 1u << j;            // an accepted triangle of the object with 0 < t < t_s
                        }
                    }
                }
                const uint32_t front = front_b | (front_i << 8);
                if (front) {
                    c_blocked++;
                    float L[3];
                    shade_hit(sc, hs.slot, hs.u, hs.v, L);
#pragma unroll
                    for (int m = 0; m < MMAX; m++) {
                        if (set_mask[m] & front) { acc[m][0] += L[0] * w; acc[m][1] += L[1] * w; acc[m][2] += L[2] * w; }
                    }
                }
            }
        }
        // reduce over the lpp lanes of this pixel (spec_kernel's butterfly)
        for (int o = lpp >> 1; o > 0; o >>= 1) {
#pragma unroll
            for (int m = 0; m < MMAX; m++) {
                acc[m][0] += __shfl_xor(acc[m][0], o, 64); acc[m][1] += __shfl_xor(acc[m][1], o, 64); acc[m][2] += __shfl_xor(acc[m][2], o, 64);
            }
        }
        if (live && sl == 0) {
#pragma unroll
            for (int m = 0; m < MMAX; m++) {
                if (m < M) {
                    float* o = out + ((int64_t)m * P + p) * 3;
                    o[0] = acc[m][0] / (float)S; o[1] = acc[m][1] / (float)S; o[2] = acc[m][2] / (float)S;
                }
            }
        }
        n_traced += c_traced; n_queries += c_queries; n_blocked += c_blocked;
    }
    if (stats) {
        const unsigned long long a = wave_sum_u64(n_traced), b = wave_sum_u64(n_queries), c = wave_sum_u64(n_blocked);
        if (lane == 0) { atomicAdd(stats, a); atomicAdd(stats + 1, b); atomicAdd(stats + 2, c); }
    }
}

// ------------------------------------------------------------------------------------------------
// launcher
// ------------------------------------------------------------------------------------------------

// the specular launcher's lanes-per-pixel rule and grid (kernels.hip lanes_per_pixel, spec_grid, restated: that file stays as it is)
static int spec_shadow_lpp(int S)
{
    int lpp = (S <= 64 && (S & (S - 1)) == 0) ? S : 64;
    if (const int v = env().spec_lpp; v >= 1 && v <= lpp) lpp = v;
    return lpp;
}

static int spec_shadow_grid(int64_t pix_per_block, int64_t n)
{
    const int64_t cap = env().spec_grid_cap;
    const int64_t want = (n + pix_per_block - 1) / pix_per_block;
    return (int)(want < 1 ? 1 : (want > cap ? cap : want));
}

hipError_t launch_spec_shadow(const SceneDev& sc, const float* normal, const float* rough, const float* points, const float* cam, const float* shift, const int32_t* ids,
                              int64_t n, int64_t P, int S, float ceps, const float* bodies, int Kb, const MeshOccluders& occ, const float* world_to_obj, int J,
                              const uint32_t* sets, int M, bool prefilter, float* out, unsigned long long* stats, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    const int lpp = spec_shadow_lpp(S);
    const int64_t pix_per_block = (int64_t)(kBlock / 64) * (64 / lpp);
    const dim3 grid(spec_shadow_grid(pix_per_block, n));
#define TEXIR_SPEC_SHADOW(MMAX) hipLaunchKernelGGL((spec_shadow_kernel<MMAX>), grid, dim3(kBlock), 0, st, sc, normal, rough, points, cam, shift, ids, n, P, S, lpp, ceps, \
                                                   bodies, Kb, occ, world_to_obj, J, sets, M, prefilter ? 1 : 0, out, stats)
    if (M <= 2) TEXIR_SPEC_SHADOW(2);
    else if (M <= 4) TEXIR_SPEC_SHADOW(4);
    else TEXIR_SPEC_SHADOW(8);
#undef TEXIR_SPEC_SHADOW
    return hipGetLastError();
}

}  // namespace texir

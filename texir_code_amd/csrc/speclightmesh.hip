// Inserted emitters behind inserted objects: the SPECULAR response to new area lights per pixel with triangle-mesh instances in the way (include/texir_hip.h
// texir_spec_lights_mesh states the rule: texir_spec_lights with one changed step, VISIBILITY).  The light and lobe terms, the order of the accumulator and the
// writes are spec_lights_kernel's (speclight.hip), operation by operation, contraction off: this file restates that body and changes the visibility step alone.
// (One body with the visibility step as a template parameter was tried first: the existing instantiations then no longer compiled to the instruction streams
// they compile to today -- other register allocation and schedule -- so the existing file stays untouched and the body lives twice.)
//
// A work item is (64-pixel group, light), dealt statically.  The light record and the matrices are wave-uniform: once per item lane j loads and validates
// matrix j; the box of instance j is parked in lane j once per kernel (mesh_instance.h).  A technique no lane needs at sample i is skipped by ballot; the
// others ask mesh_segment_blocked: ONE traversal instantiation, trace_occluded<kLstk, 4>, in a wave-uniform loop over {instances whose box some lane's
// segment meets, scene}, the instances first.  R and stats are pure functions of the inputs: one float32 accumulator per (pixel, light), the light sample's
// term before the lobe sample's in ascending i, no atomics on results, no workspace.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "mesh_instance.h"
#include "spec_sample.h"

namespace texir {

// every product, sum and quotient below is its own rounded float32 operation: the header states the arithmetic and the tests restate it
#pragma clang fp contract(off)

constexpr float kCoreSin2M = 2.02655690e-6f;        // 1 - ctmax^2 for ctmax = float32(1) - float32(1e-6) = 1 - 17 * 2^-24, rounded to float32
constexpr float kTwoPiSM = 6.28318548202514648f, kFourPiSM = 12.5663709640502930f, kPiSM = 3.14159274101257324f;      // the float32 neighbours of 2 pi, 4 pi, pi

__device__ __forceinline__ float clamp01m(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// GGX D of the half vector h about the FRAME's normal nh (the density generate_dir samples), in the cross-product form; *c_out = nh . h
__device__ __forceinline__ float ggx_dm(const Frame& f, float hx, float hy, float hz, float a2, float* c_out, float* s2_out = nullptr)
{
    const float c = (f.n[0] * hx + f.n[1] * hy) + f.n[2] * hz;
    const float qx = f.n[1] * hz - f.n[2] * hy, qy = f.n[2] * hx - f.n[0] * hz, qz = f.n[0] * hy - f.n[1] * hx;
    const float s2 = (qx * qx + qy * qy) + qz * qz;
    const float den = a2 * (c * c) + s2;
    *c_out = c;
    if (s2_out) *s2_out = s2;
    return c > 0.f ? a2 / ((kPiSM * den) * den) : 0.f;
}

// VISIBILITY: item() once per work item; add() per technique and sample under a wave-uniform condition (some lane needs the segment; `need`: this lane
// does) counts the lane's ray and adds its term where the segment is visible.
// MeshVisible: the scene and J inserted mesh instances, texir_spec_lights_mesh's question (mesh_instance.h mesh_segment_blocked: one traversal
// instantiation, the instances first)
struct MeshVisible {
    const SceneDev& sc;
    float t_max;
    const MeshOccluders& occ;
    const float* __restrict__ world_to_obj;
    int J, prefilter;
    MeshParked inst;
    __device__ __forceinline__ void item(int lane) { mesh_park_matrices(inst, world_to_obj, J, lane); }
    __device__ __forceinline__ void add(bool need, float px, float py, float pz, float dx, float dy, float dz, float term, float& acc, uint32_t& it_traced,
                                        uint32_t& it_visible)
    {
        const bool blocked = mesh_segment_blocked<kLstk>(sc, occ, inst, J, prefilter, need, px, py, pz, dx, dy, dz, t_max);
        if (need) {
            it_traced++;
            if (!blocked) { it_visible++; acc += term; }
        }
    }
};

__device__ __forceinline__ void spec_lights_mesh_body(MeshVisible& vis, const float* __restrict__ pos, const float* __restrict__ nrm, const float* __restrict__ rough,
                                                 const float* __restrict__ shift, const float* __restrict__ cam, const int32_t* __restrict__ ids, int64_t n, int64_t P,
                                                 const float* __restrict__ lights, int K, int S, float ceps, float* __restrict__ R, unsigned long long* __restrict__ stats)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t gw = (int64_t)blockIdx.x * (kBlock / 64) + wave, nw = (int64_t)gridDim.x * (kBlock / 64);
    const int64_t n_items = ((n + 63) / 64) * K;
    const float camx = cam[0], camy = cam[1], camz = cam[2];
    unsigned long long n_traced = 0, n_visible = 0;
    for (int64_t item = gw; item < n_items; item += nw) {
        const int64_t group = item / K;
        const int k = (int)(item - group * K);
        const int64_t i = group * 64 + lane;
        vis.item(lane);
        int64_t pix = i < n ? (ids ? (int64_t)ids[i] : i) : -1;
        if (pix >= P) pix = -1;                                            // an id outside [0, P) is not a pixel: nothing is read or written for it
        const bool live = pix >= 0;
        Texel x = {};
        float r = 0.1f, vx = 0.f, vy = 0.f, vz = 0.f;
        if (live) {
            x = load_texel(pos, nrm, shift, pix);
            r = rough[pix];
            vx = camx - x.px; vy = camy - x.py; vz = camz - x.pz;
            const float lv = fmaxf(sqrtf((vx * vx + vy * vy) + vz * vz), 1e-4f);
            vx = vx / lv; vy = vy / lv; vz = vz / lv;
        }
        const Frame f = make_frame(x.nx, x.ny, x.nz);
        const float a1 = r * r, a2 = a1 * a1;
        // generate_dir clamps cos(theta_h) to 1 - 1e-6: half vectors closer to the frame's normal than that (the lobe's CORE) are never sampled -- their
        // whole mass lands on the rim.  The lobe technique has no density there: core directions are the light samples' alone, a rim sample counts nothing.
        // The test is on sin^2: |nh x h|^2 < (1 - ctmax^2) |nh|^2 keeps its digits where cos^2 next to 1 has none.
        const float ctmax = 1.0f - 1e-6f;
        const float rim_a2 = (ctmax * ctmax) * a2;
        const float core_s2 = kCoreSin2M * ((f.n[0] * f.n[0] + f.n[1] * f.n[1]) + f.n[2] * f.n[2]);
        const float ndv = clamp01m((x.nx * vx + x.ny * vy) + x.nz * vz);
        const float r1 = r + 1.f, kk = (r1 * r1) * 0.125f, omk = 1.f - kk;
        const float g1v = ndv / fmaxf(omk * ndv + kk, ceps);
        // the record: wave-uniform, scalar loads.  Device data the host never saw: everything is decided here, as irt_lights_kernel decides it.
        const float* L = lights + 16 * (size_t)k;
        const float kind = L[0];
        const float cx = L[1], cy = L[2], cz = L[3], ax = L[4], ay = L[5], az = L[6], bx = L[7], by = L[8], bz = L[9];
        const bool quad = kind == 0.f, sphere = kind == 1.f;
        float mx = 0.f, my = 0.f, mz = 0.f, w = 1.f;
        float uax = 0.f, uay = 0.f, uaz = 0.f, vbx = 0.f, vby = 0.f, vbz = 0.f;       // the quad's reciprocal basis: q = u a + v b -> u = q . ua, v = q . vb
        bool valid = finite32(cx) && finite32(cy) && finite32(cz) && finite32(ax);
        if (quad) {
            mx = ay * bz - az * by;
            my = az * bx - ax * bz;
            mz = ax * by - ay * bx;
            valid = valid && finite32(mx) && finite32(my) && finite32(mz) && finite32(ay) && finite32(az) && finite32(bx) && finite32(by) &&
                    finite32(bz) && (mx != 0.f || my != 0.f || mz != 0.f);
            const float mm = (mx * mx + my * my) + mz * mz;
            uax = (by * mz - bz * my) / mm; uay = (bz * mx - bx * mz) / mm; uaz = (bx * my - by * mx) / mm;
            vbx = (my * az - mz * ay) / mm; vby = (mz * ax - mx * az) / mm; vbz = (mx * ay - my * ax) / mm;
        } else if (sphere) {
            w = (kFourPiSM * ax) * ax;
            valid = valid && ax > 0.f && finite32(w);
        } else valid = false;
        const float ex = cx - x.px, ey = cy - x.py, ez = cz - x.pz;              // the record's point seen from x
        const float rr2 = ax * ax;

        float acc = 0.f;
        uint32_t it_traced = 0, it_visible = 0;
        if (valid) {                                                        // (wave-uniform)
            for (int s = 0; s < S; s++) {
                const float s0 = shift_wrap_clamp(ham0((uint32_t)s, (uint32_t)S), x.sh0);
                const float s1 = shift_wrap_clamp(ham1((uint32_t)s), x.sh1);
                // ---- the light sample: y, m, d, dd, nd, md as irt_lights_kernel has them
                {
                    float yx, yy, yz;
                    if (quad) {
                        yx = (cx + s0 * ax) + s1 * bx;
                        yy = (cy + s0 * ay) + s1 * by;
                        yz = (cz + s0 * az) + s1 * bz;
                    } else {
                        const float z = 1.f - 2.f * s0;
                        const float q = sqrtf(fmaxf(0.f, 1.f - z * z));
                        const float phi = kTwoPiSM * s1;
                        mx = q * cosf(phi); my = q * sinf(phi); mz = z;
                        yx = cx + ax * mx; yy = cy + ax * my; yz = cz + ax * mz;
                    }
                    const float dx = yx - x.px, dy = yy - x.py, dz = yz - x.pz;
                    const float dd = (dx * dx + dy * dy) + dz * dz;
                    const float nd = (x.nx * dx + x.ny * dy) + x.nz * dz;
                    const float md = -((mx * dx + my * dy) + mz * dz);
                    float term = 0.f;
                    if (live && nd > 0.f && md > 0.f && dd > 0.f) {
                        const float ls = sqrtf(dd);
                        const float lx = dx / ls, ly = dy / ls, lz = dz / ls;
                        float hx = vx + lx, hy = vy + ly, hz = vz + lz;
                        const float hh = (hx * hx + hy * hy) + hz * hz;
                        if (hh > 0.f) {
                            const float hl = sqrtf(hh);
                            hx = hx / hl; hy = hy / hl; hz = hz / hl;
                            const float vdh = clamp01m((hx * vx + hy * vy) + hz * vz);
                            const float ndl = clamp01m((lx * x.nx + ly * x.ny) + lz * x.nz);
                            const float e = ((vdh * -5.55472f) - 6.98316f) * vdh;
                            const float fr = 0.04f + 0.96f * exp2f(e);
                            const float g1l = ndl / fmaxf(ndl * omk + kk, ceps);
                            const float brdf = (fr * (g1l * g1v)) / fmaxf(ndl * (4.f * ndv), ceps);
                            float c, s2;
                            const float D = ggx_dm(f, hx, hy, hz, a2, &c, &s2);
                            const float pL = (dd * ls) / (w * md);
                            const float pB = s2 < core_s2 ? 0.f : (D * c) / fmaxf(4.f * vdh, ceps);
                            term = ((D * brdf) * ndl) / (pL + pB);
                            if (!(finite32(term) && term > 0.f)) term = 0.f;
                        }
                    }
                    const bool need = term > 0.f;
                    if (__any(need)) vis.add(need, x.px, x.py, x.pz, dx, dy, dz, term, acc, it_traced, it_visible);
                }
                // ---- the lobe sample: l and its weight from spec_sample, the light met analytically
                {
                    float term = 0.f, dx = 0.f, dy = 0.f, dz = 0.f;
                    // (the clamp's own condition sqrt((1 - s0) / (1 + (a2 - 1) s0)) > ctmax, cleared of root and quotient: in this form it keeps its digits)
                    const bool rim = (1.0f - s0) * kCoreSin2M > rim_a2 * s0;
                    if (live && !rim) {
                        float hv[4];
                        const SpecSample ss = spec_sample(f, x.nx, x.ny, x.nz, vx, vy, vz, r, s0, s1, ceps, hv);
                        const float wv = ss.w.v, lx = ss.l[0], ly = ss.l[1], lz = ss.l[2];
                        float tL = 0.f, nmx = mx, nmy = my, nmz = mz;
                        bool hit = false;
                        if (quad) {
                            const float ml = (mx * lx + my * ly) + mz * lz;
                            const float me = (mx * ex + my * ey) + mz * ez;
                            tL = me / ml;
                            dx = tL * lx; dy = tL * ly; dz = tL * lz;
                            const float qx = dx - ex, qy = dy - ey, qz = dz - ez;
                            const float u = (qx * uax + qy * uay) + qz * uaz, v = (qx * vbx + qy * vby) + qz * vbz;
                            hit = -ml > 0.f && tL > 0.f && u >= 0.f && u <= 1.f && v >= 0.f && v <= 1.f;
                        } else {
                            const float b = (lx * ex + ly * ey) + lz * ez;
                            const float ll = (lx * lx + ly * ly) + lz * lz;
                            const float cc = ((ex * ex + ey * ey) + ez * ez) - rr2;
                            const float disc = b * b - ll * cc;
                            if (cc > 0.f && b > 0.f && disc >= 0.f) {
                                tL = cc / (b + sqrtf(disc));
                                dx = tL * lx; dy = tL * ly; dz = tL * lz;
                                nmx = (dx - ex) / ax; nmy = (dy - ey) / ax; nmz = (dz - ez) / ax;
                                hit = tL > 0.f;
                            }
                        }
                        if (hit && wv > 0.f) {
                            const float dd = (dx * dx + dy * dy) + dz * dz;
                            const float md = -((nmx * dx + nmy * dy) + nmz * dz);
                            if (md > 0.f && dd > 0.f) {
                                float c;
                                const float D = ggx_dm(f, hv[0], hv[1], hv[2], a2, &c);
                                const float pL = (dd * sqrtf(dd)) / (w * md);
                                const float pB = (D * c) / fmaxf(4.f * hv[3], ceps);
                                term = (wv * pB) / (pL + pB);
                                if (!(finite32(term) && term > 0.f)) term = 0.f;
                            }
                        }
                    }
                    const bool need = term > 0.f;
                    if (__any(need)) vis.add(need, x.px, x.py, x.pz, dx, dy, dz, term, acc, it_traced, it_visible);
                }
            }
        }
        if (live) R[(int64_t)k * P + pix] = acc / (float)S;                  // every listed pixel, zeros included
        n_traced += it_traced; n_visible += it_visible;
    }
    if (stats) {
        const unsigned long long a = wave_sum_u64(n_traced), b = wave_sum_u64(n_visible);
        if (lane == 0) { atomicAdd(stats, a); atomicAdd(stats + 1, b); }
    }
}

// the same body with the inserted objects in the way (texir_spec_lights_mesh; 4-wide trees)
__global__ __launch_bounds__(kBlock) void spec_lights_mesh_kernel(SceneDev sc, const float* __restrict__ pos, const float* __restrict__ nrm, const float* __restrict__ rough,
                                                                  const float* __restrict__ shift, const float* __restrict__ cam, const int32_t* __restrict__ ids, int64_t n,
                                                                  int64_t P, const float* __restrict__ lights, int K, int S, float t_max, float ceps, MeshOccluders occ,
                                                                  const float* __restrict__ world_to_obj, int J, int prefilter, float* __restrict__ R,
                                                                  unsigned long long* __restrict__ stats)
{
    MeshVisible vis{sc, t_max, occ, world_to_obj, J, prefilter, {}};
    mesh_park_boxes(vis.inst, occ, (int)(threadIdx.x & 63));
    spec_lights_mesh_body(vis, pos, nrm, rough, shift, cam, ids, n, P, lights, K, S, ceps, R, stats);
}

#pragma clang fp contract(fast)

hipError_t launch_spec_lights_mesh(const SceneDev& sc, const float* pos, const float* nrm, const float* rough, const float* shift, const float* cam, const int32_t* ids,
                                   int64_t n, int64_t P, const float* lights, int K, int S, float t_max, float ceps, const MeshOccluders& occ, const float* world_to_obj,
                                   int J, bool prefilter, float* R, unsigned long long* stats, hipStream_t st)
{
    if (n <= 0 || K <= 0) return hipSuccess;
    const int64_t items = ((n + 63) / 64) * K;
    const int grid = grid_capped(kBlock / 64, items);
    hipLaunchKernelGGL(spec_lights_mesh_kernel, dim3(grid), dim3(kBlock), 0, st, sc, pos, nrm, rough, shift, cam, ids, n, P, lights, K, S, t_max, ceps, occ, world_to_obj,
                       J, prefilter ? 1 : 0, R, stats);
    return hipGetLastError();
}

}  // namespace texir

// Inserted emitters behind inserted objects: the direct irradiance of new area lights per texel with triangle-mesh instances in the way (include/texir_hip.h
// texir_irt_lights_mesh states the rule: texir_irt_lights with one changed step, VISIBILITY).  Sample point, record validation, geometry term, accumulator
// and writes are irt_lights_kernel's (irtlight.hip), operation by operation, contraction off; the object-space ray and the box prefilter are
// irt_shadow_mesh_kernel's (mesh_instance.h).
//
// A work item stays (64-texel group, light), dealt statically as in irt_lights_kernel.  The light record and the matrices are wave-uniform: once per item lane
// j of the wave loads and validates matrix j (device data: a replayed graph sees a moved object); the box of instance j is parked in lane j once per kernel;
// the sample loop reads both across the wave (v_readlane: scalars, no LDS, no memory).  A sample no lane needs is skipped by ballot.  A lane that needs it maps
// its segment into the object space of each valid instance and meets the instance's padded box; then the wave walks ONE traversal instantiation,
// trace_occluded<kLstk, 4>, in a wave-uniform loop over {instances whose box some lane's ray meets, scene} -- the instances first (mesh_instance.h
// mesh_segment_blocked says why), a lane already blocked takes no further step, a step no lane needs is skipped.  One LDS stack (24 KiB per block).
// F and stats are pure functions of the inputs: one float32 accumulator per (texel, light) in ascending i, no atomics on results, no workspace.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "mesh_instance.h"

namespace texir {

// every product, sum and quotient below is its own rounded float32 operation: the header states the arithmetic and the tests restate it
#pragma clang fp contract(off)

constexpr float kTwoPiM = 6.28318548202514648f, kFourPiM = 12.5663709640502930f;      // the float32 neighbours of 2 pi and 4 pi

__global__ __launch_bounds__(kBlock) void irt_lights_mesh_kernel(SceneDev sc, const float* __restrict__ pos, const float* __restrict__ nrm, const float* __restrict__ shift,
                                                                 const int32_t* __restrict__ ids, int64_t n, int64_t Nt, const float* __restrict__ lights, int K, int S,
                                                                 float t_max, MeshOccluders occ, const float* __restrict__ world_to_obj, int J, int prefilter,
                                                                 float* __restrict__ F, unsigned long long* __restrict__ stats)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (wave-uniform: the item loop and the sample loop stay scalar)
    const int64_t gw = (int64_t)blockIdx.x * (kBlock / 64) + wave, nw = (int64_t)gridDim.x * (kBlock / 64);
    const int64_t n_items = ((n + 63) / 64) * K;
    unsigned long long n_traced = 0, n_visible = 0;
    MeshParked inst;
    mesh_park_boxes(inst, occ, lane);
    for (int64_t item = gw; item < n_items; item += nw) {
        const int64_t group = item / K;
        const int k = (int)(item - group * K);
        const int64_t i = group * 64 + lane;
        int64_t tex = i < n ? (ids ? (int64_t)ids[i] : i) : -1;
        if (tex >= Nt) tex = -1;                                           // an id outside [0, Nt) is not a texel: nothing is read or written for it
        const bool live = tex >= 0;
        Texel x = {};
        if (live) x = load_texel(pos, nrm, shift, tex);
        mesh_park_matrices(inst, world_to_obj, J, lane);
        // the record: wave-uniform, scalar loads.  Device data the host never saw: everything is decided here, as irt_lights_kernel decides it.
        const float* L = lights + 16 * (size_t)k;
        const float kind = L[0];
        const float cx = L[1], cy = L[2], cz = L[3], ax = L[4], ay = L[5], az = L[6], bx = L[7], by = L[8], bz = L[9];
        const bool quad = kind == 0.f, sphere = kind == 1.f;
        float mx = 0.f, my = 0.f, mz = 0.f, w = 1.f;
        bool valid = finite32(cx) && finite32(cy) && finite32(cz) && finite32(ax);
        if (quad) {
            mx = ay * bz - az * by;
            my = az * bx - ax * bz;
            mz = ax * by - ay * bx;
            valid = valid && finite32(mx) && finite32(my) && finite32(mz) && finite32(ay) && finite32(az) && finite32(bx) && finite32(by) &&
                    finite32(bz) && (mx != 0.f || my != 0.f || mz != 0.f);
        } else if (sphere) {
            w = (kFourPiM * ax) * ax;
            valid = valid && ax > 0.f && finite32(w);
        } else valid = false;

        float acc = 0.f;
        uint32_t it_traced = 0, it_visible = 0;
        if (valid) {                                                        // (wave-uniform)
            for (int s = 0; s < S; s++) {
                const float s0 = shift_wrap_clamp(ham0((uint32_t)s, (uint32_t)S), x.sh0);
                const float s1 = shift_wrap_clamp(ham1((uint32_t)s), x.sh1);
                float yx, yy, yz;
                if (quad) {
                    yx = (cx + s0 * ax) + s1 * bx;
                    yy = (cy + s0 * ay) + s1 * by;
                    yz = (cz + s0 * az) + s1 * bz;
                } else {
                    const float z = 1.f - 2.f * s0;
                    const float q = sqrtf(fmaxf(0.f, 1.f - z * z));
                    const float phi = kTwoPiM * s1;
                    mx = q * cosf(phi); my = q * sinf(phi); mz = z;
                    yx = cx + ax * mx; yy = cy + ax * my; yz = cz + ax * mz;
                }
                const float dx = yx - x.px, dy = yy - x.py, dz = yz - x.pz;
                const float dd = (dx * dx + dy * dy) + dz * dz;
                const float nd = (x.nx * dx + x.ny * dy) + x.nz * dz;
                const float md = -((mx * dx + my * dy) + mz * dz);
                float g = 0.f;
                if (live && nd > 0.f && md > 0.f && dd > 0.f) {
                    g = (nd * md) / (dd * dd);
                    if (!finite32(g)) g = 0.f;
                }
                const bool need = g > 0.f;
                if (!__any(need)) continue;                                 // no lane of the wave needs this sample
                const bool blocked = mesh_segment_blocked<kLstk>(sc, occ, inst, J, prefilter, need, x.px, x.py, x.pz, dx, dy, dz, t_max);
                if (need) {
                    it_traced++;
                    if (!blocked) {
                        it_visible++;
                        acc += g;
                    }
                }
            }
        }
        if (live) F[(int64_t)k * Nt + tex] = (acc * w) / (float)S;          // every listed texel, zeros included
        n_traced += it_traced; n_visible += it_visible;
    }
    if (stats) {
        const unsigned long long a = wave_sum_u64(n_traced), b = wave_sum_u64(n_visible);
        if (lane == 0) { atomicAdd(stats, a); atomicAdd(stats + 1, b); }
    }
}

#pragma clang fp contract(fast)

hipError_t launch_irt_lights_mesh(const SceneDev& sc, const float* pos, const float* nrm, const float* shift, const int32_t* ids, int64_t n, int64_t Nt,
                                  const float* lights, int K, int S, float t_max, const MeshOccluders& occ, const float* world_to_obj, int J, bool prefilter, float* F,
                                  unsigned long long* stats, hipStream_t st)
{
    if (n <= 0 || K <= 0) return hipSuccess;
    const int64_t items = ((n + 63) / 64) * K;
    const int grid = grid_capped(kBlock / 64, items);      // a fixed cap: nothing is queried per launch (the result does not depend on the grid)
    hipLaunchKernelGGL(irt_lights_mesh_kernel, dim3(grid), dim3(kBlock), 0, st, sc, pos, nrm, shift, ids, n, Nt, lights, K, S, t_max, occ, world_to_obj, J,
                       prefilter ? 1 : 0, F, stats);
    return hipGetLastError();
}

}  // namespace texir

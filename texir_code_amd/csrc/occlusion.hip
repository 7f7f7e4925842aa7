// Occlusion queries: is anything in the way of a ray inside (t_near, t_far)?  The counterpart of Open3D's RaycastingScene.test_occlusions, the sibling of the
// cast_rays that models/tracer_o3d_irt.py:240-269 calls.  include/texir_hip.h (texir_trace_occluded) states the rule; the traversal is device_common.h's
// trace_occluded: the leaf test of the closest-hit query, started with h.t = t_far and left at the first accepted triangle.
//
// One ray per lane, kBlock lanes per block, a capped grid that strides over the rays as trace_shade_kernel does; kLstk entries of LDS stack per lane.  A ray's
// answer is a pure function of the scene, its origin, its direction and the two bounds: no atomics on results, nothing depends on the launch shape.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace texir {

template <int WIDTH>
__global__ __launch_bounds__(kBlock) void trace_occluded_kernel(SceneDev sc, const float* __restrict__ org, const float* __restrict__ dir, int64_t R, float t_near,
                                                                float t_far, uint8_t* __restrict__ occluded, unsigned long long* __restrict__ stats)
{
    uint32_t n_occluded = 0;
    const bool segment = t_far > t_near;                                   // (wave-uniform; false for a NaN bound too: nothing can be accepted, nothing is traced)
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < R; r += (int64_t)gridDim.x * kBlock) {
        bool occ = false;
        if (segment) {
            const float ox = org[3 * r], oy = org[3 * r + 1], oz = org[3 * r + 2];
            const float dx = dir[3 * r], dy = dir[3 * r + 1], dz = dir[3 * r + 2];
            occ = trace_occluded<kLstk, WIDTH>(sc, ox, oy, oz, dx, dy, dz, t_near, t_far);
        }
        occluded[r] = occ ? 1 : 0;
        n_occluded += occ ? 1u : 0u;
    }
    if (stats) {
        const unsigned long long a = wave_sum_u64(n_occluded);
        if ((threadIdx.x & 63) == 0 && a) atomicAdd(stats, a);
    }
}

hipError_t launch_trace_occluded(const SceneDev& sc, const float* org, const float* dir, int64_t R, float t_near, float t_far, uint8_t* occluded,
                                 unsigned long long* stats, hipStream_t st)
{
    if (R <= 0) return hipSuccess;
    const dim3 grid(grid_capped(kBlock, R));
    if (sc.nodes4) hipLaunchKernelGGL(trace_occluded_kernel<4>, grid, dim3(kBlock), 0, st, sc, org, dir, R, t_near, t_far, occluded, stats);
    else hipLaunchKernelGGL(trace_occluded_kernel<2>, grid, dim3(kBlock), 0, st, sc, org, dir, R, t_near, t_far, occluded, stats);
    return hipGetLastError();
}

}  // namespace texir

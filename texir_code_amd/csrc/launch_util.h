// Helpers the launchers share: grid sizes, the channel-count dispatch, the block ranges of a batched launch and the parts-per-texel rule of the 64-texel IrT plan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/texir_hip.h"

namespace texir {

// blocks for n items at per_block items each: at least 1, at most `cap` (the kernels stride over what is left)
inline int grid_capped(int64_t per_block, int64_t n, int64_t cap = 2048)
{
    const int64_t want = (n + per_block - 1) / per_block;
    return (int)(want < 1 ? 1 : (want > cap ? cap : want));
}

// f(std::integral_constant<int, C>{}) for a texture's run-time channel count C in 1..4 (validated by the caller): the kernels take it at compile time.
// On the host it picks the instantiation to launch, in the batched kernels the body of the block's job.
template <class F>
__host__ __device__ __forceinline__ void with_channels(int C, F&& f)
{
    switch (C) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        default: f(std::integral_constant<int, 4>{}); break;
    }
}

// batched launches (material.hip, adam.hip): a batch structure is { int n; Job j[kMaxBatch]; }, and its jobs own consecutive block ranges [first, next job's first)
constexpr int kMaxBatch = TEXIR_MAX_BATCH;

template <class B>
__device__ __forceinline__ int job_of_block(const B& b, int bid)
{
    int k = 0;
#pragma unroll
    for (int i = 1; i < kMaxBatch; i++) if (i < b.n && bid >= b.j[i].first) k = i;
    return k;
}

// workgroups that are co-resident on the whole chip for a kernel (so a grid-stride loop has no second, partial round)
template <typename K>
inline int resident_grid(K kernel, int block)
{
    int dev = 0, cus = 256, per_cu = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, 0) != hipSuccess || per_cu < 1) per_cu = 4;
    return cus * per_cu;
}

// persistent grid of a kernel whose waves (block / 64 per workgroup) stride over or pull `waves_wanted` pieces of work: exactly the workgroups that are
// co-resident, fewer where the work does not fill them
template <typename K>
inline int persistent_grid(K kernel, int64_t waves_wanted, int block)
{
    const int64_t want = (waves_wanted + (block / 64) - 1) / (block / 64);
    const int grid = resident_grid(kernel, block);
    return want < grid ? (int)want : grid;
}

// log2 of a power of two; 0 for anything else
inline int ilog2_exact(int N) { if (N <= 0 || (N & (N - 1))) return 0; int l = 0; while ((1 << l) < N) l++; return l; }

// Parts per texel of the 64-texel IrT plan, as log2: up to 32, down to min_cells passes per part (N = 2048, min_cells = 8: 32 parts of 64 passes;
// N = 64 -- the reference's own configuration -- 8 parts of 8: with 64-pass parts its 3 053 chunks left two thirds of the 8 192 resident waves without
// work); at most 2^cap where cap >= 0; one part when N is not a power of two.  A function of N and the two switches alone, so results do not depend on
// how a texel list is cut or sharded.
inline int irt_log2parts(int N, int min_cells, int cap = -1)
{
    if (N <= 0 || (N & (N - 1))) return 0;
    int l = 0;
    while (l < 5 && (N >> (l + 1)) >= min_cells) l++;
    if (cap >= 0 && l > cap) l = cap;
    return l;
}

}  // namespace texir

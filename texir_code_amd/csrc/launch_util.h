// Host-side helpers the launchers share: grid sizes and the parts-per-texel rule of the 64-texel IrT plan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace texir {

// blocks for n items at per_block items each: at least 1, at most `cap` (the kernels stride over what is left)
inline int grid_capped(int64_t per_block, int64_t n, int64_t cap = 2048)
{
    const int64_t want = (n + per_block - 1) / per_block;
    return (int)(want < 1 ? 1 : (want > cap ? cap : want));
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

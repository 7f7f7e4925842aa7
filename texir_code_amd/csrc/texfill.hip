// Fill of the texels the atlas bake left unobserved (no reference counterpart: the reference's private capture pipeline delivers a complete atlas).  For every
// listed hole: among the listed sources within max_dist whose normal agrees with the hole's, the one at the smallest squared distance IN WORLD SPACE; an
// exact tie goes to the lowest texel id.  include/texir_hip.h (texir_atlas_fill) states the rule, the float32 operation sequence and its rounding bound; this
// file follows that text operation by operation (contraction off).
//
// THE SEARCH IS EXACT.  The sources are binned into a uniform grid over the caller's box (histogram with integer atomics, a three-launch prefix sum, a
// scatter of (pos, id), (nrm, nn) records in cell order; the order inside a cell varies from run to run and the tie rule makes the result independent of
// it).  A wave owns 64 consecutive holes of the caller's list and tests, in passes, the cells that meet the box [hmin - R, hmax + R] of its holes; the
// source under test is wave-uniform: a tile of 64 records is read with one coalesced vector load per lane and handed round lane by lane (v_readlane), never
// as 64 identical loads.  WHY A LANE MAY STOP: cell_of() is monotone in the coordinate (clamped at the border cells), so a source NOT tested in a pass has,
// on some axis, a coordinate below a = fl(hmin - R) or above b = fl(hmax + R).  With m = the smallest of fl(p - a), fl(b - p) over the axes for the lane's
// own p, that source's computed |e_i| is >= m on that axis (subtraction and rounding are monotone), hence its computed dd >= fl(m m) (products and sums of
// non-negative terms are monotone too): a lane whose best dd is < fl(m m) cannot be beaten, not even tied, by anything untested, and a lane with
// fl(m m) > r2 has nothing in range left.  No margin is involved; the statement holds in float32 as computed.  R doubles for the lanes that are not final;
// once R exceeds the diagonal of the box (or after kMaxPass passes) the pass covers the WHOLE grid, i.e. every source, and the wave is done.  Cells tested
// in an earlier pass are skipped (the boxes are nested).
// Loop bounds: passes <= kMaxPass, rows <= ny nz per pass, records <= n_src per row.  No kernel waits on another workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "kernels.h"

namespace texir {

// every product, sum and difference below is its own rounded float32 operation: the header states the arithmetic and the tests restate it
#pragma clang fp contract(off)

constexpr int kFillBlock = 256;
constexpr int kScanItems = 8;                               // cells per thread of the prefix sum
constexpr int kScanChunk = kFillBlock * kScanItems;         // cells per block: 2048
constexpr int64_t kFillMaxCells = (int64_t)1 << 24;         // 8192 chunks: one block scans their sums
constexpr int kSumsCap = (int)(kFillMaxCells / kScanChunk);
constexpr int kMaxPass = 40;

struct FillGrid {
    float lo[3];
    float inv;               // 1 / cell
    int n[3];
    float r0, r_cap, diag;
};

int64_t atlas_fill_cell_cap(int64_t n_src)
{
    int64_t c = 4 * (n_src < 1 ? 1 : n_src);
    if (c < 4096) c = 4096;
    return c > kFillMaxCells ? kFillMaxCells : c;
}

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

size_t atlas_fill_workspace_bytes(int64_t n_src, int64_t /*n_holes*/)
{
    const size_t ns = (size_t)(n_src < 1 ? 1 : n_src);
    return align256(4 * (size_t)atlas_fill_cell_cap(n_src)) + align256(4 * (size_t)kSumsCap) + 2 * align256(16 * ns);
}

// the grid of a call: cell > 0 is the caller's edge, else T = 32 records per occupied cell on surfaces of the box's own area; either is doubled until the
// grid fits the workspace's cell array.  Steers speed only.
static FillGrid make_grid(const float bounds[6], int64_t n_src, float cell, float max_dist, float* cell_out)
{
    FillGrid g;
    float e[3];
    for (int i = 0; i < 3; i++) {
        g.lo[i] = bounds[i];
        e[i] = bounds[3 + i] - bounds[i];
        if (!(e[i] > 0.f)) e[i] = 0.f;
    }
    const float emax = fmaxf(e[0], fmaxf(e[1], e[2]));
    if (!(cell > 0.f) || !std::isfinite(cell)) {
        const double area = 3.0 * ((double)e[0] * e[1] + (double)e[1] * e[2] + (double)e[0] * e[2]);
        cell = (float)std::sqrt(32.0 * area / (double)(n_src < 1 ? 1 : n_src));
        if (!(cell > 0.f) || !std::isfinite(cell)) cell = emax > 0.f ? emax : 1.f;
    }
    if (cell < emax * 1e-5f) cell = emax * 1e-5f;             // (ceil(e / cell) stays far inside int32)
    const int64_t cap = atlas_fill_cell_cap(n_src);
    for (;;) {
        int64_t tot = 1;
        for (int i = 0; i < 3; i++) {
            const double want = std::ceil((double)e[i] / (double)cell);
            g.n[i] = want < 1.0 ? 1 : (int)want;
            tot *= g.n[i];
        }
        if (tot <= cap) break;
        cell *= 2.f;
    }
    g.inv = 1.f / cell;
    g.r0 = 0.5f * cell;
    g.diag = std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    g.r_cap = max_dist * 1.0009765625f;                      // inf stays inf: the doubling then runs up to the diagonal
    if (cell_out) *cell_out = cell;
    return g;
}

float atlas_fill_cell(const float bounds[6], int64_t n_src, float cell)
{
    float c = 0.f;
    make_grid(bounds, n_src, cell, 1.f, &c);
    return c;
}

// monotone non-decreasing in x, whatever x is (a NaN lands in cell 0): positions outside the box go to the border cells
__device__ __forceinline__ int cell_of(float x, float lo, float inv, int n)
{
    return (int)fminf(fmaxf(floorf((x - lo) * inv), 0.f), (float)(n - 1));
}

__global__ __launch_bounds__(kFillBlock) void fill_zero_kernel(uint32_t* __restrict__ a, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * kFillBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kFillBlock) a[i] = 0u;
}

// SCATTER = false: cells[c] += 1 per valid source.  SCATTER = true: cells holds the exclusive prefix sum; every source takes the next slot of its cell, so
// that afterwards cells[c] is the END of cell c (and the begin of cell c + 1).
template <bool SCATTER>
__global__ __launch_bounds__(kFillBlock) void fill_bin_kernel(FillGrid g, const float* __restrict__ pos, const float* __restrict__ nrm, int64_t Nt,
                                                              const int32_t* __restrict__ ids, int64_t n, uint32_t* __restrict__ cells,
                                                              float4* __restrict__ recP, float4* __restrict__ recN)
{
    for (int64_t i = (int64_t)blockIdx.x * kFillBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kFillBlock) {
        const int64_t s = ids[i];
        if (s < 0 || s >= Nt) continue;                                   // an id outside the atlas is not a texel
        const float x = pos[3 * s], y = pos[3 * s + 1], z = pos[3 * s + 2];
        const int cx = cell_of(x, g.lo[0], g.inv, g.n[0]), cy = cell_of(y, g.lo[1], g.inv, g.n[1]), cz = cell_of(z, g.lo[2], g.inv, g.n[2]);
        const int64_t c = ((int64_t)cz * g.n[1] + cy) * g.n[0] + cx;
        const uint32_t slot = atomicAdd(cells + c, 1u);
        if (SCATTER) {
            const float nx = nrm[3 * s], ny = nrm[3 * s + 1], nz = nrm[3 * s + 2];
            const float nn = (nx * nx + ny * ny) + nz * nz;
            if ((int64_t)slot < n) {                                      // (always: the histogram counted the same sources)
                recP[slot] = make_float4(x, y, z, __int_as_float((int)s));
                recN[slot] = make_float4(nx, ny, nz, nn);
            }
        }
    }
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane)
{
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// exclusive scan over the block's threads; returns the thread's offset, *total = the block's sum (valid in every thread)
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* total)
{
    __shared__ uint32_t wsum[kFillBlock / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t inc = wave_incl_scan(v, lane);
    __syncthreads();                                                      // (the previous call's reads of wsum are over)
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t off = 0, tot = 0;
    for (int i = 0; i < kFillBlock / 64; i++) {
        if (i < w) off += wsum[i];
        tot += wsum[i];
    }
    *total = tot;
    return off + inc - v;
}

// launch 1: the sum of every chunk of kScanChunk cells
__global__ __launch_bounds__(kFillBlock) void fill_chunk_sum_kernel(const uint32_t* __restrict__ cells, int64_t n_cells, uint32_t* __restrict__ sums)
{
    const int64_t base = (int64_t)blockIdx.x * kScanChunk + (int64_t)threadIdx.x * kScanItems;
    uint32_t v = 0;
    for (int k = 0; k < kScanItems; k++)
        if (base + k < n_cells) v += cells[base + k];
    uint32_t tot;
    block_excl_scan(v, &tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// launch 2: one block turns the chunk sums (at most kSumsCap) into their exclusive prefix sum
__global__ __launch_bounds__(kFillBlock) void fill_sums_scan_kernel(uint32_t* __restrict__ sums, int n_chunks)
{
    uint32_t carry = 0;
    for (int base = 0; base < n_chunks; base += kFillBlock) {             // <= kSumsCap / kFillBlock = 32 rounds
        const int i = base + threadIdx.x;
        const uint32_t v = i < n_chunks ? sums[i] : 0u;
        uint32_t tot;
        const uint32_t off = block_excl_scan(v, &tot);
        if (i < n_chunks) sums[i] = carry + off;
        carry += tot;
    }
}

// launch 3: counts -> exclusive prefix sum, in place
__global__ __launch_bounds__(kFillBlock) void fill_chunk_scan_kernel(uint32_t* __restrict__ cells, int64_t n_cells, const uint32_t* __restrict__ sums)
{
    const int64_t base = (int64_t)blockIdx.x * kScanChunk + (int64_t)threadIdx.x * kScanItems;
    uint32_t c[kScanItems], v = 0;
    for (int k = 0; k < kScanItems; k++) {
        c[k] = base + k < n_cells ? cells[base + k] : 0u;
        v += c[k];
    }
    uint32_t tot;
    uint32_t off = sums[blockIdx.x] + block_excl_scan(v, &tot);
    for (int k = 0; k < kScanItems; k++) {
        if (base + k < n_cells) cells[base + k] = off;
        off += c[k];
    }
}

__device__ __forceinline__ float wave_min_f(float x)
{
    for (int o = 32; o > 0; o >>= 1) x = fminf(x, __shfl_xor(x, o, 64));
    return x;
}
__device__ __forceinline__ float wave_max_f(float x)
{
    for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
    return x;
}
__device__ __forceinline__ float lane_f(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }
__device__ __forceinline__ uint32_t lane_u(uint32_t v, int k) { return (uint32_t)__builtin_amdgcn_readlane((int)v, k); }

struct FillLane {
    float px, py, pz, nx, ny, nz, q;        // q = c2 * nn_t
    float best_dd;
    int best_id;
};

// records [b, e) of the sorted arrays against the wave's 64 holes; b, e are wave-uniform
__device__ __forceinline__ void fill_scan_run(const float4* __restrict__ recP, const float4* __restrict__ recN, uint32_t b, uint32_t e, int lane, float r2,
                                              FillLane& L)
{
    for (uint32_t j0 = b; j0 < e; j0 += 64u) {
        const int cnt = (int)(e - j0 < 64u ? e - j0 : 64u);
        float4 P = make_float4(0.f, 0.f, 0.f, 0.f), N = P;
        if (lane < cnt) { P = recP[j0 + lane]; N = recN[j0 + lane]; }
        for (int k = 0; k < cnt; k++) {
            const float sx = lane_f(P.x, k), sy = lane_f(P.y, k), sz = lane_f(P.z, k);
            const int sid = __builtin_amdgcn_readlane(__float_as_int(P.w), k);
            const float mx = lane_f(N.x, k), my = lane_f(N.y, k), mz = lane_f(N.z, k), nn_s = lane_f(N.w, k);
            const float ex = sx - L.px, ey = sy - L.py, ez = sz - L.pz;
            const float dd = (ex * ex + ey * ey) + ez * ez;
            const float ns = (L.nx * mx + L.ny * my) + L.nz * mz;
            const bool ok = dd <= r2 && ns > 0.f && ns * ns >= L.q * nn_s;
            if (ok && (dd < L.best_dd || (dd == L.best_dd && sid < L.best_id))) { L.best_dd = dd; L.best_id = sid; }
        }
    }
}

__global__ __launch_bounds__(kFillBlock) void atlas_fill_kernel(FillGrid g, const float* __restrict__ pos, const float* __restrict__ nrm, int64_t Nt,
                                                                const int32_t* __restrict__ holes, int64_t n_holes, const uint32_t* __restrict__ cells,
                                                                const float4* __restrict__ recP, const float4* __restrict__ recN, float cos_fill, float max_dist,
                                                                int32_t* __restrict__ src, float* __restrict__ dist2, unsigned long long* __restrict__ stats)
{
    const int lane = threadIdx.x & 63;
    const float r2 = max_dist * max_dist, c2 = cos_fill * cos_fill;
    const int nx = g.n[0], ny = g.n[1], nz = g.n[2];
    const int64_t n_cells = (int64_t)nx * ny * nz;
    const uint32_t total = cells[n_cells - 1];                            // the end of the last cell: how many valid sources there are
    uint32_t n_decided = 0, n_filled = 0;
    for (int64_t base = (int64_t)blockIdx.x * kFillBlock; base < n_holes; base += (int64_t)gridDim.x * kFillBlock) {
        const int64_t i = base + threadIdx.x;
        int64_t tex = i < n_holes ? (int64_t)holes[i] : -1;
        if (tex >= Nt) tex = -1;                                           // an id outside the atlas is not a texel: nothing is read or written for it
        const bool live = tex >= 0;
        FillLane L;
        L.px = L.py = L.pz = L.nx = L.ny = L.nz = 0.f;
        if (live) {
            L.px = pos[3 * tex]; L.py = pos[3 * tex + 1]; L.pz = pos[3 * tex + 2];
            L.nx = nrm[3 * tex]; L.ny = nrm[3 * tex + 1]; L.nz = nrm[3 * tex + 2];
        }
        const float nn_t = (L.nx * L.nx + L.ny * L.ny) + L.nz * L.nz;
        L.q = c2 * nn_t;
        L.best_dd = INFINITY;
        L.best_id = 0x7FFFFFFF;
        if (__any(live) && total > 0u) {
            const float hx0 = wave_min_f(live ? L.px : INFINITY), hy0 = wave_min_f(live ? L.py : INFINITY), hz0 = wave_min_f(live ? L.pz : INFINITY);
            const float hx1 = wave_max_f(live ? L.px : -INFINITY), hy1 = wave_max_f(live ? L.py : -INFINITY), hz1 = wave_max_f(live ? L.pz : -INFINITY);
            int px0 = 0, px1 = -1, py0 = 0, py1 = -1, pz0 = 0, pz1 = -1;     // the cell box of the previous pass (empty)
            float R = g.r0;
            for (int pass = 0; pass < kMaxPass; pass++) {
                const bool whole = !(R <= g.diag) || pass == kMaxPass - 1;
                const float ax = hx0 - R, ay = hy0 - R, az = hz0 - R, bx = hx1 + R, by = hy1 + R, bz = hz1 + R;
                const int cx0 = whole ? 0 : cell_of(ax, g.lo[0], g.inv, nx), cx1 = whole ? nx - 1 : cell_of(bx, g.lo[0], g.inv, nx);
                const int cy0 = whole ? 0 : cell_of(ay, g.lo[1], g.inv, ny), cy1 = whole ? ny - 1 : cell_of(by, g.lo[1], g.inv, ny);
                const int cz0 = whole ? 0 : cell_of(az, g.lo[2], g.inv, nz), cz1 = whole ? nz - 1 : cell_of(bz, g.lo[2], g.inv, nz);
                const int wy = cy1 - cy0 + 1, n_rows = wy * (cz1 - cz0 + 1);
                for (int r0 = 0; r0 < n_rows; r0 += 64) {
                    // 64 rows of cells (one (y, z) each, contiguous in x and so in the sorted arrays) at a time: each lane fetches one row's ends
                    const int r = r0 + lane;
                    uint32_t bA = 0, eA = 0, bB = 0, eB = 0;
                    if (r < n_rows) {
                        const int y = cy0 + r % wy, z = cz0 + r / wy;
                        const int64_t row = ((int64_t)z * ny + y) * nx;
                        int a0 = cx0, a1 = cx1, b0 = 0, b1 = -1;
                        if (y >= py0 && y <= py1 && z >= pz0 && z <= pz1) { a1 = px0 - 1; b0 = px1 + 1; b1 = cx1; }      // tested before: [px0, px1]
                        if (a1 >= a0) { bA = row + a0 > 0 ? cells[row + a0 - 1] : 0u; eA = cells[row + a1]; }
                        if (b1 >= b0) { bB = row + b0 > 0 ? cells[row + b0 - 1] : 0u; eB = cells[row + b1]; }
                    }
                    const int nr = n_rows - r0 < 64 ? n_rows - r0 : 64;
                    for (int k = 0; k < nr; k++) {
                        fill_scan_run(recP, recN, lane_u(bA, k), lane_u(eA, k), lane, r2, L);
                        fill_scan_run(recP, recN, lane_u(bB, k), lane_u(eB, k), lane, r2, L);
                    }
                }
                if (whole) break;                                          // every source has been tested
                const float m = fminf(fminf(fminf(L.px - ax, bx - L.px), fminf(L.py - ay, by - L.py)), fminf(L.pz - az, bz - L.pz));
                const float mm = m * m;
                const bool final_ = !live || (m >= 0.f && (L.best_dd < mm || mm > r2));
                if (__all(final_)) break;
                px0 = cx0; px1 = cx1; py0 = cy0; py1 = cy1; pz0 = cz0; pz1 = cz1;
                R = (R < g.r_cap && R + R > g.r_cap) ? g.r_cap : R + R;
            }
        }
        if (live) {
            const bool got = L.best_id != 0x7FFFFFFF;
            src[tex] = got ? L.best_id : -1;
            if (dist2) dist2[tex] = got ? L.best_dd : 0.f;
            n_decided++;
            n_filled += got ? 1u : 0u;
        }
    }
    if (stats) {
        const unsigned long long a = wave_sum_u64(n_decided), b = wave_sum_u64(n_filled);
        if (lane == 0) { atomicAdd(stats, a); atomicAdd(stats + 1, b); }
    }
}

hipError_t launch_atlas_fill(const float* pos, const float* nrm, int64_t Nt, const int32_t* source_ids, int64_t n_src, const int32_t* hole_ids, int64_t n_holes,
                             const float bounds[6], float cos_fill, float max_dist, float cell, int32_t* src, float* dist2, unsigned long long* stats,
                             void* workspace, hipStream_t st)
{
    if (n_holes <= 0) return hipSuccess;
    const FillGrid g = make_grid(bounds, n_src, cell, max_dist, nullptr);
    const int64_t n_cells = (int64_t)g.n[0] * g.n[1] * g.n[2];
    const size_t ns = (size_t)(n_src < 1 ? 1 : n_src);
    char* ws = (char*)workspace;
    uint32_t* cells = (uint32_t*)ws;
    ws += align256(4 * (size_t)atlas_fill_cell_cap(n_src));
    uint32_t* sums = (uint32_t*)ws;
    ws += align256(4 * (size_t)kSumsCap);
    float4* recP = (float4*)ws;
    ws += align256(16 * ns);
    float4* recN = (float4*)ws;
    const int n_chunks = (int)((n_cells + kScanChunk - 1) / kScanChunk);
    hipLaunchKernelGGL(fill_zero_kernel, dim3(grid_capped(kFillBlock, n_cells, 4096)), dim3(kFillBlock), 0, st, cells, n_cells);
    if (n_src > 0) {
        const dim3 bg(grid_capped(kFillBlock, n_src, 8192));
        hipLaunchKernelGGL(fill_bin_kernel<false>, bg, dim3(kFillBlock), 0, st, g, pos, nrm, Nt, source_ids, n_src, cells, recP, recN);
        hipLaunchKernelGGL(fill_chunk_sum_kernel, dim3(n_chunks), dim3(kFillBlock), 0, st, cells, n_cells, sums);
        hipLaunchKernelGGL(fill_sums_scan_kernel, dim3(1), dim3(kFillBlock), 0, st, sums, n_chunks);
        hipLaunchKernelGGL(fill_chunk_scan_kernel, dim3(n_chunks), dim3(kFillBlock), 0, st, cells, n_cells, sums);
        hipLaunchKernelGGL(fill_bin_kernel<true>, bg, dim3(kFillBlock), 0, st, g, pos, nrm, Nt, source_ids, n_src, cells, recP, recN);
    }
    hipLaunchKernelGGL(atlas_fill_kernel, dim3(grid_capped(kFillBlock, n_holes, (int64_t)1 << 20)), dim3(kFillBlock), 0, st, g, pos, nrm, Nt, hole_ids, n_holes, cells,
                       recP, recN, cos_fill, max_dist, src, dist2, stats);
    return hipGetLastError();
}

}  // namespace texir

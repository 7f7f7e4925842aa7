// The shadow an inserted triangle-mesh OBJECT casts on the captured light, per texel (include/texir_hip.h texir_irt_shadow_mesh states the rule, the float32
// operation sequence of the object-space ray, its rounding bound and the argument that the bounding-box prefilter never rejects a ray the traversal accepts;
// this file follows that text operation by operation, contraction off for the ray transform and the box test).
//
// The samples, rays, n.l and closest hits are those of irt_group_kernel<false, 4, 6> (kernels.hip), the chunk loop is irt_shadow_kernel's (irtshadow.hip): one
// texel per lane, one sample per pass, a chunk = 64 consecutive listed texels x one part of the passes, dealt statically; partial[part][set][i][3], added in
// part order by irt_combine_kernel: a pure function of the inputs, no atomics on results, no work counter.
//
// Per pass a lane takes its direction and n.l, maps the ray into the object space of each of the K instances (W x + t, W d: the ray parameter survives an
// affine map, nothing is normalised) and meets the instance's padded bounding box.  A lane that meets no box traces nothing, a pass in which no lane meets
// one is skipped by ballot.  The others walk ONE traversal instance -- trace_core<false, kGroupLstk, 4, false, false>, the instantiation trace_closest is --
// in a wave-uniform loop over {scene, instance 0, ..., instance K - 1}: the SceneDev (the scene's, or the three geometry pointers of the instance's occluder,
// which travel by value in the kernel arguments) is chosen by a scalar, so the kernel owns one LDS stack (20 KiB per block) and one private overflow array,
// as irt_shadow_kernel does.  The scene comes first: its accepted closest hit t_s is the far bound h.t an instance's walk STARTS with, which makes that walk
// the any-hit question "is an accepted triangle inside (0, t_s)?" (a walk that starts at h.t = t_far never culls a box that holds an accepted
// triangle with t < t_far) without a second instantiation of the traversal: slot >= 0 is the bit trace_occluded<kGroupLstk, 4>(obj, o', d', 0, t_s) gives.
//
// The K matrices are device data (a replayed graph sees a moved object): once per chunk lane j of the wave loads and validates matrix j and takes the box of
// instance j from the kernel arguments; the pass loop reads the words across the wave (v_readlane: scalars, no LDS, no memory).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env.h"
#include "kernels.h"
#include "mesh_instance.h"

namespace texir {

// waves per SIMD the kernel is compiled for (128 VGPRs): 18 parked words per lane on top of irt_shadow_kernel's state
template <int MMAX> struct MeshWaves { static constexpr int value = 4; };

// (the object-space ray row_point / row_dir, the box test box_meets and mesh_word: mesh_instance.h)

template <int MMAX>
__global__ __launch_bounds__(kBlock, MeshWaves<MMAX>::value) void irt_shadow_mesh_kernel(SceneDev sc, const float* __restrict__ pos, const float* __restrict__ nrm,
                                                                                        const float* __restrict__ shift, const int32_t* __restrict__ ids, int64_t n_ids, int N,
                                                                                        int log2N, int mode, MeshOccluders occ, const float* __restrict__ world_to_obj, int K,
                                                                                        const uint32_t* __restrict__ sets, int M, int prefilter, float* __restrict__ partial,
                                                                                        int log2parts, unsigned long long* __restrict__ stats)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (wave-uniform: the chunk loop and the pass loop stay scalar)
    const int64_t gw = (int64_t)blockIdx.x * (kBlock / 64) + wave, nw = (int64_t)gridDim.x * (kBlock / 64);
    unsigned long long n_traced = 0, n_queries = 0, n_blocked = 0;
    const int part_cells = N >> log2parts;
    // the cell order of irt_group_kernel with one sample per texel per pass (device_common.h wedge_cell)
    const int cell_bits = log2N < 0 ? 0 : log2N, bphi = (cell_bits + 1) >> 1, bth = cell_bits - bphi;
    const int64_t n_groups = (n_ids + 63) / 64;
    const int64_t n_chunks = n_groups << log2parts;
    // the sets: wave-uniform (scalar) loads; bits at or above K name no instance
    const uint32_t inst_bits = (1u << K) - 1u;
    uint32_t set_mask[MMAX];
#pragma unroll
    for (int q = 0; q < MMAX; q++) set_mask[q] = q < M ? (sets[q] & inst_bits) : 0u;
    // the box of instance `lane` (kernel arguments: scalar loads, one select per word), its largest |coordinate|
    float bx[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < kMeshMaxInst; j++)
#pragma unroll
        for (int w = 0; w < 6; w++) bx[w] = lane == j ? occ.box[j][w] : bx[w];
    const float rb = fmaxf(fmaxf(fmaxf(fabsf(bx[0]), fabsf(bx[1])), fmaxf(fabsf(bx[2]), fabsf(bx[3]))), fmaxf(fabsf(bx[4]), fabsf(bx[5])));
    for (int64_t chunk = gw; chunk < n_chunks; chunk += nw) {
        const int part = (int)(chunk & ((1ll << log2parts) - 1ll));
        const int64_t k = (chunk >> log2parts) * 64 + lane;
        const bool live = k < n_ids;
        const int64_t t = live ? (ids ? (int64_t)ids[k] : k) : 0;
        const Texel x = load_texel(pos, nrm, shift, t);
        const Frame f = make_frame(x.nx, x.ny, x.nz);
        // the matrices: device data the host never saw.  Lane j < K reads matrix j; one with a non-finite entry never blocks.
        float W[12];
        bool fin = lane < K;
#pragma unroll
        for (int w = 0; w < 12; w++) {
            W[w] = lane < K ? world_to_obj[12 * (size_t)lane + w] : 0.f;
            fin = fin && finite32(W[w]);
        }
        const uint32_t valid = (uint32_t)__ballot(fin);
        float acc[MMAX][3];
#pragma unroll
        for (int q = 0; q < MMAX; q++) { acc[q][0] = 0.f; acc[q][1] = 0.f; acc[q][2] = 0.f; }
        uint32_t c_traced = 0, c_queries = 0, c_blocked = 0;
        if (valid) {                                                        // (wave-uniform; no valid instance: nothing is met, the sums stay +0)
            for (int Lc = part * part_cells; Lc < (part + 1) * part_cells; Lc++) {
                const int J = log2N >= 0 ? wedge_cell(Lc, bphi, bth) : Lc;
                // (N not a power of two: natural sample order)
                const uint32_t i = log2N < 0 ? (uint32_t)J : sample_index_m(cell_to_pass_m((uint32_t)J, x.sh0, x.sh1, log2N, 0), 0u, log2N, 0);
                float d[3];
                texel_sample_dir(mode, i, (uint32_t)N, x.sh0, x.sh1, f, d);
                const float ndl = fminf(fmaxf(x.nx * d[0] + x.ny * d[1] + x.nz * d[2], 0.f), 1.f);       // :170, RAW normal
                // the instances whose box the object-space ray meets (prefilter off: every valid one)
                uint32_t met = valid;
                if (prefilter) {
                    met = 0;
#pragma unroll
                    for (int j = 0; j < kMeshMaxInst; j++) {
                        if ((valid >> j) & 1u) {                            // (wave-uniform)
                            const float ox = row_point(mesh_word(W[0], j), mesh_word(W[1], j), mesh_word(W[2], j), mesh_word(W[3], j), x.px, x.py, x.pz);
                            const float oy = row_point(mesh_word(W[4], j), mesh_word(W[5], j), mesh_word(W[6], j), mesh_word(W[7], j), x.px, x.py, x.pz);
                            const float oz = row_point(mesh_word(W[8], j), mesh_word(W[9], j), mesh_word(W[10], j), mesh_word(W[11], j), x.px, x.py, x.pz);
                            const float dx = row_dir(mesh_word(W[0], j), mesh_word(W[1], j), mesh_word(W[2], j), d[0], d[1], d[2]);
                            const float dy = row_dir(mesh_word(W[4], j), mesh_word(W[5], j), mesh_word(W[6], j), d[0], d[1], d[2]);
                            const float dz = row_dir(mesh_word(W[8], j), mesh_word(W[9], j), mesh_word(W[10], j), d[0], d[1], d[2]);
                            if (box_meets(mesh_word(bx[0], j), mesh_word(bx[1], j), mesh_word(bx[2], j), mesh_word(bx[3], j), mesh_word(bx[4], j), mesh_word(bx[5], j),
                                          mesh_word(rb, j), ox, oy, oz, dx, dy, dz))
                                met |= 1u << j;
                        }
                    }
                }
                if (!live) met = 0;
                if (!__any(met != 0)) continue;                             // no lane's ray meets a box: the pass is skipped
                // one traversal instance, a wave-uniform loop over {scene, instance 0, ...}: s = 0 the scene's closest hit, s = j + 1 instance j inside (0, t_s)
                Hit hs;
                hs.t = 0.f; hs.u = 0.f; hs.v = 0.f; hs.slot = -1;
                bool accepted = false;
                uint32_t front = 0;
#pragma clang loop unroll(disable)
                for (int s = 0; s <= K; s++) {
                    const int j = s > 0 ? s - 1 : 0;                        // (wave-uniform)
                    if (s > 0 && !((valid >> j) & 1u)) continue;
                    const bool need = s == 0 ? met != 0 : (accepted && ((met >> j) & 1u));
                    if (!__any(need)) continue;
                    SceneDev cur = sc;
                    float ox = x.px, oy = x.py, oz = x.pz, dx = d[0], dy = d[1], dz = d[2], t_start = __builtin_inff();
                    if (s > 0) {
                        cur.nodes4 = occ.nodes4[j]; cur.nodes4f = occ.nodes4f[j]; cur.quads = occ.quads[j];
                        ox = row_point(mesh_word(W[0], j), mesh_word(W[1], j), mesh_word(W[2], j), mesh_word(W[3], j), x.px, x.py, x.pz);
                        oy = row_point(mesh_word(W[4], j), mesh_word(W[5], j), mesh_word(W[6], j), mesh_word(W[7], j), x.px, x.py, x.pz);
                        oz = row_point(mesh_word(W[8], j), mesh_word(W[9], j), mesh_word(W[10], j), mesh_word(W[11], j), x.px, x.py, x.pz);
                        dx = row_dir(mesh_word(W[0], j), mesh_word(W[1], j), mesh_word(W[2], j), d[0], d[1], d[2]);
                        dy = row_dir(mesh_word(W[4], j), mesh_word(W[5], j), mesh_word(W[6], j), d[0], d[1], d[2]);
                        dz = row_dir(mesh_word(W[8], j), mesh_word(W[9], j), mesh_word(W[10], j), d[0], d[1], d[2]);
                        t_start = hs.t;
                    }
                    if (need) {
                        uint32_t cn = 0, ct = 0;
                        const Hit h = trace_core<false, kGroupLstk, 4, false, false>(cur, ox, oy, oz, dx, dy, dz, cn, ct, nullptr, 64, NoNext{}, t_start, 0.f);
                        if (s == 0) {
                            c_traced++;
                            hs = h;
                            accepted = h.slot >= 0 && h.t > 1e-4f;          // tracer_o3d_irt.py:248
                        } else {
                            c_queries++;
                            if (h.slot >= 0) front |= 1u << j;               // an accepted triangle of the object with 0 < t < t_s
                        }
                    }
                }
                if (front) {
                    c_blocked++;
                    float L[3];
                    shade_hit(sc, hs.slot, hs.u, hs.v, L);
#pragma unroll
                    for (int q = 0; q < MMAX; q++) {
                        if (set_mask[q] & front) { acc[q][0] += L[0] * ndl; acc[q][1] += L[1] * ndl; acc[q][2] += L[2] * ndl; }
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

// parts per texel of the 64-texel plan, as irt_plan takes them (launch_util.h irt_log2parts)
static int irt_shadow_mesh_log2parts(int N) { return irt_log2parts(N, env().irt_min_part_cells, env().irt_log2parts_cap); }

size_t irt_shadow_mesh_workspace_bytes(int64_t n_ids, int N, int M)
{
    if (n_ids <= 0 || N <= 0 || M < 1 || M > kMeshMaxSets) return 0;
    return (sizeof(float) * 3 * (size_t)n_ids * (size_t)M) << irt_shadow_mesh_log2parts(N);
}

template <int MMAX>
static void shadow_mesh_launch(const SceneDev& sc, const float* pos, const float* nrm, const float* shift, const int32_t* ids, int64_t n_ids, int N, int l2, int mode,
                               const MeshOccluders& occ, const float* world_to_obj, int K, const uint32_t* sets, int M, int prefilter, float* partial, int log2parts,
                               unsigned long long* stats, hipStream_t st)
{
    const int grid = persistent_grid(irt_shadow_mesh_kernel<MMAX>, ((n_ids + 63) / 64) << log2parts, kBlock);      // a wave per chunk, at most the resident ones
    hipLaunchKernelGGL((irt_shadow_mesh_kernel<MMAX>), dim3(grid), dim3(kBlock), 0, st, sc, pos, nrm, shift, ids, n_ids, N, l2, mode, occ, world_to_obj, K, sets, M,
                       prefilter, partial, log2parts, stats);
}

hipError_t launch_irt_shadow_mesh(const SceneDev& sc, const float* pos, const float* nrm, const float* shift, const int32_t* ids, int64_t n_ids, int64_t Nt, int N, int mode,
                                  const MeshOccluders& occ, const float* world_to_obj, int K, const uint32_t* sets, int M, bool prefilter, float* out,
                                  unsigned long long* stats, float* partial, hipStream_t st)
{
    if (n_ids <= 0) return hipSuccess;
    const bool pow2 = (N & (N - 1)) == 0;
    const int l2 = pow2 ? ilog2_exact(N) : -1;
    const int log2parts = irt_shadow_mesh_log2parts(N);
    if (M <= 2) shadow_mesh_launch<2>(sc, pos, nrm, shift, ids, n_ids, N, l2, mode, occ, world_to_obj, K, sets, M, prefilter ? 1 : 0, partial, log2parts, stats, st);
    else if (M <= 4) shadow_mesh_launch<4>(sc, pos, nrm, shift, ids, n_ids, N, l2, mode, occ, world_to_obj, K, sets, M, prefilter ? 1 : 0, partial, log2parts, stats, st);
    else shadow_mesh_launch<8>(sc, pos, nrm, shift, ids, n_ids, N, l2, mode, occ, world_to_obj, K, sets, M, prefilter ? 1 : 0, partial, log2parts, stats, st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_irt_combine(partial, ids, n_ids, Nt, M, 1 << log2parts, N, 2.f, out, st);
}

}  // namespace texir

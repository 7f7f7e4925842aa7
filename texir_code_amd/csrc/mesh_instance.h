// Inserted triangle-mesh instances as the tracing kernels see them: the object-space ray, the bounding-box prefilter and the words a wave parks per instance
// (include/texir_hip.h texir_irt_shadow_mesh states the float32 operation sequence of the ray, its rounding bound and the argument that the prefilter never
// rejects a ray the traversal accepts).  Shared by irtshadowmesh.hip (the objects' shadow on captured light), irtlightmesh.hip and speclight.hip (the objects'
// shadow on the inserted emitters' light).  Include it before the including file sets its own contraction mode: it leaves contraction at the compiler's default.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace texir {

constexpr int kMeshMaxInst = 8, kMeshMaxSets = 8;
constexpr float kBoxPad = 3.814697265625e-06f;        // 2^-18 = 64 u: the pad of a box per unit of (largest |box coordinate| + largest |o'_r|), header
constexpr float kBoxTiny = 1e-30f;                    // and an absolute term against underflow
constexpr float kSlabWiden = 4.76837158203125e-07f;   // 2^-21 = 8 u: a slab distance is moved outwards by this share of itself

// ------------------------------------------------------------------------------------------------
// the object-space ray and the box test: every product, sum and quotient is its own rounded float32 operation (the header states the arithmetic)
// ------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)

__device__ __forceinline__ float row_point(float w0, float w1, float w2, float w3, float x, float y, float z) { return ((w0 * x + w1 * y) + w2 * z) + w3; }
__device__ __forceinline__ float row_dir(float w0, float w1, float w2, float x, float y, float z) { return (w0 * x + w1 * y) + w2 * z; }

// one slab of the LINE o + t d against [lo, hi] (already padded): narrows (tn, tf); false: the line never enters the slab.  A distance that is not a
// number (inf - inf after an overflow) narrows nothing: every doubt passes.
__device__ __forceinline__ bool slab(float lo, float hi, float o, float d, float& tn, float& tf)
{
    if (d == 0.f) return o >= lo && o <= hi;
    const float inv = __builtin_amdgcn_rcpf(d);               // (within 1 ulp; inf for a denormal d: the products below are then +-inf or not a number)
    const float a = (lo - o) * inv, b = (hi - o) * inv;
    const float n = a < b ? a : b, f = a < b ? b : a;
    const float n2 = n - fabsf(n) * kSlabWiden, f2 = f + fabsf(f) * kSlabWiden;
    tn = n2 > tn ? n2 : tn;
    tf = f2 < tf ? f2 : tf;
    return true;
}

// may the traversal accept a triangle of an object inside the box (lo, hi) for the ray (o, d)?  Never false where it does (header: PREFILTER).
// rb: the largest |coordinate| of the box
__device__ __forceinline__ bool box_meets(float lox, float loy, float loz, float hix, float hiy, float hiz, float rb, float ox, float oy, float oz, float dx, float dy,
                                          float dz)
{
    const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
    const float am = fmaxf(fmaxf(ax, ay), az);
    if (!(am > 0.f && am < __builtin_inff())) return true;         // a zero or non-finite direction: the question goes to the traversal as it is
    const float P = kBoxPad * (rb + fmaxf(fmaxf(fabsf(ox), fabsf(oy)), fabsf(oz))) + kBoxTiny;
    const float lx = lox - P, ly = loy - P, lz = loz - P, hx = hix + P, hy = hiy + P, hz = hiz + P;
    // the dominant axis as the traversal picks it (device_common.h begin_ray): an accepted triangle has a corner strictly ahead of o along it
    const int kz = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    const float dk = kz == 0 ? dx : (kz == 1 ? dy : dz), ok = kz == 0 ? ox : (kz == 1 ? oy : oz);
    const float lk = kz == 0 ? lx : (kz == 1 ? ly : lz), hk = kz == 0 ? hx : (kz == 1 ? hy : hz);
    if (!(dk > 0.f ? hk > ok : lk < ok)) return false;
    float tn = -__builtin_inff(), tf = __builtin_inff();
    if (!slab(lx, hx, ox, dx, tn, tf)) return false;
    if (!slab(ly, hy, oy, dy, tn, tf)) return false;
    if (!slab(lz, hz, oz, dz, tn, tf)) return false;
    return !(tn > tf);
}

#pragma clang fp contract(fast)

// word `v` of what lane k parked, as a wave-uniform value (k wave-uniform)
__device__ __forceinline__ float mesh_word(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }

// ------------------------------------------------------------------------------------------------
// what a wave parks, one instance per lane: lane j holds matrix j (device data the host never saw) and the box of instance j (kernel arguments)
// ------------------------------------------------------------------------------------------------
struct MeshParked {
    float W[12];          // lane j < J: world-to-object matrix j
    float bx[6], rb;      // lane j: the box of instance j, its largest |coordinate|
    uint32_t valid;       // wave-uniform: bit j = instance j exists and every word of its matrix is finite
};

// the boxes: scalar loads of kernel arguments, one select per word.  Once per kernel.
__device__ __forceinline__ void mesh_park_boxes(MeshParked& p, const MeshOccluders& occ, int lane)
{
#pragma unroll
    for (int w = 0; w < 6; w++) p.bx[w] = 0.f;
#pragma unroll
    for (int j = 0; j < kMeshMaxInst; j++)
#pragma unroll
        for (int w = 0; w < 6; w++) p.bx[w] = lane == j ? occ.box[j][w] : p.bx[w];
    p.rb = fmaxf(fmaxf(fmaxf(fabsf(p.bx[0]), fabsf(p.bx[1])), fmaxf(fabsf(p.bx[2]), fabsf(p.bx[3]))), fmaxf(fabsf(p.bx[4]), fabsf(p.bx[5])));
}

// the matrices: lane j < J reads matrix j; one with a non-finite entry never blocks.  Once per work item, not per sample.
__device__ __forceinline__ void mesh_park_matrices(MeshParked& p, const float* __restrict__ world_to_obj, int J, int lane)
{
    bool fin = lane < J;
#pragma unroll
    for (int w = 0; w < 12; w++) {
        p.W[w] = lane < J ? world_to_obj[12 * (size_t)lane + w] : 0.f;
        fin = fin && finite32(p.W[w]);
    }
    p.valid = (uint32_t)__ballot(fin);
}

// the header's OBJECT-SPACE RAY of instance j (wave-uniform) for the lane's world-space ray (x, d)
__device__ __forceinline__ void mesh_ray(const MeshParked& p, int j, float px, float py, float pz, float dx, float dy, float dz, float o[3], float d[3])
{
    o[0] = row_point(mesh_word(p.W[0], j), mesh_word(p.W[1], j), mesh_word(p.W[2], j), mesh_word(p.W[3], j), px, py, pz);
    o[1] = row_point(mesh_word(p.W[4], j), mesh_word(p.W[5], j), mesh_word(p.W[6], j), mesh_word(p.W[7], j), px, py, pz);
    o[2] = row_point(mesh_word(p.W[8], j), mesh_word(p.W[9], j), mesh_word(p.W[10], j), mesh_word(p.W[11], j), px, py, pz);
    d[0] = row_dir(mesh_word(p.W[0], j), mesh_word(p.W[1], j), mesh_word(p.W[2], j), dx, dy, dz);
    d[1] = row_dir(mesh_word(p.W[4], j), mesh_word(p.W[5], j), mesh_word(p.W[6], j), dx, dy, dz);
    d[2] = row_dir(mesh_word(p.W[8], j), mesh_word(p.W[9], j), mesh_word(p.W[10], j), dx, dy, dz);
}

// the valid instances whose padded box the lane's object-space ray meets (header: PREFILTER)
__device__ __forceinline__ uint32_t mesh_boxes_met(const MeshParked& p, float px, float py, float pz, float dx, float dy, float dz)
{
    uint32_t met = 0;
#pragma unroll
    for (int j = 0; j < kMeshMaxInst; j++) {
        if ((p.valid >> j) & 1u) {                            // (wave-uniform)
            float o[3], d[3];
            mesh_ray(p, j, px, py, pz, dx, dy, dz, o, d);
            if (box_meets(mesh_word(p.bx[0], j), mesh_word(p.bx[1], j), mesh_word(p.bx[2], j), mesh_word(p.bx[3], j), mesh_word(p.bx[4], j), mesh_word(p.bx[5], j),
                          mesh_word(p.rb, j), o[0], o[1], o[2], d[0], d[1], d[2]))
                met |= 1u << j;
        }
    }
    return met;
}

// VISIBILITY of the segment (x, d) with bound t_max among the scene and J instances (include/texir_hip.h texir_irt_lights_mesh): true iff the scene or a
// valid instance occludes it.  Every question is the occlusion query: ONE traversal instantiation, trace_occluded<LSTK, 4>, walked in a wave-uniform loop over
// {instance 0, ..., instance J - 1, scene}; the SceneDev (the scene's, or the three geometry pointers of the instance's occluder) is chosen by a scalar, so
// the calling kernel owns one LDS stack.  A lane already blocked takes no further step; a step no lane needs is skipped by ballot.
// THE INSTANCES COME FIRST.  Each answer is a function of the segment alone and the result is their OR, so the order changes no bit; it changes the work.  An
// object's tree is a few levels deep, the room's is the deep one, and a wave is 64 neighbouring points looking at one small light: under a table most of its
// lanes are blocked by the table, and once every lane that needs the sample is, the scene walk -- the expensive question -- is not taken at all.  The other
// way round saves the cheap walks where the room already shadows the whole wave, which the captured room does less often than the inserted object beside it.
// `need`: the lane has a segment to ask about.  Call it under a wave-uniform condition (some lane needs the sample).
template <int LSTK>
__device__ __forceinline__ bool mesh_segment_blocked(const SceneDev& sc, const MeshOccluders& occ, const MeshParked& p, int J, int prefilter, bool need, float px,
                                                     float py, float pz, float dx, float dy, float dz, float t_max)
{
    uint32_t met = 0;
    if (p.valid) {                                            // (wave-uniform)
        met = prefilter ? mesh_boxes_met(p, px, py, pz, dx, dy, dz) : p.valid;
        if (!need) met = 0;
    }
    bool blocked = false;
#pragma clang loop unroll(disable)
    for (int s = 0; s <= J; s++) {
        const bool scene = s == J;                            // (wave-uniform)
        if (!scene && !((p.valid >> s) & 1u)) continue;
        const bool ask = need && !blocked && (scene || ((met >> s) & 1u));
        if (!__any(ask)) continue;
        SceneDev cur = sc;
        float o[3] = {px, py, pz}, d[3] = {dx, dy, dz};
        if (!scene) {
            cur.nodes4 = occ.nodes4[s]; cur.nodes4f = occ.nodes4f[s]; cur.quads = occ.quads[s];
            mesh_ray(p, s, px, py, pz, dx, dy, dz, o, d);
        }
        if (ask) blocked = trace_occluded<LSTK, 4>(cur, o[0], o[1], o[2], d[0], d[1], d[2], 0.f, t_max);
    }
    return blocked;
}

}  // namespace texir

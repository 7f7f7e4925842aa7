// Texel G-buffer by rasterising the mesh in uv space (replaces tracer_o3d_irt.py:99-142: a cube map ray-cast per view, warped to a 1024 x 512 panorama and
// gathered through the (row code, column code, panorama id) triple of 0.png).  Everything the exact answer needs is in the scene handle: the triangles'
// vertices, their per-corner uvs and (optionally) corner normals, by leaf-order slot and in STORED corner order (bvh_build.h); the slot's rotation is turned
// back first, so every value below is a function of the caller's (verts, tris, tri_uvs) alone and not of how the builder paired or rotated the triangles.
//
// Texel (r, c) of an H x W atlas in hit-shader orientation has its centre at (u, v) = ((c + 0.5) / W, (r + 0.5) / H), two float32 divisions; the outputs are
// written in FILE orientation, row H - 1 - r (what models.TracerO3d._load_texel_gbuffer reads).
//
// COVERAGE.  The three edges of a uv triangle are each evaluated from the edge's two endpoints in ONE canonical order (the lexicographically smaller
// (x, y) first), with separately rounded float32 operations:
//       E = (x1 - x0) * (v - y0) - (y1 - y0) * (u - x0)        4 subtractions, 2 products, 1 difference; when the difference is 0 its sign is taken from the
//                                                              exact error terms of the two products (fma(a, b, -fl(a b))), so E == 0 means exactly 0
// Two triangles that share an edge compute the identical E and use it with opposite signs: exact negations, no texel lost or given twice along the edge.
// With s the sign of the triangle's area (the same evaluation of edge (corner 0, corner 1) at corner 2; mirrored charts have s < 0) the texel is inside
// edge k when s e_k > 0, or when s e_k == 0 and the inward edge normal (nx, ny) = s (-(y_b - y_a), x_b - x_a) has nx > 0, or nx == 0 and ny > 0 (CRACK RULE).
// A triangle with s == 0 or a non-finite uv covers nothing.  Where several triangles cover a centre the lowest primitive id wins (OVERLAP RULE): phase 1
// is an integer atomicMin of the primitive id per texel, phase 2 a resolve pass per texel; there are no float atomics and the order in which triangles
// arrive cannot change a bit.
// A triangle is only tested against the texels of its clipped bounding box, columns max(0, floor(umin W - 0.5)) .. min(W - 1, ceil(umax W - 0.5)) and the
// same in rows: the box is part of the definition (it never cuts a centre that lies inside the triangle or on its border).
//
// WORK DISTRIBUTION.  One lane per slot computes the box.  A box of at most kSmallBox texels is tested by that lane (millimetre clutter: one to four
// tests).  A larger one is split into 8 x 8-texel tiles: the lane draws its position in the list of large triangles AND the first of its tile items from one
// 64-bit atomic add (list index in the upper 28 bits, running item count in the lower 36), so the list is sorted by first item; the second kernel's waves
// stride over the items, find the triangle of an item by bisection, and test one texel per lane.  A triangle spanning the whole 4096^2 atlas is 262 144
// items spread over every compute unit.  Which path tests a (triangle, texel) pair has no influence on the outcome: both evaluate the same predicate.
//
// ATTRIBUTES of the winning primitive, per texel: e_k = the oriented edge value opposite the caller's corner k, S = (e_0 + e_1) + e_2,
// b1 = e_1 / S, b2 = e_2 / S (the weights of the caller's corners 1 and 2: texir_trace_shade's prim_uv convention), p = P0 + b1 (P1 - P0) + b2 (P2 - P0),
// geometric normal n = cross(P1 - P0, P2 - P0) / |.|, shading normal n = N0 + b1 (N1 - N0) + b2 (N2 - N0) NOT renormalised (:105-106), pos = p + offset n.
// An uncovered texel, one whose geometric normal has zero length (or is not finite), and one with S == 0 is a seam: pos = nrm = 0, prim_id = 0xFFFFFFFF.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace texir {

// every product, difference and quotient below is its own rounded float32 operation: the header states the arithmetic and the tests restate it
#pragma clang fp contract(off)

constexpr int kRB = 256;
constexpr int kSmallBox = 64;                     // texels a single lane tests itself
constexpr int kTile = 8;                          // a wave's tile of a large box: 8 x 8 texels
constexpr int kItemBits = 36;                     // lower bits of the packed counter: running count of (triangle, tile) items
constexpr unsigned long long kItemMask = (1ull << kItemBits) - 1ull;
constexpr uint32_t kNoPrim = 0xFFFFFFFFu;

struct RasterWs {
    unsigned long long* counter;      // (large triangles << 36) | tile items
    unsigned long long* big_off;      // [n_slots] first item of large triangle j
    uint32_t* owner;                  // [H * W] hit-shader orientation: lowest covering primitive id
    uint32_t* prim2slot;              // [T]
    uint32_t* big_slot;               // [n_slots]
};

static size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

static RasterWs carve(void* ws, int64_t n_slots, int64_t T, int H, int W)
{
    char* p = (char*)ws;
    RasterWs r;
    r.counter = (unsigned long long*)p; p += 16;
    r.big_off = (unsigned long long*)p; p += align16((size_t)n_slots * 8);
    r.owner = (uint32_t*)p; p += align16((size_t)H * W * 4);
    r.prim2slot = (uint32_t*)p; p += align16((size_t)T * 4);
    r.big_slot = (uint32_t*)p;
    return r;
}

size_t texel_raster_workspace_bytes(int64_t n_slots, int64_t T, int H, int W)
{
    return 16 + align16((size_t)n_slots * 8) + align16((size_t)H * W * 4) + align16((size_t)T * 4) + align16((size_t)n_slots * 4);
}

// stored corner k = the caller's corner (rot + k) % 3: the caller's corners (c0, c1, c2) from the stored ones (s0, s1, s2)
template <typename T>
__device__ __forceinline__ void unrotate(uint32_t rot, const T& s0, const T& s1, const T& s2, T& c0, T& c1, T& c2)
{
    c0 = rot == 0u ? s0 : (rot == 1u ? s2 : s1);
    c1 = rot == 0u ? s1 : (rot == 1u ? s0 : s2);
    c2 = rot == 0u ? s2 : (rot == 1u ? s1 : s0);
}

struct UvTri {
    float x0, y0, x1, y1, x2, y2;     // caller order
    float s;                          // sign of the area (0: covers nothing)
    int c0, c1, r0, r1;               // clipped texel box (empty: c0 > c1)
};

// dx * qy - dy * qx, separately rounded; a zero difference is replaced by the (exactly signed) difference of the products' error terms
__device__ __forceinline__ float cross_exact_sign(float dx, float dy, float qx, float qy)
{
    const float p = dx * qy, q = dy * qx;
    float r = p - q;
    if (r == 0.f) r = __builtin_fmaf(dx, qy, -p) - __builtin_fmaf(dy, qx, -q);
    return r;
}

// edge a -> b (triangle order) at (px, py): e = the oriented value cross(b - a, p - a) from the canonical evaluation; returns the crack rule's verdict for
// a triangle of area sign s
__device__ __forceinline__ bool edge_inside(float ax, float ay, float bx, float by, float px, float py, float s, float& e)
{
    const bool sw = (bx < ax) || (bx == ax && by < ay);
    const float x0 = sw ? bx : ax, y0 = sw ? by : ay, x1 = sw ? ax : bx, y1 = sw ? ay : by;
    const float dx = x1 - x0, dy = y1 - y0;
    const float E = cross_exact_sign(dx, dy, px - x0, py - y0);
    const float o = sw ? -s : s;
    e = sw ? -E : E;
    const float val = o * E, nx = o * -dy, ny = o * dx;
    return val > 0.f || (val == 0.f && (nx > 0.f || (nx == 0.f && ny > 0.f)));
}

// e0, e1, e2: oriented edge values opposite the caller's corners 0, 1, 2
__device__ __forceinline__ bool tri_covers(const UvTri& t, float px, float py, float& e0, float& e1, float& e2)
{
    const bool i0 = edge_inside(t.x1, t.y1, t.x2, t.y2, px, py, t.s, e0);
    const bool i1 = edge_inside(t.x2, t.y2, t.x0, t.y0, px, py, t.s, e1);
    const bool i2 = edge_inside(t.x0, t.y0, t.x1, t.y1, px, py, t.s, e2);
    return i0 && i1 && i2;
}

__device__ __forceinline__ float centre(int i, int n) { return ((float)i + 0.5f) / (float)n; }

__device__ __forceinline__ uint32_t slot_rot(const SceneDev& sc, int slot) { return __float_as_uint(sc.tris[3 * (size_t)slot + 1].w); }

__device__ __forceinline__ void load_uv_tri(const SceneDev& sc, int slot, uint32_t rot, int H, int W, UvTri& t)
{
    float4 a, b;
    tri_uvs(sc, slot, a, b);
    const float2 s0 = make_float2(a.x, a.y), s1 = make_float2(a.z, a.w), s2 = make_float2(b.x, b.y);
    float2 c0, c1, c2;
    unrotate(rot, s0, s1, s2, c0, c1, c2);
    t.x0 = c0.x; t.y0 = c0.y; t.x1 = c1.x; t.y1 = c1.y; t.x2 = c2.x; t.y2 = c2.y;
    t.s = 0.f; t.c0 = 0; t.c1 = -1; t.r0 = 0; t.r1 = -1;
    const float z = ((((t.x0 * 0.f + t.y0 * 0.f) + t.x1 * 0.f) + t.y1 * 0.f) + t.x2 * 0.f) + t.y2 * 0.f;
    if (!(z == 0.f)) return;                                           // a NaN or an infinity among the six
    float A;
    (void)edge_inside(t.x0, t.y0, t.x1, t.y1, t.x2, t.y2, 1.f, A);
    t.s = A > 0.f ? 1.f : (A < 0.f ? -1.f : 0.f);
    if (t.s == 0.f) return;
    const float fw = (float)W, fh = (float)H;
    const float umin = fminf(fminf(t.x0, t.x1), t.x2), umax = fmaxf(fmaxf(t.x0, t.x1), t.x2);
    const float vmin = fminf(fminf(t.y0, t.y1), t.y2), vmax = fmaxf(fmaxf(t.y0, t.y1), t.y2);
    // (clamped as floats first: a uv far outside the atlas must not overflow the conversion)
    t.c0 = (int)fminf(fmaxf(floorf(umin * fw - 0.5f), 0.f), fw);
    t.c1 = (int)fminf(fmaxf(ceilf(umax * fw - 0.5f), -1.f), fw - 1.f);
    t.r0 = (int)fminf(fmaxf(floorf(vmin * fh - 0.5f), 0.f), fh);
    t.r1 = (int)fminf(fmaxf(ceilf(vmax * fh - 0.5f), -1.f), fh - 1.f);
    if (t.r0 > t.r1) { t.c0 = 0; t.c1 = -1; }
}

__global__ __launch_bounds__(kRB) void raster_init_kernel(RasterWs ws, int64_t n_texels)
{
    const int64_t i = (int64_t)blockIdx.x * kRB + threadIdx.x;
    if (i == 0) *ws.counter = 0ull;
    if (i < n_texels) ws.owner[i] = kNoPrim;
}

// phase 1a: one lane per leaf-order slot
__global__ __launch_bounds__(kRB) void raster_bin_kernel(SceneDev sc, int64_t n_slots, int64_t T, int H, int W, RasterWs ws)
{
    const int64_t slot = (int64_t)blockIdx.x * kRB + threadIdx.x;
    if (slot >= n_slots) return;
    const uint32_t prim = tri_prim(sc, (int)slot);
    if (prim >= (uint32_t)T) return;                                   // an empty slot (0xFFFFFFFF)
    ws.prim2slot[prim] = (uint32_t)slot;
    UvTri t;
    load_uv_tri(sc, (int)slot, slot_rot(sc, (int)slot), H, W, t);
    if (t.c0 > t.c1) return;
    const int bw = t.c1 - t.c0 + 1, bh = t.r1 - t.r0 + 1;
    if ((int64_t)bw * bh <= kSmallBox) {
        for (int r = t.r0; r <= t.r1; r++) {
            const float py = centre(r, H);
            for (int c = t.c0; c <= t.c1; c++) {
                float e0, e1, e2;
                if (tri_covers(t, centre(c, W), py, e0, e1, e2)) atomicMin(ws.owner + (size_t)r * W + c, prim);
            }
        }
        return;
    }
    const unsigned long long n_items = (unsigned long long)((bw + kTile - 1) / kTile) * (unsigned long long)((bh + kTile - 1) / kTile);
    const unsigned long long old = atomicAdd(ws.counter, (1ull << kItemBits) | n_items);
    const unsigned long long j = old >> kItemBits;
    if (j < (unsigned long long)n_slots) { ws.big_off[j] = old & kItemMask; ws.big_slot[j] = (uint32_t)slot; }
}

// phase 1b: one wave per (large triangle, 8 x 8 tile) item
__global__ __launch_bounds__(kRB) void raster_tile_kernel(SceneDev sc, int64_t n_slots, int H, int W, RasterWs ws)
{
    const unsigned long long packed = *ws.counter;
    unsigned long long count = packed >> kItemBits;
    if (count > (unsigned long long)n_slots) count = (unsigned long long)n_slots;
    const unsigned long long total = packed & kItemMask;
    const int lane = threadIdx.x & 63;
    const unsigned long long n_waves = (unsigned long long)gridDim.x * (kRB / 64);
    for (unsigned long long item = (unsigned long long)blockIdx.x * (kRB / 64) + (threadIdx.x >> 6); item < total; item += n_waves) {
        // the last large triangle whose first item is <= item (big_off is ascending: positions and offsets come from the same atomic)
        unsigned long long lo = 0, hi = count;
        while (hi - lo > 1) {
            const unsigned long long mid = (lo + hi) >> 1;
            if (ws.big_off[mid] <= item) lo = mid; else hi = mid;
        }
        if (lo >= count) break;
        const int slot = (int)ws.big_slot[lo];
        const unsigned long long k = item - ws.big_off[lo];
        UvTri t;
        load_uv_tri(sc, slot, slot_rot(sc, slot), H, W, t);
        if (t.c0 > t.c1) continue;
        const int ntx = (t.c1 - t.c0 + kTile) / kTile, nty = (t.r1 - t.r0 + kTile) / kTile;
        if (k >= (unsigned long long)ntx * (unsigned long long)nty) continue;
        const int ty = (int)(k / (unsigned long long)ntx), tx = (int)(k - (unsigned long long)ty * ntx);
        const int c = t.c0 + tx * kTile + (lane & (kTile - 1)), r = t.r0 + ty * kTile + (lane >> 3);
        if (c > t.c1 || r > t.r1) continue;
        float e0, e1, e2;
        if (tri_covers(t, centre(c, W), centre(r, H), e0, e1, e2)) atomicMin(ws.owner + (size_t)r * W + c, tri_prim(sc, slot));
    }
}

// phase 2: one lane per texel, in file orientation (coalesced writes)
template <bool SHADING>
__global__ __launch_bounds__(kRB) void raster_resolve_kernel(SceneDev sc, const float4* __restrict__ cnrm, int64_t T, int H, int W, float offset, RasterWs ws,
                                                             float* __restrict__ pos, float* __restrict__ nrm, uint32_t* __restrict__ prim_id,
                                                             float* __restrict__ bary)
{
    const int c = blockIdx.x * kRB + threadIdx.x, fr = blockIdx.y;
    if (c >= W) return;
    const int r = H - 1 - fr;
    const size_t o = (size_t)fr * W + c;
    uint32_t prim = ws.owner[(size_t)r * W + c];
    float P[3] = {0.f, 0.f, 0.f}, N[3] = {0.f, 0.f, 0.f}, b1 = 0.f, b2 = 0.f;
    if (prim < (uint32_t)T) {
        const int slot = (int)ws.prim2slot[prim];
        const uint32_t rot = slot_rot(sc, slot);
        UvTri t;
        load_uv_tri(sc, slot, rot, H, W, t);
        float e0, e1, e2;
        (void)tri_covers(t, centre(c, W), centre(r, H), e0, e1, e2);
        const float S = (e0 + e1) + e2;
        b1 = e1 / S; b2 = e2 / S;
        const float4 q0 = sc.tris[3 * (size_t)slot], q1 = sc.tris[3 * (size_t)slot + 1], q2 = sc.tris[3 * (size_t)slot + 2];
        const float3 s0 = make_float3(q0.x, q0.y, q0.z), s1 = make_float3(q1.x, q1.y, q1.z), s2 = make_float3(q2.x, q2.y, q2.z);      // the record holds v1, v2
        float3 p0, p1, p2;
        unrotate(rot, s0, s1, s2, p0, p1, p2);
        const float ax = p1.x - p0.x, ay = p1.y - p0.y, az = p1.z - p0.z, bx = p2.x - p0.x, by = p2.y - p0.y, bz = p2.z - p0.z;
        const float gx = ay * bz - az * by, gy = az * bx - ax * bz, gz = ax * by - ay * bx;
        const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
        const bool ok = S != 0.f && len > 0.f && len - len == 0.f;
        if (ok) {
            P[0] = (p0.x + b1 * ax) + b2 * bx; P[1] = (p0.y + b1 * ay) + b2 * by; P[2] = (p0.z + b1 * az) + b2 * bz;
            if (SHADING) {
                const float4 m0 = cnrm[3 * (size_t)slot], m1 = cnrm[3 * (size_t)slot + 1], m2 = cnrm[3 * (size_t)slot + 2];
                float4 n0, n1, n2;
                unrotate(rot, m0, m1, m2, n0, n1, n2);
                N[0] = (n0.x + b1 * (n1.x - n0.x)) + b2 * (n2.x - n0.x);
                N[1] = (n0.y + b1 * (n1.y - n0.y)) + b2 * (n2.y - n0.y);
                N[2] = (n0.z + b1 * (n1.z - n0.z)) + b2 * (n2.z - n0.z);
            } else {
                N[0] = gx / len; N[1] = gy / len; N[2] = gz / len;
            }
            P[0] = P[0] + offset * N[0]; P[1] = P[1] + offset * N[1]; P[2] = P[2] + offset * N[2];
        } else {
            prim = kNoPrim; b1 = 0.f; b2 = 0.f;
        }
    } else {
        prim = kNoPrim;
    }
    pos[3 * o] = P[0]; pos[3 * o + 1] = P[1]; pos[3 * o + 2] = P[2];
    nrm[3 * o] = N[0]; nrm[3 * o + 1] = N[1]; nrm[3 * o + 2] = N[2];
    if (prim_id) prim_id[o] = prim;
    if (bary) { bary[2 * o] = b1; bary[2 * o + 1] = b2; }
}

hipError_t launch_texel_raster(const SceneDev& sc, const float4* cnrm, int64_t n_slots, int64_t T, int H, int W, int shading, float offset, float* pos, float* nrm,
                               uint32_t* prim_id, float* bary, void* workspace, hipStream_t st)
{
    const RasterWs ws = carve(workspace, n_slots, T, H, W);
    const int64_t nt = (int64_t)H * W;
    raster_init_kernel<<<dim3((unsigned)((nt + kRB - 1) / kRB)), kRB, 0, st>>>(ws, nt);
    raster_bin_kernel<<<dim3((unsigned)((n_slots + kRB - 1) / kRB)), kRB, 0, st>>>(sc, n_slots, T, H, W, ws);
    // a fixed grid (the item count is only known on the device): 8 blocks of 4 waves for each of 256 compute units
    raster_tile_kernel<<<dim3(2048), kRB, 0, st>>>(sc, n_slots, H, W, ws);
    const dim3 gr((W + kRB - 1) / kRB, H);
    if (shading) raster_resolve_kernel<true><<<gr, kRB, 0, st>>>(sc, cnrm, T, H, W, offset, ws, pos, nrm, prim_id, bary);
    else raster_resolve_kernel<false><<<gr, kRB, 0, st>>>(sc, cnrm, T, H, W, offset, ws, pos, nrm, prim_id, bary);
    return hipGetLastError();
}

}  // namespace texir

// The cube-map G-buffer with inserted triangle-mesh instances DRAWN IN THE VIEW (include/texir_hip.h texir_gbuffer_cast_mesh states the rule, the float32
// operation sequence of an instance pixel's position and normal and their rounding bound; this file follows that text operation by operation).
//
// Per pixel the ray of gbuffer_kernel (gbuffer.hip: face_basis, the same pixel centre, the same expressions), then ONE traversal instantiation --
// trace_core<false, kLstk, 4, false, false>, the instantiation trace_closest<false, kLstk, 4> is -- walked in a wave-uniform loop over {scene, instance 0, ...,
// instance J - 1}, the shape of mesh_segment_blocked (mesh_instance.h): the SceneDev (the scene's, or the geometry pointers of the instance's occluder, which
// travel by value in the kernel arguments) is chosen by a scalar, so the kernel owns one LDS stack (24 KiB per block, gbuffer_kernel's).  The scene comes
// first and starts at +inf: the call gbuffer_kernel<4> makes.  Every instance walk STARTS at the nearest t found so far (t_start = t_best), so its leaf test
// accepts 0 < t < t_best and nothing else (a walk that starts at h.t = t_far never culls a box that holds an accepted triangle with t < t_far);
// an accepting walk becomes the pixel's surface and lowers t_best.  Acceptance is strict: the scene wins a tie, a lower instance index wins over a higher.
// A walk no lane needs -- the prefilter rejected it for every lane -- is skipped by ballot.
//
// The J matrices are device data (a replayed graph sees a moved object): lane j of every wave loads and validates matrix j once per launch and takes the box
// of instance j from the kernel arguments; the loop reads the words across the wave (v_readlane: scalars, no LDS, no memory).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "mesh_instance.h"

namespace texir {

// ------------------------------------------------------------------------------------------------------------------
// an instance pixel: every product, sum and difference is its own rounded float32 operation (the header states the arithmetic)
// ------------------------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)

// pos = eye + t d in WORLD space: the ray parameter survives the affine map, so the t of the object-space walk is the t along the camera ray
__device__ __forceinline__ void inst_position(float ex, float ey, float ez, float t, float dx, float dy, float dz, float o[3])
{
    o[0] = ex + t * dx; o[1] = ey + t * dy; o[2] = ez + t * dz;
}

// nrm = normalize(W^T n_o), W = the 3 x 3 part of world-to-object matrix j (wave-uniform) = the inverse transpose of the pose's linear part; n_o = the unit
// geometric normal of the stored record (a rotation of the caller's corners: the caller's winding), as gbuffer_kernel takes it.  Not flipped towards the viewer.
__device__ __forceinline__ void inst_normal(const MeshParked& p, int j, const float4* __restrict__ tp, float o[3])
{
    const float4 v0 = tp[0], v1 = tp[1], v2 = tp[2];
    const float e1x = v1.x - v0.x, e1y = v1.y - v0.y, e1z = v1.z - v0.z, e2x = v2.x - v0.x, e2y = v2.y - v0.y, e2z = v2.z - v0.z;
    const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const float il = rsqrtf((nx * nx + ny * ny) + nz * nz);
    const float ax = nx * il, ay = ny * il, az = nz * il;
    const float mx = (mesh_word(p.W[0], j) * ax + mesh_word(p.W[4], j) * ay) + mesh_word(p.W[8], j) * az;
    const float my = (mesh_word(p.W[1], j) * ax + mesh_word(p.W[5], j) * ay) + mesh_word(p.W[9], j) * az;
    const float mz = (mesh_word(p.W[2], j) * ax + mesh_word(p.W[6], j) * ay) + mesh_word(p.W[10], j) * az;
    const float im = rsqrtf((mx * mx + my * my) + mz * mz);
    o[0] = mx * im; o[1] = my * im; o[2] = mz * im;
}

#pragma clang fp contract(fast)

__global__ __launch_bounds__(kBlock) void gbuffer_mesh_kernel(SceneDev sc, GbufArgs g, GbufMeshOccluders mo, const float* __restrict__ world_to_obj, int J, int prefilter,
                                                              int32_t* __restrict__ inst)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (wave-uniform: the pixel loop and the surface loop stay scalar)
    const int64_t P = (int64_t)6 * g.c * g.c;
    MeshParked mp;
    mesh_park_boxes(mp, mo.occ, lane);
    mesh_park_matrices(mp, world_to_obj, J, lane);
    // gbuffer_kernel's pixel order and launch shape: pixel p0 + lane, 64 consecutive pixels per wave and trip
    for (int64_t p0 = (int64_t)blockIdx.x * kBlock + 64 * wave; p0 < P; p0 += (int64_t)gridDim.x * kBlock) {
        const bool live = p0 + lane < P;
        const int64_t p = live ? p0 + lane : P - 1;                    // (a lane past the end computes the last pixel's ray and neither traces nor writes)
        const int face = (int)(p / ((int64_t)g.c * g.c));
        const int rem = (int)(p - (int64_t)face * g.c * g.c);
        const int i = rem / g.c, j = rem - i * g.c;
        const FaceBasis& fb = g.face[face];
        const float x = ((float)j + 0.5f) / (float)g.c * 2.f - 1.f, y = ((float)i + 0.5f) / (float)g.c * 2.f - 1.f;
        const float ex = fb.eye[0], ey = fb.eye[1], ez = fb.eye[2];
        float dx = fb.d0[0] + x * fb.dx[0] + y * fb.dy[0], dy = fb.d0[1] + x * fb.dx[1] + y * fb.dy[1], dz = fb.d0[2] + x * fb.dx[2] + y * fb.dy[2];
        // the instances whose box the lane's object-space ray meets (prefilter off: every valid one)
        uint32_t met = 0;
        if (mp.valid) {                                                // (wave-uniform)
            met = prefilter ? mesh_boxes_met(mp, ex, ey, ez, dx, dy, dz) : mp.valid;
            if (!live) met = 0;
        }
        // one traversal instance, a wave-uniform loop: s = 0 the scene from +inf, s = k + 1 instance k inside (0, t_best)
        Hit h;
        h.t = __builtin_inff(); h.u = 0.f; h.v = 0.f; h.slot = -1;
        int surf = -1;                                                  // the pixel's surface: -1 the scene (or background), else the instance
        float i_pos[3] = {0.f, 0.f, 0.f}, i_n[3] = {0.f, 0.f, 0.f}; int32_t i_tri = 0;
#pragma clang loop unroll(disable)
        for (int s = 0; s <= J; s++) {
            const int k = s > 0 ? s - 1 : 0;                            // (wave-uniform)
            if (s > 0 && !((mp.valid >> k) & 1u)) continue;
            const bool ask = live && (s == 0 || ((met >> k) & 1u));
            if (!__any(ask)) continue;
            SceneDev cur = sc;
            float o[3] = {ex, ey, ez}, d[3] = {dx, dy, dz};
            if (s > 0) {
                cur.nodes4 = mo.occ.nodes4[k]; cur.nodes4f = mo.occ.nodes4f[k]; cur.quads = mo.occ.quads[k]; cur.tris = mo.tris[k];
                mesh_ray(mp, k, ex, ey, ez, dx, dy, dz, o, d);
            }
            if (ask) {
                uint32_t cn = 0, ct = 0;
                const Hit hk = trace_core<false, kLstk, 4, false, false>(cur, o[0], o[1], o[2], d[0], d[1], d[2], cn, ct, nullptr, 64, NoNext{}, h.t, 0.f);
                if (s == 0) h = hk;
                else if (hk.slot >= 0) {                                // an accepted triangle of instance k with 0 < t < t_best
                    h = hk; surf = k;
                    const float4* tp = cur.tris + kTriQuads * (size_t)hk.slot;
                    i_tri = (int32_t)__float_as_uint(tp[0].w) + 1;     // (tri_prim: the row of the occluder's own index array)
                    inst_position(ex, ey, ez, hk.t, dx, dy, dz, i_pos);
                    inst_normal(mp, k, tp, i_n);
                }
            }
        }
        // d(dir)/dX, d(dir)/dY in PIXEL units (d ndc / d pixel = 2/c)
        const float s2 = 2.f / (float)g.c;
        float dXx = s2 * fb.dx[0], dXy = s2 * fb.dx[1], dXz = s2 * fb.dx[2];
        float dYx = s2 * fb.dy[0], dYy = s2 * fb.dy[1], dYz = s2 * fb.dy[2];
        float o_pos[3] = {1.f, 0.f, 0.f}, o_n[3] = {1.f, 0.f, 0.f}, o_uv[2] = {0.f, 0.f}, o_da[4] = {0.f, 0.f, 0.f, 0.f};   // bg (mat_nvdiffrast.py:125)
        float m = 0.f; int32_t tri = 0;
        if (surf >= 0) {                                                // an instance: occluders carry no uvs, whatever flip_v is
            m = 1.f; tri = i_tri;
            for (int a = 0; a < 3; a++) { o_pos[a] = i_pos[a]; o_n[a] = i_n[a]; }
        } else if (h.slot >= 0) {
            // the scene: the text of gbuffer_kernel's hit branch, operation for operation (the tests hold the bits against texir_gbuffer_cast)
            const float4* tp = sc.tris + kTriQuads * (size_t)h.slot;
            float4 v0 = tp[0], e1 = tp[1], e2 = tp[2];
            e1.x -= v0.x; e1.y -= v0.y; e1.z -= v0.z; e2.x -= v0.x; e2.y -= v0.y; e2.z -= v0.z;      // the record holds v1, v2
            m = 1.f; tri = (int32_t)tri_prim(sc, h.slot) + 1;
            const float u = h.u, v = h.v, w = 1.f - u - v;
            o_pos[0] = v0.x + u * e1.x + v * e2.x; o_pos[1] = v0.y + u * e1.y + v * e2.y; o_pos[2] = v0.z + u * e1.z + v * e2.z;
            if (g.cnrm) {
                float4 n0 = g.cnrm[3 * (size_t)h.slot], n1 = g.cnrm[3 * (size_t)h.slot + 1], n2 = g.cnrm[3 * (size_t)h.slot + 2];
                o_n[0] = n0.x * w + n1.x * u + n2.x * v; o_n[1] = n0.y * w + n1.y * u + n2.y * v; o_n[2] = n0.z * w + n1.z * u + n2.z * v;
            } else {
                float nx = e1.y * e2.z - e1.z * e2.y, ny = e1.z * e2.x - e1.x * e2.z, nz = e1.x * e2.y - e1.y * e2.x;
                float il = rsqrtf(nx * nx + ny * ny + nz * nz);
                o_n[0] = nx * il; o_n[1] = ny * il; o_n[2] = nz * il;
            }
            // analytic d(u,v)/d(pixel): [e1 e2 -d] [u' v' t']^T = t * d'  (same Moeller-Trumbore solve, rhs b = t*d')
            float px = dy * e2.z - dz * e2.y, py = dz * e2.x - dx * e2.z, pz = dx * e2.y - dy * e2.x;
            float det = e1.x * px + e1.y * py + e1.z * pz;
            float inv = 1.f / det;
            float du[2], dv[2];
            const float bx[2] = {h.t * dXx, h.t * dYx}, by[2] = {h.t * dXy, h.t * dYy}, bz[2] = {h.t * dXz, h.t * dYz};
            for (int k = 0; k < 2; k++) {
                du[k] = (bx[k] * px + by[k] * py + bz[k] * pz) * inv;
                float qx = by[k] * e1.z - bz[k] * e1.y, qy = bz[k] * e1.x - bx[k] * e1.z, qz = bx[k] * e1.y - by[k] * e1.x;
                dv[k] = (dx * qx + dy * qy + dz * qz) * inv;
            }
            float4 a, b;
            tri_uvs(sc, h.slot, a, b);
            float a1x = a.z - a.x, a1y = a.w - a.y, a2x = b.x - a.x, a2y = b.y - a.y;
            o_uv[0] = a.x * w + a.z * u + b.x * v; o_uv[1] = a.y * w + a.w * u + b.y * v;
            o_da[0] = a1x * du[0] + a2x * dv[0]; o_da[1] = a1x * du[1] + a2x * dv[1];        // du/dX, du/dY
            o_da[2] = a1y * du[0] + a2y * dv[0]; o_da[3] = a1y * du[1] + a2y * dv[1];        // dv/dX, dv/dY
            if (g.flip_v) { o_uv[1] = 1.f - o_uv[1]; o_da[2] = -o_da[2]; o_da[3] = -o_da[3]; }
        }
        if (live) {
            for (int k = 0; k < 3; k++) { g.pos[3 * p + k] = o_pos[k]; g.nrm[3 * p + k] = o_n[k]; }
            g.mask[p] = m; g.tri[p] = tri; inst[p] = surf;
            g.uv[2 * p] = o_uv[0]; g.uv[2 * p + 1] = o_uv[1];
            for (int k = 0; k < 4; k++) g.uvda[4 * p + k] = o_da[k];
        }
    }
}

hipError_t launch_gbuffer_mesh(const SceneDev& sc, const float* mvp_host, const float4* cnrm, int c, int flip_v, const GbufMeshOccluders& mo, const float* world_to_obj,
                               int J, bool prefilter, float* pos, float* nrm, float* mask, float* uv, float* uvda, int32_t* tri, int32_t* inst, hipStream_t st)
{
    GbufArgs g;
    for (int f = 0; f < 6; f++) if (!face_basis(mvp_host + 16 * f, g.face[f])) return hipErrorInvalidValue;
    g.cnrm = cnrm; g.c = c; g.flip_v = flip_v; g.pos = pos; g.nrm = nrm; g.mask = mask; g.uv = uv; g.uvda = uvda; g.tri = tri;
    const dim3 grid(grid_capped(kBlock, (int64_t)6 * c * c));
    hipLaunchKernelGGL(gbuffer_mesh_kernel, grid, dim3(kBlock), 0, st, sc, g, mo, world_to_obj, J, prefilter ? 1 : 0, inst);
    return hipGetLastError();
}

}  // namespace texir

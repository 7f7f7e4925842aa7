// The cube-map G-buffer of libtexir_hip.so:
//   gbuffer_kernel     position, normal, uv, uv pixel-differentials, mask by PRIMARY-RAY CASTING through
//                      the same BVH -- replaces nvdiffrast rasterize + interpolate (models/mat_nvdiffrast.py:119-128,
//                      models/tracer_o3d_irt.py:102-108).  Geometry and cameras are constant, so a view's G-buffer is
//                      computed once and cached by the host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"
#include "kernels.h"

namespace texir {

// ------------------------------------------------------------------------------------------------------------------
// G-buffer by ray casting.  Row-vector convention of the reference: clip = [x,y,z,1] @ mvp (datasets/dataset.py:464-465).
// Pixel (row i, col j) of a face has ndc = ((j+.5)/c*2-1, (i+.5)/c*2-1) (nvdiffrast: row 0 is clip y = -1).
// The ray direction is LINEAR in (x,y) (see launch_gbuffer), which gives exact analytic pixel derivatives of the
// barycentrics -- what nvdiffrast's rast_db / interpolate(diff_attrs='all') provide.
// ------------------------------------------------------------------------------------------------------------------
// (FaceBasis, GbufArgs: kernels.h -- gbuffermesh.hip casts the same rays)

template <int WIDTH>
__global__ __launch_bounds__(kBlock) void gbuffer_kernel(SceneDev sc, GbufArgs g)
{
    const int64_t P = (int64_t)6 * g.c * g.c;
    uint32_t cn = 0, ct = 0;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < P; p += (int64_t)gridDim.x * kBlock) {
        const int face = (int)(p / ((int64_t)g.c * g.c));
        const int rem = (int)(p - (int64_t)face * g.c * g.c);
        const int i = rem / g.c, j = rem - i * g.c;
        const FaceBasis& fb = g.face[face];
        const float x = ((float)j + 0.5f) / (float)g.c * 2.f - 1.f, y = ((float)i + 0.5f) / (float)g.c * 2.f - 1.f;
        const float ex = fb.eye[0], ey = fb.eye[1], ez = fb.eye[2];
        float dx = fb.d0[0] + x * fb.dx[0] + y * fb.dy[0], dy = fb.d0[1] + x * fb.dx[1] + y * fb.dy[1], dz = fb.d0[2] + x * fb.dx[2] + y * fb.dy[2];
        // d(dir)/dX, d(dir)/dY in PIXEL units (d ndc / d pixel = 2/c)
        const float s2 = 2.f / (float)g.c;
        float dXx = s2 * fb.dx[0], dXy = s2 * fb.dx[1], dXz = s2 * fb.dx[2];
        float dYx = s2 * fb.dy[0], dYy = s2 * fb.dy[1], dYz = s2 * fb.dy[2];
        Hit h = trace_closest<false, kLstk, WIDTH>(sc, ex, ey, ez, dx, dy, dz, cn, ct);
        float o_pos[3] = {1.f, 0.f, 0.f}, o_n[3] = {1.f, 0.f, 0.f}, o_uv[2] = {0.f, 0.f}, o_da[4] = {0.f, 0.f, 0.f, 0.f};   // bg (mat_nvdiffrast.py:125)
        float m = 0.f; int32_t tri = 0;
        if (h.slot >= 0) {
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
        for (int k = 0; k < 3; k++) { g.pos[3 * p + k] = o_pos[k]; g.nrm[3 * p + k] = o_n[k]; }
        g.mask[p] = m; g.tri[p] = tri;
        g.uv[2 * p] = o_uv[0]; g.uv[2 * p + 1] = o_uv[1];
        for (int k = 0; k < 4; k++) g.uvda[4 * p + k] = o_da[k];
    }
}

static bool invert4(const double* m, double* out)
{
    double a[4][8];
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) { a[r][c] = m[4 * r + c]; a[r][4 + c] = (r == c) ? 1.0 : 0.0; }
    for (int col = 0; col < 4; col++) {
        int piv = col; double best = fabs(a[col][col]);
        for (int r = col + 1; r < 4; r++) if (fabs(a[r][col]) > best) { best = fabs(a[r][col]); piv = r; }
        if (best == 0.0) return false;
        if (piv != col) for (int c = 0; c < 8; c++) { double t = a[col][c]; a[col][c] = a[piv][c]; a[piv][c] = t; }
        double d = a[col][col];
        for (int c = 0; c < 8; c++) a[col][c] /= d;
        for (int r = 0; r < 4; r++) if (r != col) { double f = a[r][col]; if (f != 0.0) for (int c = 0; c < 8; c++) a[r][c] -= f * a[col][c]; }
    }
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) out[4 * r + c] = a[r][4 + c];
    return true;
}

// mvp [6,4,4] HOST, row-vector convention.  With Minv = inverse(mvp) (rows r0..r3): eye_h = r2 (the pre-image of clip
// (0,0,1,0)), and for a pixel at ndc (x,y) the world point at ANY depth z is X_h = x r0 + y r1 + z r2 + r3, so
//   dir(x,y) = X_h.xyz - eye * X_h.w = x A0 + y A1 + A3,   Ak = rk.xyz - eye * rk.w     (the z term cancels exactly).
// Evaluated in double on the host: in float32 X_h.w suffers catastrophic cancellation for n = 1e-4, f = 100.
// One face's basis from its mvp; false where the camera has none: a singular mvp, or an affine one (r2.w == 0: no eye, e.g. an orthographic projection).
bool face_basis(const float* mvp16, FaceBasis& fb)
{
    double m[16], mi[16];
    for (int k = 0; k < 16; k++) m[k] = (double)mvp16[k];
    if (!invert4(m, mi)) return false;
    const double* r0 = mi, *r1 = mi + 4, *r2 = mi + 8, *r3 = mi + 12;
    if (r2[3] == 0.0) return false;                              // not a perspective camera
    double eye[3] = {r2[0] / r2[3], r2[1] / r2[3], r2[2] / r2[3]};
    double wfar = r2[3] + r3[3];                                 // X_h.w of the face centre on the far plane
    double sgn = wfar < 0.0 ? -1.0 : 1.0;
    for (int k = 0; k < 3; k++) {
        fb.eye[k] = (float)eye[k];
        fb.dx[k] = (float)(sgn * (r0[k] - eye[k] * r0[3]));
        fb.dy[k] = (float)(sgn * (r1[k] - eye[k] * r1[3]));
        fb.d0[k] = (float)(sgn * (r3[k] - eye[k] * r3[3]));
    }
    // normalise the scale of the basis (direction length is irrelevant; keeps t in sane float range)
    double len = sqrt((double)fb.d0[0] * fb.d0[0] + (double)fb.d0[1] * fb.d0[1] + (double)fb.d0[2] * fb.d0[2]);
    if (len > 0.0) for (int k = 0; k < 3; k++) { fb.d0[k] = (float)(fb.d0[k] / len); fb.dx[k] = (float)(fb.dx[k] / len); fb.dy[k] = (float)(fb.dy[k] / len); }
    return true;
}

// the caller's argument check: every face of mvp [6,4,4] HOST has a basis
bool gbuffer_mvp_ok(const float* mvp_host)
{
    FaceBasis fb;
    for (int f = 0; f < 6; f++) if (!face_basis(mvp_host + 16 * f, fb)) return false;
    return true;
}

hipError_t launch_gbuffer(const SceneDev& sc, const float* mvp_host, const float4* cnrm, int c, int flip_v, float* pos, float* nrm, float* mask,
                          float* uv, float* uvda, int32_t* tri, hipStream_t st)
{
    GbufArgs g;
    for (int f = 0; f < 6; f++) if (!face_basis(mvp_host + 16 * f, g.face[f])) return hipErrorInvalidValue;
    g.cnrm = cnrm; g.c = c; g.flip_v = flip_v; g.pos = pos; g.nrm = nrm; g.mask = mask; g.uv = uv; g.uvda = uvda; g.tri = tri;
    const dim3 grid(grid_capped(kBlock, (int64_t)6 * c * c));
    if (sc.nodes4) hipLaunchKernelGGL(gbuffer_kernel<4>, grid, dim3(kBlock), 0, st, sc, g);
    else hipLaunchKernelGGL(gbuffer_kernel<2>, grid, dim3(kBlock), 0, st, sc, g);
    return hipGetLastError();
}

}  // namespace texir

// One GGX sample of a material pixel, shared by the specular kernels (kernels.hip spec_kernel) and the inserted lights' specular pass (speclight.hip):
// forward-mode dual numbers carry d/d(roughness) through the whole sample chain.  A caller that reads the value alone leaves the derivative dead.
#pragma once
#include <hip/hip_runtime.h>

#include "device_common.h"

namespace texir {

#pragma clang fp contract(off)
struct Dual { float v, d; };
__device__ __forceinline__ Dual dmul(Dual a, Dual b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
__device__ __forceinline__ Dual dadd(Dual a, Dual b) { return {a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ Dual dsub(Dual a, Dual b) { return {a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ Dual ddiv(Dual a, Dual b) { float q = a.v / b.v; return {q, (a.d - q * b.d) / b.v}; }
__device__ __forceinline__ Dual dconst(float c) { return {c, 0.f}; }
__device__ __forceinline__ Dual dscale(Dual a, float s) { return {a.v * s, a.d * s}; }
__device__ __forceinline__ Dual dsqrt(Dual a) { float s = sqrtf(a.v); return {s, a.d / (2.f * s)}; }
// torch.clamp backward: gradient passes where min <= x <= max (inclusive)
__device__ __forceinline__ Dual dclamp(Dual a, float lo, float hi) { return {fminf(fmaxf(a.v, lo), hi), (a.v >= lo && a.v <= hi) ? a.d : 0.f}; }
__device__ __forceinline__ Dual dclamp_min(Dual a, float lo) { return {fmaxf(a.v, lo), a.v >= lo ? a.d : 0.f}; }

struct SpecSample { Dual w; float l[3]; };

// one GGX sample of pixel (n, v, r): returns the reflected direction l and the estimator weight w (+dw/dr).  hv (nullable): also the sampled half vector
// h[0..2] and the clamped v.h in hv[3], the values the chain itself used
__device__ __forceinline__ SpecSample spec_sample(const Frame& f, float nx, float ny, float nz, float vx, float vy, float vz,
                                                  float r, float s0, float s1, float ceps, float* hv = nullptr)
{
    // generate_dir importance branch (sample_util.py:133-143)
    Dual rr = {r, 1.f};
    Dual a = dmul(rr, rr);
    Dual den = dadd(dconst(1.0f), dscale(dsub(dmul(a, a), dconst(1.f)), s0));
    Dual ct = dsqrt(ddiv(dconst(1.0f - s0), den));
    ct = dclamp(ct, -1.0f + 1e-6f, 1.0f - 1e-6f);
    Dual st = dsqrt(dsub(dconst(1.0f), dmul(ct, ct)));
    st = dclamp(st, -1.0f + 1e-6f, 1.0f - 1e-6f);
    float phi = 6.283185307179586f * s1 - 3.141592653589793f;
    float sphi, cphi;
    sincosf(phi, &sphi, &cphi);
    Dual sp = dscale(st, sphi);
    Dual cp = dscale(st, cphi); cp.v = -cp.v; cp.d = -cp.d;
    Dual h[3];
    for (int k = 0; k < 3; k++) h[k] = dadd(dadd(dscale(sp, f.V[k]), dscale(ct, f.n[k])), dscale(cp, f.U[k]));
    // render (mat_nvdiffrast.py:235-236) and specular_reflectance (:262-279); dots use the RAW normal
    Dual vdh = dclamp(dadd(dadd(dscale(h[0], vx), dscale(h[1], vy)), dscale(h[2], vz)), 0.f, 1.f);
    Dual l[3];
    const float vv[3] = {vx, vy, vz};
    for (int k = 0; k < 3; k++) l[k] = dsub(dscale(dmul(vdh, h[k]), 2.f), dconst(vv[k]));
    Dual ndl = dclamp(dadd(dadd(dscale(l[0], nx), dscale(l[1], ny)), dscale(l[2], nz)), 0.f, 1.f);
    Dual ndh = dclamp(dadd(dadd(dscale(h[0], nx), dscale(h[1], ny)), dscale(h[2], nz)), 0.f, 1.f);
    float ndv = fminf(fmaxf(nx * vx + ny * vy + nz * vz, 0.f), 1.f);
    // f = 0.04 + 0.96 * 2^((-5.55472*vdh - 6.98316)*vdh)
    Dual e = dmul(dsub(dscale(vdh, -5.55472f), dconst(6.98316f)), vdh);
    float p2 = exp2f(e.v);
    Dual fr = {0.04f + 0.96f * p2, 0.96f * p2 * 0.6931471805599453f * e.d};
    Dual kk = dscale(dmul(dadd(rr, dconst(1.f)), dadd(rr, dconst(1.f))), 0.125f);
    Dual omk = dsub(dconst(1.f), kk);
    Dual g1v = ddiv(dconst(ndv), dclamp_min(dadd(dscale(omk, ndv), kk), ceps));
    Dual g1l = ddiv(ndl, dclamp_min(dadd(dmul(ndl, omk), kk), ceps));
    Dual g = dmul(g1l, g1v);
    Dual brdf = ddiv(dmul(fr, g), dclamp_min(dscale(ndl, 4.f * ndv), ceps));
    Dual w = ddiv(dmul(dscale(dmul(brdf, ndl), 4.f), vdh), dclamp_min(ndh, ceps));
    SpecSample o;
    o.w = w;
    for (int k = 0; k < 3; k++) o.l[k] = l[k].v;
    if (hv) { hv[0] = h[0].v; hv[1] = h[1].v; hv[2] = h[2].v; hv[3] = vdh.v; }
    return o;
}
#pragma clang fp contract(fast)

}  // namespace texir

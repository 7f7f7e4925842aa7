// launchers of the gfx950 kernels (kernels.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"
#include "launch_util.h"

namespace texir {
hipError_t launch_irt(const SceneDev& sc, const float* pos, const float* nrm, const float* shift, const int32_t* ids, int64_t n_ids,
                      int N, int mode, float* irr, unsigned long long* stats, unsigned long long* work /*dev: 8 * kWorkStride chunk counters of this launch*/,
                      hipStream_t st, float* scratch = nullptr /*dev: caller-owned partial-sum scratch of >= irt_scratch_bytes(), else stream-ordered*/);
size_t irt_scratch_bytes(const SceneDev& sc, int64_t n_ids, int N);      // bytes of partial-sum scratch one launch_irt call over n_ids listed texels needs (0: none)
constexpr int kWorkStride = 16;              // unsigned long longs between the per-XCD chunk counters of one launch (a 128-byte line each)
hipError_t irt_probe_node_utilisation(const SceneDev& sc, const float* pos, const float* nrm, const float* shift, const int32_t* ids, int64_t first, int64_t count,
                                      int N, int mode, unsigned long long* work, hipStream_t st, double* util);
// out[q][t] of K planes of Nt texels = irt_scale of the listed texels' part sums partial[part][q][k][3], added in part order (K = 1: Nt is not used)
hipError_t launch_irt_combine(const float* partial, const int32_t* ids /*nullable*/, int64_t n_ids, int64_t Nt, int K, int parts, int N, float two, float* out, hipStream_t st);
// `name`: the kernel FORM (what every mode of a call shape shares); `fixed` / `variant`: whether launch_irt runs the form's fixed instantiation for this
// `mode` (sampling mode, kEstimatorCosine or-ed in), and the instantiation's full name
struct IrtPlan { int per_wave, log2parts, width; bool fixed; char name[64]; char variant[96]; };
IrtPlan irt_plan(const SceneDev& sc, int64_t n_ids, int N, int mode = 0);      // the kernel launch_irt picks for this call
hipError_t launch_prefetch(const void* p, size_t bytes, int blocks, uint32_t* sink, hipStream_t st);
size_t tex_retile_bytes(int Ht, int Wt, int layout, int* tiles_x, int* tiles_y);
hipError_t launch_tex_retile(const float* src_row_major, float* dst, int Ht, int Wt, int layout, hipStream_t st);
size_t tex_pack_bytes(int Ht, int Wt, int layout, int* tiles_x, int* tiles_y);          // layouts 3, 4 (4-byte shared-exponent texels)
hipError_t launch_tex_pack(const float* src_row_major, uint32_t* dst, int Ht, int Wt, int layout, unsigned int* bad /*dev: texels that do not pack exactly*/, hipStream_t st);
hipError_t launch_trace_shade(const SceneDev& sc, const float* org, const float* dir, int64_t R, float t_min, float* rad, float* t_hit,
                              uint32_t* prim, float* puv, hipStream_t st);
hipError_t launch_gen_dir(const float* normals, const float* rough, const float* shift, int64_t b, int N, int mode, float* L, hipStream_t st);
hipError_t launch_spec_fwd(const SceneDev& sc, const float* normal, const float* albedo, const float* rough, const float* points,
                           const float* irr, const float* cam, const float* shift, int64_t P, int S, float clamp_eps, int ls_given, float* rgb, float* Ls_ws,
                           hipStream_t st, float* dw_ws = nullptr /*dev [P,S], nullable: d w_i / d roughness for launch_spec_bwd_ws*/);
hipError_t launch_spec_bwd_ws(const float* irr, const float* Ls_ws, const float* dw_ws, const float* d_rgb, int64_t P, int S, float* d_albedo, float* d_rough,
                              hipStream_t st);
hipError_t launch_spec_bwd(const float* normal, const float* rough, const float* points, const float* irr, const float* cam,
                           const float* shift, const float* Ls_ws, const float* d_rgb, int64_t P, int S, float clamp_eps, float* d_albedo, float* d_rough,
                           hipStream_t st);
size_t loss_workspace_bytes(int64_t P, int C, int R);
hipError_t launch_loss(int stage, int l2, const float* gt, const float* rgb, const float* albedo, const float* rough, const float* rough_womip,
                       const float* empty, const float* gtm, const uint8_t* seg, const uint8_t* hl, const uint8_t* room, int64_t P, int C, int R,
                       int hw, void* workspace, float* out, float* d_rgb, float* d_albedo, float* d_rough, hipStream_t st);
// gbuffer.hip: the cube G-buffer by primary-ray casting; gbuffermesh.hip: the same rays with inserted mesh instances in the view
struct FaceBasis { float eye[3], d0[3], dx[3], dy[3]; };   // dir(ndc x, y) = d0 + x*dx + y*dy, from `eye`
struct GbufArgs {
    FaceBasis face[6];
    const float4* cnrm;     // leaf-ordered corner normals, 3 x float4 per triangle (may be null -> geometric normal)
    int c; int flip_v;
    float *pos, *nrm, *mask, *uv, *uvda; int32_t* tri;
};
bool face_basis(const float* mvp16, FaceBasis& fb);      // one face's basis from its mvp; false where the camera has none (singular or affine)
bool gbuffer_mvp_ok(const float* mvp_host);      // every face of mvp [6,4,4] has an eye: not singular, not affine
hipError_t launch_gbuffer(const SceneDev& sc, const float* mvp_host, const float4* cnrm, int c, int flip_v, float* pos, float* nrm, float* mask,
                          float* uv, float* uvda, int32_t* tri, hipStream_t st);
int mip_levels(int H, int W, int max_mip_level);
int64_t mip_total_elems(int H, int W, int C, int levels);
hipError_t launch_mip_build(const float* tex, float* rest, int H, int W, int C, int levels, int from_level, hipStream_t st);
hipError_t launch_tex_fetch_bwd(float* d_tex, float* grad_rest, int H, int W, int C, int levels, const float* uv, const float* uvda, int trilinear,
                                int64_t P, const float* d_out, int fold_to_level, hipStream_t st);
hipError_t launch_tex_taps(int H, int W, int C, int levels, const float* uv, const float* uvda, int trilinear, int64_t P, long long* keys,
                           float* weights, hipStream_t st);
hipError_t launch_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, int step,
                       float lo, float hi, const float* hyper /*dev, nullable*/, hipStream_t st);
hipError_t launch_adam_tick(double* state, float* hyper, int n, unsigned long long mask, hipStream_t st);
// on the job structures of include/texir_hip.h (validated): one texture, then the batched forms -- n >= 1 jobs, one launch per kind of kernel
hipError_t launch_tex_fetch(const texir_tex_fetch_job& q, hipStream_t st);
hipError_t launch_tex_gather_bwd(const texir_tex_gather_job& q, hipStream_t st);
hipError_t launch_adam_tex(const texir_adam_tex_job& q, float lr /*lr, step: used when q.hyper is null*/, int step, hipStream_t st);
hipError_t launch_tex_fetch_batch(const texir_tex_fetch_job* jobs, int n, hipStream_t st);
hipError_t launch_tex_gather_bwd_batch(const texir_tex_gather_job* jobs, int n, hipStream_t st);
hipError_t launch_adam_tex_batch(const texir_adam_tex_job* jobs, int n, hipStream_t st);
hipError_t launch_grad_add_masked(float* g, const float* g0, const uint32_t* mask, int64_t n_texels, int C, hipStream_t st);
// texpost.hip: the pad + denoise step between the two stages (tools/padding_texture.py:49-87)
size_t texpost_pad_workspace_bytes(int H, int W);
hipError_t launch_texture_pad(const float* img, int H, int W, int C, const int32_t* row_map, const int32_t* col_map, float* out, int32_t* src, void* workspace,
                              hipStream_t st);
hipError_t launch_texture_denoise(const float* img, int H, int W, const float* nrm, const float* pos, int iterations, float sigma_c, float sigma_n, float sigma_p,
                                  float* tmp, float* out, hipStream_t st);
// texraster.hip: the texel G-buffer as a uv-space rasterisation of the mesh (tracer_o3d_irt.py:99-142)
size_t texel_raster_workspace_bytes(int64_t n_slots, int64_t T, int H, int W);
hipError_t launch_texel_raster(const SceneDev& sc, const float4* cnrm /*nullable unless shading*/, int64_t n_slots, int64_t T, int H, int W, int shading, float offset,
                               float* pos, float* nrm, uint32_t* prim_id /*nullable*/, float* bary /*nullable*/, void* workspace, hipStream_t st);
// texbake.hip: the radiance atlas and the index texture from calibrated panoramas (tools/trans_hdr_tex.py:16-61 gathers through the codes this selects)
hipError_t launch_atlas_bake(const SceneDev& sc, const float* pos, const float* nrm, const int32_t* ids /*nullable: all Nt*/, int64_t n, int64_t Nt, const float* cams,
                             const float* cam_pos, const float* panos, const uint8_t* valid /*nullable*/, int K, int h, int w, float cos_min, int32_t* view, int32_t* pix,
                             float* rgb, unsigned long long* stats /*nullable*/, hipStream_t st, bool any = false /*the segment test as an any-hit query: same bits*/);
hipError_t launch_atlas_gather(const int32_t* view, const int32_t* pix, const int32_t* ids /*nullable: all Nt*/, int64_t n, int64_t Nt, const float* imgs, int K, int h,
                               int w, int C, float* out, hipStream_t st);
// texfill.hip: unobserved texels of a baked atlas from the nearest observed texel in world space whose normal agrees (exact grid search)
int64_t atlas_fill_cell_cap(int64_t n_src);
size_t atlas_fill_workspace_bytes(int64_t n_src, int64_t n_holes);
float atlas_fill_cell(const float bounds[6], int64_t n_src, float cell);        // the cell edge a call with these arguments searches with
hipError_t launch_atlas_fill(const float* pos, const float* nrm, int64_t Nt, const int32_t* source_ids, int64_t n_src, const int32_t* hole_ids, int64_t n_holes,
                             const float bounds[6] /*host*/, float cos_fill, float max_dist, float cell, int32_t* src, float* dist2 /*nullable*/,
                             unsigned long long* stats /*nullable*/, void* workspace, hipStream_t st);
// irtsplit.hip: per-class IrT in one traced pass (the 64-texel plan of irt_group_kernel; needs the 4-wide tree)
size_t irt_split_workspace_bytes(int64_t n_ids, int N, int K);       // 0 for arguments the launch would refuse
hipError_t launch_irt_split(const SceneDev& sc, const float* tex_row_major, const uint8_t* labels, const float* pos, const float* nrm, const float* shift,
                            const int32_t* ids /*nullable: all Nt*/, int64_t n_ids, int64_t Nt, int N, int mode, int K, int unit, float* out /*[K][Nt][3]*/,
                            float* partial /*>= irt_split_workspace_bytes()*/, hipStream_t st);
// irtmulti.hip: the IrT estimator on K caller-owned textures in one traced pass (the same plan; needs the 4-wide tree)
size_t irt_multi_workspace_bytes(int64_t n_ids, int N, int K);       // 0 for arguments the launch would refuse
hipError_t launch_irt_multi(const SceneDev& sc, const float* tex /*dev [Ht][Wt][K][3]*/, const float* pos, const float* nrm, const float* shift,
                            const int32_t* ids /*nullable: all Nt*/, int64_t n_ids, int64_t Nt, int N, int mode, int K, float* out /*[K][Nt][3]*/,
                            float* partial /*>= irt_multi_workspace_bytes()*/, hipStream_t st);
// irtshadow.hip: what the bodies of inserted emitters (the records of launch_irt_lights) take from the captured light, per set of bodies (the same plan; 4-wide tree)
size_t irt_shadow_workspace_bytes(int64_t n_ids, int N, int M);      // 0 for arguments the launch would refuse
hipError_t launch_irt_shadow(const SceneDev& sc, const float* pos, const float* nrm, const float* shift, const int32_t* ids /*nullable: all Nt*/, int64_t n_ids, int64_t Nt,
                             int N, int mode, const float* bodies /*dev [K][16]*/, int K, const uint32_t* sets /*dev [M]*/, int M, float* out /*[M][Nt][3]*/,
                             unsigned long long* stats /*nullable*/, float* partial /*>= irt_shadow_workspace_bytes()*/, hipStream_t st);
// irtshadowmesh.hip: what inserted triangle-mesh objects take from the captured light, per set of instances (the same plan; 4-wide trees).  The geometry of
// the instances' occluders and their object-space boxes travel BY VALUE in the kernel arguments, per instance (the host resolves instance -> occluder)
struct MeshOccluders {
    const float4* nodes4[8];
    const float4* nodes4f[8];
    const float4* quads[8];
    float box[8][6];             // (lo.x, lo.y, lo.z, hi.x, hi.y, hi.z) of the occluder's vertices, object space
};
// instance j of a call shows the occluder with this geometry and this object-space box (the host resolves instance -> occluder)
inline void mesh_occluder_set(MeshOccluders& occ, int j, const SceneDev& dev, const float bounds[6])
{
    occ.nodes4[j] = dev.nodes4; occ.nodes4f[j] = dev.nodes4f; occ.quads[j] = dev.quads;
    for (int a = 0; a < 6; a++) occ.box[j][a] = bounds[a];
}
size_t irt_shadow_mesh_workspace_bytes(int64_t n_ids, int N, int M);      // 0 for arguments the launch would refuse
hipError_t launch_irt_shadow_mesh(const SceneDev& sc, const float* pos, const float* nrm, const float* shift, const int32_t* ids /*nullable: all Nt*/, int64_t n_ids,
                                  int64_t Nt, int N, int mode, const MeshOccluders& occ, const float* world_to_obj /*dev [K][12]*/, int K, const uint32_t* sets /*dev [M]*/,
                                  int M, bool prefilter, float* out /*[M][Nt][3]*/, unsigned long long* stats /*nullable, [3]*/,
                                  float* partial /*>= irt_shadow_mesh_workspace_bytes()*/, hipStream_t st);
// irtlight.hip: direct irradiance factors of inserted area lights (quads, spheres) per listed texel, one closest-hit (any = true: any-hit, same bits) query per sample
hipError_t launch_irt_lights(const SceneDev& sc, const float* pos, const float* nrm, const float* shift, const int32_t* ids /*nullable: all Nt*/, int64_t n, int64_t Nt,
                             const float* lights /*dev [K][16]*/, int K, int S, float t_max, float* F /*[K][Nt]*/, unsigned long long* stats /*nullable*/, hipStream_t st,
                             bool any = false);
// speclight.hip: the specular (GGX) response factors of inserted area lights per listed pixel, balance-heuristic MIS over the light's area and the lobe
hipError_t launch_spec_lights(const SceneDev& sc, const float* pos, const float* nrm, const float* rough, const float* shift, const float* cam /*dev [3]*/,
                              const int32_t* ids /*nullable: all P*/, int64_t n, int64_t P, const float* lights /*dev [K][16]*/, int K, int S, float t_max, float ceps,
                              float* R /*[K][P]*/, unsigned long long* stats /*nullable*/, hipStream_t st, bool any = false);
// irtlightmesh.hip, speclightmesh.hip: the same factors with J inserted mesh instances in the way (every question an occlusion query; 4-wide trees)
hipError_t launch_irt_lights_mesh(const SceneDev& sc, const float* pos, const float* nrm, const float* shift, const int32_t* ids /*nullable: all Nt*/, int64_t n,
                                  int64_t Nt, const float* lights /*dev [K][16]*/, int K, int S, float t_max, const MeshOccluders& occ,
                                  const float* world_to_obj /*dev [J][12]*/, int J, bool prefilter, float* F /*[K][Nt]*/, unsigned long long* stats /*nullable*/,
                                  hipStream_t st);
hipError_t launch_spec_lights_mesh(const SceneDev& sc, const float* pos, const float* nrm, const float* rough, const float* shift, const float* cam /*dev [3]*/,
                                   const int32_t* ids /*nullable: all P*/, int64_t n, int64_t P, const float* lights /*dev [K][16]*/, int K, int S, float t_max,
                                   float ceps, const MeshOccluders& occ, const float* world_to_obj /*dev [J][12]*/, int J, bool prefilter, float* R /*[K][P]*/,
                                   unsigned long long* stats /*nullable*/, hipStream_t st);
// specshadow.hip: what the bodies of inserted emitters and J inserted mesh instances take from the SPECULAR term of the captured light, per set (bit k = body
// k, bit 8 + j = instance j) and listed pixel; spec_kernel's samples, lane assignment and reduction; no workspace (4-wide trees)
hipError_t launch_spec_shadow(const SceneDev& sc, const float* normal, const float* rough, const float* points, const float* cam /*dev [3]*/, const float* shift,
                              const int32_t* ids /*nullable: all P*/, int64_t n, int64_t P, int S, float ceps, const float* bodies /*dev [Kb][16]*/, int Kb,
                              const MeshOccluders& occ, const float* world_to_obj /*dev [J][12]*/, int J, const uint32_t* sets /*dev [M]*/, int M, bool prefilter,
                              float* out /*[M][P][3]*/, unsigned long long* stats /*nullable, [3]*/, hipStream_t st);
// gbuffermesh.hip: the cube G-buffer with J inserted mesh instances in the view -- per pixel the nearest of the scene and the instances (4-wide trees).
// The hit shading reads the occluder's triangle records, which MeshOccluders does not carry: the kernel has a struct of its own
struct GbufMeshOccluders {
    MeshOccluders occ;
    const float4* tris[8];       // instance j: the occluder's GpuTri records by leaf-order slot (corners, primitive id)
};
hipError_t launch_gbuffer_mesh(const SceneDev& sc, const float* mvp_host, const float4* cnrm, int c, int flip_v, const GbufMeshOccluders& mo,
                               const float* world_to_obj /*dev [J][12]*/, int J, bool prefilter, float* pos, float* nrm, float* mask, float* uv, float* uvda,
                               int32_t* tri, int32_t* inst /*[6 c c]*/, hipStream_t st);
// occlusion.hip: is anything in the way inside (t_near, t_far)?  One any-hit query per ray (Open3D RaycastingScene.test_occlusions)
hipError_t launch_trace_occluded(const SceneDev& sc, const float* org, const float* dir, int64_t R, float t_near, float t_far, uint8_t* occluded,
                                 unsigned long long* stats /*nullable*/, hipStream_t st);
}  // namespace texir

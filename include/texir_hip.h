/*
 * texir_hip.h -- C-ABI of libtexir_hip.so: the MI355X (gfx950) implementation of TexIR's
 * irradiance-texture + material-estimation hot path.
 *
 * The reference (LZleejean/TexIR_code) is pure Python and has no FFI of its own; its seams
 * on this path are Python-level.  Each entry point below replaces one of those
 * seams and cites it.  A reference maintainer binds them with ctypes (INTEGRATION.md shows the
 * stubs).  Conventions:
 *   - every function returns 0 on success, <0 on error; texir_last_error() gives the
 *     thread-local message.  Nothing falls back to a CPU path.
 *   - `const float* x /+dev+/` pointers are caller-owned, contiguous DEVICE pointers
 *     (tensor.data_ptr()); host pointers are marked /+host+/.
 *   - launches are asynchronous on the hipStream_t passed as `stream` (void*; 0 = null stream).
 *   - a texir_scene is immutable after creation (except texir_scene_set_texture) and may be
 *     shared by host threads; one handle per device.
 */
#ifndef TEXIR_HIP_H
#define TEXIR_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TEXIR_OK 0
#define TEXIR_ERR_INVALID (-1)
#define TEXIR_ERR_HIP (-2)
#define TEXIR_ERR_NOMEM (-3)

/* sampling modes of utils/sample_util.py:115-143 */
#define TEXIR_MODE_UNIFORM 0
#define TEXIR_MODE_COSINE 1
#define TEXIR_MODE_IMPORTANCE 2

#if defined(__GNUC__)
#define TEXIR_API __attribute__((visibility("default")))
#else
#define TEXIR_API
#endif

typedef struct texir_scene texir_scene;

TEXIR_API const char* texir_last_error(void);
TEXIR_API int texir_version(void);
/* The library's run-time switches (TEXIR_* environment variables, csrc/env.h) are parsed once when the library is loaded; this re-reads them
 * (for test suites that flip a switch between two launches; not to be called while launches are being issued from other threads). */
TEXIR_API int texir_reload_env(void);
/* the value the library's snapshot holds for one switch, by variable name ("TEXIR_MIP_PER_LEVEL" ...): host code that must agree with the library
 * on a switch asks the library instead of parsing the environment a second time with its own rule. */
TEXIR_API int texir_env_switch(const char* name, int32_t* value);

/* Replaces TracerO3d.__init__ scene part (models/tracer_o3d_irt.py:75-89) and MaterialModel.__init__
 * (models/mat_nvdiffrast.py:87-101): o3d.t.geometry.RaycastingScene().add_triangles(mesh) + the CPU-resident
 * radiance texture.  Builds the BVH on the host and uploads it.
 *   verts   [V,3]  f32 host      tris [T,3] i32 host (primitive id = row index, as in Open3D)
 *   tri_uvs [3T,2] f32 host      per-corner uvs = np.asarray(trianglemesh.triangle_uvs)
 *   hdr_tex [Ht,Wt,3] f32 host   ALREADY BGR->RGB, vertically flipped and scaled by 2^hdr_exposure exactly as
 *                                tracer_o3d_irt.py:77-81 does. */
TEXIR_API int texir_scene_create(const float* verts /*host*/, int32_t V, const int32_t* tris /*host*/, int32_t T,
                       const float* tri_uvs /*host*/, const float* hdr_tex /*host*/, int32_t Ht, int32_t Wt,
                       int32_t device, texir_scene** out);
TEXIR_API int texir_scene_destroy(texir_scene* scene);

/* Replaces the temporary `self.texture = torch.where(intensity>=0.5, ...)` swap of stage -1
 * (models/mat_nvdiffrast.py:141-150).  tex [Ht,Wt,3] f32; is_device selects pointer kind. */
TEXIR_API int texir_scene_set_texture(texir_scene* scene, const float* tex, int32_t Ht, int32_t Wt, int32_t is_device, void* stream);
/* The hit shader's copy of the radiance texture (`self.texture`, models/tracer_o3d_irt.py:77-81: an RGBE file times 2^hdr_exposure).  When EVERY
 * texel is three 8-bit integers times one power of two -- always true of such a texture -- it is kept as 4-byte shared-exponent texels that decode
 * to the identical float32 values (layout 3: 5x5-texel lines at stride 4; 4: 8x4 at stride 7x3); any other texture keeps float32 tiles (2; 1 / 0 are the
 * older A/B layouts).  Decided at texir_scene_create and again at every texir_scene_set_texture (which then synchronises `stream` once to read the
 * pack kernel's verdict; on a capturing stream the float32 layout is taken).  Results are bit-identical in every layout. */
TEXIR_API int texir_scene_texture_layout(const texir_scene* scene, int32_t* layout);
/* The axis-aligned box of the vertices the scene's triangles name, out /+host+/ = (lo.x, lo.y, lo.z, hi.x, hi.y, hi.z): exact float32 minima and maxima of
 * the coordinates texir_scene_create was given (what texir_irt_shadow_mesh's prefilter pads). */
TEXIR_API int texir_scene_bounds(const texir_scene* scene, float out[6]);
/* Host statement of the 4-byte texel: word = m_r | m_g << 8 | m_b << 16 | E << 24, value_c = m_c * 2^(E - 127).  rgb /+host+/ [n,3] f32 ->
 * words /+host+/ [n], exact /+host+/ [n] (nullable; 1 where the triple has this form: non-negative, finite, normal, one shared power of two with
 * 8-bit integers -- e.g. any cv2-decoded RGBE pixel times 2^k; 0 -> the word is 0 and the device keeps float32 texels).  unpack is the decode. */
TEXIR_API int texir_texel_pack(const float* rgb, int64_t n, uint32_t* words, uint8_t* exact);
TEXIR_API int texir_texel_unpack(const uint32_t* words, int64_t n, float* rgb);

/* out[0]=inner nodes of the traversal tree (4-wide quantised by default), [1]=triangles, [2]=max depth, [3]=node bytes,
 * [4]=triangle bytes (leaf-order slots + the quad records the 4-wide leaves name), [5]=uv bytes, [6]=texture bytes, [7]=device */
TEXIR_API int texir_scene_info(const texir_scene* scene, int64_t out[8]);
/* The traversal's phase scheduler weighs the lanes at inner nodes against the lanes at leaves (csrc/device_common.h); the weight is a property of the
 * scene.  texir_scene_tune decides it ONCE per scene from the measured fullness of the scene's node steps on a sample of the caller's own texel
 * list (a counting launch over 16 384 listed texels, ~2 ms, BLOCKING: it synchronises `stream` and must not be called while the stream is being
 * captured); lists shorter than 65 536 texels or N < 256 decide nothing.  No other entry point measures or synchronises: texir_irt_generate,
 * texir_spec_forward, ... launch with the weight in force (2 until tuned) and can be recorded into a hipGraph from their first call on.  The
 * Python host layer calls it before the first long irt_generate of a scene (scene.Scene.irt_generate); the reference has no counterpart (Embree
 * picks its traversal internally, models/tracer_o3d_irt.py:243-244).  Speed only: results never depend on the weight.
 * texir_scene_scheduler: out[0] = the weight in use (0 = not decided -> 2), out[1] = measured fullness (-1 = not measured). */
TEXIR_API int texir_scene_tune(const texir_scene* scene, const float* pos /*dev*/, const float* nrm /*dev*/, const float* shift /*dev*/,
                               const int32_t* texel_ids /*dev*/, int64_t n_ids, int32_t N, int32_t mode, void* stream);
TEXIR_API int texir_scene_scheduler(const texir_scene* scene, double out[2]);
/* Streams the scene's traversal data through the memory hierarchy (what: bit 0 quantised nodes, 1 float nodes, 2 triangles, 3 corner uvs;
 * blocks = grid size, 0 -> 512): a cache warm-up to launch beside / before a latency-bound tracing kernel that follows a cache-flushing
 * stream (the material step's fused Adam).  No reference counterpart (a speed hint: results never depend on it). */
TEXIR_API int texir_scene_prefetch(const texir_scene* scene, int32_t what, int32_t blocks, void* stream);

/* Replaces query_irf (models/tracer_o3d_irt.py:240-269, models/mat_nvdiffrast.py:292-320):
 * closest hit (Embree semantics: t>0, t in units of |dir|), hit mask t>t_min (reference: 1e-4) & finite,
 * barycentric clip, corner-uv interpolation, bilinear/border/align_corners=False fetch of the radiance
 * texture, misses -> 0.   org,dir [R,3] dev -> radiance [R,3] dev.
 * Optional raw intersection outputs (the cast_rays dict, tracer_o3d_irt.py:245-251): t_hit [R] (inf on miss),
 * prim_id [R] (0xFFFFFFFF on miss), prim_uv [R,2] (weights of the CALLER's corners 1 and 2 of triangle prim_id, as Open3D's primitive_uvs: the library
 * stores a triangle's corners rotated where its leaf record wants the shared edge, csrc/bvh_build.h, and turns the barycentrics back here); pass NULL to skip. */
TEXIR_API int texir_trace_shade(const texir_scene* scene, const float* org /*dev*/, const float* dir /*dev*/, int64_t R,
                      float t_min, float* radiance /*dev*/, float* t_hit /*dev, nullable*/,
                      uint32_t* prim_id /*dev, nullable*/, float* prim_uv /*dev, nullable*/, void* stream);

/* ---- occlusion query, csrc/occlusion.hip.  Replaces Open3D's RaycastingScene.test_occlusions(rays, tnear, tfar), the sibling of the cast_rays that query_irf
 * calls (models/tracer_o3d_irt.py:240-269): is anything in the way of the ray inside (t_near, t_far)?
 *
 * THE RULE.  occluded[r] = 1 iff SOME triangle passes the leaf test of the closest-hit query for the ray (org[r], dir[r]) with t_near < t < t_far, else 0.
 * The leaf test is texir_trace_shade's, unchanged: the watertight accept (the vertices moved to the origin and sheared so that dir becomes +z, the three edge
 * functions with exact signs, zeros inside for both neighbours), det != 0, and t the float32 t that test computes, in units of |dir|.  t_near = 0 gives the
 * closest-hit query's own t > 0.  Both ends are open: a triangle at exactly t_far does not occlude.
 *   - At t_near = 0 the answer equals (t_hit < t_far) of texir_trace_shade's t_hit for the same ray, bit for bit, on every ray: the traversal starts with the
 *     far bound where closest hit starts with +inf and stops at the first accepted triangle; it relies on what the culling of the closest-hit traversal
 *     already relies on (a box's computed entry distance is never above the computed t of a triangle inside it), so it never skips a box that holds an
 *     accepted triangle with t < t_far.  tests/test_gpu_occlusion.py binds this equality on every ray of its cases.
 *   - t_far = NaN or t_far <= t_near: no t qualifies, every ray is "not occluded" and nothing is traced.  t_far = +inf is the whole ray.
 *   - A zero or non-finite direction is not occluded (closest hit gives a miss there too).
 * occluded[r] is a pure function of the scene, the ray and the two bounds: no atomics on results; launch shape and stream do not change a byte.
 *
 *   org, dir [R,3] dev;  t_near finite and >= 0;  occluded dev [R] u8: one byte per ray, every r < R is written, nothing beyond.
 *   stats dev u64[1], nullable: += the number of occluded rays; one atomic add per wave.
 * A negative R, a t_near that is negative or not finite and a null buffer are errors with a texir_last_error() text.  R = 0 returns 0 and writes nothing.
 * Caller-owned buffers, the caller's stream, no allocation and no synchronisation: the call records into a hipGraph. */
TEXIR_API int texir_trace_occluded(const texir_scene* scene, const float* org /*dev [R,3]*/, const float* dir /*dev [R,3]*/, int64_t R, float t_near, float t_far,
                         uint8_t* occluded /*dev [R]*/, uint64_t* stats /*dev [1], nullable*/, void* stream);

/* Replaces generate_dir (utils/sample_util.py:63-146) with pre_mode='Hammersley'.  The per-point random
 * shift (torch.rand(b,1,2) on the CPU generator, :102) is an INPUT so that parity is exact.
 *   normals [b,3] dev, roughness [b] dev (importance only, else NULL), shift [b,2] dev -> L [b,N,3] dev */
TEXIR_API int texir_generate_dir(const float* normals /*dev*/, const float* roughness /*dev, nullable*/,
                       const float* shift /*dev*/, int64_t b, int32_t N, int32_t mode, float* L /*dev*/, void* stream);

/* Replaces the hot loop of TracerO3d.forward (models/tracer_o3d_irt.py:156-178): for every listed texel
 *   E = (2*pi/N) * sum_i L(pos, d_i) * clamp(nrm . d_i, 0, 1),  d_i = generate_dir(nrm, N, mode)[i]
 * fused in one kernel (sample + trace + shade + reduce).
 *   pos,nrm [Nt,3] dev (pos already offset by +1e-2*n, :110), shift [Nt,2] dev
 *   texel_ids [n_ids] i32 dev: the texels to compute (NULL => all Nt, n_ids ignored).  Seam texels
 *     (index texture all-zero, :137-139,176-178) are simply not listed; irr must be zero-initialised by the caller.
 *     texel_ids == NULL means ALL Nt texels whatever n_ids says: a caller whose list can be empty (a rank's shard of a short list) must skip the call
 *     -- an empty device array has no address to pass (the Python wrapper does, scene.Scene.irt_generate).
 *   irr [Nt,3] dev: only listed texels are written.  A texel's value has a fixed summation order per kernel form, so for lists of
 *     >= 32768 texels (the 64-texels-per-wave form; shorter lists use the one-texel-per-wave form, which differs in the last bits) the texture does
 *     not depend on the order or sharding of texel_ids nor on the launch configuration.
 *   Long lists (>= 32768 texels) use a stream-ordered scratch allocation (hipMallocAsync/hipFreeAsync on `stream`,
 *     384 bytes per listed texel at N >= 2048) for the per-pass-range partial sums.
 *   stats [8] u64 dev, nullable: += rays, 64-byte node fetches, triangle tests, hits, wave-level node steps, wave-level
 *   triangle steps (how often a wavefront executed each loop body: lane utilisation = lane count / (64 * wave count)), [6] stack entries
 *   dropped by culling when they were popped (their entry distance was not below the closest hit by then; per lane), [7] pushes + pops that
 *   went through the private overflow part of the traversal stack (depth beyond the LDS part: 10 entries in the IrT kernels; per lane). */
TEXIR_API int texir_irt_generate(const texir_scene* scene, const float* pos /*dev*/, const float* nrm /*dev*/,
                       const float* shift /*dev*/, const int32_t* texel_ids /*dev, nullable*/, int64_t n_ids,
                       int64_t Nt, int32_t N, int32_t mode, float* irr /*dev*/, uint64_t* stats /*dev, nullable*/,
                       void* stream);

/* Recording texir_irt_generate into a hipGraph: a long list's partial-sum scratch cannot be allocated stream-ordered inside a recorded graph (ROCm 7.2:
 * some replays then read wrong partial sums), so a launch on a CAPTURING stream uses scratch reserved on the scene beforehand and fails with a clear
 * message if there is not enough: call this once, outside any capture, with the largest (n_ids, N) that will be recorded (384 bytes per listed texel at
 * N >= 2048; nothing for lists < 32 768 texels).  One recorded launch per scene at a time may be in flight (they share the scratch).  Eager launches are
 * unaffected.  No reference counterpart. */
TEXIR_API int texir_scene_reserve_scratch(texir_scene* scene, int64_t n_ids, int32_t N);

/* ---- irradiance split by source label (csrc/irtsplit.hip): where a texel's irradiance comes from, K classes in ONE traced pass.  Irradiance is linear in
 * the radiance texture, so the share class k's texels contribute -- the lamps, the floor, a window -- gives every recolouring, dimming or switching off
 * of that class as a weighted sum (the reference re-traces the diffuse term per view and per colour instead: models/test_nvdiffrast.py:268-274).
 *
 * THE RULE.  Inputs: everything texir_irt_generate takes; labels dev uint8 [Ht,Wt] in the orientation of the texture the scene holds (labels[y][x] is
 * the class of the texel the hit shader reads at row y, column x); K in 1..8; the flag `unit`.
 *   SAMPLES AND RAYS  directions, n.l, the ray, the acceptance test (slot >= 0 && t > 1e-4) and the closest hit are exactly those of
 *               irt_group_kernel<false, 4, 6>, texir_irt_generate's 64-texel form: one texel per lane, one sample per pass.
 *   SHADING     for a hit, x0, y0, x1, y1, w00, w10, w01, w11 are computed exactly as the hit shader computes them (bilinear / border /
 *               align_corners=False).  For class k and channel c, separately rounded float32 operations in this order:
 *                   L_k[c] = v00 w00;  L_k[c] += v10 w10;  L_k[c] += v01 w01;  L_k[c] += v11 w11
 *               v_ab = value(tap ab)[c] if labels[y_b][x_a] == k, else +0.0f.  With `unit`, value is 1.0f in all channels and the texture is not read.
 *               A label >= K belongs to no class.  This is the float32 expression the hit shader evaluates on a texture whose other-class texels are +0.
 *   REDUCTION   the documented 64-texel plan whatever the list length: acc_k += L_k ndl per lane over the passes of a part, in irt_group_kernel's pass
 *               order (azimuthal wedges); the parts are those of the 64-texel form -- a power-of-two N is cut into up to 32 parts of at least
 *               TEXIR_IRT_MIN_PART_CELLS (8) passes, capped by TEXIR_IRT_LOG2PARTS; any other N is one part in natural sample order -- and are added in
 *               part order; out[k][t][c] = ((a * 2) * pi) / N, as texir_irt_generate writes it.
 *   CONSEQUENCE out[k] is, bit for bit, what texir_irt_generate in its 64-texel form (TEXIR_IRT_TEXELS_PER_WAVE=64, or any list of >= 32 768 texels)
 *               writes for the same scene with the texture tex * [label == k]: the rays are the same, the products are the same, and adding +0 changes
 *               no float.  With `unit`, out[k] is what it writes for the indicator texture of class k.
 * The result is a pure function of the inputs: list order, list cuts, launch shape and stream do not change a bit.
 *   out [K][Nt][3] dev: only listed texels are written.  texel_ids NULL => all Nt (n_ids ignored); a non-null list with n_ids == 0 is a no-op.
 *   workspace: texir_irt_split_workspace_bytes(n_ids, N, K) bytes of device scratch (12 bytes x K x parts per listed texel: callers cut long lists into
 *   slices that are multiples of 64 texels -- scene.Scene.irt_split does; 0 is returned for arguments the call refuses).
 * Caller-owned buffers, the caller's stream, no allocation and no synchronisation: the call records into a hipGraph.  K outside 1..8, null labels,
 * N < 1, a workspace that is too small and a scene without the 4-wide tree (TEXIR_BVH_WIDTH=2) are errors with a texir_last_error() text. */
TEXIR_API int64_t texir_irt_split_workspace_bytes(int64_t n_ids, int32_t N, int32_t K);
TEXIR_API int texir_irt_split(const texir_scene* scene, const float* pos /*dev*/, const float* nrm /*dev*/, const float* shift /*dev*/,
                       const int32_t* texel_ids /*dev, nullable*/, int64_t n_ids, int64_t Nt, int32_t N, int32_t mode, const uint8_t* labels /*dev [Ht,Wt]*/,
                       int32_t K, int32_t unit, float* out /*dev [K][Nt][3]*/, void* workspace /*dev*/, int64_t workspace_bytes, void* stream);

/* ---- several radiance textures in one traced IrT pass (csrc/irtmulti.hip): the IrT estimator applied to K caller-owned textures instead of the one the
 * scene holds.  The light a texel throws back under an inserted emitter is a radiance texture of its own (albedo / pi * colour * F, irtlight.bounce_textures);
 * its irradiance elsewhere is this estimator on that texture -- without set_texture, without a re-tile and without tracing the identical rays once per light.
 *
 * THE RULE.  Inputs: everything texir_irt_generate takes; tex dev float32 [Ht][Wt][K][3], the K textures interleaved per texel, Ht x Wt the size and the
 * orientation of the texture the scene holds (tex[y][x][k] is what the hit shader would read at row y, column x of texture k; as `labels` of
 * texir_irt_split); K in 1..8.
 *   SAMPLES AND RAYS  directions, n.l from the raw normal, the ray, the acceptance test (slot >= 0 && t > 1e-4) and the closest hit are exactly those of
 *               irt_group_kernel<false, 4, 6>, texir_irt_generate's 64-texel form: one texel per lane, one sample per pass.
 *   SHADING     for a hit, x0, y0, x1, y1, w00, w10, w01, w11 are computed exactly as the hit shader computes them (bilinear / border /
 *               align_corners=False).  For texture k and channel c, separately rounded float32 operations in this order:
 *                   L_k[c] = v00 w00;  L_k[c] += v10 w10;  L_k[c] += v01 w01;  L_k[c] += v11 w11,     v_ab = tex[y_b][x_a][k][c]
 *               No select, no label.  Textures q >= K are not read (the buffer has none); the scene's own texture is not read at all.
 *   REDUCTION   the 64-texel plan of texir_irt_split under the same switches (TEXIR_IRT_MIN_PART_CELLS, TEXIR_IRT_LOG2PARTS): acc_k += L_k ndl per lane
 *               over the passes of a part, in irt_group_kernel's pass order; partial[part][k][i][3]; the parts are added in part order;
 *               out[k][t][c] = ((a * 2) * pi) / N.
 *   CONSEQUENCE out[k] is, bit for bit, what texir_irt_generate in its 64-texel form (TEXIR_IRT_TEXELS_PER_WAVE=64, or any list of >= 32 768 texels)
 *               writes for the same scene after texir_scene_set_texture(T_k), whatever layout that scene then picks: every layout holds the identical
 *               floats.  NaN, Inf and negative texels included -- there is nothing here but the same multiplications and additions.
 * The result is a pure function of the inputs: list order, list cuts, launch shape and stream do not change a bit.
 *   out [K][Nt][3] dev: only listed texels are written.  texel_ids NULL => all Nt (n_ids ignored); a non-null list with n_ids == 0 is a no-op.
 *   workspace: texir_irt_multi_workspace_bytes(n_ids, N, K) bytes of device scratch (12 bytes x K x parts per listed texel: callers cut long lists into
 *   slices that are multiples of 64 texels -- scene.Scene.irt_multi does; 0 is returned for arguments the call refuses).
 * Caller-owned buffers, the caller's stream, no allocation, no synchronisation, no atomics on results: the call records into a hipGraph, and a replay reads
 * whatever tex holds then.  K outside 1..8 (reported before any null buffer), null tex, N < 1, a workspace that is too small and a scene without the
 * 4-wide tree (TEXIR_BVH_WIDTH=2) are errors with a texir_last_error() text. */
TEXIR_API int64_t texir_irt_multi_workspace_bytes(int64_t n_ids, int32_t N, int32_t K);
TEXIR_API int texir_irt_multi(const texir_scene* scene, const float* pos /*dev*/, const float* nrm /*dev*/, const float* shift /*dev*/,
                       const int32_t* texel_ids /*dev, nullable*/, int64_t n_ids, int64_t Nt, int32_t N, int32_t mode, const float* tex /*dev [Ht][Wt][K][3]*/,
                       int32_t K, float* out /*dev [K][Nt][3]*/, void* workspace /*dev*/, int64_t workspace_bytes, void* stream);

/* ---- the shadow an inserted emitter's BODY casts on the captured light, per texel (csrc/irtshadow.hip).  texir_irt_lights, texir_spec_lights and
 * texir_irt_multi build the response to a NEW lamp; each of them only ever adds light.  This call gives the one term of a relit room with the other sign:
 * the part of a texel's captured irradiance that arrived along rays the lamp's body now intercepts.
 *
 * THE RULE.  Inputs: everything texir_irt_generate takes; bodies: K in 0..8 records of 16 float32 in DEVICE memory, the layout and the validity rule of
 * texir_irt_lights (a replayed graph sees moved bodies, so the host never validates a record); sets: M in 1..8 uint32 bit masks over the bodies in DEVICE
 * memory -- bit k = body k; {k} is the shadow of lamp k alone, all bits the shadow of all of them together; bits at or above K are ignored; a zero mask
 * yields zeros.
 *   SAMPLES AND RAYS  directions d, ndl = n.l from the RAW normal, the ray (org = x = pos, dir = d), the acceptance test (slot >= 0 && t > 1e-4) and the
 *               closest hit t_s are exactly those of irt_group_kernel<false, 4, 6>, texir_irt_generate's 64-texel form: one texel per lane, one sample
 *               per pass.  L_i is the radiance the hit shader reads from the scene's OWN texture, in whatever layout it holds it.
 *   BODIES      per sample, body k MEETS the ray at t_b (in units of |d|, as t_s is) under the rule below; B = the mask of bodies that meet it with
 *               t_b < t_s.  A ray that meets no body is not traced (its sample adds nothing whatever it hits); nothing is skipped on ndl.
 *   RESULT      lost[m] = (2 pi / N) sum_i L_i ndl_i [sample i has an accepted hit AND (sets[m] & B_i) != 0].  A set is evaluated from the per-ray mask:
 *               the shadows of overlapping bodies are a union, not a sum.  The relit irradiance is max(E - lost[m], 0) + sum_k colour_k (F[k] + G[k])
 *               (texir_code_amd/irtlight.py add).
 *   REDUCTION   the 64-texel plan of texir_irt_multi under the same switches (TEXIR_IRT_MIN_PART_CELLS, TEXIR_IRT_LOG2PARTS): acc_m += L ndl per lane
 *               over the passes of a part, in irt_group_kernel's pass order; partial[part][m][i][3]; the parts are added in part order;
 *               out[m][t][c] = ((a * 2) * pi) / N.
 *   CONSEQUENCE for a texel and a set under which EVERY sample with an accepted hit is blocked, lost[m] is, bit for bit, what texir_irt_generate in its
 *               64-texel form (TEXIR_IRT_TEXELS_PER_WAVE=64, or any list of >= 32 768 texels) writes: the same additions in the same order.  For a set no
 *               sample's ray meets, lost[m] is exactly +0.  The result is a pure function of the inputs: list order, duplicates, list cuts, launch
 *               shape, stream and graph replay change no bit.
 *
 * BODY INTERSECTION RULE, as a FLOAT32 OPERATION SEQUENCE (each operation separately rounded, no contraction; sqrt and / correctly rounded).
 *   record      valid as texir_irt_lights has it (kind 0.0f or 1.0f, finite words, a x b != 0 and finite, r > 0 and (fourpi32 r) r finite); a quad also needs
 *               mm (below) finite and > 0.  Any other record never blocks.
 *   QUAD, two-sided as an occluder (per record):
 *               m_x = a_y b_z - a_z b_y,  m_y = a_z b_x - a_x b_z,  m_z = a_x b_y - a_y b_x;   mm = (m_x m_x + m_y m_y) + m_z m_z
 *               ua = (b x m) / mm,  vb = (m x a) / mm,  each cross-product component p q - r s as for m, each quotient on its own (the reciprocal basis of
 *               csrc/speclight.hip: h = u a + v b  ->  u = h.ua, v = h.vb)
 *         (per sample):
 *               den = (m_x d_x + m_y d_y) + m_z d_z;   q_i = o_i - x_i;   num = (m_x q_x + m_y q_y) + m_z q_z;   t = num / den
 *               h_i = t * d_i - q_i;   u = (h_x ua_x + h_y ua_y) + h_z ua_z;   v = (h_x vb_x + h_y vb_y) + h_z vb_z
 *               it MEETS the ray iff den != 0, t is finite, t > 0, 0 <= u <= 1 and 0 <= v <= 1;   t_b = t      (either side: the sign of den is not asked)
 *   SPHERE, a solid ball:
 *               rr = r * r (per record);   oc_i = c_i - x_i;   b = (oc_x d_x + oc_y d_y) + oc_z d_z;   dd = (d_x d_x + d_y d_y) + d_z d_z
 *               cc = ((oc_x oc_x + oc_y oc_y) + oc_z oc_z) - rr;   disc = b * b - dd * cc;   s = b + sqrt(disc);   far = s / dd
 *               it MEETS the ray iff disc >= 0 and far > 0 (the far root);   t_b = 0 when cc <= 0 (the texel is inside the ball), else t_b = cc / s, the near
 *               root in its cancellation-free form
 *   BLOCKED     t_b < t_s, both float32.
 * ROUNDING BOUND (first order, u = 2^-24; x and the record are exact float32 values, d_i carries e_i per component; the tests multiply every bound by their
 * factor K).  What depends on x and the record alone -- m, mm, ua, vb, q, num of a quad; rr, oc, cc of a sphere -- uses IEEE products, sums and quotients of
 * exact float32 values only: a restatement on any IEEE machine gives the same bits, and the bounds below start from them as exact float32 values (as the
 * bounds of texir_irt_lights start from s0 and s1).  This is what keeps the near root cc / s sharp where b - sqrt(disc) would cancel.
 *     quad:    |dden| <= 3 u sum_i |m_i d_i| + sum_i |m_i| e_i;   |dt| <= |t| |dden| / |den| + u |t|;   the test t > 0 is decided unless |t| <= |dt|, and
 *              den != 0 unless |den| <= |dden|
 *              |dh_i| <= |d_i| |dt| + |t| e_i + u (|t d_i| + |h_i|)
 *              |du| <= 3 u sum_i |h_i ua_i| + sum_i |ua_i| |dh_i|,  v alike;   a cut of u or v at 0 or 1 is decided unless within |du|, |dv|
 *     sphere:  |db| <= 3 u sum_i |oc_i d_i| + sum_i |oc_i| e_i;   |ddd| <= 3 u dd + 2 sum_i |d_i| e_i
 *              |ddisc| <= 2 |b| |db| + u b b + |cc| |ddd| + u |dd cc| + u |disc|;   the test disc >= 0 is decided unless |disc| <= |ddisc|
 *              |dsq| <= min(|ddisc| / (2 sqrt(max(disc - |ddisc|, 0))), sqrt(|ddisc|)) + u sqrt(disc);   |ds| <= |db| + |dsq| + u |s|
 *              far > 0 has the sign of s (dd > 0): decided unless |s| <= |ds|;   |dt_b| <= |t_b| |ds| / |s| + u |t_b|;   the cut cc <= 0 is exact
 *     BLOCKED is decided unless |t_b - t_s| <= |dt_b| + bound(t_s), bound(t_s) the closest hit's own.
 *
 *   out [M][Nt][3] dev: only listed texels are written, zeros included (K = 0: zeros).  texel_ids NULL => all Nt (n_ids ignored); a non-null list with
 *   n_ids == 0 is a no-op.
 *   stats dev u64[2], nullable: += samples whose ray meets a body (the rays traced), and the blocked ones among them (an accepted hit behind a body, of
 *   any set or none); one atomic add per wave and counter.
 *   workspace: texir_irt_shadow_workspace_bytes(n_ids, N, M) bytes of device scratch (12 bytes x M x parts per listed texel: callers cut long lists into
 *   slices that are multiples of 64 texels -- scene.Scene.irt_shadow does; 0 is returned for arguments the call refuses).
 * Caller-owned buffers, the caller's stream, no allocation, no synchronisation, no atomics on results: the call records into a hipGraph, and a replay reads
 * whatever bodies and sets hold then.  K outside 0..8 or M outside 1..8 (reported before any null buffer), a null buffer, N < 1, a workspace that is too
 * small and a scene without the 4-wide tree (TEXIR_BVH_WIDTH=2) are errors with a texir_last_error() text.
 * Not computed here: bodies shadowing each other's direct light F[j] or the bounce G, the body drawn in a view, triangle-mesh occluders.  (The body's
 * shadow in the specular term of captured light: texir_spec_shadow.) */
TEXIR_API int64_t texir_irt_shadow_workspace_bytes(int64_t n_ids, int32_t N, int32_t M);
TEXIR_API int texir_irt_shadow(const texir_scene* scene, const float* pos /*dev*/, const float* nrm /*dev*/, const float* shift /*dev*/,
                       const int32_t* texel_ids /*dev, nullable*/, int64_t n_ids, int64_t Nt, int32_t N, int32_t mode, const float* bodies /*dev [K][16]*/,
                       int32_t K /*0..8*/, const uint32_t* sets /*dev [M]*/, int32_t M /*1..8*/, float* out /*dev [M][Nt][3]*/,
                       uint64_t* stats /*dev [2], nullable*/, void* workspace /*dev*/, int64_t workspace_bytes, void* stream);

/* ---- the shadow an inserted triangle-mesh OBJECT casts on the captured light, per texel (csrc/irtshadowmesh.hip): texir_irt_shadow with meshes in the place
 * of analytic bodies -- a chair, a table, a person placed into the captured room.
 *
 * THE RULE.  Inputs: everything texir_irt_generate takes, and
 *   occluders   Q in 0..8 scene handles (HOST array) used for their geometry only: build one with texir_scene_create, any uvs and a 1 x 1 texture.  Their
 *               device pointers and boxes enter the kernel arguments by value: fixed when the call is made or recorded.
 *   instances   K in 0..8: instance j = (inst_obj[j] in 0..Q-1, HOST; W[j] = inst_world_to_obj + 12 j, a WORLD-TO-OBJECT 3 x 4 row-major float32 matrix in
 *               DEVICE memory: a replayed graph sees a moved object, so the host never reads a matrix).  Two instances may name one occluder.
 *   sets        M in 1..8 uint32 bit masks over the instances in DEVICE memory, exactly as texir_irt_shadow's: bits at or above K are ignored, a zero mask
 *               yields zeros.
 *   SAMPLES AND RAYS  directions d, ndl from the RAW normal, the ray (x = pos, d), the closest hit t_s and its acceptance test (slot >= 0 && t > 1e-4) are
 *               those of irt_group_kernel<false, 4, 6>; L_i comes from the scene's OWN texture through the hit shader.
 *   OBJECT-SPACE RAY of instance j, a FLOAT32 OPERATION SEQUENCE (each operation separately rounded, no contraction), r = 0, 1, 2, W = W[j]:
 *               o'_r = ((W[r][0] x_0 + W[r][1] x_1) + W[r][2] x_2) + W[r][3]
 *               d'_r =  (W[r][0] d_0 + W[r][1] d_1) + W[r][2] d_2
 *               The ray is NOT normalised: an affine map keeps the ray parameter, t along (o', d') is t along (x, d).  A matrix with a non-finite entry
 *               never blocks.
 *   BLOCKED     sample i with an accepted scene hit at t_s is blocked by instance j iff the occluder's tree holds a triangle the closest-hit query's leaf test
 *               accepts with 0 < t < t_s along (o', d'), t the float32 t that test computes: texir_trace_occluded's rule at t_near = 0, t_far = t_s, which
 *               is the bit `closest hit of (o', d') in the occluder has t < t_s`.  B_i = the mask of instances that block sample i.
 *   RESULT      lost[m] = (2 pi / N) sum_i L_i ndl_i [sample i has an accepted hit AND (sets[m] & B_i) != 0]: overlapping instances are a union, not a sum.
 *   REDUCTION   texir_irt_shadow's: acc_m += L ndl per lane over the passes of a part in irt_group_kernel's pass order; partial[part][m][i][3]; parts (those
 *               of the 64-texel plan under TEXIR_IRT_MIN_PART_CELLS, TEXIR_IRT_LOG2PARTS) added in part order; out[m][t][c] = ((a * 2) * pi) / N.
 *   CONSEQUENCE where every accepted sample of a texel is blocked under set m, lost[m] is bit for bit texir_irt_generate's 64-texel form; where none is, it is
 *               exactly +0.  List order, duplicates, list cuts, launch shape, stream, graph replay and the prefilter (below) change no bit.
 * ROUNDING BOUND (first order, u = 2^-24; x and W are exact float32 values, d_i carries e_i per component; the tests multiply by their factor K).  o' uses IEEE
 * products and sums of exact float32 values only: a restatement on any IEEE machine gives the same bits, and the bound starts from o' as an exact value.
 *               |dd'_r| <= sum_c |W[r][c]| e_c + 3 u sum_c |W[r][c] d_c|
 *   The traversal then sees (o', d' +- dd'): a triangle's t carries the closest-hit query's own bound_t for that direction bound (tests/trace_cases.py), and
 *   BLOCKED is decided unless |t_o - t_s| <= bound_t(t_o) + bound_t(t_s) or the triangle is within its margin of the ray.
 *
 * PREFILTER.  A lane queries instance j only if (o', d') passes a test against the occluder's object-space box (texir_scene_bounds), a lane that passes for no
 * instance does not trace the scene either, and a pass no lane needs is skipped.  The test must never fail where the traversal accepts a triangle:
 *   what is to be covered.  The tree's boxes -- quantised or float, each padded OUTWARDS by the builder's slack -- only ever REJECT: the traversal accepts a subset
 *   of what the leaf test accepts over all triangles, so it suffices to cover the leaf test (device_common.h).  With kz the dominant axis of d', S = (d'_k1 rcp
 *   d'_kz, d'_k2 rcp d'_kz) (each at most 2.5 u off, |S| <= 1 + 3 u), q = fl(p - o') per corner p and X = fl(q_k1 - S_x q_kz), Y alike: the test accepts only if
 *   the 2D origin lies in the triangle (X, Y) -- signs exact (edge2_exact) -- and the computed t > 0.  (X, Y) is the EXACT shear along D = (S_x, S_y, 1) of corners
 *   moved by at most u |p - o'| (q) + 2.01 u |q| (X, Y) <= 3.1 u R per axis, R = max_corner |p - o'|_inf <= rb + |o'|_inf, rb = the box's largest |coordinate|.
 *   So the line o' + s D meets the moved triangle at some |s| <= (1 + 3.1 u) R, and the line o' + t d' passes within 3.1 u R + 2.6 u R < 6 u R of the true
 *   triangle, per axis.  The computed t is sum U_k Z_k / det with the U_k of one sign and Z_k = fl(rcp(d'_kz) q_k,kz): t > 0 needs some Z_k > 0, i.e. a corner
 *   with (p - o')_kz d'_kz > 0, the sign of a float32 difference being exact.  (The weights U_k may be badly off under cancellation, so nothing is claimed about
 *   WHERE along the line the hit lies.)
 *   the test.   P = 2^-18 (rb + |o'|_inf) + 1e-30 = 64 u R and more; box' = box padded by P (its roundings, and that of box' - o', at most 3 u R, are inside).
 *   (1) a zero or non-finite d' passes; (2) along kz -- picked by the traversal's own comparisons -- the far plane must lie strictly ahead: d'_kz > 0 ?
 *   hi'_kz > o'_kz : lo'_kz < o'_kz; (3) the LINE must meet box': per axis with d'_r = 0, lo'_r <= o'_r <= hi'_r; else i = rcp(d'_r) (within 1 ulp), a = (lo'_r - o'_r) i, b =
 *   (hi'_r - o'_r) i, the smaller moved down and the larger moved up by 2^-21 of itself (8 u against the 2.5 u of reciprocal and product), tn = max, tf = min
 *   over the axes starting from -inf, +inf; a distance that is not a number narrows nothing; pass iff not tn > tf.  (2) and (3) hold for every accepted triangle
 *   by the paragraph above, with a tenfold margin in P.  flags bit 0 switches the test off (every lane queries every valid instance): the results must not
 *   change by a bit, which is how the tests hold this argument.
 *
 *   out [M][Nt][3] dev: only listed texels are written, zeros included (K = 0: zeros).  texel_ids NULL => all Nt (n_ids ignored); a non-null list with
 *   n_ids == 0 is a no-op.
 *   stats dev u64[3], nullable: += samples whose ray met some box (= the scene rays traced), occluder queries issued, blocked samples (an accepted hit behind an
 *   instance, of any set or none); one atomic add per wave and counter.  With the prefilter off every sample of a live texel counts as met.
 *   workspace: texir_irt_shadow_mesh_workspace_bytes(n_ids, N, M) bytes of device scratch (12 bytes x M x parts per listed texel; 0 for refused arguments).
 * Caller-owned buffers, the caller's stream, no allocation, no synchronisation, no atomics on results: the call records into a hipGraph.  Q or K outside 0..8,
 * M outside 1..8, inst_obj[j] outside 0..Q-1, N < 1 (all reported before any null buffer), a null buffer, a workspace that is too small, the scene or an
 * occluder without the 4-wide tree and an occluder on another device than the scene are errors with a texir_last_error() text.
 * Not computed here: objects shadowing the inserted emitters' F and R (texir_irt_lights_mesh, texir_spec_lights_mesh do that); the bounce G's own rays,
 * which still ignore the objects; for the DIFFUSE term, a union with analytic bodies in one call (the two lost terms
 * double-count where they overlap; texir_spec_shadow takes that union for the specular term, and computes the object's shadow in it); more than 8
 * occluders, instances or sets per call. */
TEXIR_API int64_t texir_irt_shadow_mesh_workspace_bytes(int64_t n_ids, int32_t N, int32_t M);
TEXIR_API int texir_irt_shadow_mesh(const texir_scene* scene, const float* pos /*dev*/, const float* nrm /*dev*/, const float* shift /*dev*/,
                       const int32_t* texel_ids /*dev, nullable*/, int64_t n_ids, int64_t Nt, int32_t N, int32_t mode,
                       const texir_scene* const* occluders /*host [Q]*/, int32_t Q /*0..8*/, const int32_t* inst_obj /*host [K]*/,
                       const float* inst_world_to_obj /*dev [K][12]*/, int32_t K /*0..8*/, const uint32_t* sets /*dev [M]*/, int32_t M /*1..8*/,
                       float* out /*dev [M][Nt][3]*/, uint64_t* stats /*dev [3], nullable*/, uint32_t flags /*bit 0: prefilter off*/, void* workspace /*dev*/,
                       int64_t workspace_bytes, void* stream);

/* name of the kernel form ONE texir_irt_generate call over n_ids listed texels at N samples launches on this scene
 * ("irt_group_kernel<false, 4, 6>": 64 texels per wave; "irt_kernel<false, 4|2>": one texel per wave) -- the launcher's own
 * decision, so that bench.py's roofline names the kernel that really ran.  buf receives a NUL-terminated string. */
TEXIR_API int texir_irt_kernel_name(const texir_scene* scene, int64_t n_ids, int32_t N, char* buf, int32_t cap);

/* The INSTANTIATION of that form the same call launches for sampling mode `mode` (uniform 0 | cosine 1) and estimator `cosine_estimator` (0: the IrT
 * estimator of texir_irt_generate; 1: the cosine branch of texir_diffuse_irradiance, which needs mode 1).  The 64-texel form has instantiations compiled
 * for what the IrrT stage calls it with -- N a power of two, 4-byte texels in 8x4-texel lines (texture layout 4), a scene with the float node copy:
 * "irt_group_kernel<false, 4, 6, IrtFixed<mode, estimator>>"; they compute the bits of the generic kernel.  Every other call, and every call under
 * TEXIR_IRT_SPECIALISE=0, gets the name texir_irt_kernel_name reports.  Like that name this is the PLAIN launch's kernel: a counting launch (texir_irt_generate
 * with `stats`) of the 64-texel form always runs the generic kernel's counting instantiation, irt_group_kernel<true, 4, 6>. */
TEXIR_API int texir_irt_kernel_variant(const texir_scene* scene, int64_t n_ids, int32_t N, int32_t mode, int32_t cosine_estimator, char* buf, int32_t cap);

/* Replaces MaterialModel.render + specular_reflectance (models/mat_nvdiffrast.py:201-249, 260-279), forward:
 *   rgb = irr*albedo/pi + (1/S) sum_i Ls_i * w_i(roughness)        
 * normal,albedo,points,irr [P,3] dev; rough [P] dev; cam [3] dev; shift [P,2] dev (GGX sample shift, as above)
 * Ls_ws [P,S,3] dev, nullable: traced radiance saved for texir_spec_backward.
 * clamp_eps: the floor of the BRDF denominators -- 1e-14 (TINY_TINY_NUMBER) in models/mat_nvdiffrast.py:270-279, 1e-6 (TINY_NUMBER) in
 * the evaluation model models/test_nvdiffrast.py:320-333.
 * ls_given = 1: Ls_ws is an INPUT (the `lighting` argument of specular_reflectance, function seam 3 of SURVEY 8b) and nothing is
 * traced -- specular_reflectance(lighting, h, n, v, l, roughness)/S + irr*albedo/pi on the caller's lighting. */
TEXIR_API int texir_spec_forward(const texir_scene* scene /*nullable when ls_given*/, const float* normal, const float* albedo, const float* rough,
                       const float* points, const float* irr, const float* cam, const float* shift, int64_t P,
                       int32_t S, float clamp_eps, int32_t ls_given, float* rgb /*dev [P,3]*/, float* Ls_ws /*dev, nullable*/, void* stream);

/* The training form of the pair (round 4): the forward also writes dw_ws [P,S] = d w_i / d roughness (its dual-number sample chain yields them next to the
 * weights), and the backward is a stream over what the forward kept -- d_rough[p] = (1/S) sum_i (Ls_i . d_rgb[p]) dw_i, d_albedo = d_rgb*irr/pi -- instead of
 * texir_spec_backward's recomputation of the whole sample chain.  Same values as the pair above (tests/test_gpu_parity.py). */
TEXIR_API int texir_spec_forward_train(const texir_scene* scene /*nullable when ls_given*/, const float* normal, const float* albedo, const float* rough,
                       const float* points, const float* irr, const float* cam, const float* shift, int64_t P,
                       int32_t S, float clamp_eps, int32_t ls_given, float* rgb /*dev [P,3]*/, float* Ls_ws /*dev [P,S,3]*/, float* dw_ws /*dev [P,S]*/, void* stream);
TEXIR_API int texir_spec_backward_ws(const float* irr, const float* Ls_ws, const float* dw_ws, const float* d_rgb, int64_t P, int32_t S,
                       float* d_albedo /*dev [P,3], nullable*/, float* d_rough /*dev [P], nullable*/, void* stream);

/* Analytic backward of the above (what autograd computes in the reference): given d_rgb [P,3],
 *   d_albedo [P,3] = d_rgb*irr/pi ;  d_rough [P] = sum_c d_rgb_c * (1/S) sum_i Ls_ic * dw_i/dr
 * (gradient through a=r^2 -> cos/sin theta -> h -> vdh -> l -> ndl, ndh and through k=(r+1)^2/8; Ls constant,
 * torch clamp sub-gradients).  Either output may be NULL. */
TEXIR_API int texir_spec_backward(const float* normal, const float* rough, const float* points, const float* irr,
                        const float* cam, const float* shift, const float* Ls_ws, const float* d_rgb, int64_t P,
                        int32_t S, float clamp_eps, float* d_albedo /*dev, nullable*/, float* d_rough /*dev, nullable*/, void* stream);

/* Replaces the lighting integral of diffuse_reflectance (models/mat_nvdiffrast.py:252-258; live in the evaluation model's
 * relighting branch, models/test_nvdiffrast.py:268-274): per point  E = (2*pi/N) sum_i L_i * clamp(n.l_i, 0, 1)  over uniform
 * directions (sample_type 0: the IrT estimator) or  E = (pi/N) sum_i L_i  over cosine-distributed directions (sample_type 1), so that
 * diffuse_reflectance(...)/N == E * albedo / pi.  pos (already offset), nrm [P,3], shift [P,2] dev -> irr [P,3] dev. */
TEXIR_API int texir_diffuse_irradiance(const texir_scene* scene, const float* pos, const float* nrm, const float* shift, int64_t P,
                        int32_t N, int32_t sample_type, float* irr /*dev [P,3]*/, void* stream);

/* Replaces RenderLoss.forward + SegLoss.forward + hdr_scale (models/loss.py:81-115, 214-295; utils/general.py:61-66),
 * value AND gradient in one call.  The reference's one-hot mask tensors (seg_mask/floor_max_mask [C,6,h,w,1],
 * room_seg_mask [R,6,h,w,1], built at trainer/train_material.py:255-296) are passed in their compact form:
 *   seg_id [P] u8: class of the pixel (255 = none); hl [P] u8: floor_max_mask of the pixel's own class;
 *   room_id [P] u8 (255 = none; stage 2 only, else NULL).
 * stage 0/1/2 as in RenderLoss.forward; loss_type 0 = 'L1', 1 = 'L2' (applies to the rendered-radiance term only), 2 = no
 * rendered-radiance term (SegLoss alone: the psnr / ssim / msssim variants of loss.py:65-73 add their own image term).
 * gt,rgb,albedo [P,3]; rough,rough_womip,empty_mask,gt_mask [P] (all dev; inputs a stage does not read may be NULL).
 * out [2] dev: (total loss, seg term) = the reference's (loss, seg_loss.item()).
 * d_rgb [P,3], d_albedo [P,3] (stage 0), d_rough [P] (stages 1,2): d loss / d input for an upstream gradient of 1
 *   (the means of stages 0 and 2 are differentiated through, the stage-1 quantile target is detached, as in the reference).
 * workspace: texir_loss_workspace_bytes(P, C, R) bytes of device scratch. hw = h*w (the stage-1 scale, loss.py:101). */
TEXIR_API int64_t texir_loss_workspace_bytes(int64_t P, int32_t C, int32_t R);
TEXIR_API int texir_loss_forward(int32_t stage, int32_t loss_type, const float* gt, const float* rgb, const float* albedo,
                       const float* rough, const float* rough_womip, const float* empty_mask, const float* gt_mask,
                       const uint8_t* seg_id, const uint8_t* hl, const uint8_t* room_id, int64_t P, int32_t C, int32_t R,
                       int32_t hw, void* workspace, float* out /*dev [2]*/, float* d_rgb, float* d_albedo, float* d_rough,
                       void* stream);

/* ---- G-buffer production: replaces nvdiffrast rasterize + interpolate (models/mat_nvdiffrast.py:119-128,
 * models/tracer_o3d_irt.py:102-108) by casting one primary ray per cube-map pixel through the scene's BVH.
 * Geometry and cameras never change (optim_cam=False, configs/syn.conf:20), so hosts cache the result per view. */

/* per-corner shading normals [3T,3] host (normals[indices] of pyredner.load_obj, tracer_o3d_irt.py:61,105);
 * without them the G-buffer carries geometric normals. */
TEXIR_API int texir_scene_set_corner_normals(texir_scene* scene, const float* corner_normals /*host*/);

/* mvp [6,4,4] f32 HOST: the reference's per-face mvp as passed to MaterialModel.forward (row-vector convention
 * clip = [x,y,z,1] @ mvp, datasets/dataset.py:464-465); inverted in double inside the library.  Pixel (row i, col j) is at ndc ((j+.5)/c*2-1, (i+.5)/c*2-1), i.e. nvdiffrast's layout.
 * Outputs, P = 6*c*c, all dev: pos [P,3] (interpolated vertex position; empty -> (1,0,0)), nrm [P,3] (interpolated
 * corner normals; empty -> (1,0,0)), mask [P] (1 where rast[...,3] > 0), uv [P,2] (= texc), uv_da [P,4]
 * (= texd: du/dX, du/dY, dv/dX, dv/dY per pixel), tri_id [P] (primitive id + 1, 0 = empty; nvdiffrast rast[...,3]).
 * flip_v: 1 -> uv.v := 1 - v (pyredner's OBJ convention for the nvdiffrast-side textures), and the two dv entries of uv_da negated.
 *   RAYS start at the eye (the pre-image of clip (0,0,1,0)) and are not clipped: no near or far plane, the closest hit with t > 0 counts.  mvp and
 *     s * mvp (s != 0, either sign) are the same projective map and give the same G-buffer.
 *   NORMALS are not renormalised: with corner normals w n0 + u n1 + v n2 as given; without, the unit geometric normal cross(v1 - v0, v2 - v0) /
 *     |cross| in the CALLER's winding (the library's stored corner order is a rotation of the caller's and keeps the sign).
 *   BACKGROUND values ignore flip_v: pos = nrm = (1,0,0), uv = (0,0), uv_da = 0, mask = 0, tri_id = 0.
 *   ERRORS: TEXIR_ERR_INVALID, with nothing launched and no output written, for cube_res outside 1..16384, for a singular mvp and for an affine one
 *     (an orthographic camera: the inverse's row 2 has w == 0, there is no eye).
 * Every pixel is compared with a float64 reference built from mvp, c and the mesh alone (tests/gbuffer_cases.py, tests/test_gpu_gbuffer_cast.py). */
TEXIR_API int texir_gbuffer_cast(const texir_scene* scene, const float* mvp /*host*/, int32_t cube_res, int32_t flip_v,
                       float* pos, float* nrm, float* mask, float* uv, float* uv_da, int32_t* tri_id, void* stream);

/* ---- nvdiffrast `texture` restated (models/mat_nvdiffrast.py:131-139).  Level 0 of the mip stack IS the caller's texture
 * [H,W,C] (C <= 4, no copy); levels 1.. live in a caller-provided "rest" buffer of texir_mip_elems() floats that
 * texir_mip_build fills by 2x2 box filtering.
 * filter_mode 0 = 'linear' (bilinear, level 0; mips_rest may be NULL), 1 = 'linear-mipmap-linear' (trilinear, LOD from
 * uv_da); boundary_mode 'wrap'. */
TEXIR_API int32_t texir_mip_levels(int32_t H, int32_t W, int32_t max_mip_level);
TEXIR_API int64_t texir_mip_elems(int32_t H, int32_t W, int32_t C, int32_t levels);
/* from_level 0: levels 1.. from the texture; 1: level 1 of mips_rest is already current (texir_adam_step_tex wrote it with the
 * update), build levels 2.. from it.  (TEXIR_MIP_PER_LEVEL=1 selects the one-launch-per-level reference implementation; the
 * default builds five levels per launch through LDS -- identical bits.) */
TEXIR_API int texir_mip_build(const float* tex /*dev*/, float* mips_rest /*dev*/, int32_t H, int32_t W, int32_t C, int32_t levels,
                       int32_t from_level, void* stream);
TEXIR_API int texir_tex_fetch_forward(const float* tex /*dev*/, const float* mips_rest /*dev, nullable*/, int32_t H, int32_t W,
                       int32_t C, int32_t levels, const float* uv /*dev [P,2]*/, const float* uv_da /*dev [P,4], nullable for mode 0*/,
                       int32_t filter_mode, int64_t P, float* out /*dev [P,C]*/, void* stream);
/* d_tex [H,W,C] and grad_rest [texir_mip_elems] (dev) must be zero on entry; on return d_tex holds d loss / d texture
 * (the gradient scattered into the mip levels is folded down to level 0). */
TEXIR_API int texir_tex_fetch_backward(float* d_tex /*dev*/, float* grad_rest /*dev, nullable for mode 0*/, int32_t H, int32_t W,
                       int32_t C, int32_t levels, const float* uv, const float* uv_da, int32_t filter_mode, int64_t P,
                       const float* d_out /*dev [P,C]*/, void* stream);

/* As texir_tex_fetch_backward (trilinear; the autograd backward of dr.texture, models/mat_nvdiffrast.py:131,134), but the last fold is left out: on return d_tex holds the level-0 scatter only and the first
 * (H/2)*(W/2)*C floats of grad_rest hold the level-1 gradient with all coarser levels folded in.  texir_adam_step_tex consumes the pair. */
TEXIR_API int texir_tex_fetch_backward_deferred(float* d_tex /*dev*/, float* grad_rest /*dev*/, int32_t H, int32_t W, int32_t C,
                       int32_t levels, const float* uv, const float* uv_da, int64_t P, const float* d_out /*dev [P,C]*/, void* stream);

/* Atomics-free backward of the dr.texture fetches (models/mat_nvdiffrast.py:131-139) whose (uv, uv_da) never change (a cached view:
 * geometry and cameras are constant).
 * texir_tex_taps lists the taps of every pixel: keys/weights [P*8] (4 bilinear taps x 2 mip levels; bilinear mode uses the first 4),
 * key = texel index in the unified order [level 0 | levels 1.. as in mips_rest], -1 for unused slots, weight = bilinear x level blend.
 * The caller sorts them by key once (stable), forms segments (key, start, count) + the sorted (pixel, weight) lists, and then every
 * backward is texir_tex_gather_backward: one thread per touched texel adds its list in order (deterministic), followed by the
 * same folds as texir_tex_fetch_backward (defer_last_fold = 1: as texir_tex_fetch_backward_deferred).  d_tex / grad_rest zero on entry.
 * With defer_last_fold = 1, d_tex may be NULL when no listed tap samples level 0 (no key < H*W): the level-0 gradient is then
 * identically zero and texir_adam_step_tex(grad = NULL) never reads it.
 * defer_last_fold = 2 (levels >= 4, H and W divisible by 4): the folds stop at level 2 -- grad_rest then holds the raw level-1 gradient and the
 * level-2 gradient with everything coarser folded in; texir_adam_step_tex(grad_level2 = ...) takes both remaining folds over and the
 * read-modify-write of the level-1 stack (half the traffic of the folds) disappears. */
TEXIR_API int texir_tex_taps(int32_t H, int32_t W, int32_t C, int32_t levels, const float* uv, const float* uv_da, int32_t filter_mode,
                       int64_t P, int64_t* keys /*dev [P*8]*/, float* weights /*dev [P*8]*/, void* stream);
TEXIR_API int texir_tex_gather_backward(float* d_tex, float* grad_rest, int32_t H, int32_t W, int32_t C, int32_t levels,
                       const int64_t* seg_key /*dev [n_seg]*/, const int32_t* seg_start, const int32_t* seg_count, int32_t n_seg,
                       const int32_t* pix /*dev, sorted*/, const float* weights /*dev, sorted*/, const float* d_out /*dev [P,C]*/,
                       int32_t filter_mode, int32_t defer_last_fold, void* stream);

/* ---- optimiser step of the material textures: torch.optim.Adam(lr, betas, eps) (trainer/train_material.py:122-123,448-450)
 * fused with the clamp the trainer applies right after it (:458, :592-593).  step >= 1; lo/hi = clamp range (+-inf = none). */
TEXIR_API int texir_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                       float beta1, float beta2, float eps, int32_t step, float clamp_lo, float clamp_hi, void* stream);

/* The same step (trainer/train_material.py:448-458) for a texture [H,W,C] whose gradient is grad + 0.25 * grad_level1[y/2][x/2] (texir_tex_fetch_backward_deferred): the
 * last mip fold is fused into the optimiser's read of the gradient; results equal fold + texir_adam_step bit for bit.
 * grad == NULL: no pixel of the step sampled mip level 0, the level-0 gradient is neither materialised nor read.
 * grad_mask != NULL: grad is a buffer that is never cleared; only the texels a view's tap lists touch (their bit is set) carry this
 * step's values, all others count as zero -- the usual case of a handful of level-0 taps costs 1 bit per texel instead of a fill + a read.
 * mip_level1 != NULL: level 1 of the NEXT forward's mip stack (models/mat_nvdiffrast.py:131-134 rebuild it from the updated
 * texture every step) is written on the way: texir_mip_build(..., from_level = 1) then skips the pass over the full texture. */
TEXIR_API int texir_adam_step_tex(float* param, const float* grad /*nullable: level-0 gradient identically zero*/,
                       const uint32_t* grad_mask /*nullable: 1 bit per texel (bit t&31 of word t>>5): grad is valid -- and read -- only where set*/,
                       const float* grad_level1,
                       const float* grad_level2 /*nullable: [H/4,W/4,C] level-2 gradient NOT yet folded into grad_level1 (texir_tex_gather_backward with
                                                  defer_last_fold = 2): the step also performs grad_level1 += 0.25 * grad_level2 on the fly, same fma*/,
                       float* exp_avg, float* exp_avg_sq, float* mip_level1 /*nullable: [H/2,W/2,C] <- 2x2 average of the updated texels*/,
                       int32_t H, int32_t W, int32_t C, float lr, float beta1, float beta2, float eps, int32_t step, float clamp_lo,
                       float clamp_hi, void* stream);

/* The same two steps for launches that must not depend on host arguments that change every step (a captured hipGraph of the whole
 * optimisation step, trainer/train_material.py:408-458 -- forward, loss, backward AND optimizer.step()): the step count, learning rate
 * and betas of up to 64 parameters live in device memory (`state` [n][4] doubles: step count, lr, beta1, beta2).  texir_adam_tick
 * advances the step count of the records selected by `mask` (bit i = record i) and writes hyper[i] = (lr / (1 - beta1^step),
 * sqrt(1 - beta2^step)) in double precision, the expressions of torch.optim.Adam's single-tensor path; the *_dev steps read their
 * record's pair instead of taking (lr, step).  A learning-rate scheduler writes state[i][1] between steps.
 * texir_adam_step_tex_dev: grad_level1 may be NULL when grad_level2 is given and no tap of the view's lists touches mip level 1 (its direct
 * gradient is identically zero: the level-1 stack -- a quarter of the texture -- is then not read at all). */
TEXIR_API int texir_adam_tick(double* state /*dev [n][4]*/, float* hyper /*dev [n][2]*/, int32_t n_records, uint64_t mask, void* stream);
TEXIR_API int texir_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* hyper /*dev [2]*/,
                       float beta1, float beta2, float eps, float clamp_lo, float clamp_hi, void* stream);
TEXIR_API int texir_adam_step_tex_dev(float* param, const float* grad, const uint32_t* grad_mask, const float* grad_level1, const float* grad_level2,
                       float* exp_avg, float* exp_avg_sq, float* mip_level1, int32_t H, int32_t W, int32_t C, const float* hyper /*dev [2]*/,
                       float beta1, float beta2, float eps, float clamp_lo, float clamp_hi, void* stream);

/* ---- batched forms of the texture-side launches of one material step (trainer/train_material.py:408-458: the reference fetches its albedo and roughness
 * textures with separate dr.texture calls, models/mat_nvdiffrast.py:131-139, and steps them with one torch.optim.Adam) --------------------------------------
 * A step over k material textures launches k x (mip build + tail, fetch, gather, fold, Adam); these entry points take up to TEXIR_MAX_BATCH jobs and issue ONE
 * launch per kind (blocks are dealt to the jobs by block index; every job keeps its own sizes and channel count).  Each job's result is bit-identical to the
 * corresponding single-texture entry point above.  Errors of these functions are reported through texir_batch_last_error() (thread-local), which returns the
 * library's one error text: the same string as texir_last_error().  (It used to be a text of its own: since the two were joined, texir_last_error() after a failed
 * batched call holds that call's message too, where it once kept whatever an earlier call had left.) */
#define TEXIR_MAX_BATCH 4
TEXIR_API const char* texir_batch_last_error(void);

/* texir_mip_build (when build_from >= 0) followed by texir_tex_fetch_forward, for every job: one pyramid launch, one tail launch, one fetch launch */
typedef struct texir_tex_fetch_job {
    const float* tex;          /* dev [H,W,C] */
    float* mips_rest;          /* dev: levels 1.. (texir_mip_elems floats); nullable when levels == 1 */
    int32_t H, W, C, levels;
    int32_t build_from;        /* -1: the stack is valid as it is; 0: build levels 1.. from tex; 1: level 1 is valid (texir_adam_step_tex wrote it), build levels 2.. */
    int32_t filter_mode;       /* 0 bilinear | 1 trilinear */
    const float* uv;           /* dev [P,2] */
    const float* uv_da;        /* dev [P,4]; nullable for mode 0 */
    int64_t P;
    float* out;                /* dev [P,C] */
} texir_tex_fetch_job;
TEXIR_API int texir_tex_fetch_forward_batch(const texir_tex_fetch_job* jobs /*host*/, int32_t n_jobs, void* stream);

/* texir_tex_gather_backward for every job: one gather launch, one fold launch.
 * rest_mask (nullable; needs defer_last_fold = 2): one bit per texel of grad_rest (bit t & 31 of word t >> 5; t = the key of texir_tex_taps minus H*W), set for
 * exactly the texels the job's tap lists name.  With it grad_rest need NOT be zero on entry and is never cleared: the folds read the levels above 2 through the
 * mask (an unset texel counts as zero) and WRITE level 2; level 1 is left as the gather wrote it, valid where the mask says so --
 * texir_adam_step_tex_dev_batch(level1_mask = the same mask) reads it accordingly.  The per-step fill of the gradient stacks (a third of the texture) and the
 * optimiser's dense read of the level-1 stack (a quarter) disappear; same floats as with a zero-filled stack. */
typedef struct texir_tex_gather_job {
    float* d_tex;              /* dev [H,W,C]; nullable as in texir_tex_gather_backward */
    float* grad_rest;          /* dev */
    int32_t H, W, C, levels;
    const int64_t* seg_key; const int32_t* seg_start; const int32_t* seg_count; int32_t n_seg;
    const int32_t* pix; const float* weights;
    const float* d_out;        /* dev [P,C] */
    int32_t filter_mode, defer_last_fold;
    const uint32_t* rest_mask; /* dev, nullable */
    const float* d_out2;       /* dev [P,C], nullable: a second gradient of the same fetch output (two consumers of one dr.texture result, models/mat_nvdiffrast.py:134 ->
                                  :179 render and models/loss.py:108): the gather adds the two on the fly -- the sum autograd's add launch would have written */
} texir_tex_gather_job;
TEXIR_API int texir_tex_gather_backward_batch(const texir_tex_gather_job* jobs /*host*/, int32_t n_jobs, void* stream);

/* texir_adam_step_tex_dev for every job in one launch */
typedef struct texir_adam_tex_job {
    float* param; const float* grad; const uint32_t* grad_mask;
    const float* grad_level1;
    const uint32_t* level1_mask;   /* dev, nullable; only with grad_level2: grad_level1 is valid -- and read -- only where the bit of its texel is set (see above) */
    const float* grad_level2;
    float* exp_avg; float* exp_avg_sq; float* mip_level1;
    int32_t H, W, C;
    const float* hyper;            /* dev [2] (texir_adam_tick) */
    float beta1, beta2, eps, clamp_lo, clamp_hi;
} texir_adam_tex_job;
/* g [n_texels][C] += g0 [n_texels][C] where bit t of mask (one bit per texel) is set: the sparse level-0 gradient of a trilinear fetch folded into the dense level-0
 * gradient an un-mipmapped fetch of the SAME texture produced in the same backward pass (stage 1, models/mat_nvdiffrast.py:131-139: both fetches read materials_r).
 * Errors: texir_batch_last_error(). */
TEXIR_API int texir_grad_add_masked(float* g /*dev*/, const float* g0 /*dev*/, const uint32_t* mask /*dev*/, int64_t n_texels, int32_t C, void* stream);
TEXIR_API int texir_adam_step_tex_dev_batch(const texir_adam_tex_job* jobs /*host*/, int32_t n_jobs, void* stream);

/* ---- the asset step between the two stages: replaces tools/padding_texture.py:49-87 (the script that turns the IrT stage's 0_irr_texture.hdr into the
 * Mat stage's irt.hdr: scipy's Euclidean distance transform + grid_sample on the CPU, then the external Open Image Denoise binary) by launches on the
 * device texture.  Nothing below allocates or synchronises: scratch is the caller's, so every launch can be recorded into a hipGraph.
 *
 * texir_texture_pad: img [H,W,C] f32, C in 1..4, H and W <= 16384.  A texel is a HOLE when the float32 sum of its channels in channel order
 * (c0 + c1 + c2 ...) equals 0.0 -- the reference's rule (:54-56); (1, -1, 0) is a hole.
 *   src [H*W] i32 (nullable output): src[t] = t for a non-hole; for a hole the flat index of a non-hole texel at minimal Euclidean distance, compared
 *     as exact integer squared distances, whatever that distance is (no search window); -1 everywhere when the image has no non-hole texel.
 *     TIE RULE (deterministic; independent of launch configuration and run): with the hole at (y, x), the candidate of a column is that column's non-hole
 *     row nearest to y, the UPPER one of two equidistant rows; columns are visited in the order x, x-1, x+1, x-2, x+2, ... and the first candidate at the
 *     minimal squared distance wins.
 *   out [H,W,C] (!= img): non-holes keep their bits; a hole takes img[src[t]] (mode `nearest`: row_map == col_map == NULL) or, with (r, c) the texel
 *     src[t] names, img[row_map[r], col_map[c]] and 0 where a map entry is -1 (mode `reference`: row_map [H], col_map [W] i32 tables of what
 *     F.grid_sample(mode='nearest', align_corners=False) really reads for source index i -- rint(i - 0.5) in float32, half to even, i.e. one texel too low
 *     for every odd i; texpost.reference_index_map builds them).  With src == -1 (no non-hole texel) out is a copy of img.
 *   workspace: texir_texture_pad_workspace_bytes(H, W) bytes of device scratch. */
TEXIR_API int64_t texir_texture_pad_workspace_bytes(int32_t H, int32_t W);
TEXIR_API int texir_texture_pad(const float* img /*dev*/, int32_t H, int32_t W, int32_t C, const int32_t* row_map /*dev [H], nullable*/,
                       const int32_t* col_map /*dev [W], nullable*/, float* out /*dev [H,W,C], != img*/, int32_t* src /*dev [H*W], nullable*/,
                       void* workspace /*dev*/, void* stream);
/* Stand-in for the Open Image Denoise call (:86-87; NOT a re-implementation of its network): an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010)
 * on log(1 + max(x, 0)).  `iterations` (1..6) passes of the 5x5 B3-spline kernel [1 4 6 4 1]/16 x [1 4 6 4 1]/16 with hole size 2^it in pass it; the weight of
 * tap q at texel p is k[dy] k[dx] exp(-E) valid_q,  E = |c_q - c_p|^2 / (sigma_c 0.5^it)^2 + |n_q - n_p|^2 / sigma_n^2 + |x_q - x_p|^2 / sigma_p^2;
 * c <- sum(w c_q) / max(sum w, 1e-20) on valid texels (channel sum of img != 0), unchanged elsewhere; result expm1(c) * valid.  Validity is zero outside the
 * image.  guide_nrm / guide_pos [H,W,3] are optional (NULL, or a sigma of 0, switches the term off; their sigmas do not shrink with the pass): the texel
 * G-buffers of the IrT stage, which tell neighbours of the same surface from the unrelated chart a padded gutter borders on.
 * One launch per pass, ping-pong between tmp and out (img, tmp, out [H,W,3]: three different buffers; the result is in out). */
TEXIR_API int texir_texture_denoise(const float* img /*dev [H,W,3]*/, int32_t H, int32_t W, const float* guide_nrm /*dev, nullable*/,
                       const float* guide_pos /*dev, nullable*/, int32_t iterations, float sigma_c, float sigma_n, float sigma_p,
                       float* tmp /*dev [H,W,3]*/, float* out /*dev [H,W,3]*/, void* stream);

/* ---- the texel G-buffer from the mesh: replaces models/tracer_o3d_irt.py:99-142 (generate_positions + calcute_position_normal_texture: a cube map
 * ray-cast per view, warped to a 1024 x 512 panorama, and a gather of every texel's position through the (row code, column code, panorama id) triple of
 * 0.png) by a rasterisation of the scene's triangles in uv space.  Needs no index texture; exact per texel instead of quantised to panorama pixels.
 * Nothing below allocates or synchronises: scratch is the caller's, so the call can be recorded into a hipGraph.
 *
 * Texel (r, c) of the H x W atlas, in the hit shader's orientation, has its centre at (u, v) = ((c + 0.5) / W, (r + 0.5) / H) (float32 divisions); the
 * outputs are in FILE orientation: that texel is row H - 1 - r of pos, nrm, prim_id and bary (what texel_gbuffer.npz holds).  H, W in 1..16384.
 * The uvs are the scene's tri_uvs as given (V not flipped, no wrap); the atlas is [0,1]^2, what lies outside is clipped.
 *   COVERAGE: the texel belongs to a triangle when its centre is inside the uv triangle, either winding.  Each edge is evaluated from its two endpoints
 *     in one canonical order -- (x0, y0) the lexicographically smaller (x, then y) of the two -- in separately rounded float32 operations:
 *         E = (x1 - x0) * (v - y0) - (y1 - y0) * (u - x0)
 *     and when that difference is 0 its sign is taken from the exact error terms of the two products, so E == 0 exactly when the rounded operands say so.
 *     The two triangles sharing an edge thus see the identical E with opposite orientation: exact negations.  With s = the sign of the triangle's area
 *     (the same evaluation, edge (corner 0, corner 1) at corner 2) and e = +-E the value for the edge as the triangle runs through it, the centre is
 *     inside the edge when s e > 0, or -- CRACK RULE -- s e == 0 and the edge's inward normal (nx, ny) = s (-(yb - ya), xb - xa) has nx > 0, or nx == 0
 *     and ny > 0: a centre exactly on an interior chart edge goes to exactly one of the two triangles.  A triangle with zero area (s == 0) or a
 *     non-finite uv covers nothing.  A triangle is tested against the texels of its clipped bounding box only, columns max(0, floor(umin W - 0.5)) ..
 *     min(W - 1, ceil(umax W - 0.5)), rows likewise: no centre inside or on the border of the triangle is outside that box.
 *     OVERLAP RULE: where several triangles cover a centre the lowest primitive id (row of the caller's index array) wins.
 *     The result is a pure function of (verts, tris, tri_uvs, H, W): integer atomicMin of the primitive id per texel, then one resolve pass; no float
 *     atomics; identical bits run to run, whatever the launch shape.
 *   ROUNDING BOUND of the edge function: the centre's coordinates carry one rounding each, every subtraction and product one, the difference one; to first
 *     order the computed E differs from the exact edge function of the float32 uvs at the exact centre by at most
 *         |dE| <= |x1 - x0| (4 |v - y0| + |v|) 2^-24 + |y1 - y0| (4 |u - x0| + |u|) 2^-24,
 *     i.e. in units of uv distance from the edge (E over the edge's length) by at most m = (8 D + 2) 2^-24, D = the largest coordinate difference between
 *     a centre and an endpoint.  For uvs within [-1, 2] that is 18 x 2^-24 < 2^-19; 2^-18 holds up to D = 7.75.  A triangle the exact arithmetic puts
 *     a centre more than m inside owns it here unless a lower id does; one it puts more than m outside never does.
 *   ATTRIBUTES of the winner: e_k = the edge value opposite the CALLER's corner k (the library's stored corner rotation is turned back), S = (e_0 + e_1) + e_2,
 *     bary = (b1, b2) = (e_1 / S, e_2 / S): the weights of corners 1 and 2, texir_trace_shade's prim_uv convention;
 *     p = (P0 + b1 (P1 - P0)) + b2 (P2 - P0);  normal_mode TEXIR_NORMAL_GEOMETRIC: n = cross(P1 - P0, P2 - P0) / |cross| (what synth.make_texel_gbuffer
 *     stores); TEXIR_NORMAL_SHADING: n = (N0 + b1 (N1 - N0)) + b2 (N2 - N0) of the corner normals of texir_scene_set_corner_normals, NOT renormalised
 *     (:105-106; an error when none are set);  pos = p + offset n (:110: offset 1e-2), nrm = n.  All float32, separately rounded.
 *     SEAMS: an uncovered texel, and one whose winner has a geometric normal of zero or non-finite length or S == 0, gets pos = nrm = 0, bary = 0,
 *     prim_id = 0xFFFFFFFF (:137-139 zeroes the seams of the index texture; here the seams are the texels no triangle covers).
 *   workspace: texir_texel_gbuffer_workspace_bytes bytes of device scratch (4 bytes per texel + 16 per triangle slot + 4 per triangle). */
#define TEXIR_NORMAL_GEOMETRIC 0
#define TEXIR_NORMAL_SHADING 1
TEXIR_API int texir_texel_gbuffer_workspace_bytes(const texir_scene* scene, int32_t H, int32_t W, int64_t* bytes);
TEXIR_API int texir_texel_gbuffer(const texir_scene* scene, int32_t H, int32_t W, int32_t normal_mode, float offset, float* pos /*dev [H,W,3]*/,
                       float* nrm /*dev [H,W,3]*/, uint32_t* prim_id /*dev [H,W], nullable*/, float* bary /*dev [H,W,2], nullable*/,
                       void* workspace /*dev*/, void* stream);

/* ---- the radiance atlas and the index texture from calibrated panoramas (csrc/texbake.hip).  Every stage starts from hdr_texture.hdr and 0.png; the
 * reference produces neither: its private capture pipeline writes 0.png (per texel: which panorama, at which pixel) and tools/trans_hdr_tex.py:16-61
 * (repackHDRTexture) only gathers the panoramas' pixels through those codes.  texir_atlas_bake makes the selection: one view and one panorama pixel per
 * texel, from the mesh (the scene), the texel G-buffer and calibrated panoramas.  The result is a pure function of the inputs.
 *
 * THE RULE.  Per texel: pos (ALREADY offset along the normal, as texir_texel_gbuffer delivers it) and nrm (the raw normal, not renormalised).  Per view k:
 * a 3x4 row-major float32 world-to-camera matrix W_k (rows of cams[k]), the camera position c_k, a panorama [h,w,3] float32 and optionally a validity
 * mask [h,w] uint8.  The camera frame is the one in which utils/Pano2Cube.py:57-82 measures azimuth and elevation (x right, y up, z front of its front
 * face; atlas.camera_matrices builds W_k from a final_extrinsics.txt matrix).  With d = c_k - pos, dd = d.d:
 *   FACING      nrm.d > cos_min sqrt(dd)  and  dd > 0.
 *   PIXEL       t = W_k (pos, 1);  az = atan2(t.x, t.z);  el = asin(clamp(t.y / |t|, -1, 1));  x = (az / pi + 1) / 2 w;  y = (1 - el / (pi / 2)) / 2 h;
 *               col = min(floor(x), w - 1), row = min(floor(y), h - 1), both clamped at 0: the pixel Pano2Cube's grid_sample(nearest,
 *               align_corners=False) reads for that direction, and the pixel tools/trans_hdr_tex.py:50-54 decodes from the code of its centre.
 *               |t| zero or not finite: no candidate.  With a mask, a pixel whose mask byte is 0 makes the view no candidate.
 *   VISIBILITY  the ray (org = pos, dir = d): the view is occluded iff its closest hit has t < 1.  Closest hit is what texir_trace_shade reports (Embree
 *               semantics: t > 0, t in units of |dir|); no extra t_min, because pos is already offset.
 *   SCORE       s = (nrm.d) / (dd sqrt(dd)): cosine over squared distance.  The winner is the facing, valid, visible view with the largest s; an exact tie
 *               goes to the lowest view id.
 *   OUTPUTS     per LISTED texel: view (int32; -1 when no view qualifies), pix = (row, col) (zero when none), rgb = the winner's panorama pixel copied bit
 *               for bit (zeros when none).  Unlisted texels are untouched.  The pick is nearest, never bilinear: it is what the reference's repack does,
 *               and an RGBE-born panorama's texels stay RGBE-born (the 4-byte texel layout above stays in force for a baked atlas).
 *
 * FLOAT32 OPERATION SEQUENCE (each operation separately rounded, no contraction; sqrt and / correctly rounded; pi32 = 3.14159274, hpi32 = 1.57079637, the
 * float32 neighbours of pi and pi / 2, off by less than 0.5 u relative):
 *     d_i = c_i - pos_i;   dd = (d_x d_x + d_y d_y) + d_z d_z;   nd = (n_x d_x + n_y d_y) + n_z d_z;   len = sqrt(dd)
 *     facing:  dd > 0  and  nd > cos_min * len
 *     t_i = ((W_i0 pos_x + W_i1 pos_y) + W_i2 pos_z) + W_i3;   r2 = (t_x t_x + t_y t_y) + t_z t_z;   r = sqrt(r2)      (r2 > 0 and finite, else no candidate)
 *     az = atan2f(t_x, t_z);   q = min(max(t_y / r, -1), 1);   el = asinf(q)
 *     x = ((az / pi32 + 1) * 0.5) * float(w);   y = ((1 - el / hpi32) * 0.5) * float(h);   col, row = floorf, clamped as floats to [0, w - 1] / [0, h - 1]
 *     s = nd / (dd * len);   a view replaces the best so far when s > best (views in ascending order)
 * ROUNDING BOUND (first order, u = 2^-24; the inputs pos, nrm, c, W are exact float32 values; the tests multiply every bound by their factor K):
 *     |dnd| <= 4 u N1,  N1 = sum_i |n_i d_i|       (d's rounding, three products, two adds)
 *     |ddd| <= 5 u dd;   |dlen| <= 3.5 u len;   the facing test is decided unless |nd - cos_min len| <= 4 u N1 + 4.5 u |cos_min| len
 *     |ds|  <= 4 u N1 / (dd len) + 10.5 u |s|      (dd len carries 5 + 3.5 + 1 u; the quotient one more)
 *     |dt_i| <= 4 u S_i,  S_i = |W_i0 pos_x| + |W_i1 pos_y| + |W_i2 pos_z| + |W_i3|
 *     |daz| <= (|dt_x| + |dt_z|) / hypot(t_x, t_z) + 12 u |az|          (atan2f taken as accurate to 6 ulp, OpenCL's limit): grows as 1 / hypot(t_x, t_z)
 *                                                                         towards the poles, where the column is unconstrained
 *     |dq|  <= |dt_y| / r + |q| ((|t_x| |dt_x| + |t_y| |dt_y| + |t_z| |dt_z|) / r^2 + 2.5 u) + u |q|
 *     |del| <= min(|dq| / sqrt(1 - (|q| + |dq|)^2), (pi / 2) sqrt(2 |dq|)) + 8 u |el|     (asinf to 4 ulp; asin is Hoelder-1/2 at +-1)
 *     |dx|  <= w (|daz| / (2 pi) + 3 u);   |dy| <= h (|del| / pi + 3 u)      (pi32's own error, the quotient, the sum, the product with w or h)
 * A pixel is the rule's pixel unless the exact (x, y) lies within (|dx|, |dy|) of a cell border.
 *
 *   pos, nrm [Nt,3] dev;  texel_ids [n_ids] i32 dev, nullable = all Nt texels (n_ids ignored; pass them in Morton order, dist_util.morton_order: a wave is
 *   64 consecutive ids); an id outside [0, Nt) is skipped.  cams dev [K,12]: W_k rows, then nothing else;  cam_pos dev [K,3];  panos dev [K,h,w,3];
 *   valid dev [K,h,w] u8, nullable;  K >= 1, h and w in 1..32768;  view [Nt] i32, pix [Nt,2] i32, rgb [Nt,3] f32 dev.
 *   stats dev u64[4], nullable: += (texel, view) pairs facing, pairs traced, pairs visible, texels assigned.
 * Caller-owned buffers, the caller's stream, no allocation and no synchronisation: the call records into a hipGraph. */
TEXIR_API int texir_atlas_bake(const texir_scene* scene, const float* pos /*dev*/, const float* nrm /*dev*/, const int32_t* texel_ids /*dev, nullable*/,
                       int64_t n_ids, int64_t Nt, const float* cams /*dev [K,12]*/, const float* cam_pos /*dev [K,3]*/, const float* panos /*dev [K,h,w,3]*/,
                       const uint8_t* valid /*dev [K,h,w], nullable*/, int32_t K, int32_t h, int32_t w, float cos_min, int32_t* view /*dev [Nt]*/,
                       int32_t* pix /*dev [Nt,2]*/, float* rgb /*dev [Nt,3]*/, uint64_t* stats /*dev [4], nullable*/, void* stream);
/* texir_atlas_bake with its VISIBILITY step put as the occlusion query texir_trace_occluded(pos, d, 0, 1) instead of a closest-hit query whose t is compared
 * with 1.  Same parameters, same errors, same house rules.  It returns the bits of texir_atlas_bake: view, pix, rgb and stats alike -- the two queries give
 * the same answer for every ray (see texir_trace_occluded), and the pairs counted are the same pairs.  What differs is the work: a traversal that stops at
 * the first accepted triangle and never looks beyond t = 1. */
TEXIR_API int texir_atlas_bake_any(const texir_scene* scene, const float* pos /*dev*/, const float* nrm /*dev*/, const int32_t* texel_ids /*dev, nullable*/,
                       int64_t n_ids, int64_t Nt, const float* cams /*dev [K,12]*/, const float* cam_pos /*dev [K,3]*/, const float* panos /*dev [K,h,w,3]*/,
                       const uint8_t* valid /*dev [K,h,w], nullable*/, int32_t K, int32_t h, int32_t w, float cos_min, int32_t* view /*dev [Nt]*/,
                       int32_t* pix /*dev [Nt,2]*/, float* rgb /*dev [Nt,3]*/, uint64_t* stats /*dev [4], nullable*/, void* stream);
/* The device form of the four repack*Texture gathers (tools/trans_hdr_tex.py:16-216: radiance, segmentation ids, albedo / roughness predictions of other
 * methods; the pixel is utils/Pano2Cube.py:57-82's): out[t, :] = imgs[view[t], pix[t,0], pix[t,1], :] bit for bit for the listed texels, zeros where
 * view[t] < 0 (or a code points outside the images).  imgs dev [K,h,w,C] f32, C in 1..4; out dev [Nt,C]; texel_ids as above.  Same house rules. */
TEXIR_API int texir_atlas_gather(const int32_t* view /*dev*/, const int32_t* pix /*dev*/, const int32_t* texel_ids /*dev, nullable*/, int64_t n_ids, int64_t Nt,
                       const float* imgs /*dev [K,h,w,C]*/, int32_t K, int32_t h, int32_t w, int32_t C, float* out /*dev [Nt,C]*/, void* stream);

/* ---- the fill of the texels the bake left unobserved (csrc/texfill.hip; no reference counterpart: the reference's capture pipeline delivers a complete
 * atlas).  A covered texel no panorama sees gets view = -1 and zeros from texir_atlas_bake; texir_texture_pad would fill it from its nearest neighbour IN UV
 * SPACE, which may be an unrelated chart.  texir_atlas_fill names, per hole, the nearest OBSERVED texel IN WORLD SPACE whose normal agrees with the hole's:
 * a hidden piece of floor continues the visible floor around it.  The caller copies the radiance (rgb[hole] = rgb[src[hole]]).
 *
 * THE RULE.  pos, nrm [Nt,3] float32: the texel G-buffer as texir_atlas_bake takes it (pos already offset, nrm raw, not renormalised).  source_ids: the
 * observed texels; hole_ids: the texels to decide; cos_fill in [0, 1]; max_dist > 0 (+inf allowed).  For hole t and source s, with e = pos[s] - pos[t],
 * nt = nrm[t], ns_ = nrm[s]:
 *   WITHIN      |e|^2 <= max_dist^2
 *   COMPATIBLE  nt.ns_ > 0  and  (nt.ns_)^2 >= cos_fill^2 |nt|^2 |ns_|^2      (the cosine test without a square root; a zero normal is compatible with
 *               nothing, because nt.ns_ > 0 fails)
 *   WINNER      the within, compatible source with the smallest |e|^2; an exact float32 tie goes to the lowest texel id
 *   OUTPUT      per LISTED hole: src[t] = the winner's texel id, or -1; dist2[t] = its dd (0 when none).  Unlisted texels are untouched.
 * The result is a pure function of the inputs: the order of either list, duplicates in them, the launch shape, `bounds`, the search structure and its cell
 * size do not change a bit.  An id outside [0, Nt) is skipped, in either list.  A texel in both lists is its own source (dd = 0) when its normal is not zero.
 *
 * FLOAT32 OPERATION SEQUENCE (each operation separately rounded, no contraction; only IEEE subtractions, products, sums and comparisons occur, so a
 * float32 restatement on any IEEE machine gives the same bits):
 *     e_i = pos[s]_i - pos[t]_i;   dd = (e_x e_x + e_y e_y) + e_z e_z
 *     ns = (nt_x ns_x + nt_y ns_y) + nt_z ns_z;   nn_t = (nt_x nt_x + nt_y nt_y) + nt_z nt_z;   nn_s likewise
 *     r2 = max_dist * max_dist;   c2 = cos_fill * cos_fill
 *     within:  dd <= r2;   compatible:  ns > 0  and  ns * ns >= (c2 * nn_t) * nn_s
 *     s replaces the best so far when dd < best, or dd == best and s < best's id
 * ROUNDING BOUND (first order, u = 2^-24; the inputs are exact float32 values; the tests multiply every bound by their factor K):
 *     |d dd| <= 5 u dd                              (e_i: one rounding, its square two more and one; the first sum one, the second one: (1 + u)^5 on the
 *                                                    x and y terms, (1 + u)^4 on z; every term is non-negative)
 *     |d ns| <= 3 u N1,  N1 = sum_i |nt_i ns_i|     (a product, two sums);   |d nn| <= 3 u nn  likewise
 *     the compatibility test is decided unless |ns^2 - c^2 nn_t nn_s| <= 6 u N1 |ns| + u ns^2 + 9 u c^2 nn_t nn_s
 *                                                   (2 |ns| |d ns| and the square's own rounding; c2 one, nn_t three, their product one, nn_s three, the
 *                                                    last product one)
 *     the range test is decided unless |dd - r2| <= 5 u dd + u r2
 *
 *   bounds: HOST float[6] = (min x, y, z, max x, y, z), finite: a box around the listed positions over which the sources are binned.  It steers speed only,
 *   never the result: positions outside it are searched through the border cells, slower and still exact.   cell: the edge of a grid cell, 0 = the
 *   library chooses (texir_atlas_fill_cell reports the edge a call will use: a given edge is doubled until the grid fits the workspace).
 *   src dev [Nt] i32;  dist2 dev [Nt] f32, nullable;  stats dev u64[2], nullable: += list entries decided (valid hole ids, a duplicate counts again), and
 *   those of them that were filled.  n_src == 0 is no error: every hole gets -1.  Pass the holes in Morton order (dist_util.morton_order): a wave owns 64
 *   consecutive holes and searches the cells around their common box.
 *   workspace: texir_atlas_fill_workspace_bytes(n_src, n_holes) bytes of device scratch, 16-byte aligned.
 * Caller-owned buffers, the caller's stream, no allocation and no synchronisation: the call records into a hipGraph. */
TEXIR_API int64_t texir_atlas_fill_workspace_bytes(int64_t n_src, int64_t n_holes);
TEXIR_API float texir_atlas_fill_cell(const float* bounds /*host [6]*/, int64_t n_src, float cell);
TEXIR_API int texir_atlas_fill(const float* pos /*dev*/, const float* nrm /*dev*/, int64_t Nt, const int32_t* source_ids /*dev*/, int64_t n_src,
                       const int32_t* hole_ids /*dev*/, int64_t n_holes, const float* bounds /*host [6]*/, float cos_fill, float max_dist, float cell,
                       int32_t* src /*dev [Nt]*/, float* dist2 /*dev [Nt], nullable*/, uint64_t* stats /*dev [2], nullable*/, void* workspace /*dev*/,
                       void* stream);

/* ---- inserted emitters: the direct irradiance of NEW area lights per texel (csrc/irtlight.hip).  The irradiance split recolours light that is in the
 * capture; this adds light that is not.  The reference's relighting demo leaves its "moving" half -- an emitter at a new position per frame -- to an
 * external renderer (tools/relighting_varying.py).  Irradiance is linear in emitted radiance: an emitter of radiance c adds c * F to 0_irr_texture.hdr,
 * with F the per-texel geometry-and-visibility factor below, traced once.  Direct light only: no bounce of the new light is computed.
 *
 * THE RULE.  Per texel: x = pos (already offset), n = nrm (RAW, as the IrT estimator uses it), the texel's Cranley-Patterson shift (the one
 * texir_irt_generate takes).  Per light k: a record of 16 float32 in DEVICE memory (a recorded graph is replayed with moved lights, so the host never
 * validates a record):
 *     [0] kind: 0.0f = parallelogram ("quad"), 1.0f = sphere      [1..3] p: the quad's corner o, or the sphere's centre c
 *     [4..6] a: a quad edge; sphere: a.x = radius r, a.y and a.z ignored      [7..9] b: the other quad edge (sphere: ignored)      [10..15] reserved, ignored
 *   A record with another kind, a non-finite word among those its kind uses, a quad with a x b = 0 (or not finite) or a sphere with r <= 0 (or 4 pi r^2 not
 *   finite) yields F = 0 for that light, and no ray is traced for it.
 *   For sample i = 0 .. S-1:
 *   SAMPLE      s0 = shift_wrap_clamp(ham0(i, S), shift.x), s1 = shift_wrap_clamp(ham1(i), shift.y): the Hammersley point and the wrap of
 *               texir_irt_generate (csrc/device_common.h), in (0, 1).
 *   QUAD        y = (o + s0 a) + s1 b;  m = a x b, RAW: its length is the area, its direction the emitting side (one-sided: a two-sided panel is two
 *               records);  w = 1.
 *   SPHERE      z = 1 - 2 s0;  q = sqrt(max(0, 1 - z z));  phi = 2 pi s1;  u = (q cos phi, q sin phi, z);  y = c + r u;  m = u;  w = 4 pi r^2.
 *   GEOMETRY    d = y - x;  dd = d.d;  nd = n.d;  md = -(m.d);  g = (nd md) / (dd dd) when nd > 0, md > 0, dd > 0 and the quotient is finite, else g = 0.
 *               A ray is traced iff g > 0.  (Two cosines over the squared distance, times the area element: there is no square root in the quad path.)
 *   VISIBILITY  the ray (org = x, dir = d): V = 0 iff its closest hit has t < t_max, else V = 1.  Closest hit is what texir_trace_shade reports (Embree
 *               semantics: t > 0, t in units of |dir|); no t_min, because pos is already offset.  t_max = 1 is the bake's rule; scene.Scene.irt_lights
 *               defaults to 0.999 so that a light laid onto a surface is not shadowed by that surface.
 *   RESULT      acc = sum_i V_i g_i in ascending i in ONE float32 accumulator;  F[k][texel] = (acc * w) / float(S).  The irradiance under an emitted
 *               radiance c_k is c_k F[k].
 *   WRITES      every LISTED texel is written for every k, zeros included.  Unlisted texels are untouched.  An id outside [0, Nt) is not a texel.
 * F is a pure function of the inputs: no atomics on results, no workspace; list order, duplicates, launch shape and stream do not change a bit.
 *
 * FLOAT32 OPERATION SEQUENCE (each operation separately rounded, no contraction; sqrt and / correctly rounded; tau32 = 6.28318548 and fourpi32 = 12.5663710,
 * the float32 neighbours of 2 pi and 4 pi, off by less than 0.5 u relative).  s0 and s1 use IEEE additions, comparisons and one exact scaling only (ham0
 * of an S that is no power of two: one float64 quotient rounded to float32), so a restatement on any IEEE machine gives the same bits; the bounds below start
 * from them as exact float32 values.
 *     quad:    y_i = (o_i + s0 * a_i) + s1 * b_i;   m_x = a_y * b_z - a_z * b_y,  m_y = a_z * b_x - a_x * b_z,  m_z = a_x * b_y - a_y * b_x
 *     sphere:  z = 1 - 2 * s0;   q = sqrt(max(0, 1 - z * z));   phi = tau32 * s1;   u = (q * cosf(phi), q * sinf(phi), z);   y_i = c_i + r * u_i;   m = u;
 *              w = (fourpi32 * r) * r
 *     d_i = y_i - x_i;   dd = (d_x d_x + d_y d_y) + d_z d_z;   nd = (n_x d_x + n_y d_y) + n_z d_z;   md = -((m_x d_x + m_y d_y) + m_z d_z)
 *     g = (nd * md) / (dd * dd);   acc = acc + g  (visible samples, ascending i);   F = (acc * w) / float(S)
 * ROUNDING BOUND (first order, u = 2^-24; the inputs x, n, the record, s0, s1 are exact float32 values; the tests multiply every bound by their factor K).
 * With e_i the bound of d_i and f_i the bound of m_i:
 *     quad:    e_i = u (3 Y_i + |d_i|),  Y_i = |o_i| + |s0 a_i| + |s1 b_i|      (two products, two sums, the difference)
 *              f_x = 2 u (|a_y b_z| + |a_z b_y|), f_y and f_z alike              (two products, the difference)
 *     sphere:  |dz| <= u |z|;   A = 1 - z z:  |dA| <= 2 |z| |dz| + u z z + u |A|;   |dq| <= min(|dA| / (2 sqrt(max(A - |dA|, 0))), sqrt(|dA|)) + u q
 *              |dphi| <= 1.5 u phi;   cosf, sinf taken as accurate to 4 ulp (OpenCL's limit):  |dcos| <= |dphi| + 8 u |cos phi|,  |dsin| alike
 *              f_x = |cos phi| |dq| + q |dcos| + u |u_x|,  f_y alike with sin,  f_z = |dz|
 *              e_i = r f_i + u (|r u_i| + |y_i| + |d_i|)                          (the product, the sum, the difference)
 *     |ddd| <= 3 u dd + 2 sum_i |d_i| e_i
 *     |dnd| <= 3 u N1 + sum_i |n_i| e_i,  N1 = sum_i |n_i d_i|;   the test nd > 0 is decided unless |nd| <= |dnd|
 *     |dmd| <= 3 u M1 + sum_i |m_i| e_i + sum_i |d_i| f_i,  M1 = sum_i |m_i d_i|;   the test md > 0 is decided unless |md| <= |dmd|
 *     |dg|  <= |g| (3 u + 2 |ddd| / dd) + (|dnd| |md| + |nd| |dmd|) / dd^2       (the two products and the quotient)
 *     the direction of the ray carries e_i per component
 *     |dF|  <= (w / S) ((S + 4) u sum_i |g_i| + sum_i |dg_i|)                     (S - 1 additions; w: 2.5 u; the product and the quotient by S)
 *
 *   pos, nrm [Nt,3], shift [Nt,2] dev;  texel_ids [n_ids] i32 dev, nullable = all Nt texels (n_ids ignored; pass them in Morton order: a wave is 64
 *   consecutive ids);  lights dev [K][16], K in 0..8;  S in 1..65536;  t_max finite;  F dev [K][Nt].
 *   stats dev u64[2], nullable: += samples with g > 0 (the rays traced), and the visible ones; one atomic add per wave and counter.
 * K outside 0..8 (reported before any null buffer), S outside 1..65536, a t_max that is not finite, negative counts and a null buffer are errors with a
 * texir_last_error() text.  K = 0 and an empty list return 0 and write nothing.
 * Caller-owned buffers, the caller's stream, no allocation and no synchronisation: the call records into a hipGraph. */
TEXIR_API int texir_irt_lights(const texir_scene* scene, const float* pos /*dev [Nt,3]*/, const float* nrm /*dev [Nt,3], raw*/, const float* shift /*dev [Nt,2]*/,
                       const int32_t* texel_ids /*dev, nullable = all Nt*/, int64_t n_ids, int64_t Nt, const float* lights /*dev [K][16]*/, int32_t K /*0..8*/,
                       int32_t S /*1..65536*/, float t_max, float* F /*dev [K][Nt]*/, uint64_t* stats /*dev [2], nullable*/, void* stream);
/* texir_irt_lights with its VISIBILITY step put as the occlusion query texir_trace_occluded(x, d, 0, t_max) instead of a closest-hit query whose t is
 * compared with t_max.  Same parameters, same errors, same house rules.  It returns the bits of texir_irt_lights: F and stats alike -- the two queries give
 * the same answer for every ray (see texir_trace_occluded), and the rays counted are the same rays. */
TEXIR_API int texir_irt_lights_any(const texir_scene* scene, const float* pos /*dev [Nt,3]*/, const float* nrm /*dev [Nt,3], raw*/, const float* shift /*dev [Nt,2]*/,
                       const int32_t* texel_ids /*dev, nullable = all Nt*/, int64_t n_ids, int64_t Nt, const float* lights /*dev [K][16]*/, int32_t K /*0..8*/,
                       int32_t S /*1..65536*/, float t_max, float* F /*dev [K][Nt]*/, uint64_t* stats /*dev [2], nullable*/, void* stream);

/* ---- inserted emitters: the SPECULAR response to new area lights per pixel (csrc/speclight.hip).  texir_irt_lights gives the factor F of the diffuse
 * response; a view relit by new lamps is  rgb + sum_k colour_k (albedo / pi F[k] + R[k]),  and this call gives R.  The material model's Fresnel term is
 * the scalar 0.04 + 0.96 2^(..), so the GGX response to a light of radiance colour_k is colour_k times a SCALAR per-pixel factor.  The light is neither
 * in the mesh nor in the radiance texture, so texir_spec_forward cannot see it.  Sampling the lobe alone misses a small lamp from a rough surface,
 * sampling the light's area alone aliases on a glossy one: the estimate combines the two by the balance heuristic (Veach), both techniques at the SAME
 * Hammersley point.  Direct light only: no bounce of the new light.  The reference has no counterpart (tools/relighting_varying.py leaves the scene to an
 * external renderer).
 *
 * THE RULE.  Per pixel p: x = pos (already offset by the caller), n = nrm (RAW), r = rough, the pixel's Cranley-Patterson shift (the one
 * texir_spec_forward takes), the camera c (3 floats in DEVICE memory).  v = (c - x) / max(|c - x|, 1e-4);  the frame (nh, U, V) = make_frame(n) of
 * texir_generate_dir, nh = n / (|n| + 1e-6).  Light records: the 16-float DEVICE records of texir_irt_lights, same layout, same validation; a record
 * that rule refuses yields R = 0 for that light, and no ray is traced for it.
 *   For sample i = 0 .. S-1:  (s0, s1) as in texir_irt_lights, the same point for both techniques.
 *   LIGHT SAMPLE  y, m, w, d = y - x, dd, nd, md exactly as texir_irt_lights has them.  Dead (term 0, no ray) unless nd > 0, md > 0, dd > 0.
 *                 lh = d / sqrt(dd);  h = (v + lh) / |v + lh|, dead when |v + lh|^2 is not > 0.
 *                 vdh, ndl, ndh, ndv, Fresnel, k = (r + 1)^2 / 8, G and brdf = Fr G / max(4 ndl ndv, ceps) as texir_spec_forward has them: the dots with
 *                 the RAW n, clamped to [0, 1].
 *                 D = a2 / (pi den^2),  a2 = r^4,  den = a2 c^2 + s2,  c = nh . h,  s2 = |nh x h|^2;  D = 0 when c <= 0.  The frame's nh, because that is
 *                 the density generate_dir samples; the cross-product form, because c^2 (a2 - 1) + 1 loses every digit at r = 0.01 near the peak.
 *                 pL = dd sqrt(dd) / (w md)  (solid-angle density of the area sample; the quad's m carries its area, w = 1)
 *                 pB = D c / max(4 vdh, ceps)  (solid-angle density of the lobe sample), but pB = 0 in the lobe's CORE, s2 < (1 - ctmax^2) (nh . nh) with
 *                 ctmax = 1 - 1e-6 (on sin^2: cos^2 next to 1 has no digits left): generate_dir clamps cos(theta_h) to ctmax, so half vectors within 1.4e-3 rad of nh are never sampled (their mass
 *                 lands on the rim, where it is no density).  At r = 0.01 that is 99.5 % of the lobe: without this the estimate loses it.
 *                 term = (D brdf ndl) / (pL + pB)
 *   LOBE SAMPLE   Dead when the chain's cos(theta_h) = sqrt((1 - s0) / (1 + (a2 - 1) s0)) exceeds ctmax BEFORE its clamp: a rim sample, no draw from a
 *                 density (texir_spec_forward counts it; this estimate leaves the core to the light samples, so that it converges to the GGX integral).
 *                 The condition is taken cleared of root and quotient, (1 - s0) (1 - ctmax^2) > ctmax^2 a2 s0: float32 keeps its digits in this form,
 *                 while the chain's own comparison is within rounding of its edge for every s0 near the rim.
 *                 l, its weight wv = brdf ndl 4 vdh / max(ndh, ceps), the sampled h and the clamped vdh from the operations of texir_spec_forward.
 *                 Dead unless wv > 0.  The ray (x, l) meets light k analytically:
 *                 quad    ml = m . l;  e = o - x;  tL = (m . e) / ml;  d = tL l;  q = d - e;  u = q . ua,  v' = q . vb  with the reciprocal basis
 *                         ua = (b x m) / (m . m),  vb = (m x a) / (m . m);  hit iff -ml > 0, tL > 0, 0 <= u <= 1, 0 <= v' <= 1.
 *                 sphere  e = c - x;  b = l . e;  ll = l . l;  cc = e . e - r_s^2;  disc = b b - ll cc;  hit iff cc > 0 (x outside), b > 0, disc >= 0 and
 *                         tL = cc / (b + sqrt(disc)) > 0  (the nearer root, without the cancellation of b - sqrt(disc));  d = tL l;  m = (d - e) / r_s.
 *                 dd = d . d,  md = -(m . d);  dead unless md > 0, dd > 0.  pL as above, D and c at the SAMPLED h, pB = D c / max(4 vdh, ceps).
 *                 term = (wv pB) / (pL + pB)
 *   A term that is not finite or not > 0 is 0.  A ray is traced iff the term is > 0.
 *   VISIBILITY    the question of texir_irt_lights for the segment (x, d): V = 0 iff the closest hit has t < t_max.  scene.Scene.spec_lights defaults to 0.999.
 *   RESULT        acc = for ascending i: the light sample's V term, then the lobe sample's V term, in ONE float32 accumulator;  R[k][p] = acc / float(S).
 *   WRITES        every LISTED pixel is written for every k, zeros included.  Unlisted pixels are untouched.  An id outside [0, P) is not a pixel.
 * R is a pure function of the inputs: no atomics on results, no workspace; list order, duplicates, launch shape and stream do not change a bit.
 *
 * FLOAT32 OPERATION SEQUENCE (each operation separately rounded, no contraction; sqrt and / correctly rounded; pi32 = 3.14159274, tau32 and fourpi32 of
 * texir_irt_lights; clamp01(t) = min(max(t, 0), 1)).  y, m, w, d, dd, nd, md: the sequence of texir_irt_lights.  l, wv, h, vdh of the lobe sample: the
 * sequence of texir_spec_forward's sample chain (csrc/spec_sample.h), value part.
 *     pixel:   v_i = c_i - x_i;  lv = max(sqrt((v_x v_x + v_y v_y) + v_z v_z), 1e-4);  v_i = v_i / lv;  a1 = r * r;  a2 = a1 * a1
 *              ctmax = 1 - 1e-6 (float32: 1 - 17 * 2^-24);  core_s2 = 2.02655690e-6 * ((nh_x nh_x + nh_y nh_y) + nh_z nh_z)   (the constant: 1 - ctmax^2)
 *              ndv = clamp01((n_x v_x + n_y v_y) + n_z v_z);  r1 = r + 1;  k = (r1 * r1) * 0.125;  omk = 1 - k;  g1v = ndv / max(omk * ndv + k, ceps)
 *     record:  quad: mm = (m_x m_x + m_y m_y) + m_z m_z;  ua_x = (b_y * m_z - b_z * m_y) / mm, ..;  vb_x = (m_y * a_z - m_z * a_y) / mm, ..   (cyclic)
 *              e_i = p_i - x_i  (p = the record's point o or c);  sphere: rr2 = r_s * r_s
 *     D(h):    c = (nh_x h_x + nh_y h_y) + nh_z h_z;  q_x = nh_y * h_z - nh_z * h_y, ..;  s2 = (q_x q_x + q_y q_y) + q_z q_z;  den = a2 * (c * c) + s2
 *              D = a2 / ((pi32 * den) * den)
 *     light:   ls = sqrt(dd);  lh_i = d_i / ls;  h_i = v_i + lh_i;  hh = (h_x h_x + h_y h_y) + h_z h_z;  hl = sqrt(hh);  h_i = h_i / hl
 *              vdh = clamp01((h_x v_x + h_y v_y) + h_z v_z);  ndl = clamp01((lh_x n_x + lh_y n_y) + lh_z n_z)
 *              e = ((vdh * -5.55472) - 6.98316) * vdh;  fr = 0.04 + 0.96 * exp2f(e);  g1l = ndl / max(ndl * omk + k, ceps)
 *              brdf = (fr * (g1l * g1v)) / max(ndl * (4 * ndv), ceps);  pL = (dd * ls) / (w * md);  pB = s2 < core_s2 ? 0 : (D * c) / max(4 * vdh, ceps)
 *              term = ((D * brdf) * ndl) / (pL + pB)
 *     lobe:    dead when (1 - s0) * 2.02655690e-6 > ((ctmax * ctmax) * a2) * s0
 *              quad:   ml = (m_x l_x + m_y l_y) + m_z l_z;  me = (m_x e_x + m_y e_y) + m_z e_z;  tL = me / ml;  d_i = tL * l_i;  q_i = d_i - e_i
 *                      u = (q_x ua_x + q_y ua_y) + q_z ua_z;  v' alike with vb
 *              sphere: b = (l_x e_x + l_y e_y) + l_z e_z;  ll = (l_x l_x + l_y l_y) + l_z l_z;  cc = ((e_x e_x + e_y e_y) + e_z e_z) - rr2
 *                      disc = b * b - ll * cc;  tL = cc / (b + sqrt(disc));  d_i = tL * l_i;  m_i = (d_i - e_i) / r_s
 *              dd = (d_x d_x + d_y d_y) + d_z d_z;  md = -((m_x d_x + m_y d_y) + m_z d_z);  pL = (dd * sqrt(dd)) / (w * md);  pB as above
 *              term = (wv * pB) / (pL + pB)
 *     acc = acc + term  (visible terms; per i the light sample's, then the lobe sample's);   R = acc / float(S)
 * ROUNDING BOUND (first order, u = 2^-24; the inputs x, n, r, c, the record, s0, s1 are exact float32 values; the tests multiply every bound by their
 * factor K).  Number the rounded operations of the sequence above that feed a quantity y -- every sum, product, quotient, sqrt, every constant float32 has
 * to round, sinf, cosf, exp2f -- j = 1 .. J, with exact results x_j.  Replace x_j by x_j (1 + e_j).  To first order
 *     |dy| <= sum_j |dy / de_j| (u + 2^-126 / |x_j|)
 * (one rounding, or one flushed denormal, per operation; scalings by 2, 4, 1/8, negations, selections, min, max and products with 0 or 1 are exact).  This
 * is a running error bound: it is evaluated AT the operands of the case, so it is as wide as the conditioning there demands and no wider -- the
 * cross-product form of den keeps it useful at r = 0.01 on the highlight's centre, where the textbook form's bound exceeds the value.  Every decision
 * above (nd > 0, md > 0, c > 0, the two core tests, -ml > 0, tL > 0, the four edge tests of u and v', cc > 0, b > 0, disc >= 0, the sides of every clamp) is decided unless
 * the quantity lies within its own bound of the edge; the ray's direction carries the bound of d_i.  A decided live term lies within its bound of its
 * exact value, a decided dead one is 0, an undecided one lies in [0, value + bound]; a clamp is continuous, so a term with an undecided clamp lies within the
 * bounds of the values of its two sides.  With T the sum of the terms' upper ends,
 *     |dR| <= (1 / S) (sum of the terms' bounds + (2 S + 2) u T)                    (2 S - 1 additions, the quotient by S)
 *
 *   pos, nrm [P,3], rough [P], shift [P,2] dev;  cam [3] dev;  pixel_ids [n_ids] i32 dev, nullable = all P pixels (n_ids ignored);  lights dev [K][16],
 *   K in 0..8;  S in 1..65536;  t_max finite;  clamp_eps finite, > 0 (the floor of the denominators: 1e-14 in training, 1e-6 in evaluation);  R dev [K][P].
 *   stats dev u64[2], nullable: += terms > 0 (the rays traced), and the visible ones; one atomic add per wave and counter.
 * Errors as texir_irt_lights reports them: K outside 0..8 before any null buffer, S, t_max, negative counts, a null buffer.  K = 0 and an empty list return
 * 0 and write nothing.  Caller-owned buffers, the caller's stream, no allocation and no synchronisation: the call records into a hipGraph, and the
 * records and the camera are read again on every replay. */
TEXIR_API int texir_spec_lights(const texir_scene* scene, const float* pos /*dev [P,3]*/, const float* nrm /*dev [P,3], raw*/, const float* rough /*dev [P]*/,
                       const float* shift /*dev [P,2]*/, const float* cam /*dev [3]*/, const int32_t* pixel_ids /*dev, nullable = all P*/, int64_t n_ids, int64_t P,
                       const float* lights /*dev [K][16]*/, int32_t K /*0..8*/, int32_t S /*1..65536*/, float t_max, float clamp_eps, float* R /*dev [K][P]*/,
                       uint64_t* stats /*dev [2], nullable*/, void* stream);
/* texir_spec_lights with its VISIBILITY step put as the occlusion query texir_trace_occluded(x, d, 0, t_max).  Same parameters, same errors, same house
 * rules; it returns the bits of texir_spec_lights, R and stats alike (see texir_irt_lights_any). */
TEXIR_API int texir_spec_lights_any(const texir_scene* scene, const float* pos /*dev [P,3]*/, const float* nrm /*dev [P,3], raw*/, const float* rough /*dev [P]*/,
                       const float* shift /*dev [P,2]*/, const float* cam /*dev [3]*/, const int32_t* pixel_ids /*dev, nullable = all P*/, int64_t n_ids, int64_t P,
                       const float* lights /*dev [K][16]*/, int32_t K /*0..8*/, int32_t S /*1..65536*/, float t_max, float clamp_eps, float* R /*dev [K][P]*/,
                       uint64_t* stats /*dev [2], nullable*/, void* stream);

/* ---- inserted emitters BEHIND inserted mesh objects (csrc/irtlightmesh.hip, csrc/speclightmesh.hip): an inserted table darkens the captured light under
 * it (texir_irt_shadow_mesh); with these two calls it also shadows the inserted lamp above it.
 *
 * THE RULE.  texir_irt_lights_mesh is texir_irt_lights, texir_spec_lights_mesh is texir_spec_lights, each with ONE changed step.  SAMPLE, QUAD, SPHERE,
 * GEOMETRY, the LIGHT SAMPLE and LOBE SAMPLE terms, RESULT (the order of the one float32 accumulator), WRITES, the validation of a record and the FLOAT32
 * OPERATION SEQUENCES are the text of those rules, word for word.  New inputs, texir_irt_shadow_mesh's with their meaning unchanged:
 *   occluders   Q in 0..8 geometry-only scene handles (HOST array); their device pointers and boxes enter the kernel arguments by value.
 *   instances   J in 0..8: instance j = (inst_obj[j] in 0..Q-1, HOST; W[j] = inst_world_to_obj + 12 j, a WORLD-TO-OBJECT 3 x 4 row-major float32 matrix in
 *               DEVICE memory: a replayed graph sees a moved object, so the host never reads a matrix).  Two instances may name one occluder.
 *   flags       bit 0 switches the prefilter off.
 * The changed step:
 *   VISIBILITY  of the segment (x, d) with bound t_max.  V = 0 iff the scene occludes it, texir_trace_occluded(scene, x, d, 0, t_max) -- which that rule
 *               proves equal to `the closest hit has t < t_max`, the form texir_irt_lights states -- OR some instance j blocks it:
 *               texir_trace_occluded(occluder[inst_obj[j]], o', d', 0, t_max), with (o', d') the OBJECT-SPACE RAY of texir_irt_shadow_mesh, its FLOAT32
 *               OPERATION SEQUENCE unchanged (row by row, nothing normalised: t along (o', d') is t along (x, d), so the bound t_max survives the affine
 *               map).  A matrix with a non-finite entry never blocks.  An object beyond the light's sample point (every accepted t >= t_max) does not
 *               block.  Overlapping instances are a union: a segment is blocked once.
 *   Every question is put as the occlusion query; the entry points have no closest-hit twin.  The bits are those of the closest-hit form by the argument of
 *   texir_trace_occluded, and the any-hit form is the one profiles/occlusion.json measured faster.
 * ROUNDING BOUND.  The union of the two rules': the bound e of d of texir_irt_lights (for the lobe sample of texir_spec_lights: the running bound of its d)
 * is carried into object space by  |dd'_r| <= sum_c |W[r][c]| e_c + 3 u sum_c |W[r][c] d_c|  (o' is exact, as in texir_irt_shadow_mesh), and a triangle's t
 * along (o', d' +- dd') carries the occlusion query's own bound_t for that direction bound: instance j certainly blocks when a robustly hit triangle has
 * t + bound_t < t_max, possibly when one has t - bound_t < t_max.  Everything else of the two bounds is unchanged.
 * PREFILTER.  A lane asks instance j only if (o', d') passes texir_irt_shadow_mesh's box test, the proven one, unchanged: it never fails where the
 * traversal accepts a triangle, whatever t_max.  (The slab interval is NOT additionally required to meet (0, t_max): that needs its own proof.)
 * ORDER OF THE QUESTIONS.  One traversal, walked in a wave-uniform loop over {instance 0 .. J-1 whose box some lane's segment meets, scene}: the instances
 * first.  The answers are functions of the segment alone and V is their OR, so the order changes no bit; it was picked by reasoning, nobody has measured
 * it: an object's tree is shallow and the room's is deep, and where an object shadows all of a wave's 64 neighbouring points the deep walk is not taken.
 *   stats dev u64[2], nullable: += samples with g > 0 (terms > 0 for the specular rule), and the visible ones: functions of the inputs alone, whatever order
 *   the kernel asks its questions in (a blocked segment counts as traced once, however many questions it took).
 * CONSEQUENCES (the tests hold them).
 *   - With J = 0, with every matrix non-finite, or where no instance blocks a sample, F, R and stats are bit for bit those of texir_irt_lights /
 *     texir_spec_lights (and of their _any forms).
 *   - Where every live sample of a texel is blocked, the result is exactly +0.
 *   - Float32 addition is monotone and the terms are non-negative: per value F_mesh <= F and R_mesh <= R exactly.
 *   - List order, duplicates, list cuts, launch shape, stream, graph replay and the prefilter bit change no bit.
 * Errors: those of texir_irt_lights / texir_spec_lights, and texir_irt_shadow_mesh's conditions on the objects in its text style -- Q or J outside 0..8, an
 * inst_obj[j] outside 0..Q-1, a null occluder (all reported before any other argument); the scene or an occluder without the 4-wide tree, an occluder on
 * another device than the scene.  K = 0 and an empty list return 0 and write nothing.  Caller-owned buffers, the caller's stream, no allocation, no
 * synchronisation, no workspace: the calls record into a hipGraph; records, camera and matrices are read again on every replay.
 * Not computed: the bounce G's own rays (they still ignore the objects).  (The object drawn in a view: texir_gbuffer_cast_mesh.) */
TEXIR_API int texir_irt_lights_mesh(const texir_scene* scene, const float* pos /*dev [Nt,3]*/, const float* nrm /*dev [Nt,3], raw*/, const float* shift /*dev [Nt,2]*/,
                       const int32_t* texel_ids /*dev, nullable = all Nt*/, int64_t n_ids, int64_t Nt, const float* lights /*dev [K][16]*/, int32_t K /*0..8*/,
                       int32_t S /*1..65536*/, float t_max, const texir_scene* const* occluders /*host [Q]*/, int32_t Q /*0..8*/,
                       const int32_t* inst_obj /*host [J]*/, const float* inst_world_to_obj /*dev [J][12]*/, int32_t J /*0..8*/,
                       uint32_t flags /*bit 0: prefilter off*/, float* F /*dev [K][Nt]*/, uint64_t* stats /*dev [2], nullable*/, void* stream);
TEXIR_API int texir_spec_lights_mesh(const texir_scene* scene, const float* pos /*dev [P,3]*/, const float* nrm /*dev [P,3], raw*/, const float* rough /*dev [P]*/,
                       const float* shift /*dev [P,2]*/, const float* cam /*dev [3]*/, const int32_t* pixel_ids /*dev, nullable = all P*/, int64_t n_ids, int64_t P,
                       const float* lights /*dev [K][16]*/, int32_t K /*0..8*/, int32_t S /*1..65536*/, float t_max, float clamp_eps,
                       const texir_scene* const* occluders /*host [Q]*/, int32_t Q /*0..8*/, const int32_t* inst_obj /*host [J]*/,
                       const float* inst_world_to_obj /*dev [J][12]*/, int32_t J /*0..8*/, uint32_t flags /*bit 0: prefilter off*/, float* R /*dev [K][P]*/,
                       uint64_t* stats /*dev [2], nullable*/, void* stream);

/* ---- the shadow inserted emitters' BODIES and inserted mesh OBJECTS cast in the SPECULAR term of the captured light, per pixel (csrc/specshadow.hip).
 * texir_irt_shadow and texir_irt_shadow_mesh take the intercepted light from the DIFFUSE term; a table in front of a window still left the glossy floor
 * mirroring the window through it.  This call gives that missing term, for bodies and instances in ONE call and as a union.
 *
 * THE RULE.  Inputs: normal (raw), rough, points, cam, shift, P, S and clamp_eps exactly as texir_spec_forward takes them; pixel_ids (device, nullable) with
 * n_ids as texir_spec_lights has them; bodies: Kb in 0..8 records of 16 float32 in DEVICE memory, the layout and validity rule of texir_irt_shadow;
 * occluders (HOST, Q in 0..8), inst_obj (HOST) and inst_world_to_obj (DEVICE [J][12], J in 0..8) as texir_irt_shadow_mesh takes them; sets: M in 1..8
 * uint32 masks in DEVICE memory -- bit k (0..7) = body k, bit 8 + j = instance j; body bits at or above Kb, instance bits at or above 8 + J and bits 16..31
 * are ignored; a mask that is zero after that yields zeros.  flags bit 0: prefilter off.
 *   SAMPLES AND RAYS  those of spec_kernel<false, 4>, texir_spec_forward's kernel on a 4-wide tree: sample i = 0..S-1 with s0, s1 from ham0 / ham1 and
 *               shift_wrap_clamp; spec_sample (csrc/spec_sample.h) on the RAW normal and on v = (cam - x) / max(|cam - x|, 1e-4) gives the direction l and the
 *               weight w_i; the ray (x = points, l), not normalised; the closest hit t_s with the acceptance test slot >= 0 && t > 1e-4; L_i from the scene's
 *               OWN texture through the hit shader, in any layout.
 *   BLOCKED     body k meets sample i with t_b < t_s under the BODY INTERSECTION RULE of texir_irt_shadow with d = l, the same float32 operation sequence (the
 *               quad two-sided, the sphere a solid ball, t_b = 0 from inside).  Instance j blocks sample i under the BLOCKED rule of texir_irt_shadow_mesh:
 *               its OBJECT-SPACE RAY sequence, then an accepted triangle with 0 < t < t_s.  B_i = the 16-bit mask of both (bodies in bits 0..7, instances in
 *               bits 8..15).
 *   RESULT      lost[m][p] = (1/S) sum_i L_i w_i [sample i has an accepted hit AND (sets[m] & B_i) != 0]: overlapping bodies and instances are a union, not
 *               a sum.  The relit view takes it from the pixel first: max(rgb - lost[m], 0) (texir_code_amd/irtlight.py add_view(lost_spec=)).
 *   REDUCTION   spec_kernel's.  The lanes-per-pixel rule of the specular launcher (S when S is a power of two <= 64, else 64; TEXIR_SPEC_LPP is honoured);
 *               lane sl of a pixel takes the samples q * lpp + sl; per lane acc_m[c] += L[c] * w in ascending pass q, a sample that is not blocked adds
 *               nothing; then the xor butterfly over the pixel's lanes (offsets lpp / 2, ..., 1); then acc / (float)S.
 *   CONSEQUENCES (the tests hold them)
 *             - for a pixel and a set under which EVERY sample with an accepted hit is blocked, and every w_i is finite, lost[m] has, bit for bit, the value
 *               texir_spec_forward writes into rgb with irr = 0, albedo = 0: the same additions in the same order.
 *             - for a set no sample's ray meets it is exactly +0.
 *             - with a non-negative texture 0 <= lost[m] <= that specular term, per value.
 *             - lost of a superset mask is >= lost of a subset per value: the same non-negative terms are added in the same order and rounding is monotone.
 *             - the result is a pure function of the inputs: list order, duplicates, ids outside [0, P) (nothing is read or written for them), launch
 *               shape, stream, graph replay and the prefilter change no bit.
 * ROUNDING BOUND.  The three existing texts hold unchanged: the direction and weight bounds of the specular sample chain (tests/spec_cases.py derives them);
 * the body bound of texir_irt_shadow with e_i the chain's direction bound; the instance bound of texir_irt_shadow_mesh with the same e_i.
 * PREFILTER.  texir_irt_shadow_mesh's box test, unchanged.  A lane whose ray meets no body and no padded box traces nothing.
 *   out [M][P][3] dev: only listed pixels are written, zeros included (Kb = J = 0: zeros).  pixel_ids NULL => all P (n_ids ignored); a non-null list with
 *   n_ids == 0 writes nothing.
 *   stats dev u64[3], nullable: [0] += samples whose ray met some body or some instance's padded box (= the scene rays traced; with the prefilter off every
 *   valid instance counts as met); [1] += occluder queries really issued: a sample a body already blocks asks only the instances that can still add it to
 *   a set no blocking body is in (the others change no bit of out), so [1] depends on the sets and is at most the sibling call's count; [2] += blocked
 *   samples with an accepted hit (B_i != 0 among the bodies and the instances asked: a sample counts once, whichever set or none it falls in).  One atomic
 *   add per wave and counter.
 * No workspace.  Caller-owned buffers, the caller's stream, no allocation, no synchronisation, no atomics on results: the call records into a hipGraph, and a
 * replay sees moved bodies, matrices and sets.  Errors, each reported before any null buffer is touched, with a texir_last_error() text: Kb, Q or J outside
 * 0..8, M outside 1..8, inst_obj[j] outside 0..Q-1, S < 1, a null buffer, the scene or an occluder without the 4-wide tree (TEXIR_BVH_WIDTH=2), an occluder
 * on another device than the scene.
 * Not computed: the body drawn in the view (the object: texir_gbuffer_cast_mesh); the shadow on the bounce's own rays; a training backward through lost. */
TEXIR_API int texir_spec_shadow(const texir_scene* scene, const float* normal /*dev [P,3], raw*/, const float* rough /*dev [P]*/, const float* points /*dev [P,3]*/,
                       const float* cam /*dev [3]*/, const float* shift /*dev [P,2]*/, const int32_t* pixel_ids /*dev, nullable = all P*/, int64_t n_ids, int64_t P,
                       int32_t S, float clamp_eps, const float* bodies /*dev [Kb][16]*/, int32_t Kb /*0..8*/, const texir_scene* const* occluders /*host [Q]*/,
                       int32_t Q /*0..8*/, const int32_t* inst_obj /*host [J]*/, const float* inst_world_to_obj /*dev [J][12]*/, int32_t J /*0..8*/,
                       const uint32_t* sets /*dev [M]*/, int32_t M /*1..8*/, uint32_t flags /*bit 0: prefilter off*/, float* out /*dev [M][P][3]*/,
                       uint64_t* stats /*dev [3], nullable*/, void* stream);

/* ---- inserted mesh OBJECTS DRAWN IN THE VIEW: the cube G-buffer of texir_gbuffer_cast with up to eight posed mesh instances in it (csrc/gbuffermesh.hip).
 * The shadow and light passes above shade any point list, points on an object as readily as points of the room; what they lacked is the pass that says, per
 * pixel, which surface the camera sees -- the room or an instance -- and hands back its world-space position and normal.
 *
 * THE RULE.  Inputs: scene, mvp (HOST [6,4,4]), cube_res, flip_v exactly as texir_gbuffer_cast takes them; occluders (HOST, Q in 0..8), inst_obj (HOST) and
 * inst_world_to_obj (DEVICE [J][12], J in 0..8, read on every launch: a replayed graph sees a moved object) as texir_irt_shadow_mesh takes them; the
 * occluders' device pointers and boxes enter the kernel arguments by value.  Per pixel of the six faces:
 *   RAY         eye and direction d are texir_gbuffer_cast's: face_basis in double rounded to float32, the same pixel centre, the same float32 expressions.
 *   SCENE WALK  first the scene's closest hit, the call gbuffer_kernel<4> makes (trace_closest on the 4-wide tree).  It gives t_best: its t, +inf on a miss.
 *   INSTANCE WALKS  then the valid instances in index order j = 0 .. J-1 (valid: every word of W[j] is finite): the OBJECT-SPACE RAY (o', d') of
 *               texir_irt_shadow_mesh with x = eye, its FLOAT32 OPERATION SEQUENCE unchanged; a closest-hit walk of the occluder's tree that STARTS with the far
 *               bound t_best: a triangle is accepted iff 0 < t < t_best, t the float32 t the leaf test computes (the ray is not normalised, so t along (o', d')
 *               is t along (eye, d)).  An accepting instance becomes the pixel's surface, its closest accepted t the new t_best.
 *   TIES        acceptance is strict: the scene wins an exact tie, a lower instance index wins over a higher one.  (A tie is exact between equal RECORDS: the
 *               same mesh built with other uvs may pair its triangles into other quad records, whose t differs in the last bit.)
 *   OUTPUTS     a pixel whose surface is the scene, or background: pos, nrm, mask, uv, uv_da, tri_id are bit for bit what texir_gbuffer_cast writes (corner
 *               normals if set, flip_v, the background constants); inst_id = -1.
 *               a pixel whose surface is instance j: inst_id = j, mask = 1, tri_id = the row of the occluder's OWN index array + 1, uv = (0, 0) and uv_da = 0
 *               whatever flip_v is (occluders carry no uvs), and, as a FLOAT32 OPERATION SEQUENCE (each operation separately rounded, no contraction; P0, P1,
 *               P2 the corners of the stored record, a rotation of the caller's; W = W[j]; rsq = rsqrtf):
 *                 pos_k = eye_k + t d_k                                                                     (WORLD space)
 *                 e1 = P1 - P0, e2 = P2 - P0;  n = (e1_y e2_z - e1_z e2_y, e1_z e2_x - e1_x e2_z, e1_x e2_y - e1_y e2_x)
 *                 n_o = n rsq((n_x n_x + n_y n_y) + n_z n_z)                                                 (the unit geometric normal, the caller's winding)
 *                 m_c = (W[0][c] n_o,0 + W[1][c] n_o,1) + W[2][c] n_o,2                                      (W^T n_o: W's 3 x 3 part is the inverse of the pose's,
 *                 nrm_c = m_c rsq((m_0 m_0 + m_1 m_1) + m_2 m_2)                                              so W^T is the pose's inverse transpose)
 *               The normal is NOT flipped towards the viewer; it is the outward normal of an outward-wound mesh under non-uniform scale and under a mirrored
 *               pose (negative determinant) alike.
 *   J = 0, instances no ray meets, and matrices with a non-finite word give texir_gbuffer_cast's bits with inst_id = -1 everywhere.  A singular finite W is
 *   the caller's error: the outputs of the pixels it touches are unspecified, the call completes.
 * ROUNDING BOUND (first order, u = 2^-24; eye, the basis and W are exact float32 values, d carries e per component, tests/gbuffer_cases.py bound_arith; the
 * tests multiply by their factor K).  d' carries texir_irt_shadow_mesh's bound with that e; t carries the closest-hit query's bound_t for it.  Then
 *               |dpos_k| <= |d_k| bound_t + |t| e_k + u |t d_k| + u |pos_k|
 *               n_o: the geometric-normal bound e(n_o) of texir_gbuffer_cast (tests/gbuffer_cases.py geometric_normal64);
 *               e(m_c) = sum_r |W[r][c]| e(n_o,r) + 3 u sum_r |W[r][c] n_o,r|;   q = m . m: e(q) = 2 sum_c |m_c| e(m_c) + 3 u q;
 *               |dnrm_c| <= e(m_c) / |m| + |m_c| / |m| (e(q) / (2 q) + 5 u)                                  (rsq within 2 ulp = 4 u, the product u)
 *   The surface is decided unless two surfaces' t differ by less than the sum of their bound_t, or a triangle is within its margin of the ray.
 * PREFILTER.  A lane walks instance j only if (o', d') passes texir_irt_shadow_mesh's box test, unchanged.  Its argument covers the LEAF TEST -- the 2D origin
 * inside the sheared triangle and a computed t > 0 -- and the far bound only ever removes accepted triangles (t < t_best on top of t > 0), so the test never
 * rejects a ray the closest-hit form accepts a triangle for, as it is.  A walk no lane needs is skipped.  flags bit 0 switches the test off (every lane walks
 * every valid instance): the outputs must not change by a bit, which is how the tests hold this argument.
 * ONE TRAVERSAL INSTANTIATION: scene and occluders are walked in a wave-uniform loop through the closest-hit form of the traversal, so the kernel owns one LDS
 * stack, as texir_gbuffer_cast's does.
 * Outputs, P = 6 c c, all dev: pos, nrm [P,3], mask [P], uv [P,2], uv_da [P,4], tri_id [P], inst_id [P] int32.  Caller-owned buffers, the caller's stream, no
 * allocation, no synchronisation: the call records into a hipGraph.
 * ERRORS: TEXIR_ERR_INVALID with a texir_last_error() text, nothing launched and nothing written, for Q or J outside 0..8, inst_obj[j] outside 0..Q-1, a null
 * occluder handle (all reported before any null buffer), a null argument (inst_id included), cube_res outside 1..16384, a singular or affine mvp, the scene or
 * an occluder without the 4-wide tree (TEXIR_BVH_WIDTH=2), an occluder on another device than the scene.
 * Not computed: the lamps' bodies drawn in the view; textured objects (occluders carry no uvs: an object's material is the caller's, per instance); more than
 * 8 occluders or instances per call. */
TEXIR_API int texir_gbuffer_cast_mesh(const texir_scene* scene, const float* mvp /*host [6,4,4]*/, int32_t cube_res, int32_t flip_v,
                       const texir_scene* const* occluders /*host [Q]*/, int32_t Q /*0..8*/, const int32_t* inst_obj /*host [J]*/,
                       const float* inst_world_to_obj /*dev [J][12]*/, int32_t J /*0..8*/, uint32_t flags /*bit 0: prefilter off*/, float* pos, float* nrm,
                       float* mask, float* uv, float* uv_da, int32_t* tri_id, int32_t* inst_id /*dev [P]*/, void* stream);

/* ---- host-side codec loops of the file formats around the path (both take HOST pointers) ----------------------------
 * PNG scanline un-filtering (filters 0-4, PNG spec 9.2) of zlib-inflated IDAT data: raw [H][stride+1] -> out [H][stride]; replaces the
 * decode half of cv2.imread("0.png", -1) (models/tracer_o3d_irt.py:91, datasets/dataset.py:489-492). */
TEXIR_API int texir_png_unfilter(const uint8_t* raw /*host*/, int32_t H, int32_t stride, int32_t bytes_per_pixel, uint8_t* out /*host*/);
/* Radiance .hdr scanlines (flat or new-style RLE, per scanline) after the resolution line -> RGBE bytes [H][W][4]; returns the bytes
 * consumed (< 0: error).  Replaces the decode half of cv2.imread(".hdr", -1) (models/tracer_o3d_irt.py:77, datasets/dataset.py:480). */
TEXIR_API int64_t texir_hdr_decode_scanlines(const uint8_t* data /*host*/, int64_t n, int32_t W, int32_t H, uint8_t* rgbe /*host*/);
/* Radiance RGBE pixel codec, float RGB [npix][3] <-> RGBE [npix][4] (host pointers, multi-threaded): the pixel arithmetic of
 * cv2.imwrite(".hdr") / cv2.imread(".hdr", -1) (trainer/generate_ir_texture.py:82, trainer/train_material.py:350-353,
 * models/mat_nvdiffrast.py:73).  Byte-identical to io_formats.rgbe_encode / rgbe_decode (numpy, kept as the test reference). */
TEXIR_API int texir_rgbe_encode(const float* rgb /*host*/, int64_t npix, uint8_t* rgbe /*host*/);
/* RGBE bytes [H][W][4] -> new-style RLE scanlines laid out as cv2.imwrite(".hdr") writes them (its default IMWRITE_HDR_COMPRESSION_RLE);
 * returns the bytes written (< 0: error / cap too small; 4 + 4 * (W + W / 64 + 4) bytes per scanline always suffice). */
TEXIR_API int64_t texir_hdr_encode_rle(const uint8_t* rgbe /*host*/, int32_t W, int32_t H, uint8_t* out /*host*/, int64_t cap);
TEXIR_API int texir_rgbe_decode(const uint8_t* rgbe /*host*/, int64_t npix, float* rgb /*host*/);
/* Wavefront OBJ text -> arrays (host pointers, multi-threaded): the parse half of o3d.io.read_triangle_mesh / pyredner.load_obj
 * (models/tracer_o3d_irt.py:75,85,183-189; models/mat_nvdiffrast.py:87,193-199).  texir_obj_parse classifies lines by their first token
 * (v / vt / vn / f; LF, CRLF, CR), fan-triangulates polygons, resolves negative indices and fills counts = {n_v, n_vt, n_vn, n_tri};
 * texir_obj_take copies into caller-owned buffers sized from the counts (v [n_v][3], vt [n_vt][2], vn [n_vn][3] float32 -- a correctly
 * rounded double rounded once more, as float() + numpy do; fi / ft / fn [n_tri][3] int32, 0-based, -1 = absent) and frees the handle
 * (all-null outputs: only frees).  Array-identical to io_formats.load_obj_py. */
TEXIR_API int texir_obj_parse(const char* text /*host*/, int64_t n, void** handle, int64_t counts[4]);
TEXIR_API int texir_obj_take(void* handle, float* v, float* vt, float* vn, int32_t* fi, int32_t* ft, int32_t* fn);

#ifdef __cplusplus
}
#endif
#endif

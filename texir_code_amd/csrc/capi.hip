// C-ABI of libtexir_hip.so (include/texir_hip.h), all of it but the host-side file codecs of io_native.cpp.  Thin: argument checks, handle ownership, launches.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <atomic>
#include <string>
#include <vector>

#include "../../include/texir_hip.h"
#include "bvh_build.h"
#include "env.h"
#include "kernels.h"

using namespace texir;

struct texir_scene {
    int device = 0;
    SceneDev dev{};
    void* d_nodes4 = nullptr; void* d_nodes4f = nullptr;
    void* d_nodes = nullptr; void* d_tris = nullptr; void* d_quads = nullptr; void* d_uvs = nullptr; float* d_tex = nullptr;
    float* d_tex_tiled = nullptr;        // retiled copy read by the hit shader (texture layouts 1, 2); d_tex stays the row-major master
    size_t tiled_bytes = 0;
    int tiled_layout = 0;                // layout d_tex_tiled was sized for
    uint32_t* d_tex_packed = nullptr;    // 4-byte shared-exponent texels (layouts 3, 4), in force only while the texture packs EXACTLY (install_texture)
    size_t packed_bytes = 0;
    int packed_layout = 0;
    unsigned int* d_tex_flag = nullptr;  // device word: texels of the last pack that were not representable
    int64_t n_nodes = 0, n_nodes4 = 0, n_tris = 0, n_slots = 0 /* leaf-order slots behind d_tris / d_uvs / d_cnrm: 2 per quad record (bvh_build.h) */, n_quads = 0, n_uv_recs = 0 /* 32-byte uv records behind d_uvs: one per quad record */, max_depth = 0;
    int width = 2;
    float bounds[6] = {0, 0, 0, 0, 0, 0};   // (lo.x, lo.y, lo.z, hi.x, hi.y, hi.z) of the vertices the triangles name (texir_scene_bounds)
    size_t tex_bytes = 0;
    std::vector<uint32_t> slot_prim;     // leaf slot -> primitive id (host copy, for per-corner attribute uploads; 0xFFFFFFFF: an empty slot)
    std::vector<uint8_t> slot_rot;       // leaf slot -> rotation of the stored corners (stored corner k = the caller's corner (rot + k) % 3)
    void* d_cnrm = nullptr;              // leaf-ordered corner normals, 3 x float4 per triangle
    float* d_scratch = nullptr;          // texir_scene_reserve_scratch: the IrT partial-sum scratch of RECORDED launches (eager launches allocate stream-ordered)
    size_t scratch_bytes = 0;
    std::vector<float*> retired_scratch;  // smaller blocks a grown reservation replaced: recorded graphs may still name them, so they live until destroy
    // chunk counters of the persistent IrT kernel: one slot per launch, handed out round-robin so that launches of one scene that
    // overlap on different streams do not share a counter (kWorkSlots launches would have to be in flight at once)
    static constexpr int kWorkSlots = 64;
    unsigned long long* d_work = nullptr;
    mutable std::atomic<unsigned> work_next{0};      // (launching on an immutable scene still advances the slot)
    // phase-scheduler weight of this scene (device_common.h kSchedNodeWeight): decided once by texir_scene_tune, read by every tracing launch
    mutable std::atomic<int> sched_state{0};         // 0 undecided, 1 being decided, 2 decided
    mutable std::atomic<int> sched_weight{0};        // 0 = the compile-time default (2)
    mutable std::atomic<double> node_utilisation{-1.0};   // what the decision measured (texir_scene_scheduler)
};

// the kernel-argument view of a scene for one launch: the immutable part + the scheduler weight in force now
// (`coherent`: the launch traces direction cells -- texir_irt_generate, where quad leaves made weight 3 the better one for scenes whose node steps run full,
// tools/r04_session33.sh; the other kernels' rays share no direction and keep what they were measured with: at most 2)
static SceneDev dev_of(const texir_scene* s, bool coherent = false)
{
    SceneDev d = s->dev;
    const int forced = env().sched_weight;
    int w = forced ? forced : s->sched_weight.load(std::memory_order_relaxed);
    if (!forced && !coherent && w > 2) w = 2;
    d.sched_weight = w;
    return d;
}

static thread_local std::string g_err;

static int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                                    \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return fail(TEXIR_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// is `st` being recorded into a hipGraph?  (`if_unknown`: what a failed query counts as -- its callers differ)
static bool stream_capturing(hipStream_t st, bool if_unknown)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) return if_unknown;
    return cs != hipStreamCaptureStatusNone;
}

// the chunk counters of one launch: the scene's next slot, round-robin
static unsigned long long* next_work_slot(const texir_scene* s)
{
    return s->d_work + (size_t)(s->work_next.fetch_add(1) % texir_scene::kWorkSlots) * 8 * kWorkStride;
}

// a cached device copy of the texture (install_texture): kept while its layout and size stay what they were, else freed and allocated anew -- never while recording
static int resize_cached(void** buf, size_t* have_bytes, int* have_layout, size_t bytes, int layout, bool capturing)
{
    if (*buf && (*have_layout != layout || *have_bytes != bytes)) { HIP_TRY(hipFree(*buf)); *buf = nullptr; }
    if (*buf) return TEXIR_OK;
    if (capturing) return fail(TEXIR_ERR_INVALID, "texir_scene_set_texture: the stream is being captured and the float32 tiles are not allocated yet");
    HIP_TRY(hipMalloc(buf, bytes)); *have_bytes = bytes; *have_layout = layout;
    return TEXIR_OK;
}

// Chooses and fills the hit shader's copy of the radiance texture; d_tex (row-major float32 master) has been written on `st` already.
// TEXIR_TEX_LAYOUT 4 (default) / 3: 4-byte shared-exponent texels when EVERY texel is three 8-bit integers times one power of two -- what an RGBE file
// times 2^hdr_exposure always is (tracer_o3d_irt.py:77-81) -- decoding to the identical floats; any other texture (a float-valued synthetic one,
// 2.5 x an RGBE one, negative values) keeps the float32 tiles of layout 2.  The decision needs the pack kernel's verdict, i.e. one stream
// synchronisation: on a capturing stream the float32 layout is taken without asking.  0 / 1 / 2 force the float32 layouts (A/B runs).
static int install_texture(texir_scene* s, hipStream_t st)
{
    const int want = env().tex_layout, Ht = s->dev.Ht, Wt = s->dev.Wt;
    const bool capturing = stream_capturing(st, true);
    if ((want == 3 || want == 4) && !capturing && Ht < (1 << 16) && Wt < (1 << 16)) {
        int tx, ty;
        const size_t bytes = tex_pack_bytes(Ht, Wt, want, &tx, &ty);
        if (int rc = resize_cached((void**)&s->d_tex_packed, &s->packed_bytes, &s->packed_layout, bytes, want, false)) return rc;
        if (!s->d_tex_flag) HIP_TRY(hipMalloc((void**)&s->d_tex_flag, sizeof(unsigned int)));
        HIP_TRY(launch_tex_pack(s->d_tex, s->d_tex_packed, Ht, Wt, want, s->d_tex_flag, st));
        unsigned int bad = 1;
        HIP_TRY(hipMemcpyAsync(&bad, s->d_tex_flag, sizeof(bad), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (bad == 0) {
            s->dev.tex = reinterpret_cast<const float*>(s->d_tex_packed); s->dev.tex_layout = want; s->dev.tiles_x = tx;
            return TEXIR_OK;
        }
    }
    const int layout = want >= 3 ? 2 : want;
    if (layout == 1 || layout == 2) {
        int tx, ty;
        const size_t bytes = tex_retile_bytes(Ht, Wt, layout, &tx, &ty);
        if (int rc = resize_cached((void**)&s->d_tex_tiled, &s->tiled_bytes, &s->tiled_layout, bytes, layout, capturing)) return rc;
        HIP_TRY(launch_tex_retile(s->d_tex, s->d_tex_tiled, Ht, Wt, layout, st));
        s->dev.tex = s->d_tex_tiled; s->dev.tex_layout = layout; s->dev.tiles_x = tx;
    } else {
        s->dev.tex = s->d_tex; s->dev.tex_layout = 0; s->dev.tiles_x = 0;
    }
    return TEXIR_OK;
}

// ---- the argument rules of the texture side, each written once.  k = the job's index in a batched call (its messages say `job k: `), -1 = the single-texture
// call, which fills a job structure and is held to the same rules ----
static int fail_job(const char* fn, int k, const char* fmt, ...)
{
    char msg[384];
    va_list ap; va_start(ap, fmt); vsnprintf(msg, sizeof(msg), fmt, ap); va_end(ap);
    return k < 0 ? fail(TEXIR_ERR_INVALID, "%s: %s", fn, msg) : fail(TEXIR_ERR_INVALID, "%s: job %d: %s", fn, k, msg);
}

static int check_tex(const char* fn, int k, int H, int W, int C, int levels)
{
    if (H <= 0 || W <= 0 || C <= 0 || C > 4 || levels < 1 || levels > 16) return fail_job(fn, k, "bad texture H=%d W=%d C=%d levels=%d", H, W, C, levels);
    if (levels > mip_levels(H, W, 15)) return fail_job(fn, k, "%d mip levels not available for %dx%d", levels, H, W);
    return 0;
}

// (the single-texture call demands uv / out even at P = 0 and has no build_from to name)
static int check_fetch_job(const char* fn, int k, const texir_tex_fetch_job& q)
{
    const bool batched = k >= 0, trilinear = q.filter_mode == 1;
    if (!q.tex || ((!batched || q.P > 0) && (!q.uv || !q.out || (trilinear && !q.uv_da))) || (trilinear && q.levels > 1 && !q.mips_rest))
        return fail_job(fn, k, "null argument");
    if (q.filter_mode < 0 || q.filter_mode > 1 || q.P < 0 || q.build_from < -1 || q.build_from > 1)
        return fail_job(fn, k, "bad filter_mode/P%s", batched ? "/build_from" : "");
    if (q.build_from >= 0 && q.levels > 1 && !q.mips_rest) return fail_job(fn, k, "a build needs mips_rest");
    return check_tex(fn, k, q.H, q.W, q.C, q.levels);
}

static int check_gather_job(const char* fn, int k, const texir_tex_gather_job& q)
{
    // d_tex may be NULL with defer_last_fold when no tap of the lists samples level 0 (then nothing is written there and the caller's
    // optimiser step treats the level-0 gradient as identically zero)
    if ((!q.d_tex && !q.defer_last_fold) || !q.d_out || (q.n_seg > 0 && (!q.seg_key || !q.seg_start || !q.seg_count || !q.pix || !q.weights)) || (q.filter_mode == 1 && q.levels > 1 && !q.grad_rest))
        return fail_job(fn, k, "null argument");
    if (q.filter_mode < 0 || q.filter_mode > 1 || q.n_seg < 0 || q.defer_last_fold < 0 || q.defer_last_fold > 2 || (q.defer_last_fold && (q.filter_mode != 1 || q.levels < 2))
        || (q.defer_last_fold == 2 && (q.levels < 4 || (q.H & 3) || (q.W & 3))))
        return fail_job(fn, k, "bad filter_mode/n_seg/defer_last_fold");
    // (d_out2 and rest_mask: fields of the batched form alone)
    if (q.d_out2 && env().mip_per_level) return fail_job(fn, k, "d_out2 is not available with TEXIR_MIP_PER_LEVEL=1");
    if (q.rest_mask && q.defer_last_fold != 2) return fail_job(fn, k, "rest_mask needs defer_last_fold = 2");
    if (q.rest_mask && env().mip_per_level) return fail_job(fn, k, "rest_mask is not available with TEXIR_MIP_PER_LEVEL=1 (the per-level folds read a cleared stack)");
    return check_tex(fn, k, q.H, q.W, q.C, q.levels);
}

// step: the host-side step count of texir_adam_step_tex, which needs grad_level1 and no hyper; nullptr: the *_dev forms (level1_mask: a field of the batched form alone)
static int check_adam_tex_job(const char* fn, int k, const texir_adam_tex_job& q, const int32_t* step = nullptr)
{
    if (!q.param || !q.exp_avg || !q.exp_avg_sq || (step ? !q.grad_level1 : ((!q.grad_level1 && !q.grad_level2) || !q.hyper))) return fail_job(fn, k, "null argument");
    if (q.H < 2 || q.W < 2 || (q.H & 1) || (q.W & 1) || q.C < 1 || q.C > 4 || (step && *step < 1)) return fail_job(fn, k, "bad H/W/C%s", step ? "/step" : "");
    if (q.grad_level2 && ((q.H & 3) || (q.W & 3))) return fail_job(fn, k, "a level-2 gradient needs H and W divisible by 4");
    if (q.level1_mask && !q.grad_level2) return fail_job(fn, k, "level1_mask needs grad_level2");
    return 0;
}

template <class Job, class Check>
static int batch_call(const char* fn, const Job* jobs, int n, void* stream, Check check, hipError_t (*launch)(const Job*, int, hipStream_t))
{
    if (n < 0 || n > TEXIR_MAX_BATCH || (n > 0 && !jobs)) return fail(TEXIR_ERR_INVALID, "%s: 0..%d jobs (got %d)", fn, TEXIR_MAX_BATCH, n);
    for (int k = 0; k < n; k++)
        if (int rc = check(fn, k, jobs[k])) return rc;
    if (n == 0) return TEXIR_OK;
    const hipError_t e = launch(jobs, n, (hipStream_t)stream);
    return e == hipSuccess ? TEXIR_OK : fail(TEXIR_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
}

extern "C" {

const char* texir_last_error(void) { return g_err.c_str(); }
int texir_version(void) { return 100; }

int texir_scene_create(const float* verts, int32_t V, const int32_t* tris, int32_t T, const float* tri_uvs, const float* hdr_tex,
                       int32_t Ht, int32_t Wt, int32_t device, texir_scene** out)
{
    if (!verts || !tris || !tri_uvs || !hdr_tex || !out) return fail(TEXIR_ERR_INVALID, "texir_scene_create: null argument");
    if (V <= 0 || T <= 0 || Ht <= 0 || Wt <= 0) return fail(TEXIR_ERR_INVALID, "texir_scene_create: empty mesh or texture");
    // the traversal addresses nodes and triangles with 32-bit byte offsets (64-byte nodes, 48-byte triangle records)
    if ((uint64_t)(2 * (uint64_t)T + 1) * sizeof(GpuTri) >= (1ull << 32)) return fail(TEXIR_ERR_INVALID, "texir_scene_create: too many triangles (%d; limit 44 M)", (int)T);
    for (int64_t i = 0; i < 3 * (int64_t)T; i++)
        if (tris[i] < 0 || tris[i] >= V) return fail(TEXIR_ERR_INVALID, "texir_scene_create: triangle index %d out of range", (int)tris[i]);
    HIP_TRY(hipSetDevice(device));
    BvhHost h;
    try { build_bvh(verts, V, tris, T, tri_uvs, h); }
    catch (const std::bad_alloc&) { return fail(TEXIR_ERR_NOMEM, "BVH build: out of host memory"); }
    catch (const std::exception& ex) { return fail(TEXIR_ERR_INVALID, "BVH build: %s", ex.what()); }
    texir_scene* s = new (std::nothrow) texir_scene;
    if (!s) return fail(TEXIR_ERR_NOMEM, "out of host memory");
    s->n_slots = h.n_slots; s->n_quads = (int64_t)h.quads.size(); s->n_uv_recs = (int64_t)h.uvs.size();
    s->slot_prim.resize((size_t)h.n_slots); s->slot_rot.resize((size_t)h.n_slots);
    for (int64_t i = 0; i < h.n_slots; i++) { s->slot_prim[i] = h.tris[i].prim; uint32_t r; std::memcpy(&r, &h.tris[i].pad1, 4); s->slot_rot[i] = (uint8_t)(r % 3u); }
    s->device = device; s->n_nodes = (int64_t)h.nodes.size(); s->n_tris = T; s->max_depth = h.max_depth;
    for (int a = 0; a < 3; a++) { s->bounds[a] = verts[3 * (size_t)tris[0] + a]; s->bounds[3 + a] = s->bounds[a]; }
    for (int64_t i = 0; i < 3 * (int64_t)T; i++)
        for (int a = 0; a < 3; a++) {
            const float v = verts[3 * (size_t)tris[i] + a];
            if (v < s->bounds[a]) s->bounds[a] = v;
            if (v > s->bounds[3 + a]) s->bounds[3 + a] = v;
        }
    s->tex_bytes = sizeof(float) * 3 * (size_t)Ht * Wt;
    auto bail = [&](hipError_t e, const char* what) { texir_scene_destroy(s); return fail(TEXIR_ERR_HIP, "%s: %s", what, hipGetErrorString(e)); };
    // one device buffer of the scene: allocated and, where there is a host source, filled
    auto alloc_upload = [&](void** dst, const void* src, size_t bytes, const char* what) -> int {
        hipError_t e = hipMalloc(dst, bytes);
        if (e != hipSuccess) return bail(e, (std::string("hipMalloc ") + what).c_str());
        if (src && (e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice)) != hipSuccess) return bail(e, (std::string("upload ") + what).c_str());
        return TEXIR_OK;
    };
    int rc = TEXIR_OK;
    // traversal tree: 4-wide quantised by default (TEXIR_BVH_WIDTH=2 keeps the binary tree); falls back to binary when the wide
    // tree's worst-case stack (3 pushes per level) would not fit the traversal stack
    const int want_w = env().bvh_width;
    s->width = (want_w == 4 && 3 * h.max_depth4 + 2 <= kStackCap) ? 4 : 2;
    if (s->width == 4) {
        s->n_nodes4 = (int64_t)h.nodes4.size(); s->max_depth = h.max_depth4;
        if ((rc = alloc_upload(&s->d_nodes4, h.nodes4.data(), h.nodes4.size() * sizeof(GpuNode4), "nodes4"))) return rc;
        // the float form of the same nodes, read by wave-uniform node steps through the scalar cache (TEXIR_UNIFORM_FLOAT=0: A/B switch)
        if (env().uniform_float && (rc = alloc_upload(&s->d_nodes4f, h.nodes4f.data(), h.nodes4f.size() * sizeof(GpuNode4F), "nodes4f"))) return rc;
    }
    if ((rc = alloc_upload(&s->d_nodes, h.nodes.data(), h.nodes.size() * sizeof(GpuNode), "nodes"))) return rc;
    if ((rc = alloc_upload(&s->d_tris, h.tris.data(), h.tris.size() * sizeof(GpuTri), "tris"))) return rc;
    if (!h.quads.empty() && (rc = alloc_upload(&s->d_quads, h.quads.data(), h.quads.size() * sizeof(GpuQuad), "quads"))) return rc;
    if (!h.uvs.empty() && (rc = alloc_upload(&s->d_uvs, h.uvs.data(), h.uvs.size() * sizeof(GpuTriUV), "uvs"))) return rc;
    if ((rc = alloc_upload((void**)&s->d_tex, hdr_tex, s->tex_bytes, "texture"))) return rc;
    if ((rc = alloc_upload((void**)&s->d_work, nullptr, texir_scene::kWorkSlots * 8 * kWorkStride * sizeof(unsigned long long), "work counters"))) return rc;
    s->dev.nodes4 = (const float4*)s->d_nodes4; s->dev.nodes4f = (const float4*)s->d_nodes4f;
    s->dev.nodes = (const float4*)s->d_nodes; s->dev.tris = (const float4*)s->d_tris; s->dev.quads = (const float4*)s->d_quads; s->dev.uvs = (const float4*)s->d_uvs;
    s->dev.tex = s->d_tex; s->dev.Ht = Ht; s->dev.Wt = Wt; s->dev.tex_layout = 0; s->dev.tiles_x = 0; s->dev.sched_weight = 0;
    // hit-shader copy of the texture (install_texture): 4-byte texels when they decode to the identical floats, else float32 tiles
    if ((rc = install_texture(s, 0))) { texir_scene_destroy(s); return rc; }
    if (const hipError_t e = hipStreamSynchronize(0); e != hipSuccess) return bail(e, "texture layout");
    *out = s;
    return TEXIR_OK;
}

int texir_scene_destroy(texir_scene* s)
{
    if (!s) return TEXIR_OK;
    (void)hipSetDevice(s->device);
    void* const owned[] = {s->d_nodes4, s->d_nodes4f, s->d_nodes, s->d_tris, s->d_quads, s->d_uvs, s->d_tex, s->d_tex_tiled, s->d_tex_packed, s->d_tex_flag, s->d_cnrm, s->d_scratch, s->d_work};
    for (void* p : owned) if (p) (void)hipFree(p);
    for (float* p : s->retired_scratch) (void)hipFree(p);
    delete s;
    return TEXIR_OK;
}

int texir_scene_set_texture(texir_scene* s, const float* tex, int32_t Ht, int32_t Wt, int32_t is_device, void* stream)
{
    if (!s || !tex) return fail(TEXIR_ERR_INVALID, "texir_scene_set_texture: null argument");
    if (Ht != s->dev.Ht || Wt != s->dev.Wt) return fail(TEXIR_ERR_INVALID, "texir_scene_set_texture: size %dx%d != scene texture %dx%d", Ht, Wt, s->dev.Ht, s->dev.Wt);
    HIP_TRY(hipMemcpyAsync(s->d_tex, tex, s->tex_bytes, is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, (hipStream_t)stream));
    return install_texture(s, (hipStream_t)stream);
}

int texir_scene_info(const texir_scene* s, int64_t out[8])
{
    if (!s || !out) return fail(TEXIR_ERR_INVALID, "texir_scene_info: null argument");
    out[0] = s->width == 4 ? s->n_nodes4 : s->n_nodes; out[1] = s->n_tris; out[2] = s->max_depth;
    out[3] = s->width == 4 ? s->n_nodes4 * (int64_t)(sizeof(GpuNode4) + (s->d_nodes4f ? sizeof(GpuNode4F) : 0)) : s->n_nodes * (int64_t)sizeof(GpuNode);
    out[4] = s->n_slots * (int64_t)sizeof(GpuTri) + s->n_quads * (int64_t)sizeof(GpuQuad); out[5] = s->d_uvs ? s->n_uv_recs * (int64_t)sizeof(GpuTriUV) : 0; out[6] = (int64_t)(s->dev.tex_layout >= 3 ? s->packed_bytes : s->dev.tex_layout >= 1 ? s->tiled_bytes : s->tex_bytes); out[7] = s->device;
    return TEXIR_OK;
}

int texir_scene_bounds(const texir_scene* s, float out[6])
{
    if (!s || !out) return fail(TEXIR_ERR_INVALID, "texir_scene_bounds: null argument");
    for (int a = 0; a < 6; a++) out[a] = s->bounds[a];
    return TEXIR_OK;
}

int texir_scene_texture_layout(const texir_scene* s, int32_t* layout)
{
    if (!s || !layout) return fail(TEXIR_ERR_INVALID, "texir_scene_texture_layout: null argument");
    *layout = s->dev.tex_layout;
    return TEXIR_OK;
}

int texir_texel_pack(const float* rgb, int64_t n, uint32_t* words, uint8_t* exact)
{
    if ((!rgb || !words) && n > 0) return fail(TEXIR_ERR_INVALID, "texir_texel_pack: null argument");
    for (int64_t i = 0; i < n; i++) {
        uint32_t b[3], w = 0u;
        std::memcpy(b, rgb + 3 * i, 12);
        const bool ok = pack_texel(b[0], b[1], b[2], w);
        words[i] = ok ? w : 0u;
        if (exact) exact[i] = ok ? 1 : 0;
    }
    return TEXIR_OK;
}

int texir_texel_unpack(const uint32_t* words, int64_t n, float* rgb)
{
    if ((!rgb || !words) && n > 0) return fail(TEXIR_ERR_INVALID, "texir_texel_unpack: null argument");
    for (int64_t i = 0; i < n; i++) {
        const uint32_t q = words[i], sb = (q >> 1) & 0x7F800000u;
        float scale; std::memcpy(&scale, &sb, 4);
        for (int c = 0; c < 3; c++) rgb[3 * i + c] = (float)((q >> (8 * c)) & 0xFFu) * scale;
    }
    return TEXIR_OK;
}

int texir_scene_prefetch(const texir_scene* s, int32_t what, int32_t blocks, void* stream)
{
    if (!s) return fail(TEXIR_ERR_INVALID, "texir_scene_prefetch: null argument");
    if (blocks < 1) blocks = 512;
    uint32_t* sink = reinterpret_cast<uint32_t*>(s->d_work);         // (never written in practice; any device word will do)
    if ((what & 1) && s->d_nodes4) HIP_TRY(launch_prefetch(s->d_nodes4, (size_t)s->n_nodes4 * sizeof(GpuNode4), blocks, sink, (hipStream_t)stream));
    if ((what & 2) && s->d_nodes4f) HIP_TRY(launch_prefetch(s->d_nodes4f, (size_t)s->n_nodes4 * sizeof(GpuNode4F), blocks, sink, (hipStream_t)stream));
    // (what the traversal reads of the triangles: the quad records where the library has them, else the leaf-ordered triangles)
    if ((what & 4) && s->d_quads && s->width == 4) HIP_TRY(launch_prefetch(s->d_quads, (size_t)s->n_quads * sizeof(GpuQuad), blocks, sink, (hipStream_t)stream));
    else if ((what & 4) && s->d_tris) HIP_TRY(launch_prefetch(s->d_tris, (size_t)s->n_slots * sizeof(GpuTri), blocks, sink, (hipStream_t)stream));
    if ((what & 8) && s->d_uvs) HIP_TRY(launch_prefetch(s->d_uvs, (size_t)s->n_uv_recs * sizeof(GpuTriUV), blocks, sink, (hipStream_t)stream));
    return TEXIR_OK;
}

int texir_scene_scheduler(const texir_scene* s, double out[2])
{
    if (!s || !out) return fail(TEXIR_ERR_INVALID, "texir_scene_scheduler: null argument");
    out[0] = (double)s->sched_weight.load(); out[1] = s->node_utilisation.load();
    return TEXIR_OK;
}

int texir_scene_tune(const texir_scene* s, const float* pos, const float* nrm, const float* shift, const int32_t* texel_ids, int64_t n_ids,
                     int32_t N, int32_t mode, void* stream)
{
    if (!s || !pos || !nrm || !shift) return fail(TEXIR_ERR_INVALID, "texir_scene_tune: null argument");
    if (mode < 0 || mode > 1) return fail(TEXIR_ERR_INVALID, "texir_scene_tune: mode must be uniform(0) or cosine(1), got %d", mode);
    // one host thread decides (compare-exchange: 0 undecided -> 1 deciding -> 2 decided); the others return at once and launch with the weight in force
    int expect = 0;
    if (!s->sched_state.compare_exchange_strong(expect, 1)) return TEXIR_OK;
    int w = env().sched_weight;
    double util = -1.0;
    if (w == 0 && texel_ids && n_ids >= 65536 && N >= 256 && s->width == 4) {
        if (stream_capturing((hipStream_t)stream, true)) {
            s->sched_state.store(0);                 // a blocking measurement cannot be recorded: stay undecided, keep the default weight
            return fail(TEXIR_ERR_INVALID, "texir_scene_tune: the stream is being captured (tune the scene before recording)");
        }
        unsigned long long* work = next_work_slot(s);
        const int64_t count = 16384, first = ((n_ids / 3) / 64) * 64;
        const hipError_t e = irt_probe_node_utilisation(s->dev, pos, nrm, shift, texel_ids, first, count, N, mode, work, (hipStream_t)stream, &util);
        if (e != hipSuccess) { s->sched_state.store(0); return fail(TEXIR_ERR_HIP, "texir_scene_tune: %s", hipGetErrorString(e)); }
        w = (util >= 0.0 && util < 0.60) ? 1 : 3;          // (3 since the quad leaves: a leaf visit is one record step, the node lanes are worth waiting for a little longer)
    }
    if (w == 0) { s->sched_state.store(0); return TEXIR_OK; }       // a short list decides nothing: a later, longer call may
    s->sched_weight.store(w);
    s->node_utilisation.store(util);
    s->sched_state.store(2);
    return TEXIR_OK;
}

int texir_reload_env(void)
{
    env_reload();
    return TEXIR_OK;
}

int texir_env_switch(const char* name, int32_t* value)
{
    int v = 0;
    if (!name || !value || env_switch(name, &v) != 0) return fail(TEXIR_ERR_INVALID, "texir_env_switch: unknown switch %s", name ? name : "(null)");
    *value = v;
    return TEXIR_OK;
}

int texir_trace_shade(const texir_scene* s, const float* org, const float* dir, int64_t R, float t_min, float* radiance, float* t_hit,
                      uint32_t* prim_id, float* prim_uv, void* stream)
{
    if (!s || !org || !dir || !radiance) return fail(TEXIR_ERR_INVALID, "texir_trace_shade: null argument");
    if (R < 0) return fail(TEXIR_ERR_INVALID, "texir_trace_shade: negative ray count");
    HIP_TRY(launch_trace_shade(dev_of(s), org, dir, R, t_min, radiance, t_hit, prim_id, prim_uv, (hipStream_t)stream));
    return TEXIR_OK;
}

/* the any-hit query, csrc/occlusion.hip: Open3D RaycastingScene.test_occlusions, the sibling of the cast_rays at models/tracer_o3d_irt.py:240-269 */
int texir_trace_occluded(const texir_scene* s, const float* org, const float* dir, int64_t R, float t_near, float t_far, uint8_t* occluded, uint64_t* stats,
                         void* stream)
{
    if (R < 0) return fail(TEXIR_ERR_INVALID, "texir_trace_occluded: negative ray count");
    if (!(t_near >= 0.0f) || !(t_near - t_near == 0.0f)) return fail(TEXIR_ERR_INVALID, "texir_trace_occluded: t_near must be finite and >= 0");
    if (R == 0) return TEXIR_OK;
    if (!s || !org || !dir || !occluded) return fail(TEXIR_ERR_INVALID, "texir_trace_occluded: null argument (scene, org, dir and occluded are required)");
    HIP_TRY(launch_trace_occluded(dev_of(s), org, dir, R, t_near, t_far, occluded, (unsigned long long*)stats, (hipStream_t)stream));
    return TEXIR_OK;
}

int texir_generate_dir(const float* normals, const float* roughness, const float* shift, int64_t b, int32_t N, int32_t mode, float* L, void* stream)
{
    if (!normals || !shift || !L) return fail(TEXIR_ERR_INVALID, "texir_generate_dir: null argument");
    if (mode < 0 || mode > 2) return fail(TEXIR_ERR_INVALID, "texir_generate_dir: unknown mode %d", mode);
    if (mode == TEXIR_MODE_IMPORTANCE && !roughness) return fail(TEXIR_ERR_INVALID, "texir_generate_dir: importance mode needs roughness");
    if (b < 0 || N < 0) return fail(TEXIR_ERR_INVALID, "texir_generate_dir: negative size");
    HIP_TRY(launch_gen_dir(normals, roughness, shift, b, N, mode, L, (hipStream_t)stream));
    return TEXIR_OK;
}

int texir_irt_generate(const texir_scene* s, const float* pos, const float* nrm, const float* shift, const int32_t* texel_ids, int64_t n_ids,
                       int64_t Nt, int32_t N, int32_t mode, float* irr, uint64_t* stats, void* stream)
{
    if (!s || !pos || !nrm || !shift || !irr) return fail(TEXIR_ERR_INVALID, "texir_irt_generate: null argument");
    if (mode < 0 || mode > 1) return fail(TEXIR_ERR_INVALID, "texir_irt_generate: mode must be uniform(0) or cosine(1), got %d", mode);
    if (N <= 0 || Nt < 0 || n_ids < 0) return fail(TEXIR_ERR_INVALID, "texir_irt_generate: bad sizes N=%d Nt=%lld n_ids=%lld", N, (long long)Nt, (long long)n_ids);
    if (Nt >= (1ll << 31)) return fail(TEXIR_ERR_INVALID, "texir_irt_generate: Nt too large");
    int64_t n = texel_ids ? n_ids : Nt;
    unsigned long long* work = next_work_slot(s);
    // (No measurement and no synchronisation in here: the phase scheduler's weight is whatever texir_scene_tune / TEXIR_SCHED_WEIGHT has decided for
    // the scene, 2 until then.  The texture is the same bits either way.)
    // A launch that is being RECORDED into a hipGraph must not allocate: stream-ordered allocations inside a recorded graph gave wrong partial sums in
    // some replays on this stack (ROCm 7.2: profiles/r04, graph replay probe).  It uses the scratch the caller reserved on the scene beforehand.
    float* scratch = nullptr;
    if (stream_capturing((hipStream_t)stream, false)) {
        const size_t need = irt_scratch_bytes(s->dev, n, N);
        if (need > s->scratch_bytes)
            return fail(TEXIR_ERR_INVALID, "texir_irt_generate: the stream is being captured and the launch needs %zu bytes of scratch, %zu reserved -- call "
                                           "texir_scene_reserve_scratch(scene, n_ids, N) before recording", need, s->scratch_bytes);
        scratch = need ? s->d_scratch : nullptr;
    }
    HIP_TRY(launch_irt(dev_of(s, true), pos, nrm, shift, texel_ids, n, N, mode, irr, (unsigned long long*)stats, work, (hipStream_t)stream, scratch));
    return TEXIR_OK;
}

int64_t texir_irt_split_workspace_bytes(int64_t n_ids, int32_t N, int32_t K)
{
    return (int64_t)irt_split_workspace_bytes(n_ids, N, K);
}

int texir_irt_split(const texir_scene* s, const float* pos, const float* nrm, const float* shift, const int32_t* texel_ids, int64_t n_ids, int64_t Nt,
                    int32_t N, int32_t mode, const uint8_t* labels, int32_t K, int32_t unit, float* out, void* workspace, int64_t workspace_bytes, void* stream)
{
    // (K first: a caller that sized `out` by a bad K may hold no buffer at all)
    if (K < 1 || K > 8) return fail(TEXIR_ERR_INVALID, "texir_irt_split: K must be in 1..8, got %d (regroup the classes and call again)", K);
    if (!labels) return fail(TEXIR_ERR_INVALID, "texir_irt_split: labels is null");
    if (!s || !pos || !nrm || !shift || !out) return fail(TEXIR_ERR_INVALID, "texir_irt_split: null argument");
    if (mode < 0 || mode > 1) return fail(TEXIR_ERR_INVALID, "texir_irt_split: mode must be uniform(0) or cosine(1), got %d", mode);
    if (N < 1 || Nt < 0 || n_ids < 0) return fail(TEXIR_ERR_INVALID, "texir_irt_split: bad sizes N=%d Nt=%lld n_ids=%lld", N, (long long)Nt, (long long)n_ids);
    if (Nt >= (1ll << 31)) return fail(TEXIR_ERR_INVALID, "texir_irt_split: Nt too large");
    if (!s->dev.nodes4) return fail(TEXIR_ERR_INVALID, "texir_irt_split: the scene has no 4-wide tree (TEXIR_BVH_WIDTH=2 or the binary fallback): the split has the 64-texel form only");
    const int64_t n = texel_ids ? n_ids : Nt;
    if (n == 0) return TEXIR_OK;
    const int64_t need = (int64_t)irt_split_workspace_bytes(n, N, K);
    if (!workspace || workspace_bytes < need)
        return fail(TEXIR_ERR_INVALID, "texir_irt_split: the workspace holds %lld bytes, the call needs %lld (texir_irt_split_workspace_bytes)",
                    (long long)(workspace ? workspace_bytes : 0), (long long)need);
    HIP_TRY(launch_irt_split(dev_of(s, true), s->d_tex, labels, pos, nrm, shift, texel_ids, n, Nt, N, mode, K, unit != 0, out, (float*)workspace, (hipStream_t)stream));
    return TEXIR_OK;
}

int64_t texir_irt_multi_workspace_bytes(int64_t n_ids, int32_t N, int32_t K)
{
    return (int64_t)irt_multi_workspace_bytes(n_ids, N, K);
}

int texir_irt_multi(const texir_scene* s, const float* pos, const float* nrm, const float* shift, const int32_t* texel_ids, int64_t n_ids, int64_t Nt,
                    int32_t N, int32_t mode, const float* tex, int32_t K, float* out, void* workspace, int64_t workspace_bytes, void* stream)
{
    // (K first: a caller that sized `tex` and `out` by a bad K may hold no buffer at all)
    if (K < 1 || K > 8) return fail(TEXIR_ERR_INVALID, "texir_irt_multi: K must be in 1..8, got %d (call again for further textures: the results are independent)", K);
    if (!tex) return fail(TEXIR_ERR_INVALID, "texir_irt_multi: tex is null");
    if (!s || !pos || !nrm || !shift || !out) return fail(TEXIR_ERR_INVALID, "texir_irt_multi: null argument");
    if (mode < 0 || mode > 1) return fail(TEXIR_ERR_INVALID, "texir_irt_multi: mode must be uniform(0) or cosine(1), got %d", mode);
    if (N < 1 || Nt < 0 || n_ids < 0) return fail(TEXIR_ERR_INVALID, "texir_irt_multi: bad sizes N=%d Nt=%lld n_ids=%lld", N, (long long)Nt, (long long)n_ids);
    if (Nt >= (1ll << 31)) return fail(TEXIR_ERR_INVALID, "texir_irt_multi: Nt too large");
    if (!s->dev.nodes4) return fail(TEXIR_ERR_INVALID, "texir_irt_multi: the scene has no 4-wide tree (TEXIR_BVH_WIDTH=2 or the binary fallback): the pass has the 64-texel form only");
    const int64_t n = texel_ids ? n_ids : Nt;
    if (n == 0) return TEXIR_OK;
    const int64_t need = (int64_t)irt_multi_workspace_bytes(n, N, K);
    if (!workspace || workspace_bytes < need)
        return fail(TEXIR_ERR_INVALID, "texir_irt_multi: the workspace holds %lld bytes, the call needs %lld (texir_irt_multi_workspace_bytes)",
                    (long long)(workspace ? workspace_bytes : 0), (long long)need);
    HIP_TRY(launch_irt_multi(dev_of(s, true), tex, pos, nrm, shift, texel_ids, n, Nt, N, mode, K, out, (float*)workspace, (hipStream_t)stream));
    return TEXIR_OK;
}

int64_t texir_irt_shadow_workspace_bytes(int64_t n_ids, int32_t N, int32_t M)
{
    return (int64_t)irt_shadow_workspace_bytes(n_ids, N, M);
}

int texir_irt_shadow(const texir_scene* s, const float* pos, const float* nrm, const float* shift, const int32_t* texel_ids, int64_t n_ids, int64_t Nt,
                     int32_t N, int32_t mode, const float* bodies, int32_t K, const uint32_t* sets, int32_t M, float* out, uint64_t* stats, void* workspace,
                     int64_t workspace_bytes, void* stream)
{
    // (K and M first: a caller that sized `bodies`, `sets` and `out` by a bad count may hold no buffer at all)
    if (K < 0 || K > 8) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow: K must be in 0..8, got %d (call again for further bodies and take the union of the sets on the caller's side)", K);
    if (M < 1 || M > 8) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow: M must be in 1..8, got %d (call again for further sets: the results are independent)", M);
    if (K > 0 && !bodies) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow: bodies is null");
    if (!sets) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow: sets is null");
    if (!s || !pos || !nrm || !shift || !out) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow: null argument");
    if (mode < 0 || mode > 1) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow: mode must be uniform(0) or cosine(1), got %d", mode);
    if (N < 1 || Nt < 0 || n_ids < 0) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow: bad sizes N=%d Nt=%lld n_ids=%lld", N, (long long)Nt, (long long)n_ids);
    if (Nt >= (1ll << 31)) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow: Nt too large");
    const int64_t n = texel_ids ? n_ids : Nt;
    if (n == 0) return TEXIR_OK;
    const int64_t need = (int64_t)irt_shadow_workspace_bytes(n, N, M);
    if (!workspace || workspace_bytes < need)
        return fail(TEXIR_ERR_INVALID, "texir_irt_shadow: the workspace holds %lld bytes, the call needs %lld (texir_irt_shadow_workspace_bytes)",
                    (long long)(workspace ? workspace_bytes : 0), (long long)need);
    if (!s->dev.nodes4) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow: the scene has no 4-wide tree (TEXIR_BVH_WIDTH=2 or the binary fallback): the pass has the 64-texel form only");
    HIP_TRY(launch_irt_shadow(dev_of(s, true), pos, nrm, shift, texel_ids, n, Nt, N, mode, bodies, K, sets, M, out, (unsigned long long*)stats, (float*)workspace,
                              (hipStream_t)stream));
    return TEXIR_OK;
}

int64_t texir_irt_shadow_mesh_workspace_bytes(int64_t n_ids, int32_t N, int32_t M)
{
    return (int64_t)irt_shadow_mesh_workspace_bytes(n_ids, N, M);
}

int texir_irt_shadow_mesh(const texir_scene* s, const float* pos, const float* nrm, const float* shift, const int32_t* texel_ids, int64_t n_ids, int64_t Nt,
                          int32_t N, int32_t mode, const texir_scene* const* occluders, int32_t Q, const int32_t* inst_obj, const float* inst_world_to_obj, int32_t K,
                          const uint32_t* sets, int32_t M, float* out, uint64_t* stats, uint32_t flags, void* workspace, int64_t workspace_bytes, void* stream)
{
    // (the counts first: a caller that sized its buffers by a bad count may hold no buffer at all)
    if (Q < 0 || Q > 8) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow_mesh: Q must be in 0..8, got %d (a call takes at most 8 occluders)", Q);
    if (K < 0 || K > 8) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow_mesh: K must be in 0..8, got %d (a call takes at most 8 instances; the lost terms of two calls double-count where their objects overlap along a ray)", K);
    if (M < 1 || M > 8) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow_mesh: M must be in 1..8, got %d (call again for further sets: the results are independent)", M);
    if (K > 0 && !inst_obj) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow_mesh: inst_obj is null");
    for (int j = 0; j < K; j++)
        if (inst_obj[j] < 0 || inst_obj[j] >= Q) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow_mesh: inst_obj[%d] = %d names no occluder (Q = %d)", j, (int)inst_obj[j], Q);
    if (N < 1 || Nt < 0 || n_ids < 0) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow_mesh: bad sizes N=%d Nt=%lld n_ids=%lld", N, (long long)Nt, (long long)n_ids);
    if (mode < 0 || mode > 1) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow_mesh: mode must be uniform(0) or cosine(1), got %d", mode);
    if (Nt >= (1ll << 31)) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow_mesh: Nt too large");
    if (Q > 0 && !occluders) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow_mesh: occluders is null");
    for (int q = 0; q < Q; q++)
        if (!occluders[q]) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow_mesh: occluders[%d] is null", q);
    if (K > 0 && !inst_world_to_obj) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow_mesh: inst_world_to_obj is null");
    if (!sets) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow_mesh: sets is null");
    if (!s || !pos || !nrm || !shift || !out) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow_mesh: null argument");
    const int64_t n = texel_ids ? n_ids : Nt;
    if (n == 0) return TEXIR_OK;
    const int64_t need = (int64_t)irt_shadow_mesh_workspace_bytes(n, N, M);
    if (!workspace || workspace_bytes < need)
        return fail(TEXIR_ERR_INVALID, "texir_irt_shadow_mesh: the workspace holds %lld bytes, the call needs %lld (texir_irt_shadow_mesh_workspace_bytes)",
                    (long long)(workspace ? workspace_bytes : 0), (long long)need);
    if (!s->dev.nodes4) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow_mesh: the scene has no 4-wide tree (TEXIR_BVH_WIDTH=2 or the binary fallback): the pass has the 64-texel form only");
    for (int q = 0; q < Q; q++) {
        if (!occluders[q]->dev.nodes4) return fail(TEXIR_ERR_INVALID, "texir_irt_shadow_mesh: occluders[%d] has no 4-wide tree (TEXIR_BVH_WIDTH=2 or the binary fallback)", q);
        if (occluders[q]->device != s->device)
            return fail(TEXIR_ERR_INVALID, "texir_irt_shadow_mesh: occluders[%d] lives on device %d, the scene on device %d", q, occluders[q]->device, s->device);
    }
    MeshOccluders occ = {};
    for (int j = 0; j < K; j++) mesh_occluder_set(occ, j, occluders[inst_obj[j]]->dev, occluders[inst_obj[j]]->bounds);
    HIP_TRY(launch_irt_shadow_mesh(dev_of(s, true), pos, nrm, shift, texel_ids, n, Nt, N, mode, occ, inst_world_to_obj, K, sets, M, !(flags & 1u), out,
                                   (unsigned long long*)stats, (float*)workspace, (hipStream_t)stream));
    return TEXIR_OK;
}

int texir_scene_reserve_scratch(texir_scene* s, int64_t n_ids, int32_t N)
{
    if (!s || n_ids < 0 || N <= 0) return fail(TEXIR_ERR_INVALID, "texir_scene_reserve_scratch: bad argument");
    const size_t need = irt_scratch_bytes(s->dev, n_ids, N);
    if (need <= s->scratch_bytes) return TEXIR_OK;
    HIP_TRY(hipSetDevice(s->device));
    // Growing never frees: hipGraphs recorded against the smaller block have its address baked into their kernel nodes and may still be replayed.
    // The old block is retired (kept until texir_scene_destroy); launches recorded from now on use the new one.
    float* grown = nullptr;
    HIP_TRY(hipMalloc((void**)&grown, need));
    if (s->d_scratch) s->retired_scratch.push_back(s->d_scratch);
    s->d_scratch = grown;
    s->scratch_bytes = need;
    return TEXIR_OK;
}

int texir_irt_kernel_name(const texir_scene* s, int64_t n_ids, int32_t N, char* buf, int32_t cap)
{
    if (!s || !buf || cap < 1) return fail(TEXIR_ERR_INVALID, "texir_irt_kernel_name: null argument");
    const IrtPlan p = irt_plan(s->dev, n_ids, N);
    snprintf(buf, (size_t)cap, "%s", p.name);
    return TEXIR_OK;
}

int texir_irt_kernel_variant(const texir_scene* s, int64_t n_ids, int32_t N, int32_t mode, int32_t cosine_estimator, char* buf, int32_t cap)
{
    if (!s || !buf || cap < 1) return fail(TEXIR_ERR_INVALID, "texir_irt_kernel_variant: null argument");
    if (mode < 0 || mode > 1 || cosine_estimator < 0 || cosine_estimator > 1 || (cosine_estimator && mode != 1))
        return fail(TEXIR_ERR_INVALID, "texir_irt_kernel_variant: mode must be uniform(0) or cosine(1), the cosine estimator goes with mode 1; got %d, %d", mode, cosine_estimator);
    const IrtPlan p = irt_plan(s->dev, n_ids, N, mode | (cosine_estimator ? 4 : 0));
    snprintf(buf, (size_t)cap, "%s", p.variant);
    return TEXIR_OK;
}

// texir_spec_forward and its training form, which also keeps d w_i / d roughness (dw_ws) and so always needs the Ls_ws workspace
static int spec_forward_call(const char* fn, bool train, const texir_scene* s, const float* normal, const float* albedo, const float* rough, const float* points,
                             const float* irr, const float* cam, const float* shift, int64_t P, int32_t S, float clamp_eps, int32_t ls_given, float* rgb, float* Ls_ws,
                             float* dw_ws, void* stream)
{
    if ((!s && !ls_given) || !normal || !albedo || !rough || !points || !irr || !cam || !shift || !rgb || (train && (!Ls_ws || !dw_ws)))
        return fail(TEXIR_ERR_INVALID, "%s: null argument", fn);
    if (ls_given && !Ls_ws) return fail(TEXIR_ERR_INVALID, "%s: ls_given needs the lighting in Ls_ws", fn);
    if (P < 0 || S <= 0 || !(clamp_eps > 0.f)) return fail(TEXIR_ERR_INVALID, "%s: bad sizes P=%lld S=%d clamp_eps=%g", fn, (long long)P, S, (double)clamp_eps);
    SceneDev none{};
    HIP_TRY(launch_spec_fwd(s ? dev_of(s) : none, normal, albedo, rough, points, irr, cam, shift, P, S, clamp_eps, ls_given ? 1 : 0, rgb, Ls_ws, (hipStream_t)stream, dw_ws));
    return TEXIR_OK;
}

int texir_spec_forward(const texir_scene* s, const float* normal, const float* albedo, const float* rough, const float* points, const float* irr,
                       const float* cam, const float* shift, int64_t P, int32_t S, float clamp_eps, int32_t ls_given, float* rgb, float* Ls_ws, void* stream)
{
    return spec_forward_call("texir_spec_forward", false, s, normal, albedo, rough, points, irr, cam, shift, P, S, clamp_eps, ls_given, rgb, Ls_ws, nullptr, stream);
}

int texir_spec_forward_train(const texir_scene* s, const float* normal, const float* albedo, const float* rough, const float* points, const float* irr,
                             const float* cam, const float* shift, int64_t P, int32_t S, float clamp_eps, int32_t ls_given, float* rgb, float* Ls_ws, float* dw_ws,
                             void* stream)
{
    return spec_forward_call("texir_spec_forward_train", true, s, normal, albedo, rough, points, irr, cam, shift, P, S, clamp_eps, ls_given, rgb, Ls_ws, dw_ws, stream);
}

int texir_spec_backward_ws(const float* irr, const float* Ls_ws, const float* dw_ws, const float* d_rgb, int64_t P, int32_t S, float* d_albedo, float* d_rough, void* stream)
{
    if (!irr || !Ls_ws || !dw_ws || !d_rgb) return fail(TEXIR_ERR_INVALID, "texir_spec_backward_ws: null argument");
    if (P < 0 || S <= 0) return fail(TEXIR_ERR_INVALID, "texir_spec_backward_ws: bad sizes P=%lld S=%d", (long long)P, S);
    HIP_TRY(launch_spec_bwd_ws(irr, Ls_ws, dw_ws, d_rgb, P, S, d_albedo, d_rough, (hipStream_t)stream));
    return TEXIR_OK;
}

int texir_spec_backward(const float* normal, const float* rough, const float* points, const float* irr, const float* cam, const float* shift,
                        const float* Ls_ws, const float* d_rgb, int64_t P, int32_t S, float clamp_eps, float* d_albedo, float* d_rough, void* stream)
{
    if (!normal || !rough || !points || !irr || !cam || !shift || !Ls_ws || !d_rgb) return fail(TEXIR_ERR_INVALID, "texir_spec_backward: null argument");
    if (P < 0 || S <= 0 || !(clamp_eps > 0.f)) return fail(TEXIR_ERR_INVALID, "texir_spec_backward: bad sizes P=%lld S=%d", (long long)P, S);
    HIP_TRY(launch_spec_bwd(normal, rough, points, irr, cam, shift, Ls_ws, d_rgb, P, S, clamp_eps, d_albedo, d_rough, (hipStream_t)stream));
    return TEXIR_OK;
}

int texir_diffuse_irradiance(const texir_scene* s, const float* pos, const float* nrm, const float* shift, int64_t P, int32_t N, int32_t sample_type,
                             float* irr, void* stream)
{
    if (!s || !pos || !nrm || !shift || !irr) return fail(TEXIR_ERR_INVALID, "texir_diffuse_irradiance: null argument");
    if (sample_type < 0 || sample_type > 1) return fail(TEXIR_ERR_INVALID, "texir_diffuse_irradiance: sample_type must be uniform(0) or cosine(1)");
    if (N <= 0 || P < 0 || P >= (1ll << 31)) return fail(TEXIR_ERR_INVALID, "texir_diffuse_irradiance: bad sizes N=%d P=%lld", N, (long long)P);
    unsigned long long* work = next_work_slot(s);
    // uniform: (2 pi / N) sum L n.l -- the IrT estimator; cosine: (pi / N) sum L over cosine-distributed directions
    const int mode = sample_type == 1 ? (1 | 4) : 0;
    HIP_TRY(launch_irt(dev_of(s), pos, nrm, shift, nullptr, P, N, mode, irr, nullptr, work, (hipStream_t)stream));
    return TEXIR_OK;
}

int texir_scene_set_corner_normals(texir_scene* s, const float* cn)
{
    if (!s || !cn) return fail(TEXIR_ERR_INVALID, "texir_scene_set_corner_normals: null argument");
    HIP_TRY(hipSetDevice(s->device));
    std::vector<float> buf((size_t)s->n_slots * 12, 0.f);
    for (int64_t i = 0; i < s->n_slots; i++) {
        if (s->slot_prim[i] == 0xFFFFFFFFu) continue;                            // an empty slot (bvh_build.h): never hit
        const float* src = cn + 9 * (size_t)s->slot_prim[i];
        for (int k = 0; k < 3; k++) {                                            // stored corner k = the caller's corner (rot + k) % 3
            const float* c = src + 3 * ((s->slot_rot[i] + k) % 3);
            buf[12 * i + 4 * k] = c[0]; buf[12 * i + 4 * k + 1] = c[1]; buf[12 * i + 4 * k + 2] = c[2]; buf[12 * i + 4 * k + 3] = 0.f;
        }
    }
    if (!s->d_cnrm) HIP_TRY(hipMalloc(&s->d_cnrm, buf.size() * sizeof(float)));
    HIP_TRY(hipMemcpy(s->d_cnrm, buf.data(), buf.size() * sizeof(float), hipMemcpyHostToDevice));
    return TEXIR_OK;
}

int texir_gbuffer_cast(const texir_scene* s, const float* mvp, int32_t c, int32_t flip_v, float* pos, float* nrm, float* mask, float* uv,
                       float* uv_da, int32_t* tri_id, void* stream)
{
    if (!s || !mvp || !pos || !nrm || !mask || !uv || !uv_da || !tri_id) return fail(TEXIR_ERR_INVALID, "texir_gbuffer_cast: null argument");
    if (c <= 0 || c > 16384) return fail(TEXIR_ERR_INVALID, "texir_gbuffer_cast: bad cube_res %d", c);
    if (!gbuffer_mvp_ok(mvp)) return fail(TEXIR_ERR_INVALID, "texir_gbuffer_cast: an mvp is singular or affine (no eye)");
    HIP_TRY(launch_gbuffer(dev_of(s), mvp, (const float4*)s->d_cnrm, c, flip_v, pos, nrm, mask, uv, uv_da, tri_id, (hipStream_t)stream));
    return TEXIR_OK;
}

int32_t texir_mip_levels(int32_t H, int32_t W, int32_t max_mip_level) { return mip_levels(H, W, max_mip_level); }
int64_t texir_mip_elems(int32_t H, int32_t W, int32_t C, int32_t levels) { return mip_total_elems(H, W, C, levels); }

int texir_mip_build(const float* tex, float* mips_rest, int32_t H, int32_t W, int32_t C, int32_t levels, int32_t from_level, void* stream)
{
    if (!tex || !mips_rest) return fail(TEXIR_ERR_INVALID, "texir_mip_build: null argument");
    if (from_level < 0 || from_level > 1) return fail(TEXIR_ERR_INVALID, "texir_mip_build: from_level must be 0 or 1");
    if (int rc = check_tex("texir_mip_build", -1, H, W, C, levels)) return rc;
    HIP_TRY(launch_mip_build(tex, mips_rest, H, W, C, levels, from_level, (hipStream_t)stream));
    return TEXIR_OK;
}

int texir_tex_fetch_forward(const float* tex, const float* mips_rest, int32_t H, int32_t W, int32_t C, int32_t levels, const float* uv,
                            const float* uv_da, int32_t filter_mode, int64_t P, float* out, void* stream)
{
    const texir_tex_fetch_job q = {tex, const_cast<float*>(mips_rest), H, W, C, levels, /*build_from*/ -1, filter_mode, uv, uv_da, P, out};
    if (int rc = check_fetch_job("texir_tex_fetch_forward", -1, q)) return rc;
    HIP_TRY(launch_tex_fetch(q, (hipStream_t)stream));
    return TEXIR_OK;
}

int texir_tex_fetch_backward(float* d_tex, float* grad_rest, int32_t H, int32_t W, int32_t C, int32_t levels, const float* uv, const float* uv_da,
                             int32_t filter_mode, int64_t P, const float* d_out, void* stream)
{
    if (!d_tex || !uv || !d_out || (filter_mode == 1 && (!uv_da || (levels > 1 && !grad_rest)))) return fail(TEXIR_ERR_INVALID, "texir_tex_fetch_backward: null argument");
    if (filter_mode < 0 || filter_mode > 1 || P < 0) return fail(TEXIR_ERR_INVALID, "texir_tex_fetch_backward: bad filter_mode/P");
    if (int rc = check_tex("texir_tex_fetch_backward", -1, H, W, C, levels)) return rc;
    HIP_TRY(launch_tex_fetch_bwd(d_tex, grad_rest, H, W, C, levels, uv, uv_da, filter_mode, P, d_out, 0, (hipStream_t)stream));
    return TEXIR_OK;
}

int texir_tex_fetch_backward_deferred(float* d_tex, float* grad_rest, int32_t H, int32_t W, int32_t C, int32_t levels, const float* uv,
                                      const float* uv_da, int64_t P, const float* d_out, void* stream)
{
    if (!d_tex || !uv || !d_out || !uv_da || !grad_rest) return fail(TEXIR_ERR_INVALID, "texir_tex_fetch_backward_deferred: null argument");
    if (P < 0 || levels < 2) return fail(TEXIR_ERR_INVALID, "texir_tex_fetch_backward_deferred: needs P >= 0 and at least two mip levels");
    if (int rc = check_tex("texir_tex_fetch_backward_deferred", -1, H, W, C, levels)) return rc;
    HIP_TRY(launch_tex_fetch_bwd(d_tex, grad_rest, H, W, C, levels, uv, uv_da, 1, P, d_out, 1, (hipStream_t)stream));
    return TEXIR_OK;
}

int texir_tex_taps(int32_t H, int32_t W, int32_t C, int32_t levels, const float* uv, const float* uv_da, int32_t filter_mode, int64_t P,
                   int64_t* keys, float* weights, void* stream)
{
    if (!uv || !keys || !weights || (filter_mode == 1 && !uv_da)) return fail(TEXIR_ERR_INVALID, "texir_tex_taps: null argument");
    if (filter_mode < 0 || filter_mode > 1 || P < 0) return fail(TEXIR_ERR_INVALID, "texir_tex_taps: bad filter_mode/P");
    if (int rc = check_tex("texir_tex_taps", -1, H, W, C, levels)) return rc;
    HIP_TRY(launch_tex_taps(H, W, C, levels, uv, uv_da, filter_mode, P, (long long*)keys, weights, (hipStream_t)stream));
    return TEXIR_OK;
}

int texir_tex_gather_backward(float* d_tex, float* grad_rest, int32_t H, int32_t W, int32_t C, int32_t levels, const int64_t* seg_key,
                              const int32_t* seg_start, const int32_t* seg_count, int32_t n_seg, const int32_t* pix, const float* weights,
                              const float* d_out, int32_t filter_mode, int32_t defer_last_fold, void* stream)
{
    const texir_tex_gather_job q = {d_tex, grad_rest, H, W, C, levels, seg_key, seg_start, seg_count, n_seg, pix, weights, d_out, filter_mode, defer_last_fold,
                                    /*rest_mask*/ nullptr, /*d_out2*/ nullptr};
    if (int rc = check_gather_job("texir_tex_gather_backward", -1, q)) return rc;
    HIP_TRY(launch_tex_gather_bwd(q, (hipStream_t)stream));
    return TEXIR_OK;
}

int texir_adam_step_tex(float* param, const float* grad, const uint32_t* grad_mask, const float* grad_level1, const float* grad_level2, float* exp_avg,
                        float* exp_avg_sq, float* mip_level1, int32_t H, int32_t W, int32_t C, float lr, float beta1, float beta2, float eps, int32_t step,
                        float clamp_lo, float clamp_hi, void* stream)
{
    const texir_adam_tex_job q = {param, grad, grad_mask, grad_level1, /*level1_mask*/ nullptr, grad_level2, exp_avg, exp_avg_sq, mip_level1, H, W, C, /*hyper*/ nullptr,
                                  beta1, beta2, eps, clamp_lo, clamp_hi};
    if (int rc = check_adam_tex_job("texir_adam_step_tex", -1, q, &step)) return rc;
    HIP_TRY(launch_adam_tex(q, lr, step, (hipStream_t)stream));
    return TEXIR_OK;
}

int texir_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2, float eps,
                    int32_t step, float clamp_lo, float clamp_hi, void* stream)
{
    if (!param || !grad || !exp_avg || !exp_avg_sq) return fail(TEXIR_ERR_INVALID, "texir_adam_step: null argument");
    if (n < 0 || step < 1) return fail(TEXIR_ERR_INVALID, "texir_adam_step: bad n/step");
    HIP_TRY(launch_adam(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, clamp_lo, clamp_hi, nullptr, (hipStream_t)stream));
    return TEXIR_OK;
}

int texir_adam_tick(double* state, float* hyper, int32_t n_records, uint64_t mask, void* stream)
{
    if (!state || !hyper) return fail(TEXIR_ERR_INVALID, "texir_adam_tick: null argument");
    if (n_records < 0 || n_records > 64) return fail(TEXIR_ERR_INVALID, "texir_adam_tick: 0..64 records per call (got %d)", n_records);
    HIP_TRY(launch_adam_tick(state, hyper, n_records, (unsigned long long)mask, (hipStream_t)stream));
    return TEXIR_OK;
}

int texir_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* hyper, float beta1, float beta2,
                        float eps, float clamp_lo, float clamp_hi, void* stream)
{
    if (!param || !grad || !exp_avg || !exp_avg_sq || !hyper) return fail(TEXIR_ERR_INVALID, "texir_adam_step_dev: null argument");
    if (n < 0) return fail(TEXIR_ERR_INVALID, "texir_adam_step_dev: bad n");
    HIP_TRY(launch_adam(param, grad, exp_avg, exp_avg_sq, n, 0.f, beta1, beta2, eps, 1, clamp_lo, clamp_hi, hyper, (hipStream_t)stream));
    return TEXIR_OK;
}

int texir_adam_step_tex_dev(float* param, const float* grad, const uint32_t* grad_mask, const float* grad_level1, const float* grad_level2, float* exp_avg,
                            float* exp_avg_sq, float* mip_level1, int32_t H, int32_t W, int32_t C, const float* hyper, float beta1, float beta2, float eps,
                            float clamp_lo, float clamp_hi, void* stream)
{
    const texir_adam_tex_job q = {param, grad, grad_mask, grad_level1, /*level1_mask*/ nullptr, grad_level2, exp_avg, exp_avg_sq, mip_level1, H, W, C, hyper,
                                  beta1, beta2, eps, clamp_lo, clamp_hi};
    if (int rc = check_adam_tex_job("texir_adam_step_tex_dev", -1, q)) return rc;
    HIP_TRY(launch_adam_tex(q, 0.f, 1, (hipStream_t)stream));
    return TEXIR_OK;
}

/* ---- the batched forms: every job is held to the rules of its single-texture call, then one launch per kind of kernel (material.hip, adam.hip) ---- */
const char* texir_batch_last_error(void) { return texir_last_error(); }

int texir_grad_add_masked(float* g, const float* g0, const uint32_t* mask, int64_t n_texels, int32_t C, void* stream)
{
    if (n_texels < 0 || C < 1 || C > 4) return fail(TEXIR_ERR_INVALID, "texir_grad_add_masked: bad size n_texels=%lld C=%d", (long long)n_texels, (int)C);
    if (n_texels == 0) return TEXIR_OK;
    if (!g || !g0 || !mask) return fail(TEXIR_ERR_INVALID, "texir_grad_add_masked: null argument");
    HIP_TRY(launch_grad_add_masked(g, g0, mask, n_texels, C, (hipStream_t)stream));
    return TEXIR_OK;
}

int texir_tex_fetch_forward_batch(const texir_tex_fetch_job* jobs, int32_t n, void* stream)
{
    return batch_call("texir_tex_fetch_forward_batch", jobs, n, stream, check_fetch_job, launch_tex_fetch_batch);
}

int texir_tex_gather_backward_batch(const texir_tex_gather_job* jobs, int32_t n, void* stream)
{
    return batch_call("texir_tex_gather_backward_batch", jobs, n, stream, check_gather_job, launch_tex_gather_bwd_batch);
}

int texir_adam_step_tex_dev_batch(const texir_adam_tex_job* jobs, int32_t n, void* stream)
{
    auto check = [](const char* fn, int k, const texir_adam_tex_job& q) { return check_adam_tex_job(fn, k, q); };
    return batch_call("texir_adam_step_tex_dev_batch", jobs, n, stream, check, launch_adam_tex_batch);
}

int64_t texir_loss_workspace_bytes(int64_t P, int32_t C, int32_t R) { return (int64_t)loss_workspace_bytes(P, C, R); }

int texir_loss_forward(int32_t stage, int32_t loss_type, const float* gt, const float* rgb, const float* albedo, const float* rough,
                       const float* rough_womip, const float* empty_mask, const float* gt_mask, const uint8_t* seg_id, const uint8_t* hl,
                       const uint8_t* room_id, int64_t P, int32_t C, int32_t R, int32_t hw, void* workspace, float* out, float* d_rgb,
                       float* d_albedo, float* d_rough, void* stream)
{
    if (stage < 0 || stage > 2) return fail(TEXIR_ERR_INVALID, "texir_loss_forward: stage must be 0, 1 or 2 (got %d)", stage);
    if (loss_type < 0 || loss_type > 2) return fail(TEXIR_ERR_INVALID, "texir_loss_forward: loss_type must be 0 (L1), 1 (L2) or 2 (segmentation term only)");
    if (!gt || !rgb || !empty_mask || !seg_id || !workspace || !out || !d_rgb) return fail(TEXIR_ERR_INVALID, "texir_loss_forward: null argument");
    if (P <= 0 || C <= 0 || C > 255) return fail(TEXIR_ERR_INVALID, "texir_loss_forward: bad sizes P=%lld C=%d", (long long)P, C);
    if (stage == 0 && (!albedo || !gt_mask || !d_albedo)) return fail(TEXIR_ERR_INVALID, "texir_loss_forward: stage 0 needs albedo, gt_mask, d_albedo");
    if (stage == 1 && (!rough || !rough_womip || !hl || !d_rough)) return fail(TEXIR_ERR_INVALID, "texir_loss_forward: stage 1 needs rough, rough_womip, hl, d_rough");
    if (stage == 2 && (!rough || !room_id || !d_rough || R <= 0 || R > 255)) return fail(TEXIR_ERR_INVALID, "texir_loss_forward: stage 2 needs rough, room_id, d_rough, 0<R<256");
    HIP_TRY(launch_loss(stage, loss_type, gt, rgb, albedo, rough, rough_womip, empty_mask, gt_mask, seg_id, hl, room_id, P, C, R, hw, workspace, out,
                        d_rgb, d_albedo, d_rough, (hipStream_t)stream));
    return TEXIR_OK;
}

/* ---- the asset step between the stages (tools/padding_texture.py:49-87), csrc/texpost.hip ---- */
int64_t texir_texture_pad_workspace_bytes(int32_t H, int32_t W)
{
    if (H <= 0 || W <= 0) return 0;
    return (int64_t)texpost_pad_workspace_bytes(H, W);
}

int texir_texture_pad(const float* img, int32_t H, int32_t W, int32_t C, const int32_t* row_map, const int32_t* col_map, float* out, int32_t* src,
                      void* workspace, void* stream)
{
    if (!img || !out || !workspace) return fail(TEXIR_ERR_INVALID, "texir_texture_pad: null argument (img, out and workspace are required)");
    if (out == img) return fail(TEXIR_ERR_INVALID, "texir_texture_pad: out must not be img (holes read other texels of img)");
    if (C < 1 || C > 4) return fail(TEXIR_ERR_INVALID, "texir_texture_pad: C must be 1..4 (got %d)", C);
    if (H < 1 || W < 1 || H > 16384 || W > 16384) return fail(TEXIR_ERR_INVALID, "texir_texture_pad: H and W must be 1..16384 (got %d x %d)", H, W);
    if ((row_map == nullptr) != (col_map == nullptr)) return fail(TEXIR_ERR_INVALID, "texir_texture_pad: row_map and col_map go together (both for the reference mode, neither for nearest)");
    HIP_TRY(launch_texture_pad(img, H, W, C, row_map, col_map, out, src, workspace, (hipStream_t)stream));
    return TEXIR_OK;
}

int texir_texture_denoise(const float* img, int32_t H, int32_t W, const float* guide_nrm, const float* guide_pos, int32_t iterations, float sigma_c,
                          float sigma_n, float sigma_p, float* tmp, float* out, void* stream)
{
    if (!img || !tmp || !out) return fail(TEXIR_ERR_INVALID, "texir_texture_denoise: null argument (img, tmp and out are required)");
    if (out == img || tmp == img || tmp == out) return fail(TEXIR_ERR_INVALID, "texir_texture_denoise: img, tmp and out must be three different buffers");
    if (iterations < 1 || iterations > 6) return fail(TEXIR_ERR_INVALID, "texir_texture_denoise: iterations must be 1..6 (got %d)", iterations);
    if (H < 1 || W < 1 || (int64_t)H * W > (int64_t)1 << 30) return fail(TEXIR_ERR_INVALID, "texir_texture_denoise: bad size %d x %d", H, W);
    if (!(sigma_c > 0.0f) || !(sigma_n >= 0.0f) || !(sigma_p >= 0.0f)) return fail(TEXIR_ERR_INVALID, "texir_texture_denoise: sigma_c must be > 0, sigma_n and sigma_p >= 0");
    HIP_TRY(launch_texture_denoise(img, H, W, guide_nrm, guide_pos, iterations, sigma_c, sigma_n, sigma_p, tmp, out, (hipStream_t)stream));
    return TEXIR_OK;
}

/* ---- the texel G-buffer from the mesh (tracer_o3d_irt.py:99-142), csrc/texraster.hip ---- */
int texir_texel_gbuffer_workspace_bytes(const texir_scene* s, int32_t H, int32_t W, int64_t* bytes)
{
    if (!s || !bytes) return fail(TEXIR_ERR_INVALID, "texir_texel_gbuffer_workspace_bytes: null argument");
    if (H < 1 || W < 1 || H > 16384 || W > 16384) return fail(TEXIR_ERR_INVALID, "texir_texel_gbuffer_workspace_bytes: H and W must be 1..16384 (got %d x %d)", H, W);
    *bytes = (int64_t)texel_raster_workspace_bytes(s->n_slots, s->n_tris, H, W);
    return TEXIR_OK;
}

int texir_texel_gbuffer(const texir_scene* s, int32_t H, int32_t W, int32_t normal_mode, float offset, float* pos, float* nrm, uint32_t* prim_id, float* bary,
                        void* workspace, void* stream)
{
    if (!s || !pos || !nrm || !workspace) return fail(TEXIR_ERR_INVALID, "texir_texel_gbuffer: null argument (scene, pos, nrm and workspace are required)");
    if (H < 1 || W < 1 || H > 16384 || W > 16384) return fail(TEXIR_ERR_INVALID, "texir_texel_gbuffer: H and W must be 1..16384 (got %d x %d)", H, W);
    if (normal_mode != TEXIR_NORMAL_GEOMETRIC && normal_mode != TEXIR_NORMAL_SHADING)
        return fail(TEXIR_ERR_INVALID, "texir_texel_gbuffer: normal_mode must be TEXIR_NORMAL_GEOMETRIC (0) or TEXIR_NORMAL_SHADING (1), got %d", normal_mode);
    if (normal_mode == TEXIR_NORMAL_SHADING && !s->d_cnrm)
        return fail(TEXIR_ERR_INVALID, "texir_texel_gbuffer: shading normals asked for but texir_scene_set_corner_normals has not been called");
    if (!(offset - offset == 0.0f)) return fail(TEXIR_ERR_INVALID, "texir_texel_gbuffer: offset must be finite");
    if (!s->d_uvs) return fail(TEXIR_ERR_INVALID, "texir_texel_gbuffer: the scene has no corner uvs");
    HIP_TRY(launch_texel_raster(dev_of(s), (const float4*)s->d_cnrm, s->n_slots, s->n_tris, H, W, normal_mode == TEXIR_NORMAL_SHADING, offset, pos, nrm, prim_id,
                                bary, workspace, (hipStream_t)stream));
    return TEXIR_OK;
}

/* ---- the radiance atlas + index texture from calibrated panoramas, csrc/texbake.hip.  The reference has no producer of either file: its private capture
 * pipeline writes 0.png and tools/trans_hdr_tex.py:16-61 (repackHDRTexture) only gathers the panoramas' pixels through those codes; the panorama pixel of
 * a direction is the one utils/Pano2Cube.py:57-82 reads (grid_sample nearest, align_corners=False). ---- */
static int atlas_bake_call(const char* fn, bool any, const texir_scene* s, const float* pos, const float* nrm, const int32_t* texel_ids, int64_t n_ids, int64_t Nt,
                           const float* cams, const float* cam_pos, const float* panos, const uint8_t* valid, int32_t K, int32_t h, int32_t w, float cos_min,
                           int32_t* view, int32_t* pix, float* rgb, uint64_t* stats, void* stream)
{
    if (!s || !pos || !nrm || !cams || !cam_pos || !panos) return fail(TEXIR_ERR_INVALID, "%s: null argument (scene, pos, nrm, cams, cam_pos and panos are required)", fn);
    if (!view || !pix || !rgb) return fail(TEXIR_ERR_INVALID, "%s: null output (view, pix and rgb are required)", fn);
    if (K < 1) return fail(TEXIR_ERR_INVALID, "%s: K must be >= 1 (got %d)", fn, K);
    if (h < 1 || w < 1 || h > 32768 || w > 32768) return fail(TEXIR_ERR_INVALID, "%s: h and w must be 1..32768 (got %d x %d)", fn, h, w);
    if (Nt < 0 || (texel_ids && n_ids < 0)) return fail(TEXIR_ERR_INVALID, "%s: negative texel count", fn);
    if (!(cos_min - cos_min == 0.0f)) return fail(TEXIR_ERR_INVALID, "%s: cos_min must be finite", fn);
    HIP_TRY(launch_atlas_bake(dev_of(s), pos, nrm, texel_ids, texel_ids ? n_ids : Nt, Nt, cams, cam_pos, panos, valid, K, h, w, cos_min, view, pix, rgb,
                              (unsigned long long*)stats, (hipStream_t)stream, any));
    return TEXIR_OK;
}

int texir_atlas_bake(const texir_scene* s, const float* pos, const float* nrm, const int32_t* texel_ids, int64_t n_ids, int64_t Nt, const float* cams,
                     const float* cam_pos, const float* panos, const uint8_t* valid, int32_t K, int32_t h, int32_t w, float cos_min, int32_t* view, int32_t* pix,
                     float* rgb, uint64_t* stats, void* stream)
{
    return atlas_bake_call("texir_atlas_bake", false, s, pos, nrm, texel_ids, n_ids, Nt, cams, cam_pos, panos, valid, K, h, w, cos_min, view, pix, rgb, stats, stream);
}

/* the same bake with the segment test as an any-hit query (trace_occluded): the bits of texir_atlas_bake */
int texir_atlas_bake_any(const texir_scene* s, const float* pos, const float* nrm, const int32_t* texel_ids, int64_t n_ids, int64_t Nt, const float* cams,
                         const float* cam_pos, const float* panos, const uint8_t* valid, int32_t K, int32_t h, int32_t w, float cos_min, int32_t* view, int32_t* pix,
                         float* rgb, uint64_t* stats, void* stream)
{
    return atlas_bake_call("texir_atlas_bake_any", true, s, pos, nrm, texel_ids, n_ids, Nt, cams, cam_pos, panos, valid, K, h, w, cos_min, view, pix, rgb, stats, stream);
}

/* the gathers of tools/trans_hdr_tex.py:16-216 (repackHDRTexture, repackSegTexture, repackAlbedoTexture, repackRoughnessTexture: pixel (row, col) of
 * panorama `view`, utils/Pano2Cube.py:57-82's pixel) through the (view, pix) texir_atlas_bake wrote */
int texir_atlas_gather(const int32_t* view, const int32_t* pix, const int32_t* texel_ids, int64_t n_ids, int64_t Nt, const float* imgs, int32_t K, int32_t h,
                       int32_t w, int32_t C, float* out, void* stream)
{
    if (!view || !pix || !imgs) return fail(TEXIR_ERR_INVALID, "texir_atlas_gather: null argument (view, pix and imgs are required)");
    if (!out) return fail(TEXIR_ERR_INVALID, "texir_atlas_gather: null output");
    if (K < 1) return fail(TEXIR_ERR_INVALID, "texir_atlas_gather: K must be >= 1 (got %d)", K);
    if (h < 1 || w < 1 || h > 32768 || w > 32768) return fail(TEXIR_ERR_INVALID, "texir_atlas_gather: h and w must be 1..32768 (got %d x %d)", h, w);
    if (C < 1 || C > 4) return fail(TEXIR_ERR_INVALID, "texir_atlas_gather: C must be 1..4 (got %d)", C);
    if (Nt < 0 || (texel_ids && n_ids < 0)) return fail(TEXIR_ERR_INVALID, "texir_atlas_gather: negative texel count");
    HIP_TRY(launch_atlas_gather(view, pix, texel_ids, texel_ids ? n_ids : Nt, Nt, imgs, K, h, w, C, out, (hipStream_t)stream));
    return TEXIR_OK;
}

/* ---- the fill of the texels the bake left unobserved, csrc/texfill.hip: nearest compatible observed texel in world space (no reference counterpart) ---- */
int64_t texir_atlas_fill_workspace_bytes(int64_t n_src, int64_t n_holes)
{
    if (n_src < 0 || n_holes < 0) return 0;
    return (int64_t)atlas_fill_workspace_bytes(n_src, n_holes);
}

static bool fill_bounds_ok(const float* b)
{
    if (!b) return false;
    for (int i = 0; i < 6; i++)
        if (!(b[i] - b[i] == 0.0f)) return false;
    return b[3] >= b[0] && b[4] >= b[1] && b[5] >= b[2];
}

float texir_atlas_fill_cell(const float* bounds, int64_t n_src, float cell)
{
    if (!fill_bounds_ok(bounds) || n_src < 0) return 0.0f;
    return atlas_fill_cell(bounds, n_src, cell);
}

int texir_atlas_fill(const float* pos, const float* nrm, int64_t Nt, const int32_t* source_ids, int64_t n_src, const int32_t* hole_ids, int64_t n_holes,
                     const float* bounds, float cos_fill, float max_dist, float cell, int32_t* src, float* dist2, uint64_t* stats, void* workspace, void* stream)
{
    if (!pos || !nrm || !src || !workspace) return fail(TEXIR_ERR_INVALID, "texir_atlas_fill: null argument (pos, nrm, src and workspace are required)");
    if (Nt < 0 || n_src < 0 || n_holes < 0) return fail(TEXIR_ERR_INVALID, "texir_atlas_fill: negative count");
    if ((n_src > 0 && !source_ids) || (n_holes > 0 && !hole_ids)) return fail(TEXIR_ERR_INVALID, "texir_atlas_fill: null id list");
    if (n_src > 0xFFFFFFFFll) return fail(TEXIR_ERR_INVALID, "texir_atlas_fill: n_src must fit 32 bits");
    if (!fill_bounds_ok(bounds)) return fail(TEXIR_ERR_INVALID, "texir_atlas_fill: bounds must be six finite floats (min x y z, max x y z) with max >= min");
    if (!(cos_fill >= 0.0f && cos_fill <= 1.0f)) return fail(TEXIR_ERR_INVALID, "texir_atlas_fill: cos_fill must be in [0, 1] (got %g)", (double)cos_fill);
    if (!(max_dist > 0.0f)) return fail(TEXIR_ERR_INVALID, "texir_atlas_fill: max_dist must be > 0 (+inf allowed; got %g)", (double)max_dist);
    if (!(cell >= 0.0f) || !(cell - cell == 0.0f)) return fail(TEXIR_ERR_INVALID, "texir_atlas_fill: cell must be finite and >= 0 (0: the library chooses)");
    if (((uintptr_t)workspace & 15) != 0) return fail(TEXIR_ERR_INVALID, "texir_atlas_fill: workspace must be 16-byte aligned");
    HIP_TRY(launch_atlas_fill(pos, nrm, Nt, source_ids, n_src, hole_ids, n_holes, bounds, cos_fill, max_dist, cell, src, dist2, (unsigned long long*)stats,
                              workspace, (hipStream_t)stream));
    return TEXIR_OK;
}

/* ---- inserted emitters, csrc/irtlight.hip: the direct irradiance factor F of K new area lights per listed texel (the "moving" half of
 * tools/relighting_varying.py leaves the reference for an external renderer; include/texir_hip.h states the rule) ---- */
static int irt_lights_call(const char* fn, bool any, const texir_scene* s, const float* pos, const float* nrm, const float* shift, const int32_t* texel_ids,
                           int64_t n_ids, int64_t Nt, const float* lights, int32_t K, int32_t S, float t_max, float* F, uint64_t* stats, void* stream)
{
    // (K first: a caller that sized `lights` and `F` by a bad K may hold no buffer at all)
    if (K < 0 || K > 8) return fail(TEXIR_ERR_INVALID, "%s: K must be in 0..8, got %d (call again for further lights: the factors add)", fn, K);
    if (S < 1 || S > 65536) return fail(TEXIR_ERR_INVALID, "%s: S must be in 1..65536, got %d", fn, S);
    if (!(t_max - t_max == 0.0f)) return fail(TEXIR_ERR_INVALID, "%s: t_max must be finite", fn);
    if (Nt < 0 || (texel_ids && n_ids < 0)) return fail(TEXIR_ERR_INVALID, "%s: negative texel count", fn);
    if (Nt >= (1ll << 31)) return fail(TEXIR_ERR_INVALID, "%s: Nt too large", fn);
    const int64_t n = texel_ids ? n_ids : Nt;
    if (K == 0 || n == 0) return TEXIR_OK;
    if (!s || !pos || !nrm || !shift || !lights || !F) return fail(TEXIR_ERR_INVALID, "%s: null argument (scene, pos, nrm, shift, lights and F are required)", fn);
    HIP_TRY(launch_irt_lights(dev_of(s), pos, nrm, shift, texel_ids, n, Nt, lights, K, S, t_max, F, (unsigned long long*)stats, (hipStream_t)stream, any));
    return TEXIR_OK;
}

int texir_irt_lights(const texir_scene* s, const float* pos, const float* nrm, const float* shift, const int32_t* texel_ids, int64_t n_ids, int64_t Nt,
                     const float* lights, int32_t K, int32_t S, float t_max, float* F, uint64_t* stats, void* stream)
{
    return irt_lights_call("texir_irt_lights", false, s, pos, nrm, shift, texel_ids, n_ids, Nt, lights, K, S, t_max, F, stats, stream);
}

/* the same factors with visibility as an any-hit query (trace_occluded): the bits of texir_irt_lights */
int texir_irt_lights_any(const texir_scene* s, const float* pos, const float* nrm, const float* shift, const int32_t* texel_ids, int64_t n_ids, int64_t Nt,
                         const float* lights, int32_t K, int32_t S, float t_max, float* F, uint64_t* stats, void* stream)
{
    return irt_lights_call("texir_irt_lights_any", true, s, pos, nrm, shift, texel_ids, n_ids, Nt, lights, K, S, t_max, F, stats, stream);
}

/* ---- inserted emitters, csrc/speclight.hip: the specular response factor R of K new area lights per listed pixel (multiple importance sampling over
 * the light's area and the GGX lobe; include/texir_hip.h states the rule).  The argument checks and error text are the light pass's ---- */
static int spec_lights_call(const char* fn, bool any, const texir_scene* s, const float* pos, const float* nrm, const float* rough, const float* shift, const float* cam,
                            const int32_t* pixel_ids, int64_t n_ids, int64_t P, const float* lights, int32_t K, int32_t S, float t_max, float ceps, float* R,
                            uint64_t* stats, void* stream)
{
    if (K < 0 || K > 8) return fail(TEXIR_ERR_INVALID, "%s: K must be in 0..8, got %d (call again for further lights: the factors add)", fn, K);
    if (S < 1 || S > 65536) return fail(TEXIR_ERR_INVALID, "%s: S must be in 1..65536, got %d", fn, S);
    if (!(t_max - t_max == 0.0f)) return fail(TEXIR_ERR_INVALID, "%s: t_max must be finite", fn);
    if (!(ceps > 0.0f) || !(ceps - ceps == 0.0f)) return fail(TEXIR_ERR_INVALID, "%s: clamp_eps must be finite and > 0 (got %g)", fn, (double)ceps);
    if (P < 0 || (pixel_ids && n_ids < 0)) return fail(TEXIR_ERR_INVALID, "%s: negative pixel count", fn);
    if (P >= (1ll << 31)) return fail(TEXIR_ERR_INVALID, "%s: P too large", fn);
    const int64_t n = pixel_ids ? n_ids : P;
    if (K == 0 || n == 0) return TEXIR_OK;
    if (!s || !pos || !nrm || !rough || !shift || !cam || !lights || !R)
        return fail(TEXIR_ERR_INVALID, "%s: null argument (scene, pos, nrm, rough, shift, cam, lights and R are required)", fn);
    HIP_TRY(launch_spec_lights(dev_of(s), pos, nrm, rough, shift, cam, pixel_ids, n, P, lights, K, S, t_max, ceps, R, (unsigned long long*)stats, (hipStream_t)stream, any));
    return TEXIR_OK;
}

int texir_spec_lights(const texir_scene* s, const float* pos, const float* nrm, const float* rough, const float* shift, const float* cam, const int32_t* pixel_ids,
                      int64_t n_ids, int64_t P, const float* lights, int32_t K, int32_t S, float t_max, float clamp_eps, float* R, uint64_t* stats, void* stream)
{
    return spec_lights_call("texir_spec_lights", false, s, pos, nrm, rough, shift, cam, pixel_ids, n_ids, P, lights, K, S, t_max, clamp_eps, R, stats, stream);
}

/* the same factors with visibility as an any-hit query (trace_occluded): the bits of texir_spec_lights */
int texir_spec_lights_any(const texir_scene* s, const float* pos, const float* nrm, const float* rough, const float* shift, const float* cam, const int32_t* pixel_ids,
                          int64_t n_ids, int64_t P, const float* lights, int32_t K, int32_t S, float t_max, float clamp_eps, float* R, uint64_t* stats, void* stream)
{
    return spec_lights_call("texir_spec_lights_any", true, s, pos, nrm, rough, shift, cam, pixel_ids, n_ids, P, lights, K, S, t_max, clamp_eps, R, stats, stream);
}

/* ---- inserted emitters behind inserted mesh objects, csrc/irtlightmesh.hip and csrc/speclightmesh.hip (include/texir_hip.h texir_irt_lights_mesh states
 * the rule).  The conditions on the objects are texir_irt_shadow_mesh's, in its text style, reported before any null buffer; `early`: the counts, `late`:
 * what needs the handles ---- */
static int mesh_counts_check(const char* fn, const texir_scene* const* occluders, int32_t Q, const int32_t* inst_obj, int32_t J)
{
    if (Q < 0 || Q > 8) return fail(TEXIR_ERR_INVALID, "%s: Q must be in 0..8, got %d (a call takes at most 8 occluders)", fn, Q);
    if (J < 0 || J > 8) return fail(TEXIR_ERR_INVALID, "%s: J must be in 0..8, got %d (a call takes at most 8 instances)", fn, J);
    if (J > 0 && !inst_obj) return fail(TEXIR_ERR_INVALID, "%s: inst_obj is null", fn);
    for (int j = 0; j < J; j++)
        if (inst_obj[j] < 0 || inst_obj[j] >= Q) return fail(TEXIR_ERR_INVALID, "%s: inst_obj[%d] = %d names no occluder (Q = %d)", fn, j, (int)inst_obj[j], Q);
    if (Q > 0 && !occluders) return fail(TEXIR_ERR_INVALID, "%s: occluders is null", fn);
    for (int q = 0; q < Q; q++)
        if (!occluders[q]) return fail(TEXIR_ERR_INVALID, "%s: occluders[%d] is null", fn, q);
    return TEXIR_OK;
}

static int mesh_handles_check(const char* fn, const texir_scene* s, const texir_scene* const* occluders, int32_t Q, const int32_t* inst_obj,
                              const float* inst_world_to_obj, int32_t J, MeshOccluders& occ)
{
    if (J > 0 && !inst_world_to_obj) return fail(TEXIR_ERR_INVALID, "%s: inst_world_to_obj is null", fn);
    if (!s->dev.nodes4) return fail(TEXIR_ERR_INVALID, "%s: the scene has no 4-wide tree (TEXIR_BVH_WIDTH=2 or the binary fallback): the pass has the 4-wide form only", fn);
    for (int q = 0; q < Q; q++) {
        if (!occluders[q]->dev.nodes4) return fail(TEXIR_ERR_INVALID, "%s: occluders[%d] has no 4-wide tree (TEXIR_BVH_WIDTH=2 or the binary fallback)", fn, q);
        if (occluders[q]->device != s->device)
            return fail(TEXIR_ERR_INVALID, "%s: occluders[%d] lives on device %d, the scene on device %d", fn, q, occluders[q]->device, s->device);
    }
    for (int j = 0; j < J; j++) mesh_occluder_set(occ, j, occluders[inst_obj[j]]->dev, occluders[inst_obj[j]]->bounds);
    return TEXIR_OK;
}

int texir_irt_lights_mesh(const texir_scene* s, const float* pos, const float* nrm, const float* shift, const int32_t* texel_ids, int64_t n_ids, int64_t Nt,
                          const float* lights, int32_t K, int32_t S, float t_max, const texir_scene* const* occluders, int32_t Q, const int32_t* inst_obj,
                          const float* inst_world_to_obj, int32_t J, uint32_t flags, float* F, uint64_t* stats, void* stream)
{
    const char* fn = "texir_irt_lights_mesh";
    if (int e = mesh_counts_check(fn, occluders, Q, inst_obj, J)) return e;
    if (K < 0 || K > 8) return fail(TEXIR_ERR_INVALID, "%s: K must be in 0..8, got %d (call again for further lights: the factors add)", fn, K);
    if (S < 1 || S > 65536) return fail(TEXIR_ERR_INVALID, "%s: S must be in 1..65536, got %d", fn, S);
    if (!(t_max - t_max == 0.0f)) return fail(TEXIR_ERR_INVALID, "%s: t_max must be finite", fn);
    if (Nt < 0 || (texel_ids && n_ids < 0)) return fail(TEXIR_ERR_INVALID, "%s: negative texel count", fn);
    if (Nt >= (1ll << 31)) return fail(TEXIR_ERR_INVALID, "%s: Nt too large", fn);
    const int64_t n = texel_ids ? n_ids : Nt;
    if (K == 0 || n == 0) return TEXIR_OK;
    if (!s || !pos || !nrm || !shift || !lights || !F) return fail(TEXIR_ERR_INVALID, "%s: null argument (scene, pos, nrm, shift, lights and F are required)", fn);
    MeshOccluders occ = {};
    if (int e = mesh_handles_check(fn, s, occluders, Q, inst_obj, inst_world_to_obj, J, occ)) return e;
    HIP_TRY(launch_irt_lights_mesh(dev_of(s), pos, nrm, shift, texel_ids, n, Nt, lights, K, S, t_max, occ, inst_world_to_obj, J, !(flags & 1u), F,
                                   (unsigned long long*)stats, (hipStream_t)stream));
    return TEXIR_OK;
}

int texir_spec_lights_mesh(const texir_scene* s, const float* pos, const float* nrm, const float* rough, const float* shift, const float* cam, const int32_t* pixel_ids,
                           int64_t n_ids, int64_t P, const float* lights, int32_t K, int32_t S, float t_max, float ceps, const texir_scene* const* occluders, int32_t Q,
                           const int32_t* inst_obj, const float* inst_world_to_obj, int32_t J, uint32_t flags, float* R, uint64_t* stats, void* stream)
{
    const char* fn = "texir_spec_lights_mesh";
    if (int e = mesh_counts_check(fn, occluders, Q, inst_obj, J)) return e;
    if (K < 0 || K > 8) return fail(TEXIR_ERR_INVALID, "%s: K must be in 0..8, got %d (call again for further lights: the factors add)", fn, K);
    if (S < 1 || S > 65536) return fail(TEXIR_ERR_INVALID, "%s: S must be in 1..65536, got %d", fn, S);
    if (!(t_max - t_max == 0.0f)) return fail(TEXIR_ERR_INVALID, "%s: t_max must be finite", fn);
    if (!(ceps > 0.0f) || !(ceps - ceps == 0.0f)) return fail(TEXIR_ERR_INVALID, "%s: clamp_eps must be finite and > 0 (got %g)", fn, (double)ceps);
    if (P < 0 || (pixel_ids && n_ids < 0)) return fail(TEXIR_ERR_INVALID, "%s: negative pixel count", fn);
    if (P >= (1ll << 31)) return fail(TEXIR_ERR_INVALID, "%s: P too large", fn);
    const int64_t n = pixel_ids ? n_ids : P;
    if (K == 0 || n == 0) return TEXIR_OK;
    if (!s || !pos || !nrm || !rough || !shift || !cam || !lights || !R)
        return fail(TEXIR_ERR_INVALID, "%s: null argument (scene, pos, nrm, rough, shift, cam, lights and R are required)", fn);
    MeshOccluders occ = {};
    if (int e = mesh_handles_check(fn, s, occluders, Q, inst_obj, inst_world_to_obj, J, occ)) return e;
    HIP_TRY(launch_spec_lights_mesh(dev_of(s), pos, nrm, rough, shift, cam, pixel_ids, n, P, lights, K, S, t_max, ceps, occ, inst_world_to_obj, J, !(flags & 1u), R,
                                    (unsigned long long*)stats, (hipStream_t)stream));
    return TEXIR_OK;
}

/* ---- the shadow of inserted bodies and mesh objects in the specular term of captured light, csrc/specshadow.hip (include/texir_hip.h texir_spec_shadow
 * states the rule).  The counts first, in the text style of texir_irt_shadow / texir_irt_shadow_mesh: a caller that sized its buffers by a bad count may
 * hold no buffer at all ---- */
int texir_spec_shadow(const texir_scene* s, const float* normal, const float* rough, const float* points, const float* cam, const float* shift, const int32_t* pixel_ids,
                      int64_t n_ids, int64_t P, int32_t S, float ceps, const float* bodies, int32_t Kb, const texir_scene* const* occluders, int32_t Q,
                      const int32_t* inst_obj, const float* inst_world_to_obj, int32_t J, const uint32_t* sets, int32_t M, uint32_t flags, float* out, uint64_t* stats,
                      void* stream)
{
    const char* fn = "texir_spec_shadow";
    if (Kb < 0 || Kb > 8) return fail(TEXIR_ERR_INVALID, "%s: Kb must be in 0..8, got %d (a call takes at most 8 bodies)", fn, Kb);
    if (int e = mesh_counts_check(fn, occluders, Q, inst_obj, J)) return e;
    if (M < 1 || M > 8) return fail(TEXIR_ERR_INVALID, "%s: M must be in 1..8, got %d (call again for further sets: the results are independent)", fn, M);
    if (S < 1 || S > 65536) return fail(TEXIR_ERR_INVALID, "%s: S must be in 1..65536, got %d", fn, S);
    if (!(ceps > 0.0f) || !(ceps - ceps == 0.0f)) return fail(TEXIR_ERR_INVALID, "%s: clamp_eps must be finite and > 0 (got %g)", fn, (double)ceps);
    if (P < 0 || (pixel_ids && n_ids < 0)) return fail(TEXIR_ERR_INVALID, "%s: negative pixel count", fn);
    if (P >= (1ll << 31)) return fail(TEXIR_ERR_INVALID, "%s: P too large", fn);
    if (Kb > 0 && !bodies) return fail(TEXIR_ERR_INVALID, "%s: bodies is null", fn);
    if (!sets) return fail(TEXIR_ERR_INVALID, "%s: sets is null", fn);
    const int64_t n = pixel_ids ? n_ids : P;
    if (n == 0) return TEXIR_OK;
    if (!s || !normal || !rough || !points || !cam || !shift || !out)
        return fail(TEXIR_ERR_INVALID, "%s: null argument (scene, normal, rough, points, cam, shift and out are required)", fn);
    MeshOccluders occ = {};
    if (int e = mesh_handles_check(fn, s, occluders, Q, inst_obj, inst_world_to_obj, J, occ)) return e;
    HIP_TRY(launch_spec_shadow(dev_of(s), normal, rough, points, cam, shift, pixel_ids, n, P, S, ceps, bodies, Kb, occ, inst_world_to_obj, J, sets, M, !(flags & 1u), out,
                               (unsigned long long*)stats, (hipStream_t)stream));
    return TEXIR_OK;
}

/* ---- the cube G-buffer with inserted mesh objects drawn in the view, csrc/gbuffermesh.hip (include/texir_hip.h texir_gbuffer_cast_mesh states the rule).
 * The conditions on the objects first, as in the sibling passes, then texir_gbuffer_cast's own; nothing is launched or written on an error ---- */
int texir_gbuffer_cast_mesh(const texir_scene* s, const float* mvp, int32_t c, int32_t flip_v, const texir_scene* const* occluders, int32_t Q, const int32_t* inst_obj,
                            const float* inst_world_to_obj, int32_t J, uint32_t flags, float* pos, float* nrm, float* mask, float* uv, float* uv_da, int32_t* tri_id,
                            int32_t* inst_id, void* stream)
{
    const char* fn = "texir_gbuffer_cast_mesh";
    if (int e = mesh_counts_check(fn, occluders, Q, inst_obj, J)) return e;
    if (!s || !mvp || !pos || !nrm || !mask || !uv || !uv_da || !tri_id || !inst_id)
        return fail(TEXIR_ERR_INVALID, "%s: null argument (scene, mvp, pos, nrm, mask, uv, uv_da, tri_id and inst_id are required)", fn);
    if (c <= 0 || c > 16384) return fail(TEXIR_ERR_INVALID, "%s: bad cube_res %d", fn, c);
    if (!gbuffer_mvp_ok(mvp)) return fail(TEXIR_ERR_INVALID, "%s: an mvp is singular or affine (no eye)", fn);
    GbufMeshOccluders mo = {};
    if (int e = mesh_handles_check(fn, s, occluders, Q, inst_obj, inst_world_to_obj, J, mo.occ)) return e;
    for (int j = 0; j < J; j++) mo.tris[j] = occluders[inst_obj[j]]->dev.tris;
    HIP_TRY(launch_gbuffer_mesh(dev_of(s), mvp, (const float4*)s->d_cnrm, c, flip_v, mo, inst_world_to_obj, J, !(flags & 1u), pos, nrm, mask, uv, uv_da, tri_id, inst_id,
                                (hipStream_t)stream));
    return TEXIR_OK;
}

}  // extern "C"

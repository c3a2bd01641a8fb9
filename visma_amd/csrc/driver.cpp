// driver.cpp -- the host driver's C ABI: contexts, cloud upload, passes, the RegistrationICP loop and its
// batched forms, options, multi-GPU bring-up.  (Engine / HipEngine: engine.hpp, hip_engine.cpp; the steps either
// side of ICP: aux_api.cpp; the corpus work queue: corpus.cpp.)
#include "driver_ctx.hpp"
#include "colormap_solve.hpp"
#ifdef VISMA_TEST_SEAMS
#include "../../include/visma_icp_testing.h"
#endif

namespace {

#ifdef VISMA_TEST_SEAMS
class HookEngine : public Engine {
public:
    HookEngine(const visma_icp_engine &vt, void *user) : vt_(vt), user_(user) {}
    int set_source(const float *p, int64_t n) override { ns_ = n; has_source_normals_ = has_source_colors_ = false; return wrap(vt_.set_source(user_, p, n)); }
    int set_target(const float *p, int64_t n) override { nt_ = n; has_normals_ = has_target_colors_ = false; drop_color_gradient(); return wrap(vt_.set_target(user_, p, n)); }
    int set_target_normals(const float *p, int64_t n) override
    {
        if (!vt_.set_target_normals) { err_ = "engine has no normals support"; return VISMA_ICP_ERR_ENGINE; }
        has_normals_ = true;
        drop_color_gradient();
        return wrap(vt_.set_target_normals(user_, p, n));
    }
    int nn_pass(const Mat4 &Tc, double r) override { return wrap(vt_.nn_pass(user_, Tc.m, r)); }
    int reduce(const Mat4 &Tc, bool plane, const double offset[3], double *st) override
    {
        const double zero[3] = {0, 0, 0};
        return wrap(vt_.reduce(user_, Tc.m, offset ? offset : zero, plane ? 1 : 0, st));
    }
    int get_correspondences(int32_t *idx, float *d2) override
    {
        std::vector<float> tmp;
        if (!d2) { tmp.resize((size_t)(ns_ > 0 ? ns_ : 1)); d2 = tmp.data(); }
        return wrap(vt_.get_correspondences(user_, idx, d2));
    }

private:
    int wrap(int rc)
    {
        if (rc == 0) return VISMA_ICP_OK;
        err_ = "engine callback returned " + std::to_string(rc);
        return VISMA_ICP_ERR_ENGINE;
    }
    visma_icp_engine vt_;
    void *user_;
};
#endif  // VISMA_TEST_SEAMS


}  // namespace

namespace {

// (x - c) as fp32 (x,y,z,0) rows; `par`: spread over host threads
void pack_f64_to(const double *xyz, int64_t n, int stride, const double c[3], float *out, bool par)
{
    auto body = [&](int64_t ch) {
        const int64_t lo = ch * kHostChunk, hi = std::min(n, lo + kHostChunk);
        for (int64_t i = lo; i < hi; i++) {
            const double *p = xyz + (size_t)i * stride;
            out[4 * i + 0] = (float)(p[0] - c[0]);
            out[4 * i + 1] = (float)(p[1] - c[1]);
            out[4 * i + 2] = (float)(p[2] - c[2]);
            out[4 * i + 3] = 0.f;
        }
    };
    const int64_t nch = (n + kHostChunk - 1) / kHostChunk;
    if (par) parallel_for(nch, 1, body);
    else for (int64_t ch = 0; ch < nch; ch++) body(ch);
}

int pack_f64(const double *xyz, int64_t n, int stride, const double c[3], std::vector<float> &out)
{
    out.resize((size_t)(n > 0 ? n : 1) * 4);
    pack_f64_to(xyz, n, stride, c, out.data(), false);
    return 0;
}

void pack_f32_to(const float *xyz, int64_t n, int stride, float *out)
{
    for (int64_t i = 0; i < n; i++) {
        const float *p = xyz + (size_t)i * stride;
        out[4 * i + 0] = p[0];
        out[4 * i + 1] = p[1];
        out[4 * i + 2] = p[2];
        out[4 * i + 3] = 0.f;
    }
}

// Centroid in f64.  Fixed chunks summed in index order and combined in chunk order: the
// value does not depend on the number of threads (every rank of a multi-GPU run, and every
// repeat, gets the same centre).
void centroid_f64(const double *xyz, int64_t n, int stride, double c[3], bool par)
{
    c[0] = c[1] = c[2] = 0.0;
    if (n <= 0) return;
    const int64_t nch = (n + kHostChunk - 1) / kHostChunk;
    std::vector<double> part((size_t)nch * 3, 0.0);
    auto body = [&](int64_t ch) {
        const int64_t lo = ch * kHostChunk, hi = std::min(n, lo + kHostChunk);
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int64_t i = lo; i < hi; i++) {
            const double *p = xyz + (size_t)i * stride;
            s0 += p[0]; s1 += p[1]; s2 += p[2];
        }
        part[3 * ch] = s0; part[3 * ch + 1] = s1; part[3 * ch + 2] = s2;
    };
    if (par) parallel_for(nch, 1, body);
    else for (int64_t ch = 0; ch < nch; ch++) body(ch);
    for (int64_t ch = 0; ch < nch; ch++)
        for (int a = 0; a < 3; a++) c[a] += part[3 * ch + a];
    for (int a = 0; a < 3; a++) c[a] /= (double)n;
}

// Spatial (Morton / Z-order) permutation of packed xyzw points.  Neighbouring
// lanes then query neighbouring grid cells, so a wave's candidate runs overlap
// in L1/L2.  Returns order[pos] = original index and permutes `pts` in place.
inline uint32_t spread10(uint32_t v)
{
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

void morton_order_ptr(float *pts, int64_t n, std::vector<int32_t> &order, bool par)
{
    order.resize((size_t)n);
    if (n <= 0) return;
    float mn[3] = {pts[0], pts[1], pts[2]}, mx[3] = {pts[0], pts[1], pts[2]};
    for (int64_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) {
            const float v = pts[4 * i + a];
            if (v < mn[a]) mn[a] = v;
            if (v > mx[a]) mx[a] = v;
        }
    float ext = 0.f;
    for (int a = 0; a < 3; a++) ext = std::max(ext, mx[a] - mn[a]);
    const float scale = (ext > 0.f && std::isfinite(ext)) ? 1023.0f / ext : 0.f;
    std::vector<uint32_t> key((size_t)n), key2((size_t)n);
    std::vector<int32_t> idx2((size_t)n);
    const int64_t nch = (n + kHostChunk - 1) / kHostChunk;
    auto keys_body = [&](int64_t ch) {
        const int64_t lo = ch * kHostChunk, hi = std::min(n, lo + kHostChunk);
        for (int64_t i = lo; i < hi; i++) {
            uint32_t q[3];
            for (int a = 0; a < 3; a++) {
                float u = (pts[4 * i + a] - mn[a]) * scale;
                if (!(u >= 0.f)) u = 0.f;
                if (u > 1023.f) u = 1023.f;
                q[a] = (uint32_t)u;
            }
            key[i] = spread10(q[0]) | (spread10(q[1]) << 1) | (spread10(q[2]) << 2);
            order[i] = (int32_t)i;
        }
    };
    if (par) parallel_for(nch, 1, keys_body);
    else for (int64_t ch = 0; ch < nch; ch++) keys_body(ch);
    // stable LSD radix sort, 3 passes of 10 bits: ties keep the original index order
    uint32_t *ka = key.data(), *kb = key2.data();
    int32_t *ia = order.data(), *ib = idx2.data();
    for (int pass = 0; pass < 3; pass++) {
        const int sh = 10 * pass;
        uint32_t hist[1025];
        std::memset(hist, 0, sizeof(hist));
        for (int64_t i = 0; i < n; i++) hist[((ka[i] >> sh) & 1023u) + 1]++;
        for (int b = 0; b < 1024; b++) hist[b + 1] += hist[b];
        for (int64_t i = 0; i < n; i++) {
            const uint32_t d = (ka[i] >> sh) & 1023u;
            const uint32_t pos = hist[d]++;
            kb[pos] = ka[i];
            ib[pos] = ia[i];
        }
        std::swap(ka, kb);
        std::swap(ia, ib);
    }
    if (ia != order.data()) std::memcpy(order.data(), ia, (size_t)n * sizeof(int32_t));
    std::vector<float> out((size_t)n * 4);
    auto gather = [&](int64_t ch) {
        const int64_t lo = ch * kHostChunk, hi = std::min(n, lo + kHostChunk);
        for (int64_t pos = lo; pos < hi; pos++)
            std::memcpy(&out[4 * pos], &pts[4 * (size_t)order[pos]], 4 * sizeof(float));
    };
    if (par) parallel_for(nch, 1, gather);
    else for (int64_t ch = 0; ch < nch; ch++) gather(ch);
    std::memcpy(pts, out.data(), out.size() * sizeof(float));
}

void morton_order(std::vector<float> &pts, int64_t n, std::vector<int32_t> &order)
{
    morton_order_ptr(pts.data(), n, order, false);
}

}  // namespace

// ---- what the yaw sweeps and the per-source outputs share ------------------------------------------------------------
// start i of `level` yaw starts (src/annotation.cpp:35-39): the rotation by i * 2 pi / level about the y axis
static Mat4 yaw_start(int i, int level)
{
    const double interval = 2.0 * M_PI / (double)level;
    const double a = interval * i, c = std::cos(a), s = std::sin(a);
    Mat4 init = Mat4::identity();
    init(0, 0) = c; init(0, 2) = s; init(2, 0) = -s; init(2, 2) = c;
    return init;
}

struct NoInfo {};
// src/annotation.cpp:35-61, one start after the other: run_one(init, &result, &info) per start, the start with the most
// correspondences wins (strict >: the first of equals)
template <class Info, class RunOne>
static int sweep_sequential(int level, RunOne run_one, visma_icp_result *best, int *best_level, visma_icp_result *per_level,
                            Info *best_info = nullptr, Info *per_level_info = nullptr)
{
    visma_icp_result b;
    Info bi;
    std::memset(&b, 0, sizeof(b));
    std::memset(&bi, 0, sizeof(bi));
    const Mat4 I = Mat4::identity();
    std::memcpy(b.transformation, I.m, sizeof(I.m));
    int bl = -1;
    for (int i = 0; i < level; i++) {
        visma_icp_result r;
        Info ri;
        int rc = run_one(yaw_start(i, level), &r, &ri);
        if (rc) return rc;
        if (per_level) per_level[i] = r;
        if (per_level_info) per_level_info[i] = ri;
        if (r.num_correspondences > b.num_correspondences) { b = r; bi = ri; bl = i; }   // strict >
    }
    *best = b;
    if (best_info) *best_info = bi;
    if (best_level) *best_level = bl;
    return VISMA_ICP_OK;
}

// a value per engine position -> per caller's source index
template <class T>
static void scatter_by_order(const visma_icp_ctx *ctx, const std::vector<T> &by_pos, T *per_src)
{
    const int32_t *order = ctx->order_ptr();
    const int64_t ns = ctx->eng->ns();
    for (int64_t pos = 0; pos < ns; pos++) per_src[order ? order[pos] : pos] = by_pos[(size_t)pos];
}

extern "C" {

const char *visma_icp_version(void) { return "visma-icp-mi355x 0.1 (gfx950)"; }

int visma_icp_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

int visma_icp_create(visma_icp_ctx **out, int device)
{
    if (!out) { g_create_error = "out is NULL"; return VISMA_ICP_ERR_INVALID; }
    *out = nullptr;
    int rc = VISMA_ICP_OK;
    std::string emsg;
    std::unique_ptr<Engine> e(new_hip_engine(device, &rc, &emsg));
    if (!e) { g_create_error = emsg; return rc ? rc : VISMA_ICP_ERR_NO_DEVICE; }
    visma_icp_ctx *c = new visma_icp_ctx();
    c->eng = std::move(e);
    if (const char *p = std::getenv("VISMA_ICP_SEARCH_PRECISION")) {     // initial value of the option
        const int v = std::atoi(p);
        if (v >= 0 && v <= 2) c->search_precision = v;
    }
    c->eng->set_exact(c->search_precision == 1);
    *out = c;
    return VISMA_ICP_OK;
}

#ifdef VISMA_TEST_SEAMS
int visma_icp_create_with_engine(visma_icp_ctx **out, const visma_icp_engine *engine, void *user)
{
    if (!out || !engine || !engine->set_source || !engine->set_target || !engine->nn_pass ||
        !engine->reduce || !engine->get_correspondences) {
        g_create_error = "incomplete engine table";
        return VISMA_ICP_ERR_INVALID;
    }
    visma_icp_ctx *c = new visma_icp_ctx();
    c->eng.reset(new HookEngine(*engine, user));
    *out = c;
    return VISMA_ICP_OK;
}
#endif  // VISMA_TEST_SEAMS

int visma_icp_destroy(visma_icp_ctx *ctx)
{
    delete ctx;
    return VISMA_ICP_OK;
}

const char *visma_icp_last_error(const visma_icp_ctx *ctx)
{
    return ctx ? ctx->err.c_str() : g_create_error.c_str();
}


struct MeshSourceSpec {                  // the source comes from meshes sampled on the device (src == NULL then)
    const Engine::MeshSource *meshes;
    int n;
    int quirks;
    unsigned long long seed;
    int64_t *ns_out;
};

static int set_clouds_f64_impl(visma_icp_ctx *ctx, const double *src, int64_t ns, int sstride, const double *tgt,
                               int64_t nt, int tstride, double voxel, int64_t *nt_out, const MeshSourceSpec *ms = nullptr);

int visma_icp_set_clouds_f64(visma_icp_ctx *ctx, const double *src, int64_t ns, int sstride,
                             const double *tgt, int64_t nt, int tstride)
{
    return set_clouds_f64_impl(ctx, src, ns, sstride, tgt, nt, tstride, 0.0, nullptr);
}

int visma_icp_set_clouds_f64_voxel_target(visma_icp_ctx *ctx, const double *src, int64_t ns, int sstride,
                                          const double *scene, int64_t n_scene, int tstride, double voxel_size,
                                          int64_t *nt_out)
{
    if (ctx && (!nt_out || !(voxel_size > 0.0))) return ctx->fail(VISMA_ICP_ERR_INVALID, "voxel_size must be positive, nt_out not NULL");
    return set_clouds_f64_impl(ctx, src, ns, sstride, scene, n_scene, tstride, voxel_size, nt_out);
}

int visma_icp_set_clouds_meshes_f64(visma_icp_ctx *ctx, const visma_icp_mesh_source *meshes, int n_meshes,
                                    int reference_quirks, uint64_t seed, const double *scene_xyz, int64_t n_scene,
                                    int scene_stride, double voxel_size, int64_t *ns_out, int64_t *nt_out)
{
    CTX_CHECK();
    if (n_meshes < 0 || (n_meshes > 0 && !meshes) || !ns_out || !nt_out || !(voxel_size >= 0.0))
        return ctx->fail(VISMA_ICP_ERR_INVALID, "bad mesh-source arguments");
    *ns_out = 0;
    *nt_out = 0;
    std::vector<Engine::MeshSource> ms((size_t)n_meshes);
    for (int k = 0; k < n_meshes; k++) {
        ms[(size_t)k].V = meshes[k].V; ms[(size_t)k].nv = meshes[k].nv;
        ms[(size_t)k].F = meshes[k].F; ms[(size_t)k].nf = meshes[k].nf;
        ms[(size_t)k].samples = meshes[k].samples;
        ms[(size_t)k].has_transform = meshes[k].model_to_scene != nullptr;
        if (meshes[k].model_to_scene) std::memcpy(ms[(size_t)k].T, meshes[k].model_to_scene, sizeof(double) * 16);
    }
    MeshSourceSpec spec{ms.data(), n_meshes, reference_quirks, (unsigned long long)seed, ns_out};
    int64_t nt = n_scene;
    int rc = set_clouds_f64_impl(ctx, nullptr, 0, 3, scene_xyz, n_scene, scene_stride, voxel_size, &nt, &spec);
    if (rc) return rc;
    *nt_out = voxel_size > 0.0 ? nt : n_scene;
    return VISMA_ICP_OK;
}

int visma_icp_set_radius_hint(visma_icp_ctx *ctx, double max_correspondence_distance)
{
    CTX_CHECK();
    if (!(max_correspondence_distance >= 0.0)) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad radius");
    ctx->radius_hint = max_correspondence_distance;
    return VISMA_ICP_OK;
}

int visma_icp_get_mesh_source(visma_icp_ctx *ctx, double *xyz_out, int64_t ns)
{
    CTX_CHECK();
    if (ns < 0 || (ns > 0 && !xyz_out)) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad arguments");
    int rc = ctx->eng->get_mesh_source(xyz_out, ns);
    if (rc) return ctx->eng_fail(rc);
    return VISMA_ICP_OK;
}

int visma_icp_get_voxel_target(visma_icp_ctx *ctx, double *xyz_out, int64_t nt)
{
    CTX_CHECK();
    if (nt < 0 || (nt > 0 && !xyz_out)) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad arguments");
    int rc = ctx->eng->get_voxel_target(xyz_out, nt);
    if (rc) return ctx->eng_fail(rc);
    return VISMA_ICP_OK;
}

// voxel > 0: the target is VoxelDownSample(tgt, voxel), made and installed on the device (*nt_out = its size)
static int set_clouds_f64_impl(visma_icp_ctx *ctx, const double *src, int64_t ns, int sstride, const double *tgt,
                               int64_t nt, int tstride, double voxel, int64_t *nt_out, const MeshSourceSpec *ms)
{
    CTX_CHECK();
    if (ns < 0 || nt < 0 || sstride < 3 || tstride < 3 || (ns > 0 && !src) || (nt > 0 && !tgt))
        return ctx->fail(VISMA_ICP_ERR_INVALID, "bad cloud arguments");
    // centre on the target centroid: sequential f64 sum in index order
    // centre on the target centroid (fixed chunked f64 sum: thread-count independent)
    auto t_now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    static const bool trace = std::getenv("VISMA_ICP_UPLOAD_TRACE") != nullptr;
    double tm[8]; int ti = 0; tm[ti++] = t_now();
    double c[3] = {0, 0, 0};
    // (the HIP engine sums the centroid while it stages the target: one pass over the caller's memory instead
    //  of two; engines without a raw upload get it from centroid_f64 -- the same chunk sums, the same value)
    if (ctx->fixed_centre) std::memcpy(c, ctx->centre, sizeof(c));
    tm[ti++] = t_now();   // (centroid: inside the target upload)
    const bool want64 = ctx->search_precision != 0;     // (target-sharded ranks too: they compare shards in f64)
    // the target goes up as the caller's f64 values and is expanded on the device (HIP engine); otherwise it
    // is packed on a few host threads straight into the engine's (pinned) staging memory
    static const int64_t raw_min = []() {                 // VISMA_ICP_RAW_UPLOAD_MIN: smallest target sent up raw
        const char *e = std::getenv("VISMA_ICP_RAW_UPLOAD_MIN");
        return e ? (int64_t)std::atoll(e) : (int64_t)0;
    }();
    int rc;
    if (voxel > 0.0) {
        rc = ctx->eng->set_target_voxel_f64(tgt, nt, tstride, voxel, c, !ctx->fixed_centre, want64 && ctx->eng->supports_device_loop(), nt_out);
        if (rc == VISMA_ICP_ERR_STATE) return ctx->fail(VISMA_ICP_ERR_STATE, "the voxel-grid target needs the HIP engine");
        if (rc) return ctx->eng_fail(rc);
        nt = *nt_out;                                            // (what follows only needs the count)
    } else {
        rc = nt >= raw_min ? ctx->eng->set_target_f64(tgt, nt, tstride, c, !ctx->fixed_centre, want64 && ctx->eng->supports_device_loop())
                           : (int)VISMA_ICP_ERR_STATE;
    }
    const bool raw_target = rc == VISMA_ICP_OK;
    if (!raw_target) {
        if (rc != VISMA_ICP_ERR_STATE) return ctx->eng_fail(rc);
        if (!ctx->fixed_centre) centroid_f64(tgt, nt, tstride, c, true);
        float *tb = ctx->eng->staging(0, (size_t)std::max<int64_t>(nt, 1) * 4);
        pack_f64_to(tgt, nt, tstride, c, tb, true);
        rc = ctx->eng->set_target(tb, nt);
        if (rc) return ctx->eng_fail(rc);
    }
    tm[ti++] = t_now();   // target
    // the source too goes up raw and is Morton-ordered on the device (HIP engine with a raw target)
    bool raw_source = false;
    if (ms) {
        if (!raw_target) return ctx->fail(VISMA_ICP_ERR_STATE, "a mesh-sampled source needs the HIP engine");
        rc = ctx->eng->set_source_meshes_f64(ms->meshes, ms->n, ms->quirks, ms->seed, c, want64 && ctx->eng->supports_device_loop(),
                                             ctx->src_order, ms->ns_out);
        ctx->src_order_gen++;
        if (rc == VISMA_ICP_ERR_STATE) return ctx->fail(VISMA_ICP_ERR_STATE, "a mesh-sampled source needs the HIP engine");
        if (rc) return ctx->eng_fail(rc);
        raw_source = true;
        ns = *ms->ns_out;
    } else if (raw_target) {
        // the radius of the coming registration, if known (visma_icp_set_radius_hint, or the last one used): the grid
        // is built on the stream while the source is staged
        // (the hint speaks about the NEXT registration only: consumed here, so that a context that once got one and is
        //  later driven with another radius falls back to its previous radius instead of building a wasted grid per upload)
        const double hint = ctx->radius_hint > 0.0 ? ctx->radius_hint : ctx->last_radius;
        ctx->radius_hint = 0.0;
        if (hint > 0.0 && ctx->search_precision == 1) {
            ctx->eng->set_exact(true);
            rc = ctx->eng->prepare_search(ns, want64 && ctx->eng->supports_device_loop(), hint);
            if (rc) return ctx->eng_fail(rc);
        }
        rc = ctx->eng->set_source_f64(src, ns, sstride, c, want64 && ctx->eng->supports_device_loop(), ctx->src_order);
        ctx->src_order_gen++;
        raw_source = rc == VISMA_ICP_OK;
        if (!raw_source && rc != VISMA_ICP_ERR_STATE) return ctx->eng_fail(rc);
    }
    float *sb = nullptr;
    if (!raw_source) {
        sb = ctx->eng->staging(1, (size_t)std::max<int64_t>(ns, 1) * 4);
        pack_f64_to(src, ns, sstride, c, sb, true);
    }
    tm[ti++] = t_now();   // source pack
    if (!raw_source) { morton_order_ptr(sb, ns, ctx->src_order, true); ctx->src_order_gen++; }
    tm[ti++] = t_now();   // morton
    if (!raw_source) {
        rc = ctx->eng->set_source(sb, ns);
        if (rc) return ctx->eng_fail(rc);
    }
    // double-precision search: the caller's own f64 coordinates (centred in f64) go along
    // (the size-keyed policy of round 1 is gone: the exact search costs the same as the fp32 one)
    ctx->eng->set_exact(ctx->search_precision == 1);
    if (raw_source) {
        if (!(want64 && ctx->eng->supports_device_loop())) {
            rc = ctx->eng->set_clouds64(nullptr, nullptr);
            if (rc) return ctx->eng_fail(rc);
        }
    } else if (want64 && ctx->eng->supports_device_loop()) {
        // (Pt64 = 8 floats of staging; pinned on the HIP engine)
        Pt64 *t8 = raw_target ? nullptr : reinterpret_cast<Pt64 *>(ctx->eng->staging(2, (size_t)std::max<int64_t>(nt, 1) * 8));
        Pt64 *s8 = reinterpret_cast<Pt64 *>(ctx->eng->staging(3, (size_t)std::max<int64_t>(ns, 1) * 8));
        if (!raw_target) parallel_for((nt + kHostChunk - 1) / kHostChunk, 1, [&](int64_t ch) {
            const int64_t lo = ch * kHostChunk, hi = std::min(nt, lo + kHostChunk);
            for (int64_t j = lo; j < hi; j++) {
                const double *q = tgt + (size_t)j * tstride;
                t8[(size_t)j] = Pt64{q[0] - c[0], q[1] - c[1], q[2] - c[2], (unsigned long long)j};
            }
        });
        parallel_for((ns + kHostChunk - 1) / kHostChunk, 1, [&](int64_t ch) {
            const int64_t lo = ch * kHostChunk, hi = std::min(ns, lo + kHostChunk);
            for (int64_t pos = lo; pos < hi; pos++) {
                const double *q = src + (size_t)ctx->src_order[(size_t)pos] * sstride;    // Morton order, like sb
                s8[(size_t)pos] = Pt64{q[0] - c[0], q[1] - c[1], q[2] - c[2], (unsigned long long)ctx->src_order[(size_t)pos]};
            }
        });
        rc = raw_target ? ctx->eng->set_source64(s8) : ctx->eng->set_clouds64(s8, t8);
        if (rc) return ctx->eng_fail(rc);
    } else if (ctx->eng->supports_device_loop()) {
        rc = ctx->eng->set_clouds64(nullptr, nullptr);
        if (rc) return ctx->eng_fail(rc);
    }
    tm[ti++] = t_now();   // source upload + f64
    if (trace) std::fprintf(stderr, "upload trace: centroid %.2f target %.2f src-pack %.2f morton %.2f src-upload+f64 %.2f ms\n",
                            tm[1] - tm[0], tm[2] - tm[1], tm[3] - tm[2], tm[4] - tm[3], tm[5] - tm[4]);
    std::memcpy(ctx->centre, c, sizeof(c));
    ctx->have_src = ctx->have_tgt = true;
    ctx->centred_upload = true;
    return VISMA_ICP_OK;
}

int visma_icp_set_target(visma_icp_ctx *ctx, const float *xyz, int64_t nt, int stride)
{
    CTX_CHECK();
    ctx->eng->set_exact(ctx->search_precision == 1);     // (the search precision applies from an upload on)
    if (nt < 0 || stride < 3 || (nt > 0 && !xyz)) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad target arguments");
    float *buf = ctx->eng->staging(0, (size_t)std::max<int64_t>(nt, 1) * 4);
    pack_f32_to(xyz, nt, stride, buf);
    int rc = ctx->eng->set_target(buf, nt);
    if (rc) return ctx->eng_fail(rc);
    ctx->enter_uncentred_frame(false);
    ctx->have_tgt = true;
    return VISMA_ICP_OK;
}

int visma_icp_set_source(visma_icp_ctx *ctx, const float *xyz, int64_t ns, int stride)
{
    CTX_CHECK();
    ctx->eng->set_exact(ctx->search_precision == 1);     // (the search precision applies from an upload on)
    if (ns < 0 || stride < 3 || (ns > 0 && !xyz)) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad source arguments");
    float *buf = ctx->eng->staging(1, (size_t)std::max<int64_t>(ns, 1) * 4);
    pack_f32_to(xyz, ns, stride, buf);
    morton_order_ptr(buf, ns, ctx->src_order, true);
    ctx->src_order_gen++;
    int rc = ctx->eng->set_source(buf, ns);
    if (rc) return ctx->eng_fail(rc);
    ctx->enter_uncentred_frame(true);
    ctx->have_src = true;
    return VISMA_ICP_OK;
}

int visma_icp_set_target_device(visma_icp_ctx *ctx, const void *d, int64_t nt)
{
    CTX_CHECK();
    ctx->eng->set_exact(ctx->search_precision == 1);     // (the search precision applies from an upload on)
    if (nt < 0 || (nt > 0 && !d)) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad target arguments");
    int rc = ctx->eng->set_target_device(d, nt);
    if (rc) return ctx->eng_fail(rc);
    ctx->enter_uncentred_frame(false);
    ctx->have_tgt = true;
    return VISMA_ICP_OK;
}

int visma_icp_set_source_device(visma_icp_ctx *ctx, const void *d, int64_t ns)
{
    CTX_CHECK();
    ctx->eng->set_exact(ctx->search_precision == 1);     // (the search precision applies from an upload on)
    if (ns < 0 || (ns > 0 && !d)) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad source arguments");
    int rc = ctx->eng->set_source_device(d, ns);
    if (rc) return ctx->eng_fail(rc);
    ctx->src_order.clear();   // device-resident source is used in the caller's order
    ctx->src_order_gen++;
    ctx->enter_uncentred_frame(true);
    ctx->have_src = true;
    return VISMA_ICP_OK;
}

int visma_icp_set_target_normals_f64(visma_icp_ctx *ctx, const double *n, int64_t nt, int stride)
{
    CTX_CHECK();
    if (!ctx->have_tgt) return ctx->fail(VISMA_ICP_ERR_STATE, "set the target first");
    if (nt != ctx->eng->nt() || stride < 3 || (nt > 0 && !n))
        return ctx->fail(VISMA_ICP_ERR_INVALID, "bad normals arguments");
    const double zero[3] = {0, 0, 0};
    float *buf = ctx->eng->staging(0, (size_t)std::max<int64_t>(nt, 1) * 4);
    pack_f64_to(n, nt, stride, zero, buf, true);
    int rc = ctx->eng->set_target_normals(buf, nt);
    if (rc) return ctx->eng_fail(rc);
    if (ctx->eng->supports_device_loop()) {                 // the f64 search takes the normals in f64 as well
        std::vector<Pt64> n8((size_t)std::max<int64_t>(nt, 1));
        for (int64_t j = 0; j < nt; j++)
            n8[(size_t)j] = Pt64{n[(size_t)j * stride], n[(size_t)j * stride + 1], n[(size_t)j * stride + 2], 0ull};
        rc = ctx->eng->set_target_normals64(n8.data());
        if (rc) return ctx->eng_fail(rc);
    }
    return VISMA_ICP_OK;
}

int visma_icp_nn_pass(visma_icp_ctx *ctx, const double T[16], double max_dist)
{
    CTX_CHECK();
    if (!T) return ctx->fail(VISMA_ICP_ERR_INVALID, "T is NULL");
    if (!ctx->have_src || !ctx->have_tgt) return ctx->fail(VISMA_ICP_ERR_STATE, "clouds not set");
    if (!(max_dist > 0.0)) return ctx->fail(VISMA_ICP_ERR_INVALID, "max_dist must be > 0");
    ctx->last_Tc = to_centred(Mat4::from(T), ctx->centre);
    int rc = ctx->eng->nn_pass(ctx->last_Tc, max_dist);
    if (rc) return ctx->eng_fail(rc);
    return VISMA_ICP_OK;
}

int visma_icp_reduce(visma_icp_ctx *ctx, double out_stats[VISMA_ICP_NSTATS])
{
    CTX_CHECK();
    if (!out_stats) return ctx->fail(VISMA_ICP_ERR_INVALID, "out_stats is NULL");
    const double zero[3] = {0, 0, 0};
    int rc = ctx->eng->reduce(ctx->last_Tc, false, zero, out_stats);
    if (rc) return ctx->eng_fail(rc);
    if (ctx->host_allreduce && !ctx->eng->has_device_allreduce())
        if (ctx->host_allreduce(ctx->host_allreduce_user, out_stats, VISMA_ICP_NSTATS) != 0)
            return ctx->fail(VISMA_ICP_ERR_ENGINE, "host all-reduce callback failed");
    return VISMA_ICP_OK;
}

int visma_icp_get_correspondences(visma_icp_ctx *ctx, int32_t *src_idx, int32_t *tgt_idx, float *d2,
                                  int64_t *k)
{
    CTX_CHECK();
    if (!src_idx || !tgt_idx || !k) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output buffer");
    const int64_t ns = ctx->eng->ns();
    std::vector<int32_t> idx((size_t)(ns > 0 ? ns : 1));
    std::vector<float> dd((size_t)(ns > 0 ? ns : 1));
    int rc = ctx->eng->get_correspondences(idx.data(), dd.data());
    if (rc) return ctx->eng_fail(rc);
    if ((int64_t)ctx->src_order.size() == ns && ns > 0) {
        // the engine holds the source in Morton order: back to the caller's order
        std::vector<int32_t> idx2((size_t)ns);
        std::vector<float> dd2((size_t)ns);
        for (int64_t pos = 0; pos < ns; pos++) {
            idx2[ctx->src_order[pos]] = idx[pos];
            dd2[ctx->src_order[pos]] = dd[pos];
        }
        idx.swap(idx2);
        dd.swap(dd2);
    }
    int64_t c = 0;
    for (int64_t i = 0; i < ns; i++)
        if (idx[i] >= 0) {
            src_idx[c] = (int32_t)i;
            tgt_idx[c] = idx[i];
            if (d2) d2[c] = dd[i];
            ++c;
        }
    *k = c;
    return VISMA_ICP_OK;
}

int visma_icp_solve_from_stats(const double stats[VISMA_ICP_NSTATS], int solver, int with_scaling,
                               double T_update[16])
{
    if (!stats || !T_update) return VISMA_ICP_ERR_INVALID;
    Mat4 T;
    bool ok = true;
    switch (solver) {
    case VISMA_ICP_SOLVER_KABSCH: T = kabsch_from_stats(stats, with_scaling != 0); break;
    case VISMA_ICP_SOLVER_GN_EULER: T = gn_from_stats(stats, false, &ok); break;
    case VISMA_ICP_SOLVER_GN_EXPMAP: T = gn_from_stats(stats, true, &ok); break;
    default: return VISMA_ICP_ERR_INVALID;
    }
    std::memcpy(T_update, T.m, sizeof(T.m));
    return VISMA_ICP_OK;
}

int visma_icp_solve_from_stats_axis(const double stats[VISMA_ICP_NSTATS], int plane, const double axis[3],
                                    double T_update[16])
{
    double a[3];
    if (!stats || !axis || !T_update || !normalise_axis(axis, a)) return VISMA_ICP_ERR_INVALID;
    bool ok = true;
    const Mat4 T = plane ? gn_axis_from_stats(stats, a, &ok) : kabsch_axis_from_stats(stats, a);
    std::memcpy(T_update, T.m, sizeof(T.m));
    return VISMA_ICP_OK;
}

int visma_icp_set_rotation_axis(visma_icp_ctx *ctx, const double axis[3])
{
    CTX_CHECK();
    if (!axis) {
        ctx->use_axis = false;
        ctx->axis[0] = ctx->axis[1] = ctx->axis[2] = 0.0;
        return VISMA_ICP_OK;
    }
    double a[3];
    if (!normalise_axis(axis, a)) return ctx->fail(VISMA_ICP_ERR_INVALID, "rotation axis is zero, near zero or not finite");
    if (ctx->sharded()) return ctx->fail(VISMA_ICP_ERR_INVALID, "sharded ranks take no rotation axis");
    ctx->use_axis = true;
    std::memcpy(ctx->axis, a, sizeof(a));
    return VISMA_ICP_OK;
}

int visma_icp_get_rotation_axis(const visma_icp_ctx *ctx, double axis_out[3], int *enabled)
{
    if (!ctx) { g_create_error = "ctx is NULL"; return VISMA_ICP_ERR_INVALID; }
    if (!axis_out && !enabled) return VISMA_ICP_ERR_INVALID;
    if (axis_out) std::memcpy(axis_out, ctx->axis, sizeof(ctx->axis));
    if (enabled) *enabled = ctx->use_axis ? 1 : 0;
    return VISMA_ICP_OK;
}

int visma_icp_run(visma_icp_ctx *ctx, const double init[16], double max_dist, int max_iter,
                  double rel_fitness, double rel_rmse, int solver, int with_scaling,
                  visma_icp_result *out)
{
    CTX_CHECK();
    if (!init || !out || max_iter < 0) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad run arguments");
    if (solver < 0 || solver > VISMA_ICP_SOLVER_GN_EXPMAP) return ctx->fail(VISMA_ICP_ERR_INVALID, "unknown solver");
    if (int rc = ctx->check_axis_solver(solver, with_scaling != 0)) return rc;
    return ctx->run(init, max_dist, max_iter, rel_fitness, rel_rmse, solver, with_scaling != 0, false, out);
}

// ---- trimmed ICP ----------------------------------------------------------------------------------------------------
static int check_trimmed(visma_icp_ctx *ctx, double keep)
{
    if (!(keep > 0.0) || !(keep <= 1.0) || !std::isfinite(keep)) return ctx->fail(VISMA_ICP_ERR_INVALID, "keep must lie in (0, 1]");
    if (ctx->sharded() || ctx->eng->is_sharded())
        return ctx->fail(VISMA_ICP_ERR_INVALID, "trimmed ICP runs on one rank: an order statistic across ranks is not available");
    if (!ctx->have_src || !ctx->have_tgt) return ctx->fail(VISMA_ICP_ERR_STATE, "clouds not set");
    return VISMA_ICP_OK;
}

int visma_icp_reduce_trimmed(visma_icp_ctx *ctx, double keep, double out_stats[VISMA_ICP_NSTATS], visma_icp_trim_info *info)
{
    CTX_CHECK();
    if (!out_stats || !info) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    if (int rc = check_trimmed(ctx, keep)) return rc;
    Engine::TrimPass tr;
    int rc = ctx->eng->reduce_trimmed(ctx->last_Tc, nullptr, keep, ctx->order_ptr(), ctx->src_order_gen, out_stats, &tr);
    if (rc) return ctx->eng_fail(rc);
    ctx->trim_state = 1;
    visma_icp_ctx::fill_trim_info(info, out_stats, tr);
    return VISMA_ICP_OK;
}

int visma_icp_run_trimmed(visma_icp_ctx *ctx, const double init[16], double max_dist, double keep, int max_iter,
                          double rel_fitness, double rel_rmse, int solver, int with_scaling, visma_icp_result *out,
                          visma_icp_trim_info *info)
{
    CTX_CHECK();
    if (!init || !out || max_iter < 0) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad run arguments");
    if (solver != VISMA_ICP_SOLVER_KABSCH) return ctx->fail(VISMA_ICP_ERR_INVALID, "trimmed ICP: the closed-form solver only");
    if (int rc = ctx->check_axis_solver(solver, with_scaling != 0)) return rc;
    if (int rc = check_trimmed(ctx, keep)) return rc;
    if (keep == 1.0) {
        // every pair is kept: the plain run, bit for bit
        int rc = ctx->run(init, max_dist, max_iter, rel_fitness, rel_rmse, solver, with_scaling != 0, false, out);
        if (rc) return rc;
        ctx->trim_state = max_dist > 0.0 ? 2 : 0;
        if (info) {
            std::memset(info, 0, sizeof(*info));
            info->kept = out->num_correspondences;
            info->trimmed_rmse = out->inlier_rmse;
            if (max_dist > 0.0 && out->num_correspondences > 0) {
                const int64_t ns = ctx->eng->ns();
                std::vector<int32_t> idx((size_t)std::max<int64_t>(ns, 1));
                std::vector<float> dd((size_t)std::max<int64_t>(ns, 1));
                rc = ctx->eng->get_correspondences(idx.data(), dd.data());
                if (rc) return ctx->eng_fail(rc);
                float mx = 0.f;
                for (int64_t i = 0; i < ns; i++)
                    if (idx[(size_t)i] >= 0) mx = std::max(mx, dd[(size_t)i]);
                info->d2_cut = (double)mx;
            }
        }
        return VISMA_ICP_OK;
    }
    if (info) std::memset(info, 0, sizeof(*info));
    Engine::TrimPass tr;
    return ctx->run_pair_passes(
        init, max_dist, false, max_iter, rel_fitness, rel_rmse, with_scaling != 0, out, &ctx->trim_state, tr,
        [&](const Mat4 &Tc, double *stats) { return ctx->eng->reduce_trimmed(Tc, nullptr, keep, ctx->order_ptr(), ctx->src_order_gen, stats, &tr); },
        [&](const double *stats) { if (info) visma_icp_ctx::fill_trim_info(info, stats, tr); });
}

int visma_icp_run_yaw_sweep_trimmed(visma_icp_ctx *ctx, int level, double max_dist, double keep, int max_iter,
                                    double rel_fitness, double rel_rmse, int solver, visma_icp_result *best, int *best_level,
                                    visma_icp_result *per_level, visma_icp_trim_info *best_info,
                                    visma_icp_trim_info *per_level_info)
{
    CTX_CHECK();
    if (level <= 0 || !best || max_iter < 0) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad sweep arguments");
    if (solver != VISMA_ICP_SOLVER_KABSCH) return ctx->fail(VISMA_ICP_ERR_INVALID, "trimmed ICP: the closed-form solver only");
    if (int rc = ctx->check_axis_solver(solver, false)) return rc;
    if (int rc = check_trimmed(ctx, keep)) return rc;
    return sweep_sequential(level, [&](const Mat4 &init, visma_icp_result *r, visma_icp_trim_info *ri) {
        return visma_icp_run_trimmed(ctx, init.m, max_dist, keep, max_iter, rel_fitness, rel_rmse, solver, 0, r, ri);
    }, best, best_level, per_level, best_info, per_level_info);
}

int visma_icp_get_kept_mask(visma_icp_ctx *ctx, uint8_t *kept_per_src)
{
    CTX_CHECK();
    if (!kept_per_src) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output buffer");
    if (ctx->trim_state == 0) return ctx->fail(VISMA_ICP_ERR_STATE, "no trimmed pass yet");
    const int64_t ns = ctx->eng->ns();
    std::vector<uint8_t> mask((size_t)std::max<int64_t>(ns, 1));
    if (ctx->trim_state == 2) {
        std::vector<int32_t> idx((size_t)std::max<int64_t>(ns, 1));
        int rc = ctx->eng->get_correspondences(idx.data(), nullptr);
        if (rc) return ctx->eng_fail(rc);
        for (int64_t i = 0; i < ns; i++) mask[(size_t)i] = idx[(size_t)i] >= 0 ? 1 : 0;
    } else {
        int rc = ctx->eng->get_kept_mask(mask.data());
        if (rc) return ctx->eng_fail(rc);
    }
    scatter_by_order(ctx, mask, kept_per_src);
    return VISMA_ICP_OK;
}

// ---- robust ICP -----------------------------------------------------------------------------------------------------
// the configuration as the engine takes it (tune resolved); everything that is wrong with it before any pass
static int check_robust(visma_icp_ctx *ctx, const visma_icp_robust *cfg, Engine::RobustConfig *rc_out)
{
    if (!cfg) return ctx->fail(VISMA_ICP_ERR_INVALID, "robust configuration is NULL");
    if (cfg->kernel < VISMA_ICP_ROBUST_L2 || cfg->kernel > VISMA_ICP_ROBUST_CAUCHY)
        return ctx->fail(VISMA_ICP_ERR_INVALID, "unknown robust kernel");
    if (!std::isfinite(cfg->scale) || cfg->scale < 0.0) return ctx->fail(VISMA_ICP_ERR_INVALID, "robust scale must be finite and >= 0");
    if (!std::isfinite(cfg->tune) || cfg->tune < 0.0) return ctx->fail(VISMA_ICP_ERR_INVALID, "robust tune must be finite and >= 0");
    if (!std::isfinite(cfg->min_scale) || cfg->min_scale < 0.0)
        return ctx->fail(VISMA_ICP_ERR_INVALID, "robust min_scale must be finite and >= 0");
    if (ctx->sharded() || ctx->eng->is_sharded())
        return ctx->fail(VISMA_ICP_ERR_INVALID, "robust ICP runs on one rank: a median across ranks is not available");
    if (!ctx->have_src || !ctx->have_tgt) return ctx->fail(VISMA_ICP_ERR_STATE, "clouds not set");
    rc_out->kernel = cfg->kernel;
    rc_out->scale = cfg->scale;
    rc_out->min_scale = cfg->min_scale;
    rc_out->tune = cfg->tune;
    if (cfg->tune == 0.0)   // the 95 %-efficiency constants (Holland & Welsch 1977)
        rc_out->tune = cfg->kernel == VISMA_ICP_ROBUST_HUBER ? 1.345 : cfg->kernel == VISMA_ICP_ROBUST_TUKEY ? 4.685 : 2.385;
    return VISMA_ICP_OK;
}

int visma_icp_reduce_robust(visma_icp_ctx *ctx, const visma_icp_robust *cfg, int plane, double out_stats[VISMA_ICP_NSTATS],
                            visma_icp_robust_info *info)
{
    CTX_CHECK();
    if (!out_stats || !info) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    Engine::RobustConfig rc_cfg;
    if (int rc = check_robust(ctx, cfg, &rc_cfg)) return rc;
    if (plane && !ctx->eng->has_normals()) return ctx->fail(VISMA_ICP_ERR_STATE, "point-to-plane needs target normals");
    if (rc_cfg.kernel == VISMA_ICP_ROBUST_L2) {
        // every weight is 1: the plain statistics
        const double zero[3] = {0, 0, 0};
        int rc = ctx->eng->reduce(ctx->last_Tc, plane != 0, plane ? ctx->centre : zero, out_stats);
        if (rc) return ctx->eng_fail(rc);
        ctx->robust_state = 2;
        std::memset(info, 0, sizeof(*info));
        info->weight_sum = out_stats[0];
        info->robust_rmse = visma_icp_ctx::trimmed_rmse(out_stats);
        return VISMA_ICP_OK;
    }
    Engine::RobustPass rp;
    int rc = ctx->eng->reduce_robust(ctx->last_Tc, plane ? ctx->centre : nullptr, plane != 0, rc_cfg, out_stats, &rp);
    if (rc) return ctx->eng_fail(rc);
    ctx->robust_state = 1;
    ctx->last_plane = plane != 0;
    visma_icp_ctx::fill_robust_info(info, out_stats, rp);
    return VISMA_ICP_OK;
}

int visma_icp_run_robust(visma_icp_ctx *ctx, const double init[16], double max_dist, const visma_icp_robust *cfg, int plane,
                         int max_iter, double rel_fitness, double rel_rmse, int with_scaling, visma_icp_result *out,
                         visma_icp_robust_info *info)
{
    CTX_CHECK();
    if (!init || !out || max_iter < 0) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad run arguments");
    Engine::RobustConfig rc_cfg;
    if (int rc = check_robust(ctx, cfg, &rc_cfg)) return rc;
    if (!plane) { if (int rc = ctx->check_axis_solver(VISMA_ICP_SOLVER_KABSCH, with_scaling != 0)) return rc; }
    if (rc_cfg.kernel == VISMA_ICP_ROBUST_L2) {
        // every weight is 1: the plain run, bit for bit
        int rc = plane ? ctx->run(init, max_dist, max_iter, rel_fitness, rel_rmse, VISMA_ICP_SOLVER_GN_EULER, false, true, out)
                       : ctx->run(init, max_dist, max_iter, rel_fitness, rel_rmse, VISMA_ICP_SOLVER_KABSCH, with_scaling != 0, false, out);
        if (rc) return rc;
        const bool ran = max_dist > 0.0 && !(plane && !ctx->eng->has_normals());
        ctx->robust_state = ran ? 2 : 0;
        if (info) {
            std::memset(info, 0, sizeof(*info));
            info->weight_sum = (double)out->num_correspondences;
            info->robust_rmse = out->inlier_rmse;
        }
        return VISMA_ICP_OK;
    }
    if (info) std::memset(info, 0, sizeof(*info));
    Engine::RobustPass rp;
    return ctx->run_pair_passes(
        init, max_dist, plane != 0, max_iter, rel_fitness, rel_rmse, with_scaling != 0, out, &ctx->robust_state, rp,
        [&](const Mat4 &Tc, double *stats) { return ctx->eng->reduce_robust(Tc, plane ? ctx->centre : nullptr, plane != 0, rc_cfg, stats, &rp); },
        [&](const double *stats) { if (info) visma_icp_ctx::fill_robust_info(info, stats, rp); });
}

int visma_icp_run_yaw_sweep_robust(visma_icp_ctx *ctx, int level, double max_dist, const visma_icp_robust *cfg, int plane,
                                   int max_iter, double rel_fitness, double rel_rmse, visma_icp_result *best, int *best_level,
                                   visma_icp_result *per_level, visma_icp_robust_info *best_info,
                                   visma_icp_robust_info *per_level_info)
{
    CTX_CHECK();
    if (level <= 0 || !best || max_iter < 0) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad sweep arguments");
    Engine::RobustConfig rc_cfg;
    if (int rc = check_robust(ctx, cfg, &rc_cfg)) return rc;
    return sweep_sequential(level, [&](const Mat4 &init, visma_icp_result *r, visma_icp_robust_info *ri) {
        return visma_icp_run_robust(ctx, init.m, max_dist, cfg, plane, max_iter, rel_fitness, rel_rmse, 0, r, ri);
    }, best, best_level, per_level, best_info, per_level_info);
}

int visma_icp_get_pair_weights(visma_icp_ctx *ctx, double *w_per_src)
{
    CTX_CHECK();
    if (!w_per_src) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output buffer");
    if (ctx->robust_state == 0) return ctx->fail(VISMA_ICP_ERR_STATE, "no robust pass yet");
    const int64_t ns = ctx->eng->ns();
    std::vector<double> w((size_t)std::max<int64_t>(ns, 1));
    if (ctx->robust_state == 2) {
        std::vector<int32_t> idx((size_t)std::max<int64_t>(ns, 1));
        int rc = ctx->eng->get_correspondences(idx.data(), nullptr);
        if (rc) return ctx->eng_fail(rc);
        for (int64_t i = 0; i < ns; i++) w[(size_t)i] = idx[(size_t)i] >= 0 ? 1.0 : 0.0;
    } else {
        int rc = ctx->eng->get_pair_weights(w.data());
        if (rc) return ctx->eng_fail(rc);
    }
    scatter_by_order(ctx, w, w_per_src);
    return VISMA_ICP_OK;
}

// ---- generalized ICP --------------------------------------------------------------------------------------------------
// everything that is wrong with a call before any pass
static int check_gicp(visma_icp_ctx *ctx, double epsilon)
{
    if (!std::isfinite(epsilon) || !(epsilon > 0.0) || epsilon > 1.0)
        return ctx->fail(VISMA_ICP_ERR_INVALID, "generalized ICP: epsilon must lie in (0, 1]");
    if (ctx->sharded() || ctx->eng->is_sharded()) return ctx->fail(VISMA_ICP_ERR_INVALID, "generalized ICP runs on one rank");
    if (!ctx->have_src || !ctx->have_tgt) return ctx->fail(VISMA_ICP_ERR_STATE, "clouds not set");
    return VISMA_ICP_OK;
}

int visma_icp_set_source_normals_f64(visma_icp_ctx *ctx, const double *n, int64_t ns, int stride)
{
    CTX_CHECK();
    if (!ctx->have_src) return ctx->fail(VISMA_ICP_ERR_STATE, "set the source first");
    if (ns != ctx->eng->ns() || stride < 3 || (ns > 0 && !n)) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad normals arguments");
    // by source POSITION: the engine holds the source in Morton order
    const int32_t *order = ctx->order_ptr();
    std::vector<float> n4((size_t)std::max<int64_t>(ns, 1) * 4);
    std::vector<Pt64> n8;
    if (ctx->eng->supports_device_loop()) n8.resize((size_t)std::max<int64_t>(ns, 1));
    for (int64_t pos = 0; pos < ns; pos++) {
        const double *q = n + (size_t)(order ? order[pos] : pos) * stride;
        float *f = &n4[(size_t)pos * 4];
        f[0] = (float)q[0]; f[1] = (float)q[1]; f[2] = (float)q[2]; f[3] = 0.f;
        if (!n8.empty()) n8[(size_t)pos] = Pt64{q[0], q[1], q[2], 0ull};
    }
    int rc = ctx->eng->set_source_normals(n4.data(), n8.empty() ? nullptr : n8.data(), ns);
    if (rc) return ctx->eng_fail(rc);
    return VISMA_ICP_OK;
}

int visma_icp_reduce_gicp(visma_icp_ctx *ctx, double epsilon, double out_stats[VISMA_ICP_NSTATS], visma_icp_gicp_info *info)
{
    CTX_CHECK();
    if (!out_stats || !info) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    if (int rc = check_gicp(ctx, epsilon)) return rc;
    if (!ctx->eng->has_normals() || !ctx->eng->has_source_normals())
        return ctx->fail(VISMA_ICP_ERR_STATE, "generalized ICP needs source and target normals");
    Engine::GicpPass gp;
    int rc = ctx->eng->reduce_gicp(ctx->last_Tc, ctx->centre, epsilon, out_stats, &gp);
    if (rc) return ctx->eng_fail(rc);
    ctx->last_plane = true;
    visma_icp_ctx::fill_gicp_info(info, gp);
    return VISMA_ICP_OK;
}

int visma_icp_run_gicp(visma_icp_ctx *ctx, const double init[16], double max_dist, double epsilon, int max_iter,
                       double rel_fitness, double rel_rmse, visma_icp_result *out, visma_icp_gicp_info *info)
{
    CTX_CHECK();
    if (!init || !out || max_iter < 0) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad run arguments");
    if (int rc = check_gicp(ctx, epsilon)) return rc;
    if (info) std::memset(info, 0, sizeof(*info));
    if (!ctx->eng->has_source_normals()) {                       // Registration.cpp:152-157, as without target normals
        std::memset(out, 0, sizeof(*out));
        std::memcpy(out->transformation, init, sizeof(double) * 16);
        if (max_dist > 0.0) ctx->last_radius = max_dist;
        return VISMA_ICP_OK;
    }
    Engine::GicpPass gp;
    return ctx->run_pair_passes(
        init, max_dist, true, max_iter, rel_fitness, rel_rmse, false, out, nullptr, gp,
        [&](const Mat4 &Tc, double *stats) { return ctx->eng->reduce_gicp(Tc, ctx->centre, epsilon, stats, &gp); },
        [&](const double *) { if (info) visma_icp_ctx::fill_gicp_info(info, gp); },
        [&](const double *) { return gp.found > 0 ? std::sqrt(gp.cost / (double)gp.found) : 0.0; });
}

int visma_icp_run_yaw_sweep_gicp(visma_icp_ctx *ctx, int level, double max_dist, double epsilon, int max_iter,
                                 double rel_fitness, double rel_rmse, visma_icp_result *best, int *best_level,
                                 visma_icp_result *per_level, visma_icp_gicp_info *best_info,
                                 visma_icp_gicp_info *per_level_info)
{
    CTX_CHECK();
    if (level <= 0 || !best || max_iter < 0) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad sweep arguments");
    if (int rc = check_gicp(ctx, epsilon)) return rc;
    return sweep_sequential(level, [&](const Mat4 &init, visma_icp_result *r, visma_icp_gicp_info *ri) {
        return visma_icp_run_gicp(ctx, init.m, max_dist, epsilon, max_iter, rel_fitness, rel_rmse, r, ri);
    }, best, best_level, per_level, best_info, per_level_info);
}

// ---- colored ICP ------------------------------------------------------------------------------------------------------
// ColoredICP.cpp:54-55: a lambda_geometric outside [0, 1] (or not finite) is replaced, not refused
static double colored_lambda(double lambda) { return (std::isfinite(lambda) && lambda >= 0.0 && lambda <= 1.0) ? lambda : 0.968; }

// everything that is wrong with a call before any pass
static int check_colored(visma_icp_ctx *ctx)
{
    if (ctx->sharded() || ctx->eng->is_sharded()) return ctx->fail(VISMA_ICP_ERR_INVALID, "colored ICP runs on one rank");
    if (!ctx->have_src || !ctx->have_tgt) return ctx->fail(VISMA_ICP_ERR_STATE, "clouds not set");
    return VISMA_ICP_OK;
}

int visma_icp_set_source_colors_f64(visma_icp_ctx *ctx, const double *rgb, int64_t ns, int stride)
{
    CTX_CHECK();
    if (!ctx->have_src) return ctx->fail(VISMA_ICP_ERR_STATE, "set the source first");
    if (ns != ctx->eng->ns() || stride < 3 || (ns > 0 && !rgb)) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad colours arguments");
    // by source POSITION: the engine holds the source in Morton order
    std::vector<double> inten((size_t)std::max<int64_t>(ns, 1));
    color_intensities(rgb, ns, stride, ctx->order_ptr(), inten.data());
    int rc = ctx->eng->set_source_intensity(inten.data(), ns);
    if (rc) return ctx->eng_fail(rc);
    return VISMA_ICP_OK;
}

int visma_icp_set_target_colors_f64(visma_icp_ctx *ctx, const double *rgb, int64_t nt, int stride)
{
    CTX_CHECK();
    if (!ctx->have_tgt) return ctx->fail(VISMA_ICP_ERR_STATE, "set the target first");
    if (nt != ctx->eng->nt() || stride < 3 || (nt > 0 && !rgb)) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad colours arguments");
    std::vector<double> inten((size_t)std::max<int64_t>(nt, 1));
    color_intensities(rgb, nt, stride, nullptr, inten.data());
    int rc = ctx->eng->set_target_intensity(inten.data(), nt);
    if (rc) return ctx->eng_fail(rc);
    return VISMA_ICP_OK;
}

int visma_icp_prepare_colored(visma_icp_ctx *ctx, double radius, int max_nn)
{
    CTX_CHECK();
    if (max_nn < 3 || max_nn > kNormalsMaxList) return ctx->fail(VISMA_ICP_ERR_INVALID, "prepare_colored: max_nn must lie in [3, 170]");
    if (std::isnan(radius)) return ctx->fail(VISMA_ICP_ERR_INVALID, "prepare_colored: radius is not a number");
    if (ctx->sharded() || ctx->eng->is_sharded()) return ctx->fail(VISMA_ICP_ERR_INVALID, "colored ICP runs on one rank");
    if (!ctx->have_tgt) return ctx->fail(VISMA_ICP_ERR_STATE, "target not set");       // (the source is not looked at)
    if (!ctx->eng->has_normals() || !ctx->eng->has_target_colors())
        return ctx->fail(VISMA_ICP_ERR_STATE, "colored ICP needs target normals and target colours");
    int rc = ctx->eng->prepare_colored(radius, max_nn);
    if (rc) return ctx->eng_fail(rc);
    return VISMA_ICP_OK;
}

int visma_icp_get_color_gradient(visma_icp_ctx *ctx, double *out, int64_t nt)
{
    CTX_CHECK();
    if (nt != ctx->eng->nt() || (nt > 0 && !out)) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad get_color_gradient arguments");
    if (!ctx->eng->has_color_gradient()) return ctx->fail(VISMA_ICP_ERR_STATE, "no colour gradient: prepare_colored first");
    int rc = ctx->eng->get_color_gradient(out);
    if (rc) return ctx->eng_fail(rc);
    return VISMA_ICP_OK;
}

int visma_icp_reduce_colored(visma_icp_ctx *ctx, double lambda_geometric, double out_stats[VISMA_ICP_NSTATS],
                             visma_icp_colored_info *info)
{
    CTX_CHECK();
    if (!out_stats || !info) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    if (int rc = check_colored(ctx)) return rc;
    if (!ctx->eng->has_normals() || !ctx->eng->has_target_colors() || !ctx->eng->has_source_colors() || !ctx->eng->has_color_gradient())
        return ctx->fail(VISMA_ICP_ERR_STATE, "colored ICP needs target normals, both clouds' colours and the colour gradient");
    Engine::ColoredPass cp;
    int rc = ctx->eng->reduce_colored(ctx->last_Tc, ctx->centre, colored_lambda(lambda_geometric), out_stats, &cp);
    if (rc) return ctx->eng_fail(rc);
    ctx->last_plane = true;
    visma_icp_ctx::fill_colored_info(info, cp);
    return VISMA_ICP_OK;
}

int visma_icp_run_colored(visma_icp_ctx *ctx, const double init[16], double max_dist, double lambda_geometric, int max_iter,
                          double rel_fitness, double rel_rmse, visma_icp_result *out, visma_icp_colored_info *info)
{
    CTX_CHECK();
    if (!init || !out || max_iter < 0) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad run arguments");
    if (int rc = check_colored(ctx)) return rc;
    if (info) std::memset(info, 0, sizeof(*info));
    const double lambda = colored_lambda(lambda_geometric);
    // Registration.cpp:148-157 and ColoredICP.cpp:144-146: no radius, no normals or no colours return init
    if (!(max_dist > 0.0) || !ctx->eng->has_normals() || !ctx->eng->has_target_colors() || !ctx->eng->has_source_colors()) {
        std::memset(out, 0, sizeof(*out));
        std::memcpy(out->transformation, init, sizeof(double) * 16);
        if (max_dist > 0.0) ctx->last_radius = max_dist;
        return VISMA_ICP_OK;
    }
    if (!ctx->eng->has_color_gradient(2.0 * max_dist, 30)) {     // ColoredICP.cpp:242-243
        int rc = ctx->eng->prepare_colored(2.0 * max_dist, 30);
        if (rc) return ctx->eng_fail(rc);
    }
    Engine::ColoredPass cp;
    return ctx->run_pair_passes(
        init, max_dist, true, max_iter, rel_fitness, rel_rmse, false, out, nullptr, cp,
        [&](const Mat4 &Tc, double *stats) { return ctx->eng->reduce_colored(Tc, ctx->centre, lambda, stats, &cp); },
        [&](const double *) { if (info) visma_icp_ctx::fill_colored_info(info, cp); });
}

int visma_icp_iterate(visma_icp_ctx *ctx, double T_inout[16], double max_dist, int steps, int solver,
                      int with_scaling, visma_icp_result *out)
{
    CTX_CHECK();
    if (!T_inout || steps < 0 || !(max_dist > 0.0)) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad iterate arguments");
    if (solver < 0 || solver > VISMA_ICP_SOLVER_GN_EXPMAP) return ctx->fail(VISMA_ICP_ERR_INVALID, "unknown solver");
    if (int rc = ctx->check_axis_solver(solver, with_scaling != 0)) return rc;
    if (!ctx->have_src || !ctx->have_tgt) return ctx->fail(VISMA_ICP_ERR_STATE, "clouds not set");
    Mat4 Tc = to_centred(Mat4::from(T_inout), ctx->centre);
    double stats[VISMA_ICP_NSTATS], fit = 0, rmse = 0;
    int64_t k = 0;
    const bool world = visma_icp_ctx::wants_world_frame(solver, false);
    if (ctx->use_device_loop() && steps > 0) {
        Engine::LoopParams lp;
        lp.Tc0 = Tc;
        std::memcpy(lp.centre, ctx->centre, sizeof(ctx->centre));
        lp.max_dist = max_dist; lp.rel_fit = 0.0; lp.rel_rmse = 0.0;
        lp.max_iter = steps; lp.solver = solver; lp.passes = steps;
        lp.scaling = with_scaling != 0; lp.plane = false; lp.world = world; lp.check_stop = false;
        lp.ns_total = ctx->ns_total > 0 ? ctx->ns_total : ctx->eng->ns();
        ctx->fill_axis(lp);
        Engine::LoopResult r;
        int rc = ctx->eng->run_loop(lp, nullptr, 1, &r);
        if (rc) return ctx->eng_fail(rc);
        ctx->last_Tc = r.Tc;
        const Mat4 T = from_centred(r.Tc, ctx->centre);
        std::memcpy(T_inout, T.m, sizeof(T.m));
        if (out) {
            std::memset(out, 0, sizeof(*out));
            std::memcpy(out->transformation, T.m, sizeof(T.m));
            out->fitness = r.fit;
            out->inlier_rmse = r.rmse;
            out->num_correspondences = r.k;
            out->iterations = r.iters;
            out->nn_passes = r.passes;
        }
        return VISMA_ICP_OK;
    }
    {
        Engine::LoopScope scope(ctx->eng.get(), ctx->solo() ? steps : 0);
        for (int i = 0; i < steps; i++) {
            int rc = ctx->pass(Tc, max_dist, false, world, stats, &fit, &rmse, &k);
            if (rc) return rc;
            Tc = ctx->apply_update(ctx->solve(stats, solver, with_scaling != 0, false), Tc, world);
        }
    }
    const Mat4 T = from_centred(Tc, ctx->centre);
    std::memcpy(T_inout, T.m, sizeof(T.m));
    if (out) {
        std::memset(out, 0, sizeof(*out));
        std::memcpy(out->transformation, T.m, sizeof(T.m));
        out->fitness = fit;
        out->inlier_rmse = rmse;
        out->num_correspondences = k;
        out->iterations = steps;
        out->nn_passes = steps;
    }
    return VISMA_ICP_OK;
}

int visma_icp_run_point_to_plane(visma_icp_ctx *ctx, const double init[16], double max_dist,
                                 int max_iter, double rel_fitness, double rel_rmse,
                                 visma_icp_result *out)
{
    CTX_CHECK();
    if (!init || !out || max_iter < 0) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad run arguments");
    return ctx->run(init, max_dist, max_iter, rel_fitness, rel_rmse, VISMA_ICP_SOLVER_GN_EULER, false, true, out);
}

static int yaw_sweep(visma_icp_ctx *ctx, int level, double max_dist, int max_iter, double rel_fitness,
                     double rel_rmse, int solver, bool plane, visma_icp_result *best, int *best_level,
                     visma_icp_result *per_level);

int visma_icp_run_yaw_sweep(visma_icp_ctx *ctx, int level, double max_dist, int max_iter,
                            double rel_fitness, double rel_rmse, int solver, visma_icp_result *best,
                            int *best_level, visma_icp_result *per_level)
{
    CTX_CHECK();
    if (solver < 0 || solver > VISMA_ICP_SOLVER_GN_EXPMAP) return ctx->fail(VISMA_ICP_ERR_INVALID, "unknown solver");
    if (int rc = ctx->check_axis_solver(solver, false)) return rc;
    return yaw_sweep(ctx, level, max_dist, max_iter, rel_fitness, rel_rmse, solver, false, best, best_level, per_level);
}

int visma_icp_run_yaw_sweep_point_to_plane(visma_icp_ctx *ctx, int level, double max_dist, int max_iter,
                                           double rel_fitness, double rel_rmse, visma_icp_result *best,
                                           int *best_level, visma_icp_result *per_level)
{
    CTX_CHECK();
    return yaw_sweep(ctx, level, max_dist, max_iter, rel_fitness, rel_rmse, VISMA_ICP_SOLVER_GN_EULER, true, best,
                     best_level, per_level);
}

static int yaw_sweep(visma_icp_ctx *ctx, int level, double max_dist, int max_iter, double rel_fitness,
                     double rel_rmse, int solver, bool plane, visma_icp_result *best, int *best_level,
                     visma_icp_result *per_level)
{
    if (level <= 0 || !best || max_iter < 0) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad sweep arguments");
    if (plane && ctx->have_tgt && !ctx->eng->has_normals() && max_dist > 0.0) {
        // Registration.cpp:152-157: every start returns RegistrationResult(init); none has correspondences
        std::memset(best, 0, sizeof(*best));
        const Mat4 I = Mat4::identity();
        std::memcpy(best->transformation, I.m, sizeof(I.m));
        if (best_level) *best_level = -1;
        for (int i = 0; per_level && i < level; i++) {
            const Mat4 init = yaw_start(i, level);
            std::memset(&per_level[i], 0, sizeof(per_level[i]));
            std::memcpy(per_level[i].transformation, init.m, sizeof(init.m));
        }
        return VISMA_ICP_OK;
    }
    // src/annotation.cpp:35-61
    if (ctx->use_device_loop_batched() && max_dist > 0.0 && ctx->have_src && ctx->have_tgt) {
        // all `level` ICPs in flight together: one launch per iteration covers every
        // (yaw, source point) pair over the shared grid, `level` solves run in parallel
        std::vector<Mat4> Tc0((size_t)level);
        for (int i = 0; i < level; i++) Tc0[i] = to_centred(yaw_start(i, level), ctx->centre);
        Engine::LoopParams lp;
        lp.Tc0 = Tc0[0];
        std::memcpy(lp.centre, ctx->centre, sizeof(ctx->centre));
        lp.max_dist = max_dist; lp.rel_fit = rel_fitness; lp.rel_rmse = rel_rmse;
        lp.max_iter = max_iter; lp.solver = solver; lp.passes = max_iter + 1;
        lp.scaling = false; lp.plane = plane;
        lp.world = visma_icp_ctx::wants_world_frame(solver, plane);
        lp.check_stop = true;
        lp.ns_total = ctx->ns_total > 0 ? ctx->ns_total : ctx->eng->ns();
        ctx->fill_axis(lp);
        std::vector<Engine::LoopResult> rs((size_t)level);
        int rc = ctx->eng->run_loop(lp, Tc0.data(), level, rs.data());
        if (rc == VISMA_ICP_OK) {
            visma_icp_result bb;
            std::memset(&bb, 0, sizeof(bb));
            const Mat4 I = Mat4::identity();
            std::memcpy(bb.transformation, I.m, sizeof(I.m));
            int bl = -1;
            for (int i = 0; i < level; i++) {
                visma_icp_result r;
                std::memset(&r, 0, sizeof(r));
                const Mat4 T = from_centred(rs[i].Tc, ctx->centre);
                std::memcpy(r.transformation, T.m, sizeof(T.m));
                r.fitness = rs[i].fit; r.inlier_rmse = rs[i].rmse;
                r.num_correspondences = rs[i].k;
                r.iterations = rs[i].iters; r.nn_passes = rs[i].passes;
                if (per_level) per_level[i] = r;
                if (r.num_correspondences > bb.num_correspondences) { bb = r; bl = i; }   // strict >
            }
            ctx->eng->select_problem(bl >= 0 ? bl : 0);
            if (bl >= 0) ctx->last_Tc = rs[bl].Tc;
            *best = bb;
            if (best_level) *best_level = bl;
            return VISMA_ICP_OK;
        }
        if (rc != VISMA_ICP_ERR_STATE) return ctx->eng_fail(rc);
        // (brute-force search selected, or RCCL attached): fall through to the sequential sweep
    }
    return sweep_sequential<NoInfo>(level, [&](const Mat4 &init, visma_icp_result *r, NoInfo *) {
        return ctx->run(init.m, max_dist, max_iter, rel_fitness, rel_rmse, solver, false, plane, r);
    }, best, best_level, per_level);
}

// normals == NULL: the point-to-point estimator with `solver`; otherwise normals[i] are the target
// normals of problem i (AoS stride 3; NULL = that cloud has none) and the estimator is point-to-plane
static int run_batch_impl(visma_icp_ctx *ctx, const visma_icp_problem *probs, const double *const *normals, int n,
                          int max_iter, double rel_fitness, double rel_rmse, int solver, visma_icp_result *out)
{
    ctx->eng->set_exact(ctx->search_precision == 1);     // (a batch uploads its own clouds)
    const bool plane = normals != nullptr;
    bool all_normals = plane;
    for (int i = 0; plane && i < n; i++)
        if (probs[i].nt > 0 && !normals[i]) all_normals = false;
    // (a problem without normals returns its initial transform, Registration.cpp:152-157: sequential path;
    //  point-to-plane batches run the exact or the fp32 search)
    const bool batch_ok = !plane || (all_normals && ctx->search_precision != 2);
    if (ctx->use_device_loop_batched() && n > 1 && batch_ok) {
        // every problem in flight together: concatenated clouds, one grid per problem,
        // one NN launch + one fold/solve launch per pass for the whole batch
        StageTrace tr("batch/driver");
        std::vector<std::vector<float>> sbuf((size_t)n), tbuf((size_t)n);
        std::vector<Engine::BatchProblem> pb((size_t)n);
        bool ok = true;
        for (int i = 0; i < n; i++) {
            const visma_icp_problem &q = probs[i];
            if (q.ns < 0 || q.nt < 0 || (q.ns > 0 && !q.src_xyz) || (q.nt > 0 && !q.tgt_xyz))
                return ctx->fail(VISMA_ICP_ERR_INVALID, "bad batch problem");
            if (!(q.max_dist > 0.0)) ok = false;   // rare: handled by the sequential path
        }
        // Problems often share clouds: the 24 yaw starts of one model (src/annotation.cpp:35-61),
        // every model against the same scene.  Equal (pointer, count) pairs are packed, uploaded
        // and gridded ONCE.
        std::vector<int> tshare((size_t)n, -1), sshare((size_t)n, -1), gshare((size_t)n, -1);
        for (int i = 0; ok && i < n; i++)
            for (int j = 0; j < i; j++) {
                if (tshare[j] >= 0) continue;                      // only first occurrences are referenced
                if (probs[j].tgt_xyz == probs[i].tgt_xyz && probs[j].nt == probs[i].nt) { tshare[i] = j; break; }
            }
        for (int i = 0; ok && i < n; i++) {
            const int t = tshare[i] >= 0 ? tshare[i] : i;
            for (int j = 0; j < i; j++) {
                const int tj = tshare[j] >= 0 ? tshare[j] : j;
                if (tj != t) continue;
                if (gshare[i] < 0 && gshare[j] < 0 && probs[j].max_dist == probs[i].max_dist) gshare[i] = j;
                if (sshare[i] < 0 && sshare[j] < 0 && probs[j].src_xyz == probs[i].src_xyz && probs[j].ns == probs[i].ns)
                    sshare[i] = j;
            }
        }
        tr.mark("sharing found");
        std::vector<std::array<double, 3>> cen((size_t)n);
        std::vector<std::array<float, 6>> tbox((size_t)n);
        // double-precision search for the whole batch when every problem qualifies
        const bool want64 = ctx->search_precision != 0;
        std::vector<std::vector<Pt64>> s8((size_t)n), t8((size_t)n), n8((size_t)n);
        std::vector<std::vector<float>> nbuf((size_t)n);
        if (plane)
            for (int i = 0; ok && i < n; i++)                     // clouds passed twice carry the same normals
                if (tshare[i] >= 0 && normals[tshare[i]] != normals[i]) ok = false;
        if (ok)
            parallel_for(n, 1, [&](int64_t i) {                    // targets: first occurrences only
                if (tshare[i] >= 0) return;
                if (plane && want64) {
                    n8[i].resize((size_t)std::max<int64_t>(probs[i].nt, 1));
                    for (int64_t j = 0; j < probs[i].nt; j++)
                        n8[i][(size_t)j] = Pt64{normals[i][3 * j], normals[i][3 * j + 1], normals[i][3 * j + 2], 0ull};
                } else if (plane) {
                    const double zero[3] = {0, 0, 0};
                    pack_f64(normals[i], probs[i].nt, 3, zero, nbuf[i]);
                }
                const visma_icp_problem &q = probs[i];
                double c[3];
                centroid_f64(q.tgt_xyz, q.nt, 3, c, false);       // the same value as set_clouds_f64 computes
                for (int a = 0; a < 3; a++) cen[i][a] = c[a];
                // the target itself is uploaded as it is and expanded on the device; the host only needs the
                // bounding box of its fp32 copy: the rounding (float)(x - c) is monotone, so the box of the
                // f64 values, rounded the same way, is the box of the rounded values
                double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
                for (int64_t j = 0; j < q.nt; j++)
                    for (int a = 0; a < 3; a++) {
                        const double v = q.tgt_xyz[3 * j + a];
                        if (j == 0 || v < lo[a]) lo[a] = v;
                        if (j == 0 || v > hi[a]) hi[a] = v;
                    }
                for (int a = 0; a < 3; a++) { tbox[i][a] = (float)(lo[a] - c[a]); tbox[i][3 + a] = (float)(hi[a] - c[a]); }
            });
        tr.mark("targets: centroid, box");
        if (ok)
            parallel_for(n, 1, [&](int64_t i) {
                const visma_icp_problem &q = probs[i];
                const int t = tshare[i] >= 0 ? tshare[i] : (int)i;
                const double *c = cen[t].data();
                if (sshare[i] < 0) {
                    pack_f64(q.src_xyz, q.ns, 3, c, sbuf[i]);
                    std::vector<int32_t> order;
                    morton_order(sbuf[i], q.ns, order);
                    if (want64) {
                        s8[i].resize((size_t)std::max<int64_t>(q.ns, 1));
                        for (int64_t pos = 0; pos < q.ns; pos++) {
                            const double *sp = q.src_xyz + 3 * (size_t)order[(size_t)pos];
                            s8[i][(size_t)pos] = Pt64{sp[0] - c[0], sp[1] - c[1], sp[2] - c[2], (unsigned long long)order[(size_t)pos]};
                        }
                    }
                }
                Engine::BatchProblem &b = pb[i];
                b.src64 = (want64 && sshare[i] < 0) ? s8[i].data() : nullptr;
                b.tgt64 = nullptr;
                b.tgt_raw = probs[t].tgt_xyz;
                b.tgt_f64 = want64;
                b.nrm64 = (plane && want64) ? n8[t].data() : nullptr;
                b.nrm_xyzw = (plane && !want64) ? nbuf[t].data() : nullptr;
                b.src_xyzw = sshare[i] < 0 ? sbuf[i].data() : nullptr; b.ns = q.ns;
                b.tgt_xyzw = nullptr; b.nt = q.nt;
                b.src_share = sshare[i];
                b.grid_share = gshare[i];
                b.Tc0 = to_centred(Mat4::from(q.init), c);
                std::memcpy(b.centre, c, 3 * sizeof(double));
                b.max_dist = q.max_dist;
                for (int a = 0; a < 3; a++) { b.bb_min[a] = 0.f; b.bb_max[a] = 0.f; }
                if (gshare[i] >= 0) return;                        // the grid (and its box) is reused
                if (q.nt > 0)
                    for (int a = 0; a < 3; a++) { b.bb_min[a] = tbox[t][a]; b.bb_max[a] = tbox[t][3 + a]; }
            });
        tr.mark("sources: pack, order");
        if (ok) {
            Engine::LoopParams lp;
            lp.Tc0 = Mat4::identity();
            lp.centre[0] = lp.centre[1] = lp.centre[2] = 0.0;
            lp.max_dist = 0.0; lp.rel_fit = rel_fitness; lp.rel_rmse = rel_rmse;
            lp.max_iter = max_iter; lp.solver = solver; lp.passes = max_iter + 1;
            lp.scaling = false; lp.plane = plane;
            lp.world = visma_icp_ctx::wants_world_frame(solver, plane);
            lp.check_stop = true; lp.ns_total = 0;
            ctx->fill_axis(lp);
            std::vector<Engine::LoopResult> rs((size_t)n);
            int rc = ctx->eng->run_loop_batch(lp, pb, rs.data());
            tr.mark("engine batch loop");
            if (rc == VISMA_ICP_OK) {
                for (int i = 0; i < n; i++) {
                    std::memset(&out[i], 0, sizeof(out[i]));
                    const Mat4 T = from_centred(rs[i].Tc, pb[i].centre);
                    std::memcpy(out[i].transformation, T.m, sizeof(T.m));
                    out[i].fitness = rs[i].fit; out[i].inlier_rmse = rs[i].rmse;
                    out[i].num_correspondences = rs[i].k;
                    out[i].iterations = rs[i].iters; out[i].nn_passes = rs[i].passes;
                }
                return VISMA_ICP_OK;
            }
            if (rc != VISMA_ICP_ERR_STATE) return ctx->eng_fail(rc);
        }
    }
    for (int i = 0; i < n; i++) {
        int rc = visma_icp_set_clouds_f64(ctx, probs[i].src_xyz, probs[i].ns, 3, probs[i].tgt_xyz, probs[i].nt, 3);
        if (rc) return rc;
        if (plane && normals[i]) {
            rc = visma_icp_set_target_normals_f64(ctx, normals[i], probs[i].nt, 3);
            if (rc) return rc;
        }
        rc = ctx->run(probs[i].init, probs[i].max_dist, max_iter, rel_fitness, rel_rmse, solver, false, plane, &out[i]);
        if (rc) return rc;
    }
    return VISMA_ICP_OK;
}

int visma_icp_run_batch(visma_icp_ctx *ctx, const visma_icp_problem *probs, int n, int max_iter,
                        double rel_fitness, double rel_rmse, int solver, visma_icp_result *out)
{
    CTX_CHECK();
    if (n < 0 || (n > 0 && (!probs || !out)) || max_iter < 0) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad batch arguments");
    if (solver < 0 || solver > VISMA_ICP_SOLVER_GN_EXPMAP) return ctx->fail(VISMA_ICP_ERR_INVALID, "unknown solver");
    if (int rc = ctx->check_axis_solver(solver, false)) return rc;
    return run_batch_impl(ctx, probs, nullptr, n, max_iter, rel_fitness, rel_rmse, solver, out);
}

int visma_icp_run_batch_point_to_plane(visma_icp_ctx *ctx, const visma_icp_problem *probs,
                                       const double *const *tgt_normals, int n, int max_iter, double rel_fitness,
                                       double rel_rmse, visma_icp_result *out)
{
    CTX_CHECK();
    if (n < 0 || (n > 0 && (!probs || !out || !tgt_normals)) || max_iter < 0)
        return ctx->fail(VISMA_ICP_ERR_INVALID, "bad batch arguments");
    static const double *const none[1] = {nullptr};
    return run_batch_impl(ctx, probs, n > 0 ? tgt_normals : none, n, max_iter, rel_fitness, rel_rmse,
                          VISMA_ICP_SOLVER_GN_EULER, out);
}

// ---- the information matrix of an edge (information.hip) ---------------------------------------------------------------
static int check_information(visma_icp_ctx *ctx)
{
    if (ctx->sharded() || ctx->eng->is_sharded()) return ctx->fail(VISMA_ICP_ERR_INVALID, "the information matrix runs on one rank");
    if (!ctx->have_src || !ctx->have_tgt) return ctx->fail(VISMA_ICP_ERR_STATE, "clouds not set");
    return VISMA_ICP_OK;
}

int visma_icp_reduce_information(visma_icp_ctx *ctx, double out[36])
{
    CTX_CHECK();
    if (!out) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    if (int rc = check_information(ctx)) return rc;
    double sums[kInfoAcc];
    Engine::PairPass pp;
    int rc = ctx->eng->reduce_information(ctx->last_Tc, ctx->centre, sums, &pp);
    if (rc) return ctx->eng_fail(rc);
    information_from_sums(sums, out);
    return VISMA_ICP_OK;
}

int visma_icp_information_matrix(visma_icp_ctx *ctx, const double T[16], double max_dist, double out[36], int64_t *k)
{
    CTX_CHECK();
    if (!T || !out) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL argument");
    if (!(max_dist > 0.0)) return ctx->fail(VISMA_ICP_ERR_INVALID, "max_dist must be > 0");
    if (int rc = check_information(ctx)) return rc;
    for (int i = 0; i < 36; i++) out[i] = 0.0;
    if (k) *k = 0;
    for (int i = 0; i < 16; i++)
        if (!std::isfinite(T[i])) return VISMA_ICP_OK;           // (a pose that is no pose has no pairs)
    int rc = visma_icp_nn_pass(ctx, T, max_dist);
    if (rc) return rc;
    rc = visma_icp_reduce_information(ctx, out);
    if (rc) return rc;
    if (k) *k = (int64_t)std::llround(out[35]);
    return VISMA_ICP_OK;
}

// A new source next to the target of the last visma_icp_set_clouds_f64, centred where that call centred: the source half
// of that call on the engine's raw path.  VISMA_ICP_ERR_STATE: not on this engine (the caller uploads both clouds).
static int set_source_beside_target_f64(visma_icp_ctx *ctx, const double *src, int64_t ns)
{
    if (!ctx->centred_upload || !ctx->have_tgt || ctx->fixed_centre || std::getenv("VISMA_ICP_RAW_UPLOAD_MIN")) return VISMA_ICP_ERR_STATE;
    const bool want64 = ctx->search_precision != 0 && ctx->eng->supports_device_loop();
    int rc = ctx->eng->set_source_f64(src, ns, 3, ctx->centre, want64, ctx->src_order);
    ctx->src_order_gen++;
    if (rc) { ctx->have_src = false; return rc; }
    ctx->eng->set_exact(ctx->search_precision == 1);
    if (!want64) {
        rc = ctx->eng->set_clouds64(nullptr, nullptr);
        if (rc) { ctx->have_src = false; return rc; }
    }
    ctx->have_src = true;
    return VISMA_ICP_OK;
}

int visma_icp_get_cloud_sizes(visma_icp_ctx *ctx, int64_t *ns, int64_t *nt)
{
    CTX_CHECK();
    if (!ns || !nt) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    *ns = ctx->have_src ? ctx->eng->ns() : 0;
    *nt = ctx->have_tgt ? ctx->eng->nt() : 0;
    return VISMA_ICP_OK;
}

int visma_icp_information_matrices(visma_icp_ctx *ctx, const visma_icp_problem *probs, int n, double *out, int64_t *k)
{
    CTX_CHECK();
    if (n < 0 || (n > 0 && (!probs || !out))) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad batch arguments");
    if (ctx->sharded() || ctx->eng->is_sharded()) return ctx->fail(VISMA_ICP_ERR_INVALID, "the information matrix runs on one rank");
    for (int i = 0; i < n; i++) {
        const visma_icp_problem &q = probs[i];
        if (q.ns < 0 || q.nt < 0 || (q.ns > 0 && !q.src_xyz) || (q.nt > 0 && !q.tgt_xyz) || !(q.max_dist > 0.0))
            return ctx->fail(VISMA_ICP_ERR_INVALID, "bad batch problem");
    }
    // edges in groups of one target (first occurrences in the caller's order): the target is uploaded once per group.
    // (Its search grid is NOT kept: a new source invalidates it on the engine, so every edge builds its own.)
    std::vector<int> order;
    std::vector<char> taken((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        if (taken[(size_t)i]) continue;
        std::vector<int> group;
        for (int j = i; j < n; j++)
            if (!taken[(size_t)j] && probs[j].tgt_xyz == probs[i].tgt_xyz && probs[j].nt == probs[i].nt) { group.push_back(j); taken[(size_t)j] = 1; }
        order.insert(order.end(), group.begin(), group.end());
    }
    int prev = -1;
    for (int e : order) {
        const visma_icp_problem &q = probs[e];
        double *o = out + (size_t)e * 36;
        for (int i = 0; i < 36; i++) o[i] = 0.0;
        if (k) k[e] = 0;
        bool finite = true;
        for (int i = 0; i < 16; i++) finite = finite && std::isfinite(q.init[i]);
        if (!finite) continue;
        int rc = VISMA_ICP_ERR_STATE;
        if (prev >= 0 && probs[prev].tgt_xyz == q.tgt_xyz && probs[prev].nt == q.nt) {
            rc = set_source_beside_target_f64(ctx, q.src_xyz, q.ns);
            if (rc && rc != VISMA_ICP_ERR_STATE) return ctx->eng_fail(rc);
        }
        if (rc) {
            rc = visma_icp_set_clouds_f64(ctx, q.src_xyz, q.ns, 3, q.tgt_xyz, q.nt, 3);
            if (rc) return rc;
        }
        prev = e;
        rc = visma_icp_information_matrix(ctx, q.init, q.max_dist, o, k ? &k[e] : nullptr);
        if (rc) return rc;
    }
    return VISMA_ICP_OK;
}

// ---- RGB-D odometry (odometry_image.hip, odometry.hip) -----------------------------------------------------------------
int visma_icp_odometry_option_default(visma_icp_odometry_option *opt)
{
    if (!opt) return VISMA_ICP_ERR_INVALID;
    std::memset(opt, 0, sizeof(*opt));
    opt->n_levels = 3;
    opt->iterations[0] = 20; opt->iterations[1] = 10; opt->iterations[2] = 5;
    opt->max_depth_diff = 0.03; opt->min_depth = 0.0; opt->max_depth = 4.0;
    return VISMA_ICP_OK;
}

// an all-zero pose is the identity (visma_icp.h)
static Mat4 odometry_pose(const double T[16])
{
    bool zero = true;
    for (int i = 0; i < 16; i++) zero = zero && T[i] == 0.0;
    return zero ? Mat4::identity() : Mat4::from(T);
}

// every argument check of a frame pair, before anything reaches a device; *in is what the engine is given
static int check_odometry_frames(visma_icp_ctx *ctx, int w, int h, const float *src_gray, const float *src_depth, const float *tgt_gray,
                                 const float *tgt_depth, const double *intrinsic, const double *init,
                                 const visma_icp_odometry_option *option, visma_icp_odometry_option *opt, Engine::OdometryInput *in)
{
    if (!src_gray || !src_depth || !tgt_gray || !tgt_depth || !intrinsic || !init) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL argument");
    if (w < 1 || h < 1) return ctx->fail(VISMA_ICP_ERR_INVALID, "an image needs w >= 1 and h >= 1");
    if ((int64_t)w * h > (int64_t)1 << 30) return ctx->fail(VISMA_ICP_ERR_INVALID, "an image of more than 2^30 pixels");
    if (option) *opt = *option; else visma_icp_odometry_option_default(opt);
    if (opt->n_levels < 1 || opt->n_levels > VISMA_ICP_ODOMETRY_MAX_LEVELS) return ctx->fail(VISMA_ICP_ERR_INVALID, "n_levels outside 1 .. 8");
    if ((std::min(w, h) >> (opt->n_levels - 1)) < 1) return ctx->fail(VISMA_ICP_ERR_INVALID, "a pyramid level without pixels");
    for (int l = 0; l < opt->n_levels; l++)
        if (opt->iterations[l] < 0) return ctx->fail(VISMA_ICP_ERR_INVALID, "a negative iteration count");
    if (!std::isfinite(intrinsic[0]) || !std::isfinite(intrinsic[1]) || intrinsic[0] == 0.0 || intrinsic[1] == 0.0)
        return ctx->fail(VISMA_ICP_ERR_INVALID, "a focal length that is zero or not finite");
    if (ctx->sharded() || ctx->eng->is_sharded()) return ctx->fail(VISMA_ICP_ERR_INVALID, "RGB-D odometry runs on one rank");
    in->w = w; in->h = h; in->n_levels = opt->n_levels;
    in->src_gray = src_gray; in->src_depth = src_depth; in->tgt_gray = tgt_gray; in->tgt_depth = tgt_depth;
    in->fx = intrinsic[0]; in->fy = intrinsic[1]; in->cx = intrinsic[2]; in->cy = intrinsic[3];
    in->init = odometry_pose(init);
    in->max_depth_diff = opt->max_depth_diff; in->min_depth = opt->min_depth; in->max_depth = opt->max_depth;
    return VISMA_ICP_OK;
}

static int odometry_prepare_checked(visma_icp_ctx *ctx, const Engine::OdometryInput &in)
{
    ctx->odo.ready = false;
    int rc = ctx->eng->odometry_prepare(in);
    if (rc) return ctx->eng_fail(rc);
    ctx->odo.ready = true; ctx->odo.w = in.w; ctx->odo.h = in.h; ctx->odo.n_levels = in.n_levels;
    return VISMA_ICP_OK;
}

int visma_icp_odometry_prepare(visma_icp_ctx *ctx, int w, int h, const float *src_gray, const float *src_depth, const float *tgt_gray,
                               const float *tgt_depth, const double intrinsic[4], const double init[16],
                               const visma_icp_odometry_option *option)
{
    CTX_CHECK();
    visma_icp_odometry_option opt;
    Engine::OdometryInput in;
    if (int rc = check_odometry_frames(ctx, w, h, src_gray, src_depth, tgt_gray, tgt_depth, intrinsic, init, option, &opt, &in)) return rc;
    return odometry_prepare_checked(ctx, in);
}

// a level no pyramid can have is INVALID whatever the state; then the call order; then the resident pyramid's own depth
static int check_odometry_level(visma_icp_ctx *ctx, int level)
{
    if (level < 0 || level >= VISMA_ICP_ODOMETRY_MAX_LEVELS) return ctx->fail(VISMA_ICP_ERR_INVALID, "level out of range");
    if (!ctx->odo.ready) return ctx->fail(VISMA_ICP_ERR_STATE, "no odometry frames: visma_icp_odometry_prepare first");
    if (level >= ctx->odo.n_levels) return ctx->fail(VISMA_ICP_ERR_INVALID, "level out of range");
    return VISMA_ICP_OK;
}

int visma_icp_odometry_get_image(visma_icp_ctx *ctx, int which, int level, float *out)
{
    CTX_CHECK();
    if (!out) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    if (which < 0 || which >= kOdoImages) return ctx->fail(VISMA_ICP_ERR_INVALID, "which out of range");
    if (int rc = check_odometry_level(ctx, level)) return rc;
    int rc = ctx->eng->odometry_get_image(which, level, out);
    return rc ? ctx->eng_fail(rc) : VISMA_ICP_OK;
}

int visma_icp_odometry_correspondences(visma_icp_ctx *ctx, int level, const double T[16], int32_t *out_idx, int64_t *out_k)
{
    CTX_CHECK();
    if (!T || !out_k) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL argument");
    if (int rc = check_odometry_level(ctx, level)) return rc;
    int rc = ctx->eng->odometry_correspondences(level, odometry_pose(T), out_idx, out_k);
    return rc ? ctx->eng_fail(rc) : VISMA_ICP_OK;
}

int visma_icp_odometry_step(visma_icp_ctx *ctx, int level, const double T[16], int method, double out_stats[VISMA_ICP_NSTATS],
                            int64_t *out_k, double *out_sum_r2)
{
    CTX_CHECK();
    if (!T || !out_stats) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL argument");
    if (method != VISMA_ICP_ODOMETRY_COLOR && method != VISMA_ICP_ODOMETRY_HYBRID) return ctx->fail(VISMA_ICP_ERR_INVALID, "unknown odometry method");
    if (int rc = check_odometry_level(ctx, level)) return rc;
    int rc = ctx->eng->odometry_step(level, odometry_pose(T), method, out_stats);
    if (rc) return ctx->eng_fail(rc);
    if (out_k) *out_k = (int64_t)std::llround(out_stats[0]);
    if (out_sum_r2) *out_sum_r2 = out_stats[1];
    return VISMA_ICP_OK;
}

int visma_icp_odometry_information(visma_icp_ctx *ctx, const double T[16], double out[36], int64_t *out_k)
{
    CTX_CHECK();
    if (!T || !out) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL argument");
    if (int rc = check_odometry_level(ctx, 0)) return rc;
    double sums[kInfoAcc];
    int rc = ctx->eng->odometry_information(odometry_pose(T), sums);
    if (rc) return ctx->eng_fail(rc);
    information_from_sums(sums, out);
    if (out_k) *out_k = (int64_t)std::llround(sums[0]);
    return VISMA_ICP_OK;
}

// ComputeRGBDOdometry: prepare, ComputeMultiscale (per iteration the correspondence kernel and the reduction on the
// stream, the 6 x 6 solve here), CreateInformationMatrix
static int rgbd_odometry_frames(visma_icp_ctx *ctx, int w, int h, const float *src_gray, const float *src_depth, const float *tgt_gray,
                                const float *tgt_depth, bool on_device, const double intrinsic[4], const double init[16], int method,
                                const visma_icp_odometry_option *option, double out_T[16], double out_info[36],
                                visma_icp_odometry_result *out_result)
{
    if (!out_T) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    if (method != VISMA_ICP_ODOMETRY_COLOR && method != VISMA_ICP_ODOMETRY_HYBRID) return ctx->fail(VISMA_ICP_ERR_INVALID, "unknown odometry method");
    if (out_result && (out_result->pairs_capacity < 0 || (out_result->pairs_capacity > 0 && !out_result->pairs)))
        return ctx->fail(VISMA_ICP_ERR_INVALID, "pairs_capacity without room");
    visma_icp_odometry_option opt;
    Engine::OdometryInput in;
    if (int rc = check_odometry_frames(ctx, w, h, src_gray, src_depth, tgt_gray, tgt_depth, intrinsic, init, option, &opt, &in)) return rc;
    in.on_device = on_device;
    int64_t schedule = 0;
    for (int l = 0; l < opt.n_levels; l++) schedule += opt.iterations[l];
    if (out_result && out_result->pairs_capacity > 0 && out_result->pairs_capacity < schedule)
        return ctx->fail(VISMA_ICP_ERR_INVALID, "pairs_capacity below the sum of the schedule");
    if (int rc = odometry_prepare_checked(ctx, in)) return rc;
    Mat4 T = in.init;
    bool ok = true;
    int steps = 0;
    for (int level = opt.n_levels - 1; level >= 0 && ok; level--)
        for (int it = 0; it < opt.iterations[opt.n_levels - level - 1] && ok; it++) {
            double stats[kNStats];
            int rc = ctx->eng->odometry_step(level, T, method, stats);
            if (rc) return ctx->eng_fail(rc);
            if (out_result && out_result->pairs_capacity > 0) out_result->pairs[steps] = (int64_t)std::llround(stats[0]);
            steps++;
            const Mat4 step = gn_from_stats(stats, false, &ok);
            T = step * T;
        }
    const Mat4 I = Mat4::identity();
    for (int i = 0; i < 16; i++) out_T[i] = ok ? T.m[i] : I.m[i];
    if (out_info) for (int i = 0; i < 36; i++) out_info[i] = 0.0;
    int64_t K = 0;
    if (ok && (out_info || out_result)) {
        double info[36];
        int rc = visma_icp_odometry_information(ctx, T.m, info, &K);
        if (rc) return rc;
        if (out_info) std::memcpy(out_info, info, sizeof(info));
    }
    if (out_result) { out_result->success = ok ? 1 : 0; out_result->iterations = steps; out_result->information_pairs = K; }
    return VISMA_ICP_OK;
}

int visma_icp_rgbd_odometry(visma_icp_ctx *ctx, int w, int h, const float *src_gray, const float *src_depth, const float *tgt_gray,
                            const float *tgt_depth, const double intrinsic[4], const double init[16], int method,
                            const visma_icp_odometry_option *option, double out_T[16], double out_info[36],
                            visma_icp_odometry_result *out_result)
{
    CTX_CHECK();
    return rgbd_odometry_frames(ctx, w, h, src_gray, src_depth, tgt_gray, tgt_depth, false, intrinsic, init, method, option, out_T,
                                out_info, out_result);
}

// ---- the hand-offs of resident Images (image.hip): the same device cores, the pixels taken device to device ----------------
// the four frames of an odometry call: images of this context, 1 x float, of one size; -> their pixels
static int odometry_images(visma_icp_ctx *ctx, visma_icp_image *const img[4], const float *px[4], int *w, int *h)
{
    for (int k = 0; k < 4; k++) {
        if (!img[k]) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL image");
        if (!ctx->owns(img[k])) return ctx->fail(VISMA_ICP_ERR_INVALID, "not an image of this context");
        int iw, ih, ch, bpc;
        image_device_info(img[k]->dev, &iw, &ih, &ch, &bpc);
        if (ch != 1 || bpc != 4 || image_device_is_integer(img[k]->dev)) return ctx->fail(VISMA_ICP_ERR_INVALID, "an odometry frame is a 1 x float image");
        if (k == 0) { *w = iw; *h = ih; }
        else if (iw != *w || ih != *h) return ctx->fail(VISMA_ICP_ERR_INVALID, "the four images differ in size");
        px[k] = static_cast<const float *>(image_device_pixels(img[k]->dev));
    }
    if (*w < 1 || *h < 1) return ctx->fail(VISMA_ICP_ERR_INVALID, "an image needs w >= 1 and h >= 1");
    return VISMA_ICP_OK;
}

int visma_icp_odometry_prepare_images(visma_icp_ctx *ctx, visma_icp_image *src_gray, visma_icp_image *src_depth, visma_icp_image *tgt_gray,
                                      visma_icp_image *tgt_depth, const double intrinsic[4], const double init[16],
                                      const visma_icp_odometry_option *option)
{
    CTX_CHECK();
    visma_icp_image *const img[4] = {src_gray, src_depth, tgt_gray, tgt_depth};
    const float *px[4];
    int w = 0, h = 0;
    if (int rc = odometry_images(ctx, img, px, &w, &h)) return rc;
    visma_icp_odometry_option opt;
    Engine::OdometryInput in;
    if (int rc = check_odometry_frames(ctx, w, h, px[0], px[1], px[2], px[3], intrinsic, init, option, &opt, &in)) return rc;
    in.on_device = true;
    return odometry_prepare_checked(ctx, in);
}

int visma_icp_rgbd_odometry_images(visma_icp_ctx *ctx, visma_icp_image *src_gray, visma_icp_image *src_depth, visma_icp_image *tgt_gray,
                                   visma_icp_image *tgt_depth, const double intrinsic[4], const double init[16], int method,
                                   const visma_icp_odometry_option *option, double out_T[16], double out_info[36],
                                   visma_icp_odometry_result *out_result)
{
    CTX_CHECK();
    visma_icp_image *const img[4] = {src_gray, src_depth, tgt_gray, tgt_depth};
    const float *px[4];
    int w = 0, h = 0;
    if (int rc = odometry_images(ctx, img, px, &w, &h)) return rc;
    return rgbd_odometry_frames(ctx, w, h, px[0], px[1], px[2], px[3], true, intrinsic, init, method, option, out_T, out_info, out_result);
}

int visma_icp_image_from_odometry(visma_icp_ctx *ctx, int which, int level, visma_icp_image **out)
{
    CTX_CHECK();
    if (!out) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    *out = nullptr;
    if (which < 0 || which >= kOdoSrcXyz) return ctx->fail(VISMA_ICP_ERR_INVALID, "which out of range (the xyz image has three floats per pixel: not an Image)");
    if (int rc = check_odometry_level(ctx, level)) return rc;
    const float *px = nullptr;
    int w = 0, h = 0;
    if (int rc = ctx->eng->odometry_image_view(which, level, &px, &w, &h)) return ctx->eng_fail(rc);
    ImageDevice *dev = nullptr;
    const hipError_t e = image_device_create(w, h, 1, 4, px, true, ctx->eng->aux_stream(), &dev);
    if (e != hipSuccess) { (void)hipGetLastError(); return ctx->fail(VISMA_ICP_ERR_HIP, std::string("image_from_odometry: ") + hipGetErrorString(e)); }
    *out = ctx->adopt(dev);
    return VISMA_ICP_OK;
}

// ---- TSDF integration (tsdf.hip) -----------------------------------------------------------------------------------------
// every argument check of a volume call, before anything reaches a device
static int check_tsdf_volume(visma_icp_ctx *ctx, visma_icp_tsdf *volume)
{
    if (!volume) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL volume");
    for (const auto &v : ctx->volumes)
        if (v.get() == volume) return VISMA_ICP_OK;
    return ctx->fail(VISMA_ICP_ERR_INVALID, "not a volume of this context");
}

static bool finite_positive(double v) { return std::isfinite(v) && v > 0.0; }

// ... and of a frame: sizes, intrinsic, colour by colour type; *f is what the engine is given
static int check_tsdf_frame(visma_icp_ctx *ctx, int w, int h, const float *depth, const void *color, int color_type, const double *intrinsic,
                            int intrinsic_w, int intrinsic_h, const double *extrinsic, TsdfFrame *f)
{
    if (!depth || !intrinsic) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL argument");
    if (w < 1 || h < 1) return ctx->fail(VISMA_ICP_ERR_INVALID, "an image needs w >= 1 and h >= 1");
    if ((int64_t)w * h > (int64_t)1 << 30) return ctx->fail(VISMA_ICP_ERR_INVALID, "an image of more than 2^30 pixels");
    if (w != intrinsic_w || h != intrinsic_h) return ctx->fail(VISMA_ICP_ERR_INVALID, "the image size differs from the intrinsic's");
    if (color_type != kTsdfColorNone && !color) return ctx->fail(VISMA_ICP_ERR_INVALID, "no colour image for a coloured volume");
    if (!std::isfinite(intrinsic[0]) || !std::isfinite(intrinsic[1]) || intrinsic[0] == 0.0 || intrinsic[1] == 0.0)
        return ctx->fail(VISMA_ICP_ERR_INVALID, "a focal length that is zero or not finite");
    if (ctx->sharded() || ctx->eng->is_sharded()) return ctx->fail(VISMA_ICP_ERR_INVALID, "TSDF integration runs on one rank");
    f->w = w; f->h = h; f->depth = depth; f->color = color_type != kTsdfColorNone ? color : nullptr;
    f->fx = intrinsic[0]; f->fy = intrinsic[1]; f->cx = intrinsic[2]; f->cy = intrinsic[3];
    const Mat4 E = extrinsic ? Mat4::from(extrinsic) : Mat4::identity();
    std::memcpy(f->extrinsic, E.m, sizeof(E.m));
    return VISMA_ICP_OK;
}

int visma_icp_tsdf_create_uniform(visma_icp_ctx *ctx, double length, int resolution, double sdf_trunc, int color_type,
                                  const double origin[3], visma_icp_tsdf **out)
{
    CTX_CHECK();
    if (!out) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    *out = nullptr;
    if (resolution < 1) return ctx->fail(VISMA_ICP_ERR_INVALID, "resolution < 1");
    if (!finite_positive(length) || !finite_positive(sdf_trunc))
        return ctx->fail(VISMA_ICP_ERR_INVALID, "length and sdf_trunc must be positive and finite");
    if (color_type != kTsdfColorNone && color_type != kTsdfColorRgb8 && color_type != kTsdfColorGray32)
        return ctx->fail(VISMA_ICP_ERR_INVALID, "unknown colour type");
    if (origin && !(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2])))
        return ctx->fail(VISMA_ICP_ERR_INVALID, "an origin that is not finite");
    // the reference's voxel index is an int: 1290^3 < 2^31 <= 1291^3 (five floats per voxel: 43 GB at most)
    if (resolution > 1290) return ctx->fail(VISMA_ICP_ERR_INVALID, "a volume too large for memory");
    if (ctx->sharded() || ctx->eng->is_sharded()) return ctx->fail(VISMA_ICP_ERR_INVALID, "TSDF integration runs on one rank");
    std::unique_ptr<visma_icp_tsdf> v(new visma_icp_tsdf);
    v->cfg.resolution = resolution; v->cfg.length = length; v->cfg.sdf_trunc = sdf_trunc; v->cfg.color_type = color_type;
    for (int a = 0; a < 3; a++) v->cfg.origin[a] = origin ? origin[a] : 0.0;
    int rc = ctx->eng->tsdf_create(v->cfg, &v->id);
    if (rc) return ctx->eng_fail(rc);
    *out = v.get();
    ctx->volumes.push_back(std::move(v));
    return VISMA_ICP_OK;
}

int visma_icp_tsdf_create_scalable(visma_icp_ctx *ctx, double voxel_length, double sdf_trunc, int color_type, int volume_unit_resolution,
                                   int depth_sampling_stride, int initial_units, visma_icp_tsdf **out)
{
    CTX_CHECK();
    if (!out) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    *out = nullptr;
    if (volume_unit_resolution < 1) return ctx->fail(VISMA_ICP_ERR_INVALID, "resolution < 1");
    if (volume_unit_resolution > 256) return ctx->fail(VISMA_ICP_ERR_INVALID, "a volume unit too large for memory");
    if (!finite_positive(voxel_length) || !finite_positive(sdf_trunc))
        return ctx->fail(VISMA_ICP_ERR_INVALID, "voxel_length and sdf_trunc must be positive and finite");
    if (color_type != kTsdfColorNone && color_type != kTsdfColorRgb8 && color_type != kTsdfColorGray32)
        return ctx->fail(VISMA_ICP_ERR_INVALID, "unknown colour type");
    if (depth_sampling_stride < 1) return ctx->fail(VISMA_ICP_ERR_INVALID, "stride < 1");
    if (initial_units < 0 || initial_units > 1 << 20) return ctx->fail(VISMA_ICP_ERR_INVALID, "initial_units outside 0 .. 2^20");
    if (ctx->sharded() || ctx->eng->is_sharded()) return ctx->fail(VISMA_ICP_ERR_INVALID, "TSDF integration runs on one rank");
    std::unique_ptr<visma_icp_tsdf> v(new visma_icp_tsdf);
    v->cfg.scalable = 1;
    v->cfg.resolution = volume_unit_resolution; v->cfg.voxel_length = voxel_length;
    v->cfg.length = voxel_length * volume_unit_resolution;           // volume_unit_length_
    v->cfg.sdf_trunc = sdf_trunc; v->cfg.color_type = color_type;
    v->cfg.stride = depth_sampling_stride;
    v->cfg.initial_units = initial_units > 0 ? initial_units : 256;
    int rc = ctx->eng->tsdf_create(v->cfg, &v->id);
    if (rc) return ctx->eng_fail(rc);
    *out = v.get();
    ctx->volumes.push_back(std::move(v));
    return VISMA_ICP_OK;
}

int visma_icp_tsdf_get_units(visma_icp_ctx *ctx, visma_icp_tsdf *volume, int32_t *indices, int64_t capacity, int64_t *out_n)
{
    CTX_CHECK();
    if (int rc = check_tsdf_volume(ctx, volume)) return rc;
    if (!out_n) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    *out_n = 0;
    if (!volume->cfg.scalable) return ctx->fail(VISMA_ICP_ERR_INVALID, "a uniform volume has no units");
    std::vector<int32_t> keys;
    int rc = ctx->eng->tsdf_get_units(volume->id, &keys);
    if (rc) return ctx->eng_fail(rc);
    *out_n = (int64_t)(keys.size() / 3);
    if (!indices) return VISMA_ICP_OK;
    if (capacity < *out_n) return ctx->fail(VISMA_ICP_ERR_INVALID, "capacity below the number of units");
    std::copy(keys.begin(), keys.end(), indices);
    return VISMA_ICP_OK;
}

int visma_icp_tsdf_destroy(visma_icp_ctx *ctx, visma_icp_tsdf *volume)
{
    CTX_CHECK();
    if (int rc = check_tsdf_volume(ctx, volume)) return rc;
    int rc = ctx->eng->tsdf_destroy(volume->id);
    for (size_t i = 0; i < ctx->volumes.size(); i++)
        if (ctx->volumes[i].get() == volume) { ctx->volumes.erase(ctx->volumes.begin() + (std::ptrdiff_t)i); break; }
    return rc ? ctx->eng_fail(rc) : VISMA_ICP_OK;
}

int visma_icp_tsdf_reset(visma_icp_ctx *ctx, visma_icp_tsdf *volume)
{
    CTX_CHECK();
    if (int rc = check_tsdf_volume(ctx, volume)) return rc;
    volume->rows[0] = volume->rows[1] = -1;
    volume->mesh_rows[0] = volume->mesh_rows[1] = -1;
    int rc = ctx->eng->tsdf_reset(volume->id);
    return rc ? ctx->eng_fail(rc) : VISMA_ICP_OK;
}

int visma_icp_tsdf_integrate(visma_icp_ctx *ctx, visma_icp_tsdf *volume, int w, int h, const float *depth, const void *color,
                             const double intrinsic[4], int intrinsic_w, int intrinsic_h, const double extrinsic[16])
{
    CTX_CHECK();
    if (int rc = check_tsdf_volume(ctx, volume)) return rc;
    if (!extrinsic) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL argument");
    TsdfFrame f;
    if (int rc = check_tsdf_frame(ctx, w, h, depth, color, volume->cfg.color_type, intrinsic, intrinsic_w, intrinsic_h, extrinsic, &f))
        return rc;
    volume->rows[0] = volume->rows[1] = -1;
    volume->mesh_rows[0] = volume->mesh_rows[1] = -1;
    int rc = ctx->eng->tsdf_integrate(volume->id, f);
    return rc ? ctx->eng_fail(rc) : VISMA_ICP_OK;
}

// Integrate of resident images: the depth 1 x float, the colour what the volume's colour type takes (RGB8: 3 x uint8,
// Gray32: 1 x float; a volume without colour reads none).  Anything else: INVALID before the volume is touched.
int visma_icp_tsdf_integrate_images(visma_icp_ctx *ctx, visma_icp_tsdf *volume, visma_icp_image *depth, visma_icp_image *color,
                                    const double intrinsic[4], int intrinsic_w, int intrinsic_h, const double extrinsic[16])
{
    CTX_CHECK();
    if (int rc = check_tsdf_volume(ctx, volume)) return rc;
    if (!extrinsic || !depth) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL argument");
    if (!ctx->owns(depth) || (color && !ctx->owns(color))) return ctx->fail(VISMA_ICP_ERR_INVALID, "not an image of this context");
    int w, h, ch, bpc;
    image_device_info(depth->dev, &w, &h, &ch, &bpc);
    if (ch != 1 || bpc != 4 || image_device_is_integer(depth->dev)) return ctx->fail(VISMA_ICP_ERR_INVALID, "the depth is a 1 x float image");
    const int ct = volume->cfg.color_type;
    const void *color_px = nullptr;
    if (ct != kTsdfColorNone) {
        if (!color) return ctx->fail(VISMA_ICP_ERR_INVALID, "no colour image for a coloured volume");
        int cw, chh, cch, cb;
        image_device_info(color->dev, &cw, &chh, &cch, &cb);
        if (cw != w || chh != h) return ctx->fail(VISMA_ICP_ERR_INVALID, "the colour image differs in size from the depth");
        if (ct == kTsdfColorRgb8 ? (cch != 3 || cb != 1) : (cch != 1 || cb != 4))
            return ctx->fail(VISMA_ICP_ERR_INVALID, "the colour image is not of the volume's colour type");
        color_px = image_device_pixels(color->dev);
    }
    TsdfFrame f;
    if (int rc = check_tsdf_frame(ctx, w, h, static_cast<const float *>(image_device_pixels(depth->dev)), color_px, ct, intrinsic,
                                  intrinsic_w, intrinsic_h, extrinsic, &f))
        return rc;
    f.on_device = true;
    volume->rows[0] = volume->rows[1] = -1;
    volume->mesh_rows[0] = volume->mesh_rows[1] = -1;
    int rc = ctx->eng->tsdf_integrate(volume->id, f);
    return rc ? ctx->eng_fail(rc) : VISMA_ICP_OK;
}

static int tsdf_extract(visma_icp_ctx *ctx, visma_icp_tsdf *volume, int voxel_cloud, int64_t *out_n)
{
    if (int rc = check_tsdf_volume(ctx, volume)) return rc;
    if (!out_n) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    volume->rows[voxel_cloud] = -1;
    int rc = ctx->eng->tsdf_extract(volume->id, voxel_cloud, out_n);
    if (rc) return ctx->eng_fail(rc);
    volume->rows[voxel_cloud] = *out_n;
    return VISMA_ICP_OK;
}

static int tsdf_get_extract(visma_icp_ctx *ctx, visma_icp_tsdf *volume, int voxel_cloud, double *points, double *normals,
                            double *colors, int64_t n)
{
    if (int rc = check_tsdf_volume(ctx, volume)) return rc;
    if (volume->rows[voxel_cloud] < 0) return ctx->fail(VISMA_ICP_ERR_STATE, "no extraction: extract first");
    if (n != volume->rows[voxel_cloud]) return ctx->fail(VISMA_ICP_ERR_INVALID, "n differs from the extraction's row count");
    int rc = ctx->eng->tsdf_get_extract(volume->id, voxel_cloud, points, normals, colors);
    return rc ? ctx->eng_fail(rc) : VISMA_ICP_OK;
}

int visma_icp_tsdf_extract_point_cloud(visma_icp_ctx *ctx, visma_icp_tsdf *volume, int64_t *out_n)
{
    CTX_CHECK();
    return tsdf_extract(ctx, volume, 0, out_n);
}

int visma_icp_tsdf_get_point_cloud(visma_icp_ctx *ctx, visma_icp_tsdf *volume, double *points, double *normals, double *colors,
                                   int64_t n)
{
    CTX_CHECK();
    return tsdf_get_extract(ctx, volume, 0, points, normals, colors, n);
}

int visma_icp_tsdf_extract_voxel_point_cloud(visma_icp_ctx *ctx, visma_icp_tsdf *volume, int64_t *out_n)
{
    CTX_CHECK();
    return tsdf_extract(ctx, volume, 1, out_n);
}

int visma_icp_tsdf_get_voxel_point_cloud(visma_icp_ctx *ctx, visma_icp_tsdf *volume, double *points, double *colors, int64_t n)
{
    CTX_CHECK();
    return tsdf_get_extract(ctx, volume, 1, points, nullptr, colors, n);
}

int visma_icp_tsdf_extract_triangle_mesh(visma_icp_ctx *ctx, visma_icp_tsdf *volume, int64_t *out_nv, int64_t *out_nt)
{
    CTX_CHECK();
    if (int rc = check_tsdf_volume(ctx, volume)) return rc;
    if (!out_nv || !out_nt) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    *out_nv = *out_nt = 0;
    if (ctx->sharded() || ctx->eng->is_sharded()) return ctx->fail(VISMA_ICP_ERR_INVALID, "TSDF integration runs on one rank");
    volume->mesh_rows[0] = volume->mesh_rows[1] = -1;
    int rc = ctx->eng->tsdf_extract_mesh(volume->id, out_nv, out_nt);
    if (rc) return ctx->eng_fail(rc);
    volume->mesh_rows[0] = *out_nv; volume->mesh_rows[1] = *out_nt;
    return VISMA_ICP_OK;
}

int visma_icp_tsdf_get_triangle_mesh(visma_icp_ctx *ctx, visma_icp_tsdf *volume, double *vertices, double *colors, int32_t *triangles,
                                     int64_t nv, int64_t nt)
{
    CTX_CHECK();
    if (int rc = check_tsdf_volume(ctx, volume)) return rc;
    if (ctx->sharded() || ctx->eng->is_sharded()) return ctx->fail(VISMA_ICP_ERR_INVALID, "TSDF integration runs on one rank");
    if (volume->mesh_rows[0] < 0) return ctx->fail(VISMA_ICP_ERR_STATE, "no mesh: extract first");
    if (nv != volume->mesh_rows[0] || nt != volume->mesh_rows[1])
        return ctx->fail(VISMA_ICP_ERR_INVALID, "nv or nt differs from the extraction's counts");
    int rc = ctx->eng->tsdf_get_mesh(volume->id, vertices, colors, triangles);
    return rc ? ctx->eng_fail(rc) : VISMA_ICP_OK;
}

int visma_icp_tsdf_get_volume(visma_icp_ctx *ctx, visma_icp_tsdf *volume, const int32_t unit_index[3], float *tsdf, float *weight,
                              float *color)
{
    CTX_CHECK();
    if (int rc = check_tsdf_volume(ctx, volume)) return rc;
    if (volume->cfg.scalable && !unit_index) return ctx->fail(VISMA_ICP_ERR_INVALID, "a scalable volume is read unit by unit: no unit index");
    if (!volume->cfg.scalable && unit_index) return ctx->fail(VISMA_ICP_ERR_INVALID, "a uniform volume has no units");
    int rc = ctx->eng->tsdf_get_volume(volume->id, unit_index, tsdf, weight, color);
    return rc ? ctx->eng_fail(rc) : VISMA_ICP_OK;
}

static int point_cloud_from_frame(visma_icp_ctx *ctx, int w, int h, const float *depth, const void *color, int color_type,
                                  const double *intrinsic, const double *extrinsic, int stride, double *points, double *colors,
                                  int64_t capacity, int64_t *out_n)
{
    if (!out_n) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    *out_n = 0;
    if (stride < 1) return ctx->fail(VISMA_ICP_ERR_INVALID, "stride < 1");
    TsdfFrame f;
    if (int rc = check_tsdf_frame(ctx, w, h, depth, color, color_type, intrinsic, w, h, extrinsic, &f)) return rc;
    const int64_t most = (((int64_t)w - 1) / stride + 1) * (((int64_t)h - 1) / stride + 1);   // (in 64 bits: stride may be INT_MAX)
    if (points && capacity < most) return ctx->fail(VISMA_ICP_ERR_INVALID, "capacity below ceil(w / stride) * ceil(h / stride)");
    int rc = ctx->eng->point_cloud_from_depth(f, color_type, stride, points, points ? colors : nullptr, out_n, nullptr);
    return rc ? ctx->eng_fail(rc) : VISMA_ICP_OK;
}

// CreatePointCloudFromDepthImage / FromRGBDImage of resident images into a resident cloud.  depth: the float pixels on the
// device; color (may be NULL) with its colour type
static int cloud_from_images(visma_icp_ctx *ctx, int w, int h, const float *depth, const void *color, int color_type, const double *intrinsic,
                             const double *extrinsic, int stride, visma_icp_cloud **out)
{
    TsdfFrame f;
    if (int rc = check_tsdf_frame(ctx, w, h, depth, color, color_type, intrinsic, w, h, extrinsic, &f)) return rc;
    f.on_device = true;
    int64_t n = 0;
    CloudDevice *dev = nullptr;
    if (int rc = ctx->eng->point_cloud_from_depth(f, color_type, stride, nullptr, nullptr, &n, &dev)) return ctx->eng_fail(rc);
    *out = ctx->adopt(dev);
    return VISMA_ICP_OK;
}

static int empty_cloud(visma_icp_ctx *ctx, visma_icp_cloud **out)
{
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    CloudDevice *dev = nullptr;
    const hipError_t e = cloud_device_create(nullptr, 0, nullptr, nullptr, false, ctx->eng->aux_stream(), &dev);
    if (e != hipSuccess) { (void)hipGetLastError(); return ctx->fail(VISMA_ICP_ERR_HIP, hipGetErrorString(e)); }
    *out = ctx->adopt(dev);
    return VISMA_ICP_OK;
}

static int cloud_from_images_enter(visma_icp_ctx *ctx, visma_icp_image *depth, visma_icp_image *color, const double *intrinsic, visma_icp_cloud **out)
{
    if (!out) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    *out = nullptr;
    if (!depth || !intrinsic) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL argument");
    if (!ctx->owns(depth) || (color && !ctx->owns(color))) return ctx->fail(VISMA_ICP_ERR_INVALID, "not an image of this context");
    if (ctx->sharded() || ctx->eng->is_sharded()) return ctx->fail(VISMA_ICP_ERR_INVALID, "a point cloud lives on one rank");
    if (!ctx->eng->supports_device_loop()) return ctx->fail(VISMA_ICP_ERR_STATE, "a point cloud needs the HIP engine");
    return VISMA_ICP_OK;
}

int visma_icp_cloud_from_depth_image(visma_icp_ctx *ctx, visma_icp_image *depth, const double intrinsic[4], const double extrinsic[16],
                                     double depth_scale, double depth_trunc, int stride, visma_icp_cloud **out)
{
    CTX_CHECK();
    if (int rc = cloud_from_images_enter(ctx, depth, nullptr, intrinsic, out)) return rc;
    if (stride < 1) return ctx->fail(VISMA_ICP_ERR_INVALID, "stride < 1");
    int w, h, ch, bpc;
    image_device_info(depth->dev, &w, &h, &ch, &bpc);
    if (ch != 1 || (bpc != 2 && bpc != 4) || image_device_is_integer(depth->dev) || w < 1 || h < 1) return empty_cloud(ctx, out);      // unsupported format: the empty cloud
    if (bpc == 4)
        return cloud_from_images(ctx, w, h, static_cast<const float *>(image_device_pixels(depth->dev)), nullptr, kTsdfColorNone, intrinsic,
                                 extrinsic, stride, out);
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    ImageDevice *metres = nullptr;                           // ConvertDepthToFloatImage first, as the reference does
    const hipError_t e = image_device_depth_to_float(depth->dev, depth_scale, depth_trunc, ctx->eng->aux_stream(), &metres);
    if (e != hipSuccess) { (void)hipGetLastError(); return ctx->fail(VISMA_ICP_ERR_HIP, hipGetErrorString(e)); }
    const int rc = cloud_from_images(ctx, w, h, static_cast<const float *>(image_device_pixels(metres)), nullptr, kTsdfColorNone, intrinsic,
                                     extrinsic, stride, out);
    image_device_destroy(metres);
    return rc;
}

int visma_icp_cloud_from_rgbd_images(visma_icp_ctx *ctx, visma_icp_image *depth, visma_icp_image *color, const double intrinsic[4],
                                     const double extrinsic[16], visma_icp_cloud **out)
{
    CTX_CHECK();
    if (int rc = cloud_from_images_enter(ctx, depth, color, intrinsic, out)) return rc;
    if (!color) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL argument");
    int w, h, ch, bpc, cw, chh, cch, cb;
    image_device_info(depth->dev, &w, &h, &ch, &bpc);
    image_device_info(color->dev, &cw, &chh, &cch, &cb);
    const int color_type = cch == 3 && cb == 1 ? kTsdfColorRgb8 : cch == 1 && cb == 4 ? kTsdfColorGray32 : kTsdfColorNone;
    if (ch != 1 || bpc != 4 || image_device_is_integer(depth->dev) || color_type == kTsdfColorNone || w < 1 || h < 1) return empty_cloud(ctx, out);
    if (cw != w || chh != h) return ctx->fail(VISMA_ICP_ERR_INVALID, "the colour image differs in size from the depth");
    return cloud_from_images(ctx, w, h, static_cast<const float *>(image_device_pixels(depth->dev)), image_device_pixels(color->dev), color_type,
                             intrinsic, extrinsic, 1, out);
}

int visma_icp_point_cloud_from_depth(visma_icp_ctx *ctx, int w, int h, const float *depth, const double intrinsic[4],
                                     const double extrinsic[16], int stride, double *points, int64_t capacity, int64_t *out_n)
{
    CTX_CHECK();
    return point_cloud_from_frame(ctx, w, h, depth, nullptr, kTsdfColorNone, intrinsic, extrinsic, stride, points, nullptr, capacity, out_n);
}

int visma_icp_point_cloud_from_rgbd(visma_icp_ctx *ctx, int w, int h, const float *depth, const void *color, int color_type,
                                    const double intrinsic[4], const double extrinsic[16], double *points, double *colors,
                                    int64_t capacity, int64_t *out_n)
{
    CTX_CHECK();
    if (color_type != kTsdfColorRgb8 && color_type != kTsdfColorGray32) return ctx->fail(VISMA_ICP_ERR_INVALID, "unknown colour type");
    return point_cloud_from_frame(ctx, w, h, depth, color, color_type, intrinsic, extrinsic, 1, points, colors, capacity, out_n);
}

// ---- color map optimization (colormap.hip) --------------------------------------------------------------------------------
void visma_icp_color_map_option_default(visma_icp_color_map_option *o)
{
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->number_of_vertical_anchors = 16;
    o->non_rigid_anchor_point_weight = 0.316;
    o->maximum_iteration = 300.0;
    o->maximum_allowable_depth = 2.5;
    o->depth_threshold_for_visiblity_check = 0.03;
    o->depth_threshold_for_discontinuity_check = 0.1;
    o->half_dilation_kernel_size_for_discontinuity_map = 3;
}

// every argument check of a color map call, before anything reaches a device; stage 0: created, 1: prepared
static int check_color_map(visma_icp_ctx *ctx, visma_icp_color_map *map, int stage)
{
    if (!map) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL color map");
    for (const auto &m : ctx->color_maps)
        if (m.get() == map) {
            if (stage > 0 && !map->prepared) return ctx->fail(VISMA_ICP_ERR_INVALID, "the color map is not prepared: set the images and the vertices, then prepare");
            return VISMA_ICP_OK;
        }
    return ctx->fail(VISMA_ICP_ERR_INVALID, "not a color map of this context");
}

static int check_color_map_option(visma_icp_ctx *ctx, const visma_icp_color_map_option &o, bool non_rigid)
{
    if (!non_rigid && o.non_rigid_camera_coordinate) return ctx->fail(VISMA_ICP_ERR_INVALID, "non_rigid_camera_coordinate is set: the non-rigid optimization has entry points of its own, visma_icp_color_map_create_non_rigid and visma_icp_color_map_optimization_non_rigid");
    if (std::isnan(o.maximum_iteration) || std::isnan(o.maximum_allowable_depth) || std::isnan(o.depth_threshold_for_visiblity_check) ||
        std::isnan(o.depth_threshold_for_discontinuity_check))
        return ctx->fail(VISMA_ICP_ERR_INVALID, "an option that is not a number");
    if (o.half_dilation_kernel_size_for_discontinuity_map < 0 || o.half_dilation_kernel_size_for_discontinuity_map > 64)
        return ctx->fail(VISMA_ICP_ERR_INVALID, "half_dilation_kernel_size_for_discontinuity_map outside 0 .. 64");
    return VISMA_ICP_OK;
}

#define COLOR_MAP_CALL(map, expr)                                                                           \
    do {                                                                                                    \
        int rc__ = ctx->eng->color_map_call((map)->id, [&](ColorMapDevice *D) -> hipError_t { return (expr); }); \
        if (rc__) return ctx->eng_fail(rc__);                                                               \
    } while (0)

// create and create_non_rigid
static int color_map_create(visma_icp_ctx *ctx, int w, int h, int n_images, const double intrinsic[4],
                            const visma_icp_color_map_option *option, bool non_rigid, visma_icp_color_map **out)
{
    if (!out) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    *out = nullptr;
    if (!intrinsic) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL argument");
    if (n_images < 1) return ctx->fail(VISMA_ICP_ERR_INVALID, "n_images < 1");
    if (w <= 20 || h <= 20) return ctx->fail(VISMA_ICP_ERR_INVALID, "w and h must be above 20: the 10-pixel margin leaves no interior");
    if ((int64_t)w * h > (int64_t)1 << 26 || (int64_t)w * h * n_images > (int64_t)1 << 30)
        return ctx->fail(VISMA_ICP_ERR_INVALID, "images of more than 2^30 pixels in all");
    for (int k = 0; k < 4; k++)
        if (!std::isfinite(intrinsic[k])) return ctx->fail(VISMA_ICP_ERR_INVALID, "an intrinsic that is not finite");
    if (intrinsic[0] == 0.0 || intrinsic[1] == 0.0) return ctx->fail(VISMA_ICP_ERR_INVALID, "a focal length that is zero");
    visma_icp_color_map_option o;
    visma_icp_color_map_option_default(&o);
    if (option) o = *option;
    if (int rc = check_color_map_option(ctx, o, non_rigid)) return rc;
    int aw = 0, ah = 0;
    double step = 0.0;
    if (non_rigid) {                                     // (the flag field is not read: these entry points ARE the flag)
        if (o.number_of_vertical_anchors < 2 || o.number_of_vertical_anchors > 64)
            return ctx->fail(VISMA_ICP_ERR_INVALID, "number_of_vertical_anchors outside 2 .. 64");
        cm_warp_shape(w, h, o.number_of_vertical_anchors, &aw, &ah, &step);
        if ((int64_t)aw * ah > kCmWarpMaxAnchors) return ctx->fail(VISMA_ICP_ERR_INVALID, "more than 8192 anchors per image");
        if (!std::isfinite(o.non_rigid_anchor_point_weight) || o.non_rigid_anchor_point_weight < 0.0)
            return ctx->fail(VISMA_ICP_ERR_INVALID, "non_rigid_anchor_point_weight must be finite and not negative");
    }
    if (ctx->sharded() || ctx->eng->is_sharded()) return ctx->fail(VISMA_ICP_ERR_INVALID, "color map optimization runs on one rank");
    std::unique_ptr<visma_icp_color_map> m(new visma_icp_color_map);
    m->cfg.w = w; m->cfg.h = h; m->cfg.n_images = n_images;
    m->cfg.fx = intrinsic[0]; m->cfg.fy = intrinsic[1]; m->cfg.cx = intrinsic[2]; m->cfg.cy = intrinsic[3];
    m->cfg.max_depth = o.maximum_allowable_depth; m->cfg.visibility_threshold = o.depth_threshold_for_visiblity_check;
    m->cfg.discontinuity_threshold = o.depth_threshold_for_discontinuity_check;
    m->cfg.half_dilation = o.half_dilation_kernel_size_for_discontinuity_map;
    m->iterations = o.maximum_iteration > 0.0 ? (o.maximum_iteration < 1e9 ? (int)std::ceil(o.maximum_iteration) : 1000000000) : 0;
    m->image_set.assign((size_t)n_images, 0);
    if (non_rigid) {
        m->non_rigid = true; m->anchor_w = aw; m->anchor_h = ah; m->anchor_step = step;
        m->cfg.anchors = o.number_of_vertical_anchors; m->cfg.anchor_weight = o.non_rigid_anchor_point_weight;
    }
    int rc = ctx->eng->color_map_create(m->cfg, &m->id);
    if (rc) return ctx->eng_fail(rc);
    *out = m.get();
    ctx->color_maps.push_back(std::move(m));
    return VISMA_ICP_OK;
}

int visma_icp_color_map_create(visma_icp_ctx *ctx, int w, int h, int n_images, const double intrinsic[4],
                               const visma_icp_color_map_option *option, visma_icp_color_map **out)
{
    CTX_CHECK();
    return color_map_create(ctx, w, h, n_images, intrinsic, option, false, out);
}

int visma_icp_color_map_create_non_rigid(visma_icp_ctx *ctx, int w, int h, int n_images, const double intrinsic[4],
                                         const visma_icp_color_map_option *option, visma_icp_color_map **out)
{
    CTX_CHECK();
    return color_map_create(ctx, w, h, n_images, intrinsic, option, true, out);
}

int visma_icp_color_map_destroy(visma_icp_ctx *ctx, visma_icp_color_map *map)
{
    CTX_CHECK();
    if (int rc = check_color_map(ctx, map, 0)) return rc;
    int rc = ctx->eng->color_map_destroy(map->id);
    for (size_t i = 0; i < ctx->color_maps.size(); i++)
        if (ctx->color_maps[i].get() == map) { ctx->color_maps.erase(ctx->color_maps.begin() + (std::ptrdiff_t)i); break; }
    return rc ? ctx->eng_fail(rc) : VISMA_ICP_OK;
}

int visma_icp_color_map_set_image(visma_icp_ctx *ctx, visma_icp_color_map *map, int i, const float *depth, const uint8_t *color,
                                  int color_channels, const double extrinsic[16])
{
    CTX_CHECK();
    if (int rc = check_color_map(ctx, map, 0)) return rc;
    if (!depth || !color || !extrinsic) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL argument");
    if (color_channels != 3) return ctx->fail(VISMA_ICP_ERR_INVALID, "the colour image must be RGB8: 3 channels of uint8");
    if (i < 0 || i >= map->cfg.n_images) return ctx->fail(VISMA_ICP_ERR_INVALID, "image index out of range");
    map->prepared = false;
    map->image_set[(size_t)i] = 0;
    COLOR_MAP_CALL(map, color_map_device_set_image(D, i, depth, color, extrinsic));
    map->image_set[(size_t)i] = 1;
    return VISMA_ICP_OK;
}

int visma_icp_color_map_set_vertices(visma_icp_ctx *ctx, visma_icp_color_map *map, const double *vertices, int64_t n)
{
    CTX_CHECK();
    if (int rc = check_color_map(ctx, map, 0)) return rc;
    if (!vertices) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL argument");
    if (n < 1) return ctx->fail(VISMA_ICP_ERR_INVALID, "no vertices");
    // (vertex ids are int32, as the reference's; the compaction walks n_images lists of them)
    if (n > (int64_t)1 << 30 || (n + 256) * map->cfg.n_images > (int64_t)1 << 36) return ctx->fail(VISMA_ICP_ERR_INVALID, "too many vertices");
    map->prepared = false;
    map->n_vertices = -1;
    COLOR_MAP_CALL(map, color_map_device_set_vertices(D, vertices, n));
    map->n_vertices = n;
    return VISMA_ICP_OK;
}

int visma_icp_color_map_prepare(visma_icp_ctx *ctx, visma_icp_color_map *map, int64_t *visible_counts)
{
    CTX_CHECK();
    if (int rc = check_color_map(ctx, map, 0)) return rc;
    for (char s : map->image_set)
        if (!s) return ctx->fail(VISMA_ICP_ERR_INVALID, "an image is not set");
    if (map->n_vertices < 0) return ctx->fail(VISMA_ICP_ERR_INVALID, "the vertices are not set");
    map->prepared = false;
    std::vector<int64_t> counts((size_t)map->cfg.n_images);
    COLOR_MAP_CALL(map, color_map_device_prepare(D, counts.data()));
    if (visible_counts) std::copy(counts.begin(), counts.end(), visible_counts);
    map->prepared = true;
    return VISMA_ICP_OK;
}

int visma_icp_color_map_get_image(visma_icp_ctx *ctx, visma_icp_color_map *map, int i, int which, void *out)
{
    CTX_CHECK();
    if (int rc = check_color_map(ctx, map, 1)) return rc;
    if (!out) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    if (i < 0 || i >= map->cfg.n_images) return ctx->fail(VISMA_ICP_ERR_INVALID, "image index out of range");
    if (which < VISMA_ICP_COLOR_MAP_GRAY || which > VISMA_ICP_COLOR_MAP_MASK) return ctx->fail(VISMA_ICP_ERR_INVALID, "unknown image");
    COLOR_MAP_CALL(map, color_map_device_get_image(D, i, which, out));
    return VISMA_ICP_OK;
}

int visma_icp_color_map_get_visible(visma_icp_ctx *ctx, visma_icp_color_map *map, int i, int32_t *indices, int64_t capacity,
                                    int64_t *out_n)
{
    CTX_CHECK();
    if (int rc = check_color_map(ctx, map, 1)) return rc;
    if (!out_n) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    *out_n = 0;
    if (i < 0 || i >= map->cfg.n_images) return ctx->fail(VISMA_ICP_ERR_INVALID, "image index out of range");
    COLOR_MAP_CALL(map, (*out_n = color_map_device_visible_count(D, i), hipSuccess));
    if (!indices) return VISMA_ICP_OK;
    if (capacity < *out_n) return ctx->fail(VISMA_ICP_ERR_INVALID, "capacity below the number of visible vertices");
    COLOR_MAP_CALL(map, color_map_device_get_visible(D, i, indices));
    return VISMA_ICP_OK;
}

int visma_icp_color_map_get_proxy(visma_icp_ctx *ctx, visma_icp_color_map *map, double *proxy, int64_t n)
{
    CTX_CHECK();
    if (int rc = check_color_map(ctx, map, 1)) return rc;
    if (!proxy) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    if (n != map->n_vertices) return ctx->fail(VISMA_ICP_ERR_INVALID, "n differs from the vertex count");
    COLOR_MAP_CALL(map, color_map_device_get_proxy(D, proxy));
    return VISMA_ICP_OK;
}

int visma_icp_color_map_sums(visma_icp_ctx *ctx, visma_icp_color_map *map, double *sums)
{
    CTX_CHECK();
    if (int rc = check_color_map(ctx, map, 1)) return rc;
    if (!sums) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    if (map->non_rigid) return ctx->fail(VISMA_ICP_ERR_INVALID, "a non-rigid color map has cell sums: visma_icp_color_map_cell_sums");
    COLOR_MAP_CALL(map, color_map_device_sums(D, sums));
    return VISMA_ICP_OK;
}

int visma_icp_color_map_step(visma_icp_ctx *ctx, visma_icp_color_map *map, double *rr, int64_t *count)
{
    CTX_CHECK();
    if (int rc = check_color_map(ctx, map, 1)) return rc;
    if (!rr || !count) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    if (map->non_rigid) {
        std::vector<double> reg((size_t)map->cfg.n_images);
        COLOR_MAP_CALL(map, color_map_device_step_non_rigid(D, rr, reg.data(), count));
        return VISMA_ICP_OK;
    }
    COLOR_MAP_CALL(map, color_map_device_step(D, rr, count));
    return VISMA_ICP_OK;
}

// the calls of a non-rigid map alone
static int check_non_rigid(visma_icp_ctx *ctx, visma_icp_color_map *map, int stage)
{
    if (int rc = check_color_map(ctx, map, stage)) return rc;
    if (!map->non_rigid) return ctx->fail(VISMA_ICP_ERR_INVALID, "not a non-rigid color map (visma_icp_color_map_create_non_rigid makes one)");
    return VISMA_ICP_OK;
}

int visma_icp_color_map_get_anchor_shape(visma_icp_ctx *ctx, visma_icp_color_map *map, int *anchor_w, int *anchor_h, double *anchor_step)
{
    CTX_CHECK();
    if (int rc = check_non_rigid(ctx, map, 0)) return rc;
    if (anchor_w) *anchor_w = map->anchor_w;
    if (anchor_h) *anchor_h = map->anchor_h;
    if (anchor_step) *anchor_step = map->anchor_step;
    return VISMA_ICP_OK;
}

int visma_icp_color_map_get_flow(visma_icp_ctx *ctx, visma_icp_color_map *map, double *flow)
{
    CTX_CHECK();
    if (int rc = check_non_rigid(ctx, map, 0)) return rc;
    if (!flow) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    COLOR_MAP_CALL(map, color_map_device_get_flow(D, flow));
    return VISMA_ICP_OK;
}

int visma_icp_color_map_set_flow(visma_icp_ctx *ctx, visma_icp_color_map *map, const double *flow)
{
    CTX_CHECK();
    if (int rc = check_non_rigid(ctx, map, 0)) return rc;
    if (!flow) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL argument");
    COLOR_MAP_CALL(map, color_map_device_set_flow(D, flow));
    return VISMA_ICP_OK;
}

int visma_icp_color_map_cell_sums(visma_icp_ctx *ctx, visma_icp_color_map *map, double *sums)
{
    CTX_CHECK();
    if (int rc = check_non_rigid(ctx, map, 1)) return rc;
    if (!sums) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    COLOR_MAP_CALL(map, color_map_device_cell_sums(D, sums));
    return VISMA_ICP_OK;
}

int visma_icp_color_map_step_non_rigid(visma_icp_ctx *ctx, visma_icp_color_map *map, double *rr, double *rr_reg, int64_t *count)
{
    CTX_CHECK();
    if (int rc = check_non_rigid(ctx, map, 1)) return rc;
    if (!rr || !rr_reg || !count) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    COLOR_MAP_CALL(map, color_map_device_step_non_rigid(D, rr, rr_reg, count));
    return VISMA_ICP_OK;
}

int visma_icp_color_map_solve_non_rigid(int anchor_w, int anchor_h, const double *cell_sums, int64_t n_vertex, double weight_option,
                                        const double *flow, const double *flow_init, double *x, double *rr_reg, int *kept)
{
    if (anchor_w < 2 || anchor_h < 2 || (int64_t)anchor_w * anchor_h > kCmWarpMaxAnchors) return VISMA_ICP_ERR_INVALID;
    if (!cell_sums || !flow || !flow_init || !x || n_vertex < 1) return VISMA_ICP_ERR_INVALID;
    if (!std::isfinite(weight_option) || weight_option < 0.0) return VISMA_ICP_ERR_INVALID;
    double rr = 0.0, reg = 0.0;
    int64_t count = 0;
    const bool moved = cm_warp_solve_camera(anchor_w, anchor_h, cell_sums, (double)n_vertex, weight_option, flow, flow_init, x, &rr, &reg, &count);
    if (rr_reg) *rr_reg = reg;
    if (kept) *kept = moved ? 0 : 1;
    return VISMA_ICP_OK;
}

int visma_icp_color_map_run(visma_icp_ctx *ctx, visma_icp_color_map *map, int k, double *residual)
{
    CTX_CHECK();
    if (int rc = check_color_map(ctx, map, 1)) return rc;
    if (k < 0) k = map->iterations;
    const size_t n = (size_t)map->cfg.n_images;
    std::vector<double> rr(n);
    std::vector<int64_t> count(n);
    for (int it = 0; it < k; it++) {
        if (map->non_rigid) {
            std::vector<double> reg(n);
            COLOR_MAP_CALL(map, color_map_device_step_non_rigid(D, rr.data(), reg.data(), count.data()));
        } else {
            COLOR_MAP_CALL(map, color_map_device_step(D, rr.data(), count.data()));
        }
        if (residual) {
            double s = 0.0;
            for (double v : rr) s += v;
            residual[it] = s;
        }
    }
    return VISMA_ICP_OK;
}

int visma_icp_color_map_get_extrinsics(visma_icp_ctx *ctx, visma_icp_color_map *map, double *extrinsics)
{
    CTX_CHECK();
    if (int rc = check_color_map(ctx, map, 0)) return rc;
    if (!extrinsics) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    for (char s : map->image_set)
        if (!s) return ctx->fail(VISMA_ICP_ERR_INVALID, "an image is not set");
    COLOR_MAP_CALL(map, (color_map_device_get_extrinsics(D, extrinsics), hipSuccess));
    return VISMA_ICP_OK;
}

int visma_icp_color_map_set_extrinsics(visma_icp_ctx *ctx, visma_icp_color_map *map, const double *extrinsics)
{
    CTX_CHECK();
    if (int rc = check_color_map(ctx, map, 0)) return rc;
    if (!extrinsics) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL argument");
    COLOR_MAP_CALL(map, color_map_device_set_extrinsics(D, extrinsics));
    return VISMA_ICP_OK;
}

int visma_icp_color_map_get_colors(visma_icp_ctx *ctx, visma_icp_color_map *map, double *colors, int64_t n)
{
    CTX_CHECK();
    if (int rc = check_color_map(ctx, map, 1)) return rc;
    if (!colors) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    if (n != map->n_vertices) return ctx->fail(VISMA_ICP_ERR_INVALID, "n differs from the vertex count");
    COLOR_MAP_CALL(map, color_map_device_get_colors(D, colors));
    return VISMA_ICP_OK;
}

// optimization and optimization_non_rigid
static int color_map_optimization(visma_icp_ctx *ctx, int w, int h, int n_images, const double intrinsic[4], const float *depth,
                                  const uint8_t *color, double *extrinsics, const double *vertices, int64_t n,
                                  const visma_icp_color_map_option *option, double *colors, bool non_rigid, double *flow)
{
    if (!depth || !color || !extrinsics || !vertices || !colors) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL argument");
    if (n < 1) return ctx->fail(VISMA_ICP_ERR_INVALID, "no vertices");
    visma_icp_color_map *map = nullptr;
    int rc = color_map_create(ctx, w, h, n_images, intrinsic, option, non_rigid, &map);
    if (rc) return rc;
    const size_t px = (size_t)w * h;
    for (int i = 0; i < n_images && !rc; i++)
        rc = visma_icp_color_map_set_image(ctx, map, i, depth + (size_t)i * px, color + (size_t)i * px * 3, 3, extrinsics + 16 * (size_t)i);
    if (!rc) rc = visma_icp_color_map_set_vertices(ctx, map, vertices, n);
    if (!rc) rc = visma_icp_color_map_prepare(ctx, map, nullptr);
    if (!rc) rc = visma_icp_color_map_run(ctx, map, -1, nullptr);
    if (!rc) rc = visma_icp_color_map_get_colors(ctx, map, colors, n);
    if (!rc) rc = visma_icp_color_map_get_extrinsics(ctx, map, extrinsics);
    if (!rc && non_rigid && flow) rc = visma_icp_color_map_get_flow(ctx, map, flow);
    const std::string err = ctx->err;
    (void)visma_icp_color_map_destroy(ctx, map);
    if (rc) ctx->err = err;
    return rc;
}

int visma_icp_color_map_optimization(visma_icp_ctx *ctx, int w, int h, int n_images, const double intrinsic[4], const float *depth,
                                     const uint8_t *color, double *extrinsics, const double *vertices, int64_t n,
                                     const visma_icp_color_map_option *option, double *colors)
{
    CTX_CHECK();
    return color_map_optimization(ctx, w, h, n_images, intrinsic, depth, color, extrinsics, vertices, n, option, colors, false, nullptr);
}

int visma_icp_color_map_optimization_non_rigid(visma_icp_ctx *ctx, int w, int h, int n_images, const double intrinsic[4],
                                               const float *depth, const uint8_t *color, double *extrinsics, const double *vertices,
                                               int64_t n, const visma_icp_color_map_option *option, double *colors, double *flow)
{
    CTX_CHECK();
    return color_map_optimization(ctx, w, h, n_images, intrinsic, depth, color, extrinsics, vertices, n, option, colors, true, flow);
}

int visma_icp_set_nn_mode(visma_icp_ctx *ctx, int nn_mode)
{
    CTX_CHECK();
    int rc = ctx->eng->set_nn_mode(nn_mode);
    if (rc) return ctx->eng_fail(rc);
    return VISMA_ICP_OK;
}

int visma_icp_get_nn_mode_used(visma_icp_ctx *ctx, int *nn_mode)
{
    CTX_CHECK();
    if (!nn_mode) return ctx->fail(VISMA_ICP_ERR_INVALID, "nn_mode is NULL");
    *nn_mode = ctx->eng->nn_mode_used();
    return VISMA_ICP_OK;
}

int visma_icp_get_search_kernel_used(visma_icp_ctx *ctx, int *kernel)
{
    CTX_CHECK();
    if (!kernel) return ctx->fail(VISMA_ICP_ERR_INVALID, "kernel is NULL");
    *kernel = ctx->eng->search_kernel_used();
    return VISMA_ICP_OK;
}

int visma_icp_forget_winners(visma_icp_ctx *ctx)
{
    CTX_CHECK();
    int rc = ctx->eng->forget_winners();
    if (rc) return ctx->eng_fail(rc);
    return VISMA_ICP_OK;
}

int visma_icp_set_device_loop(visma_icp_ctx *ctx, int enabled)
{
    CTX_CHECK();
    ctx->loop_mode = enabled < 0 ? 2 : (enabled != 0 ? 1 : 0);
    return VISMA_ICP_OK;
}

int visma_icp_set_persistent(visma_icp_ctx *ctx, int enabled, double timeout_ms)
{
    CTX_CHECK();
    ctx->eng->set_persistent(enabled, timeout_ms);
    return VISMA_ICP_OK;
}

int visma_icp_set_persistent_cu_share(double share)
{
    if (!(share > 0.0) || share > 1.0) return VISMA_ICP_ERR_INVALID;
    persist_cu_share_ref().store(share);
    return VISMA_ICP_OK;
}

int visma_icp_get_persistent_info(visma_icp_ctx *ctx, visma_icp_persistent_info *out)
{
    CTX_CHECK();
    if (!out || out->struct_size < (int)sizeof(visma_icp_persistent_info))
        return ctx->fail(VISMA_ICP_ERR_INVALID, "visma_icp_persistent_info: set struct_size = sizeof(visma_icp_persistent_info)");
    const int sz = out->struct_size;
    std::memset(out, 0, sizeof(*out));
    out->struct_size = sz;
    out->cu_share = 1.0;
    ctx->eng->get_persistent_info(out);
    return VISMA_ICP_OK;
}

int visma_icp_set_ring_search(visma_icp_ctx *ctx, int mode)
{
    CTX_CHECK();
    ctx->eng->set_ring_search(mode);
    return VISMA_ICP_OK;
}

int visma_icp_get_ring_search(visma_icp_ctx *ctx, int *rings, double *cell, double *occupancy)
{
    CTX_CHECK();
    ctx->eng->get_ring_search(rings, cell, occupancy);
    return VISMA_ICP_OK;
}

int visma_icp_get_sweep_info(visma_icp_ctx *ctx, double *launches, double *aborts)
{
    CTX_CHECK();
    ctx->eng->get_sweep_info(launches, aborts);
    return VISMA_ICP_OK;
}

int visma_icp_test_stall_command(visma_icp_ctx *ctx, int nth, double ms)
{
    CTX_CHECK();
    if (nth < 0 || !(ms >= 0.0) || ms > 10000.0) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad stall arguments");
    ctx->eng->stall_command(nth, ms);
    return VISMA_ICP_OK;
}

int visma_icp_set_profiling(visma_icp_ctx *ctx, int enabled)
{
    CTX_CHECK();
    ctx->eng->set_profiling(enabled);
    return VISMA_ICP_OK;
}

int visma_icp_get_timing(visma_icp_ctx *ctx, visma_icp_timing *out, int reset)
{
    CTX_CHECK();
    if (!out) return ctx->fail(VISMA_ICP_ERR_INVALID, "out is NULL");
    ctx->eng->get_timing(out, reset != 0);
    return VISMA_ICP_OK;
}

int visma_icp_get_timing_sized(visma_icp_ctx *ctx, void *out, size_t struct_size, int reset)
{
    CTX_CHECK();
    if (!out) return ctx->fail(VISMA_ICP_ERR_INVALID, "out is NULL");
    visma_icp_timing t;
    ctx->eng->get_timing(&t, reset != 0);
    std::memcpy(out, &t, struct_size < sizeof(t) ? struct_size : sizeof(t));
    return VISMA_ICP_OK;
}

int visma_icp_plan_ring_grid(const float mn[3], const float mx[3], double max_dist, double cell, int dims[3], double *cell_out, int *rings)
{
    if (!mn || !mx) return VISMA_ICP_ERR_INVALID;
    const visma::GridParams g = visma::grid_plan_ring(mn, mx, max_dist, cell, visma::kGridMaxCells);
    if (dims) for (int a = 0; a < 3; a++) dims[a] = g.dim[a];
    if (cell_out) *cell_out = (double)g.h;
    if (rings) *rings = g.ring;
    return VISMA_ICP_OK;
}

int visma_icp_ring_visiting_order(int rings, int capacity, short *dy, short *dz, float *base, int *nrows)
{
    const std::vector<visma::RingRow> rows = visma::ring_visiting_order(rings);
    if (nrows) *nrows = (int)rows.size();
    if (rows.empty()) return VISMA_ICP_ERR_INVALID;
    for (int k = 0; k < (int)rows.size() && k < capacity; k++) {
        if (dy) dy[k] = rows[k].dy;
        if (dz) dz[k] = rows[k].dz;
        if (base) base[k] = rows[k].base;
    }
    return VISMA_ICP_OK;
}

int visma_icp_get_tile_config(int *s_tile, int *t_chunk, int *block)
{
    if (s_tile) *s_tile = kSTile;
    if (t_chunk) *t_chunk = kTChunk;
    if (block) *block = kBlock;
    return VISMA_ICP_OK;
}

int visma_icp_get_launch_config(visma_icp_ctx *ctx, int *src_tiles, int *tgt_splits)
{
    CTX_CHECK();
    int a = 0, b = 0;
    ctx->eng->launch_config(&a, &b);
    if (src_tiles) *src_tiles = a;
    if (tgt_splits) *tgt_splits = b;
    return VISMA_ICP_OK;
}

int visma_icp_comm_unique_id(void *out_id)
{
    if (!out_id) return VISMA_ICP_ERR_INVALID;
    if (!g_rccl.load()) { g_create_error = g_rccl.error; return VISMA_ICP_ERR_RCCL; }
    NcclId id;
    int rc = g_rccl.GetUniqueId(&id);
    if (rc != 0) { g_create_error = "ncclGetUniqueId failed"; return VISMA_ICP_ERR_RCCL; }
    std::memcpy(out_id, &id, sizeof(id));
    return VISMA_ICP_OK;
}

int visma_icp_comm_init(visma_icp_ctx *ctx, int rank, int nranks, const void *unique_id)
{
    CTX_CHECK();
    if (!unique_id || nranks < 1 || rank < 0 || rank >= nranks) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad comm arguments");
    if (ctx->use_axis && nranks > 1) return ctx->fail(VISMA_ICP_ERR_INVALID, "sharded ranks take no rotation axis");
    int rc = ctx->eng->comm_init(rank, nranks, unique_id);
    if (rc) return ctx->eng_fail(rc);
    ctx->rank = rank;
    ctx->nranks = nranks;
    return VISMA_ICP_OK;
}

int visma_icp_comm_ipc_export(visma_icp_ctx *ctx, void *out_handle)
{
    CTX_CHECK();
    if (!out_handle) return ctx->fail(VISMA_ICP_ERR_INVALID, "out_handle is NULL");
    int rc = ctx->eng->ipc_export(out_handle);
    if (rc) return ctx->eng_fail(rc);
    return VISMA_ICP_OK;
}

int visma_icp_comm_ipc_init(visma_icp_ctx *ctx, int rank, int nranks, const void *handles)
{
    CTX_CHECK();
    if (!handles || nranks < 1 || rank < 0 || rank >= nranks) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad comm arguments");
    if (ctx->use_axis && nranks > 1) return ctx->fail(VISMA_ICP_ERR_INVALID, "sharded ranks take no rotation axis");
    int rc = ctx->eng->ipc_init(rank, nranks, handles);
    if (rc) return ctx->eng_fail(rc);
    ctx->rank = rank;
    ctx->nranks = nranks;
    return VISMA_ICP_OK;
}

int visma_icp_set_allreduce(visma_icp_ctx *ctx, visma_icp_allreduce_fn fn, void *user, int rank, int nranks)
{
    CTX_CHECK();
    if (nranks < 1 || rank < 0 || rank >= nranks) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad rank arguments");
    if (ctx->use_axis && nranks > 1) return ctx->fail(VISMA_ICP_ERR_INVALID, "sharded ranks take no rotation axis");
    ctx->host_allreduce = fn;
    ctx->host_allreduce_user = user;
    ctx->rank = rank;
    ctx->nranks = nranks;
    return VISMA_ICP_OK;
}

int visma_icp_set_search_precision(visma_icp_ctx *ctx, int mode)
{
    CTX_CHECK();
    if (mode < 0 || mode > 2) return ctx->fail(VISMA_ICP_ERR_INVALID, "search precision must be 0, 1 or 2");
    // takes effect at the next cloud upload (the header's contract): the clouds resident now were laid out
    // for the mode they were uploaded under (fp32 only / fp32 + f64 copies), and switching the flag alone would
    // run a third kernel (mode 0 over f64 copies = the all-f64 search), not the one asked for
    ctx->search_precision = mode;
    return VISMA_ICP_OK;
}

int visma_icp_get_search_precision_used(visma_icp_ctx *ctx, int *is_f64)
{
    CTX_CHECK();
    if (!is_f64) return ctx->fail(VISMA_ICP_ERR_INVALID, "null output");
    *is_f64 = ctx->eng->search_is_f64() ? 2 : (ctx->eng->search_is_exact() ? 1 : 0);
    return VISMA_ICP_OK;
}

int visma_icp_set_target_shard(visma_icp_ctx *ctx, int64_t global_offset, int64_t global_nt, const double centre[3])
{
    CTX_CHECK();
    if (ctx->use_axis && global_nt > 0) return ctx->fail(VISMA_ICP_ERR_INVALID, "sharded ranks take no rotation axis");
    int rc = ctx->eng->set_target_shard(global_offset, global_nt);
    if (rc) return ctx->eng_fail(rc);
    ctx->target_sharded = global_nt > 0;
    ctx->fixed_centre = centre != nullptr && global_nt > 0;
    if (ctx->fixed_centre) std::memcpy(ctx->centre, centre, 3 * sizeof(double));
    return VISMA_ICP_OK;
}

int visma_icp_set_minreduce(visma_icp_ctx *ctx, visma_icp_minreduce_fn fn, void *user)
{
    CTX_CHECK();
    ctx->eng->set_minreduce(fn, user);
    return VISMA_ICP_OK;
}

int visma_icp_set_global_source_count(visma_icp_ctx *ctx, int64_t ns_total)
{
    CTX_CHECK();
    if (ns_total < 0) return ctx->fail(VISMA_ICP_ERR_INVALID, "negative count");
    ctx->ns_total = ns_total;
    return VISMA_ICP_OK;
}

}  // extern "C"


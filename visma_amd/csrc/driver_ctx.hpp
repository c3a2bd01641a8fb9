// driver_ctx.hpp -- struct visma_icp_ctx: the host driver's state and its loops (internal).
#pragma once
#include "engine.hpp"

using namespace visma;
using namespace visma::drv;

// a TSDF volume of a context: the engine's id, what it was created with, and the rows of its last extractions
struct visma_icp_tsdf {
    int id = 0;
    TsdfConfig cfg;
    int64_t rows[2] = {-1, -1};       // [0] ExtractPointCloud, [1] ExtractVoxelPointCloud; -1: none since the last change
    int64_t mesh_rows[2] = {-1, -1};  // ExtractTriangleMesh: vertices, triangles; -1: none since the last change
};

// a color map object of a context: the engine's id, what it was created with and how far its staged calls have come
struct visma_icp_color_map {
    int id = 0;
    ColorMapConfig cfg;
    int iterations = 0;               // the option's maximum_iteration
    std::vector<char> image_set;      // per frame: set since create
    int64_t n_vertices = -1;          // -1: no vertices yet
    bool prepared = false;
    bool non_rigid = false;           // made by visma_icp_color_map_create_non_rigid: a warping field per image
    int anchor_w = 0, anchor_h = 0;
    double anchor_step = 0.0;
};

// a KDTreeFlann of a context: the cloud resident on the device with the grid of its last search (kdtree.hip)
struct visma_icp_kdtree {
    visma_icp_ctx *ctx = nullptr;
    KdTreeDevice *dev = nullptr;
    int64_t n = 0;
    visma_icp_kdtree() = default;
    visma_icp_kdtree(const visma_icp_kdtree &) = delete;
    visma_icp_kdtree &operator=(const visma_icp_kdtree &) = delete;
    ~visma_icp_kdtree() { kdtree_device_destroy(dev); }
};

// a TriangleMesh of a context, resident on the device (trimesh.hip)
struct visma_icp_trimesh {
    visma_icp_ctx *ctx = nullptr;
    TriMeshDevice *dev = nullptr;
    visma_icp_trimesh() = default;
    visma_icp_trimesh(const visma_icp_trimesh &) = delete;
    visma_icp_trimesh &operator=(const visma_icp_trimesh &) = delete;
    ~visma_icp_trimesh() { trimesh_device_destroy(dev); }
};

// a PointCloud of a context, resident on the device (cloud.hip)
struct visma_icp_cloud {
    visma_icp_ctx *ctx = nullptr;
    CloudDevice *dev = nullptr;
    visma_icp_cloud() = default;
    visma_icp_cloud(const visma_icp_cloud &) = delete;
    visma_icp_cloud &operator=(const visma_icp_cloud &) = delete;
    ~visma_icp_cloud() { cloud_device_destroy(dev); }
};

// an Image of a context, resident on the device (image.hip)
struct visma_icp_image {
    visma_icp_ctx *ctx = nullptr;
    ImageDevice *dev = nullptr;
    visma_icp_image() = default;
    visma_icp_image(const visma_icp_image &) = delete;
    visma_icp_image &operator=(const visma_icp_image &) = delete;
    ~visma_icp_image() { image_device_destroy(dev); }
};

// ---- the driver -----------------------------------------------------------------
struct visma_icp_ctx {
    std::unique_ptr<Engine> eng;
    std::string err;
    double centre[3] = {0, 0, 0};
    double radius_hint = 0.0;         // visma_icp_set_radius_hint: the search radius the next registration will use
    double last_radius = 0.0;         // ... else the one the last registration used (a caller's loop keeps it)
    int search_precision = 1;         // 0 fp32 search, 1 f64 for small clouds (auto, default), 2 f64 always
    bool fixed_centre = false;        // centre given by the caller (target-sharded ranks share one)
    bool target_sharded = false;
    bool have_src = false, have_tgt = false;
    // Frame bookkeeping: visma_icp_set_clouds_f64 centres BOTH clouds on one point; the fp32 / device
    // setters upload a cloud as given (centre 0).  A cloud uploaded in the other frame cannot be combined
    // with it: the setter that changes the frame invalidates the other cloud (it has to be set again).
    bool centred_upload = false;
    void enter_uncentred_frame(bool setting_source)
    {
        if (centred_upload && (centre[0] != 0.0 || centre[1] != 0.0 || centre[2] != 0.0)) {
            if (setting_source) have_tgt = false; else have_src = false;
        }
        centred_upload = false;
        centre[0] = centre[1] = centre[2] = 0.0;
    }
    visma_icp_allreduce_fn host_allreduce = nullptr;
    void *host_allreduce_user = nullptr;
    int rank = 0, nranks = 1;
    int64_t ns_total = 0;
    // the frame pair of the last visma_icp_odometry_prepare (resident on the engine): what the later calls check against
    struct { bool ready = false; int w = 0, h = 0, n_levels = 0; } odo;
    std::vector<std::unique_ptr<visma_icp_color_map>> color_maps;   // likewise
    std::vector<std::unique_ptr<visma_icp_tsdf>> volumes;   // the engine frees their device memory with itself
    std::vector<std::unique_ptr<visma_icp_kdtree>> trees;   // each frees its own, before the engine goes
    std::vector<std::unique_ptr<visma_icp_trimesh>> meshes;   // likewise
    std::vector<std::unique_ptr<visma_icp_cloud>> clouds;   // likewise
    std::vector<std::unique_ptr<visma_icp_image>> images;   // likewise
    // what the two-pass image operations work in: one for all images of the context, made at the first use
    struct ImageScratchOwner {
        ImageScratch *p = nullptr;
        ImageScratchOwner() = default;
        ImageScratchOwner(const ImageScratchOwner &) = delete;
        ImageScratchOwner &operator=(const ImageScratchOwner &) = delete;
        ~ImageScratchOwner() { image_scratch_destroy(p); }
    } image_scratch_owner;
    ImageScratch *image_scratch()
    {
        if (!image_scratch_owner.p) image_scratch_owner.p = image_scratch_create();
        return image_scratch_owner.p;
    }
    // what a render works in: one for all renders of the context, made at the first use
    struct RenderScratchOwner {
        RenderScratch *p = nullptr;
        RenderScratchOwner() = default;
        RenderScratchOwner(const RenderScratchOwner &) = delete;
        RenderScratchOwner &operator=(const RenderScratchOwner &) = delete;
        ~RenderScratchOwner() { render_scratch_destroy(p); }
    } render_scratch_owner;
    RenderScratch *render_scratch()
    {
        if (!render_scratch_owner.p) render_scratch_owner.p = render_scratch_create();
        return render_scratch_owner.p;
    }
    bool owns(const visma_icp_image *img) const
    {
        for (const auto &i : images) if (i.get() == img) return true;
        return false;
    }
    visma_icp_cloud *adopt(CloudDevice *dev)
    {
        std::unique_ptr<visma_icp_cloud> c(new visma_icp_cloud);
        c->ctx = this; c->dev = dev;
        clouds.push_back(std::move(c));
        return clouds.back().get();
    }
    visma_icp_image *adopt(ImageDevice *dev)
    {
        std::unique_ptr<visma_icp_image> i(new visma_icp_image);
        i->ctx = this; i->dev = dev;
        images.push_back(std::move(i));
        return images.back().get();
    }
    Mat4 last_Tc = Mat4::identity();
    bool last_plane = false;
    std::vector<int32_t> src_order;   // engine position -> caller's source index (Morton order)
    unsigned long long src_order_gen = 0;   // advanced with every change of src_order (the engine keeps a device copy)
    int trim_state = 0;               // the last trimmed pass: 0 none, 1 on the engine, 2 plain pass with every pair kept
    int robust_state = 0;             // the last robust pass: 0 none, 1 on the engine, 2 plain pass (L2: every weight 1)
    double last_aux_kernel_ms = 0.0;  // kernel time of the last mesh-distance call
    double last_aux_build_ms = 0.0;   // ... and of building its search structure
    int mesh_method = 0;              // 0 choose, 1 brute force, 2 BVH
    // visma_icp_set_rotation_axis: every solve of this context rotates about `axis` (unit, target frame) only
    bool use_axis = false;
    double axis[3] = {0, 0, 0};
    bool sharded() const { return target_sharded || nranks > 1; }
    // (an axis admits the closed form and point-to-plane: a Gauss-Newton point-to-point solver or scaling is refused)
    int check_axis_solver(int solver, bool scaling)
    {
        if (use_axis && (solver != VISMA_ICP_SOLVER_KABSCH || scaling))
            return fail(VISMA_ICP_ERR_INVALID, "a rotation axis is set: only the closed-form solver without scaling applies");
        return VISMA_ICP_OK;
    }
    void fill_axis(Engine::LoopParams &lp) const
    {
        lp.use_axis = use_axis;
        for (int a = 0; a < 3; a++) lp.axis[a] = axis[a];
    }

    int fail(int code, const std::string &msg) { err = msg; return code; }
    int eng_fail(int code) { err = eng->error(); return code; }

    // one NN pass + reduction (+ cross-rank sum); fills stats, fitness, rmse
    // world_frame: express the statistics in the caller's frame (needed by the
    // Gauss-Newton updates, whose Euler / exp-map retraction is not invariant to
    // the choice of origin); the closed-form solve uses the centred frame.
    int pass(const Mat4 &Tc, double max_dist, bool plane, bool world_frame, double *stats,
             double *fit, double *rmse, int64_t *k)
    {
        int rc = eng->nn_pass(Tc, max_dist);
        if (rc) return eng_fail(rc);
        last_Tc = Tc;
        last_plane = plane;
        const double zero[3] = {0, 0, 0};
        rc = eng->reduce(Tc, plane, world_frame ? centre : zero, stats);
        if (rc) return eng_fail(rc);
        if (host_allreduce && !eng->has_device_allreduce()) {
            if (host_allreduce(host_allreduce_user, stats, VISMA_ICP_NSTATS) != 0)
                return fail(VISMA_ICP_ERR_ENGINE, "host all-reduce callback failed");
        }
        *k = (int64_t)std::llround(stats[0]);
        fit_rmse(stats[0], stats[1], fit, rmse);
        return VISMA_ICP_OK;
    }

    // 0 = synchronous host loop, 1 = on-device loop, 2 = auto: host loop for one
    // problem (spin-wait on mapped memory beats a one-thread f64 SVD on the GPU:
    // measured 46 vs 68 us per iteration at 5k x 20k), device loop for sweeps of
    // many transforms (their solves run in parallel and nothing syncs per pass)
    int loop_mode = 2;
    bool device_loop_possible() const
    {
        return eng->supports_device_loop() && !host_allreduce && (!target_sharded || eng->shard_loop_on_device());
    }
    bool use_device_loop() const { return loop_mode == 1 && device_loop_possible(); }
    bool use_device_loop_batched() const { return loop_mode != 0 && device_loop_possible(); }
    // one rank, nothing summed on the host between a pass and the next: the engine may keep one launch alive across
    // the passes of a loop (ranks that share a GPU would wait for each other's workgroups)
    // (source-sharded ranks that exchange through their peer-to-peer mailboxes, one rank per GPU: the exchange happens
    //  inside the launch, so it may stay alive there too -- the engine knows whether the ranks share a device)
    bool solo() const { return !host_allreduce && !target_sharded && (nranks == 1 || eng->loop_across_ranks_ok()); }
    static bool wants_world_frame(int solver, bool plane) { return plane || solver != VISMA_ICP_SOLVER_KABSCH; }

    // T_centred <- update o T_centred, with the update expressed in `world` or centred frame
    Mat4 apply_update(const Mat4 &upd, const Mat4 &Tc, bool world_frame) const
    {
        if (!world_frame) return upd * Tc;
        return to_centred(upd * from_centred(Tc, centre), centre);
    }

    Mat4 solve(const double *stats, int solver, bool scaling, bool plane) const
    {
        bool ok;
        if (use_axis) return plane ? gn_axis_from_stats(stats, axis, &ok) : kabsch_axis_from_stats(stats, axis);
        if (plane) return gn_from_stats(stats, false, &ok);  // TransformationEstimation.cpp:94-102
        switch (solver) {
        case VISMA_ICP_SOLVER_GN_EULER: return gn_from_stats(stats, false, &ok);
        case VISMA_ICP_SOLVER_GN_EXPMAP: return gn_from_stats(stats, true, &ok);
        default: return kabsch_from_stats(stats, scaling);
        }
    }

    const int32_t *order_ptr() const { return (int64_t)src_order.size() == eng->ns() && eng->ns() > 0 ? src_order.data() : nullptr; }

    // fitness and inlier_rmse over all K pairs of a pass (Registration.cpp:87-94)
    void fit_rmse(double K, double sum_d2, double *fit, double *rmse) const
    {
        const int64_t denom = ns_total > 0 ? ns_total : eng->ns();
        *fit = K > 0.0 ? K / (double)denom : 0.0;
        *rmse = K > 0.0 ? std::sqrt(sum_d2 / K) : 0.0;
    }
    // the rmse of a trimmed or weighted pass's own statistics
    static double trimmed_rmse(const double *stats) { return stats[0] > 0.0 ? std::sqrt(stats[1] / stats[0]) : 0.0; }
    static void fill_trim_info(visma_icp_trim_info *info, const double *stats, const Engine::TrimPass &tr)
    {
        info->kept = tr.kept;
        info->trimmed_rmse = trimmed_rmse(stats);
        info->d2_cut = tr.d2_cut;
    }
    static void fill_robust_info(visma_icp_robust_info *info, const double *stats, const Engine::RobustPass &rp)
    {
        info->scale = rp.scale;
        info->median_residual = std::sqrt(rp.v);
        info->weight_sum = stats[0];
        info->zero_weight = rp.zero_weight;
        info->robust_rmse = trimmed_rmse(stats);
    }

    static void fill_gicp_info(visma_icp_gicp_info *info, const Engine::GicpPass &gp)
    {
        info->cost = gp.cost;
        info->mahalanobis_rmse = gp.found > 0 ? std::sqrt(gp.cost / (double)gp.found) : 0.0;
    }

    static void fill_colored_info(visma_icp_colored_info *info, const Engine::ColoredPass &cp)
    {
        info->cost = cp.geometric_cost + cp.photometric_cost;
        info->geometric_cost = cp.geometric_cost;
        info->photometric_cost = cp.photometric_cost;
    }

    // RegistrationICP's loop around a pass over the pairs (trimmed, robust, generalized, colored).  reduce(Tc, stats) is the engine's reduction
    // behind each NN pass: its statistics feed the solve, `pp` (filled by it) has K and the sum over all K pairs for
    // fitness and inlier_rmse.  The stop test looks at fitness and the rmse of the pass's OWN statistics.  *state (may be NULL): 1 once
    // a pass ran on the engine.  fill_info(stats) runs behind the last pass.
    template <class Reduce, class FillInfo>
    int run_pair_passes(const double *init, double max_dist, bool plane, int max_iter, double rel_fit, double rel_rmse,
                        bool scaling, visma_icp_result *out, int *state, const Engine::PairPass &pp, Reduce reduce,
                        FillInfo fill_info)
    {
        return run_pair_passes(init, max_dist, plane, max_iter, rel_fit, rel_rmse, scaling, out, state, pp, reduce, fill_info,
                               [](const double *stats) { return trimmed_rmse(stats); });
    }
    // ... own_rmse(stats): the rmse the stop test compares, where it is not that of the statistics' [1] / [0] (generalized
    // ICP: the Mahalanobis rmse of the pass, which `reduce` left with the caller)
    template <class Reduce, class FillInfo, class OwnRmse>
    int run_pair_passes(const double *init, double max_dist, bool plane, int max_iter, double rel_fit, double rel_rmse,
                        bool scaling, visma_icp_result *out, int *state, const Engine::PairPass &pp, Reduce reduce,
                        FillInfo fill_info, OwnRmse own_rmse)
    {
        std::memset(out, 0, sizeof(*out));
        std::memcpy(out->transformation, init, sizeof(double) * 16);
        if (!(max_dist > 0.0)) return VISMA_ICP_OK;                 // Registration.cpp:148-151
        last_radius = max_dist;
        if (plane && !eng->has_normals()) return VISMA_ICP_OK;      // Registration.cpp:152-157
        Mat4 Tc = to_centred(Mat4::from(init), centre);
        double stats[VISMA_ICP_NSTATS], fit = 0.0, rmse = 0.0, own = 0.0;
        auto pass = [&]() -> int {
            int rc = eng->nn_pass(Tc, max_dist);
            if (rc) return eng_fail(rc);
            last_Tc = Tc;
            last_plane = plane;
            rc = reduce(Tc, stats);
            if (rc) return eng_fail(rc);
            if (state) *state = 1;
            fit_rmse((double)pp.found, pp.sum_all, &fit, &rmse);
            own = own_rmse(stats);
            return VISMA_ICP_OK;
        };
        int rc = pass();
        if (rc) return rc;
        int it = 0;
        for (int i = 0; i < max_iter; i++) {
            const Mat4 upd = solve(stats, VISMA_ICP_SOLVER_KABSCH, scaling, plane);
            Tc = apply_update(upd, Tc, plane);                      // (point-to-plane: world frame, as run())
            const double bfit = fit, bown = own;
            rc = pass();
            if (rc) return rc;
            it = i + 1;
            if (std::fabs(bfit - fit) < rel_fit && std::fabs(bown - own) < rel_rmse) break;
        }
        const Mat4 T = from_centred(Tc, centre);
        std::memcpy(out->transformation, T.m, sizeof(T.m));
        out->fitness = fit;
        out->inlier_rmse = rmse;
        out->num_correspondences = pp.found;
        out->iterations = it;
        out->nn_passes = it + 1;
        fill_info(stats);
        return VISMA_ICP_OK;
    }

    int run(const double *init, double max_dist, int max_iter, double rel_fit, double rel_rmse,
            int solver, bool scaling, bool plane, visma_icp_result *out)
    {
        std::memset(out, 0, sizeof(*out));
        std::memcpy(out->transformation, init, sizeof(double) * 16);
        if (!(max_dist > 0.0)) return VISMA_ICP_OK;                 // Registration.cpp:148-151
        last_radius = max_dist;
        if (plane && !eng->has_normals()) return VISMA_ICP_OK;      // Registration.cpp:152-157
        if (!have_src || !have_tgt) return fail(VISMA_ICP_ERR_STATE, "clouds not set");
        Mat4 Tc = to_centred(Mat4::from(init), centre);
        const bool world = wants_world_frame(solver, plane);
        if (use_device_loop()) {
            Engine::LoopParams lp;
            lp.Tc0 = Tc;
            std::memcpy(lp.centre, centre, sizeof(centre));
            lp.max_dist = max_dist; lp.rel_fit = rel_fit; lp.rel_rmse = rel_rmse;
            lp.max_iter = max_iter; lp.solver = solver; lp.passes = max_iter + 1;
            lp.scaling = scaling; lp.plane = plane; lp.world = world; lp.check_stop = true;
            lp.ns_total = ns_total > 0 ? ns_total : eng->ns();
            fill_axis(lp);
            Engine::LoopResult r;
            int rc = eng->run_loop(lp, nullptr, 1, &r);
            if (rc) return eng_fail(rc);
            last_Tc = r.Tc;
            last_plane = plane;
            const Mat4 T = from_centred(r.Tc, centre);
            std::memcpy(out->transformation, T.m, sizeof(T.m));
            out->fitness = r.fit;
            out->inlier_rmse = r.rmse;
            out->num_correspondences = r.k;
            out->iterations = r.iters;
            out->nn_passes = r.passes;
            return VISMA_ICP_OK;
        }
        double stats[VISMA_ICP_NSTATS], fit, rmse;
        int64_t k;
        Engine::LoopScope scope(eng.get(), solo() ? max_iter + 1 : 0);   // (at most max_iter + 1 passes follow, nothing else)
        int rc = pass(Tc, max_dist, plane, world, stats, &fit, &rmse, &k);  // Registration.cpp:166-168
        if (rc) return rc;
        int it = 0;
        for (int i = 0; i < max_iter; i++) {                          // Registration.cpp:169-184
            const Mat4 upd = solve(stats, solver, scaling, plane);
            Tc = apply_update(upd, Tc, world);
            const double bfit = fit, brmse = rmse;
            rc = pass(Tc, max_dist, plane, world, stats, &fit, &rmse, &k);
            if (rc) return rc;
            it = i + 1;
            if (std::fabs(bfit - fit) < rel_fit && std::fabs(brmse - rmse) < rel_rmse) break;
        }
        const Mat4 T = from_centred(Tc, centre);
        std::memcpy(out->transformation, T.m, sizeof(T.m));
        out->fitness = fit;
        out->inlier_rmse = rmse;
        out->num_correspondences = k;
        out->iterations = it;
        out->nn_passes = it + 1;
        return VISMA_ICP_OK;
    }
};

#define CTX_CHECK()                                                             \
    if (!ctx) { g_create_error = "ctx is NULL"; return VISMA_ICP_ERR_INVALID; }

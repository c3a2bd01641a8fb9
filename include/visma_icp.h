/*
 * visma_icp.h -- C ABI of the MI355X-native ICP registration path.
 *
 * This is the drop-in boundary under the C++ shim (include/constrained_ICP.h,
 * include/Core/Registration/Registration.h).  The reference has no C ABI or
 * FFI for this path (it is a C++ virtual plugin called from a C++ free
 * function), so each entry point cites the reference C++ interface it
 * replaces.  Paths are relative to the reference root;
 * O3D = thirdparty/Open3D/src.
 *
 * Conventions: every function returns a visma_icp_status (0 = OK) and never
 * throws; 4x4 matrices are ROW-MAJOR double[16]; point arrays are AoS with a
 * caller-given stride in elements; the caller owns every pointer it passes
 * and the library copies what it keeps.  One ctx per host thread per GPU
 * (thread-compatible, not thread-safe).
 */
#ifndef VISMA_ICP_H
#define VISMA_ICP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define VISMA_ICP_API __attribute__((visibility("default")))
#else
#define VISMA_ICP_API
#endif

typedef struct visma_icp_ctx visma_icp_ctx;

typedef enum {
    VISMA_ICP_OK = 0,
    VISMA_ICP_ERR_INVALID = 1,   /* bad argument                              */
    VISMA_ICP_ERR_NO_DEVICE = 2, /* no usable gfx950 device / HIP unavailable */
    VISMA_ICP_ERR_HIP = 3,       /* a HIP call failed (see last_error)        */
    VISMA_ICP_ERR_RCCL = 4,      /* RCCL unavailable or a collective failed   */
    VISMA_ICP_ERR_STATE = 5,     /* call order violated (e.g. no clouds set)  */
    VISMA_ICP_ERR_ENGINE = 6     /* an injected engine callback failed        */
} visma_icp_status;

/* Per-iteration solve.  KABSCH is the reference's arithmetic
 * (src/constrained_ICP.cpp:25-37 -> Eigen umeyama); the GN modes are single
 * Gauss-Newton steps on the 6x6 normal equations
 * (O3D/Core/Utility/Eigen.cpp:88-106; exp-map update via core/rodrigues.h:143). */
typedef enum {
    VISMA_ICP_SOLVER_KABSCH = 0,
    VISMA_ICP_SOLVER_GN_EULER = 1,
    VISMA_ICP_SOLVER_GN_EXPMAP = 2
} visma_icp_solver;

/* Nearest-neighbour search implementation (identical results at equal search
 * precision, see visma_icp_set_search_precision). */
typedef enum {
    VISMA_ICP_NN_AUTO = 0,
    VISMA_ICP_NN_BRUTE = 1, /* brute force over the whole target           */
    VISMA_ICP_NN_GRID = 2   /* radius-cell uniform grid (exact, radius-limited) */
} visma_icp_nn_mode;

#define VISMA_ICP_NSTATS 38
/* Layout of the reduced statistics (one ICP iteration's normal equations):
 *   [0]      K            number of correspondences
 *   [1]      sum |p-q|^2
 *   [2..22]  upper triangle of J^T J (6x6), row by row
 *   [23..28] J^T r
 *   [29..37] sum q p^T   (3x3 row-major, q = row)
 * rows J = [p x e_k | e_k], r_k = (p-q).e_k (k = x,y,z), parameter order
 * x = [alpha beta gamma tx ty tz] -- the convention of
 * O3D/Core/Registration/TransformationEstimation.cpp:82-92 and
 * O3D/Core/Utility/Eigen.cpp:137-182 (ComputeJTJandJTr). */

/* Mirrors open3d::RegistrationResult (O3D/Core/Registration/Registration.h:81-94)
 * plus bookkeeping. */
typedef struct {
    double transformation[16]; /* transformation_  (row-major)              */
    double fitness;            /* fitness_                                  */
    double inlier_rmse;        /* inlier_rmse_                              */
    int64_t num_correspondences; /* correspondence_set_.size()              */
    int32_t iterations;        /* solves performed                          */
    int32_t nn_passes;         /* NN passes performed (= iterations + 1)    */
} visma_icp_result;

/* Kernel timing accumulated since the last reset (HIP events on the ctx's
 * stream; only collected while profiling is enabled). */
typedef struct {
    double nn_ms;        /* total time in the NN-correspondence kernel       */
    int64_t nn_launches;
    double reduce_ms;    /* total time in the Jacobian/residual reduction    */
    int64_t reduce_launches;
    double aux_ms;       /* grid build / refine / other kernels              */
    int64_t aux_launches;
    double grid_candidates; /* target points examined by the grid search (sum) */
    double grid_candidates_27cell; /* ... points in the full 3x3x3 cell blocks (before row pruning) */
    /* streamed (LDS-tile) search, profiled launches only: */
    double tile_workgroups;          /* workgroups of the streamed search */
    double tile_fallback_workgroups; /* parts (see tile_parts) searched from global memory: footprint larger than the tile */
    double tile_parts;               /* parts the chunks were searched in (1 per workgroup unless a footprint had to be split) */
    double tile_points;              /* target points streamed into LDS (sum over workgroups) */
    double tile_rows;                /* (y,z) rows of the footprints (sum over workgroups) */
    double f64_reranks;              /* queries re-ranked in f64 (runner-up or radius inside the rounding band) */
    double tile_phase_cycles[7];     /* shader cycles per workgroup phase, summed over workgroups: source + transform,
                                        run bounds + footprint rows + scan, tile streaming, search + re-rank,
                                        winner fetch, moments + row; [6] unused */
    double grid_certified;           /* queries of profiled passes whose previous winner was CERTIFIED unchanged (no search:
                                        the warm-started kernel's triangle-inequality test, visma_amd/csrc/grid_coop.hip) */
    /* persistent launches (one launch of the certificate kernel running several passes of a host loop, the next
     * transform handed over through mapped host memory): nn_ms holds their whole duration -- the time the launch
     * waits for the host included -- and nn_launches counts their PASSES, so that nn_ms / nn_launches stays the
     * time of one pass whichever way it ran; these two say how many launches and passes that were. */
    double persist_launches;
    double persist_passes;
    double persist_ms;               /* their share of nn_ms */
    double persist_aborts;           /* persistent launches that ended by themselves (no command in time); counted always */
} visma_icp_timing;

/* ---- lifetime ---------------------------------------------------------- */

/* Create a context on HIP device `device`.  Fails with NO_DEVICE (never falls
 * back to the CPU) when there is no GPU.  Replaces the per-call state of
 * open3d::RegistrationICP (KD-tree + source copy, Registration.cpp:159-165). */
VISMA_ICP_API int visma_icp_create(visma_icp_ctx **out, int device);
VISMA_ICP_API int visma_icp_destroy(visma_icp_ctx *ctx);
/* Message of the last failure on ctx (or of the last failed create if NULL). */
VISMA_ICP_API const char *visma_icp_last_error(const visma_icp_ctx *ctx);
VISMA_ICP_API const char *visma_icp_version(void);
/* Number of HIP devices this process sees (0 without a GPU or a driver); no context needed. */
VISMA_ICP_API int visma_icp_device_count(void);

/* ---- clouds ------------------------------------------------------------ */

/* Upload both clouds from the reference's own storage: AoS float64 xyz
 * (open3d::PointCloud::points_, O3D/Core/Geometry/PointCloud.h:86; stride 3).
 * Centres both on the target centroid in f64, rounds to fp32 (design rule R2),
 * and remembers the centre so every transform in this API stays in the
 * caller's frame.  Replaces KDTreeFlann::SetGeometry + `PointCloud pcd = source`
 * (Registration.cpp:160-162). */
VISMA_ICP_API int visma_icp_set_clouds_f64(visma_icp_ctx *ctx, const double *src_xyz,
                                           int64_t ns, int src_stride,
                                           const double *tgt_xyz, int64_t nt,
                                           int tgt_stride);
/* The same with target = open3d::VoxelDownSample(scene, voxel_size) (O3D/Core/Geometry/DownSample.cpp:179-220):
 * the step both callers run on the scene right before RegistrationICP (src/evaluation.cpp:258-271,
 * src/annotation.cpp:112), fused with the target upload.  The scene crosses PCIe once, is down-sampled on the
 * device (the reference's point values bit for bit; voxels in ascending voxel-index order instead of the
 * reference's hash-map iteration order) and becomes the target where it lies; *nt_out = its point count.
 * Target indices of the results refer to that order; visma_icp_get_voxel_target copies the down-sampled points
 * out (nt x 3 f64) for a caller that wants them too.  The registration that follows equals, bit for bit, the one
 * after visma_icp_voxel_down_sample + visma_icp_set_clouds_f64. */
VISMA_ICP_API int visma_icp_set_clouds_f64_voxel_target(visma_icp_ctx *ctx, const double *src_xyz, int64_t ns,
                                                        int src_stride, const double *scene_xyz, int64_t n_scene,
                                                        int scene_stride, double voxel_size, int64_t *nt_out);
VISMA_ICP_API int visma_icp_get_voxel_target(visma_icp_ctx *ctx, double *xyz_out, int64_t nt);
/* The max_correspondence_distance the NEXT registration on this context will use (RegistrationICP's third argument,
 * Registration.h:102-107), told before the clouds are uploaded: visma_icp_set_clouds_f64 then builds the search
 * structure on the GPU while the host is still staging the source (C4: 0.7 ms of a 3.7 ms registration hidden).
 * One-shot: the upload that uses the hint clears it.  Without a hint the radius of the context's previous
 * registration is assumed; 0 clears a pending hint.  A wrong value
 * only costs the wasted build: results never depend on it. */
VISMA_ICP_API int visma_icp_set_radius_hint(visma_icp_ctx *ctx, double max_correspondence_distance);
/* feh::ICPRefinement's clouds (src/evaluation.cpp:248-271) made on the device, source side too:
 *   for every model: SamplePointCloudFromMesh(V, F, samples) (include/geometry.h:29-64; visma_icp_sample_mesh's
 *   draws: mesh k uses the stream `seed + k`, reference_quirks as there), PointCloud::Transform(model_to_scene)
 *   (O3D/Core/Geometry/PointCloud.cpp:75-80; row-major 4x4, NULL = identity), `*scene_est += *model`;
 *   scene = VoxelDownSample(scene, voxel_size)  (voxel_size == 0: the scene as it is).
 * The sampled points never cross PCIe: they are sampled, moved, concatenated, ordered and widened where the search
 * reads them.  *ns_out / *nt_out = the sizes of the two clouds; source indices of the results refer to the
 * concatenation in mesh order, visma_icp_get_mesh_source copies it (ns x 3 doubles) to the host.  Same values as
 * visma_icp_sample_mesh + a host transform + visma_icp_set_clouds_f64[_voxel_target] (tests/test_mesh_source.py). */
typedef struct {
    const double *V; int64_t nv;        /* vertices, nv x 3 */
    const int32_t *F; int64_t nf;       /* faces, nf x 3 */
    int64_t samples;                    /* options["samples_per_model"] */
    const double *model_to_scene;       /* 16 doubles, row-major, or NULL */
} visma_icp_mesh_source;
VISMA_ICP_API int visma_icp_set_clouds_meshes_f64(visma_icp_ctx *ctx, const visma_icp_mesh_source *meshes, int n_meshes,
                                                  int reference_quirks, uint64_t seed, const double *scene_xyz,
                                                  int64_t n_scene, int scene_stride, double voxel_size,
                                                  int64_t *ns_out, int64_t *nt_out);
VISMA_ICP_API int visma_icp_get_mesh_source(visma_icp_ctx *ctx, double *xyz_out, int64_t ns);
/* fp32 uploads, no centring (the caller's coordinates are used as they are; the exact search
 * takes the fp32 values as its f64 coordinates).  FRAME RULE: visma_icp_set_clouds_f64 centres
 * BOTH clouds on one point; these setters (and the _device ones) upload in the caller's frame.
 * The two frames cannot be combined: the first uncentred upload after a centred one INVALIDATES
 * the other cloud -- set it again (the next run fails with VISMA_ICP_ERR_STATE "clouds not set"
 * otherwise).
 *
 * POINTS THAT ARE NOT FINITE (NaN or +-inf in a coordinate; the NaN rows of an organised cloud from a depth camera) are
 * no error, in any upload, search kernel (brute force, lane-serial, warm cooperative one launch per pass or persistent,
 * ring, wave; fp32, exact or f64 precision), nn_mode or loop.  The rule is DELETE AND REMAP; it is the arithmetic of
 * vk_nn_pass_f32 in oracle/icp_oracle.c, where `d < best` is false for a NaN and for an inf:
 *   1. a source point whose TRANSFORMED position has a coordinate that is not finite has no pair;
 *   2. a target point with a coordinate that is not finite is nobody's partner;
 *   3. every other query gets the partner, the d2 bits and the tie-break (lowest original index) it gets on the clouds
 *      with those rows deleted; indices refer to the caller's order;
 *   4. K, the kept pairs of a trimmed pass, the weights of a robust one and the 38 statistics are those of the deleted
 *      clouds (the trimmed share stays floor(keep * ns) with ns the source rows as uploaded, finite or not);
 *   5. a run / iterate / sweep / batch over such clouds ends and returns the pose of the same call on the deleted clouds;
 *   6. visma_icp_set_clouds_f64 centres both clouds on the target's centroid: a TARGET coordinate that is not finite
 *      makes that centre non-finite, so nothing has a pair -- K = 0 and the pose stays the initial one; a SOURCE row
 *      that is not finite follows 1, 3 and 4 there too.
 * The grid's bounding box is the box of the target coordinates that ARE finite (a target without any is one empty
 * cell); a finite row far away (1e30) only makes the cells coarse.  A box of finite coordinates wider than half the
 * fp32 range (1.7e38) on an axis cannot be binned in fp32: the grid searches refuse it with VISMA_ICP_ERR_INVALID,
 * VISMA_ICP_NN_BRUTE searches it.  tests/test_core_hostile.py pins all of this against an independent reference. */
VISMA_ICP_API int visma_icp_set_target(visma_icp_ctx *ctx, const float *xyz, int64_t nt,
                                       int stride_floats);
VISMA_ICP_API int visma_icp_set_source(visma_icp_ctx *ctx, const float *xyz, int64_t ns,
                                       int stride_floats);
/* Same from DEVICE memory (float4 xyzw per point, w ignored), copied D2D. */
VISMA_ICP_API int visma_icp_set_target_device(visma_icp_ctx *ctx, const void *d_xyzw,
                                              int64_t nt);
VISMA_ICP_API int visma_icp_set_source_device(visma_icp_ctx *ctx, const void *d_xyzw,
                                              int64_t ns);
/* Target normals (AoS f64, stride 3) for the point-to-plane estimator. */
VISMA_ICP_API int visma_icp_set_target_normals_f64(visma_icp_ctx *ctx,
                                                   const double *nxyz, int64_t nt,
                                                   int stride);

/* ---- the three kernels, individually ----------------------------------- */

/* Fused PointCloud::Transform (O3D/Core/Geometry/PointCloud.cpp:75-80) +
 * GetRegistrationResultAndCorrespondences (Registration.cpp:41-96): apply T
 * (caller frame) to the pristine source and find, per source point, the
 * nearest target point with d^2 < (float)(max_dist^2).  Results stay on the
 * device.  Points that are not finite: the rule at visma_icp_set_target. */
VISMA_ICP_API int visma_icp_nn_pass(visma_icp_ctx *ctx, const double T[16],
                                    double max_dist);
/* Per-correspondence Jacobian/residual + wavefront-shuffle reduction to the
 * statistics above for the last nn_pass (replaces ComputeJTJandJTr,
 * O3D/Core/Utility/Eigen.cpp:137-182, and the gathers of
 * src/constrained_ICP.cpp:30-35).  Statistics are in the CENTRED frame. */
VISMA_ICP_API int visma_icp_reduce(visma_icp_ctx *ctx,
                                   double out_stats[VISMA_ICP_NSTATS]);
/* Correspondences of the last nn_pass, sorted by source index
 * (RegistrationResult::correspondence_set_).  Buffers hold >= ns entries;
 * d2 may be NULL. */
VISMA_ICP_API int visma_icp_get_correspondences(visma_icp_ctx *ctx, int32_t *src_idx,
                                                int32_t *tgt_idx, float *d2,
                                                int64_t *k);

/* ---- host solves (pure functions; no ctx, no GPU) ----------------------- */

/* Update from the statistics.  KABSCH: closed-form Umeyama
 * (Eigen/src/Geometry/Umeyama.h:118-159) from the moments; GN_*: solve
 * J^T J x = -J^T r with the |det| < 1e-6 guard (Eigen.cpp:35-56) and map x to
 * SE(3) by Rz*Ry*Rx (Eigen.cpp:58-68) or by the exponential map
 * (core/rodrigues.h:143-182).  Identity when K = 0 or the solve is rejected
 * (src/constrained_ICP.cpp:29; TransformationEstimation.cpp:102). */
VISMA_ICP_API int visma_icp_solve_from_stats(const double stats[VISMA_ICP_NSTATS],
                                             int solver, int with_scaling,
                                             double T_update[16]);

/* The two updates constrained to a rotation about the axis `axis` (target
 * frame; normalised here, a zero, near-zero or non-finite axis returns
 * VISMA_ICP_ERR_INVALID) plus a 3-D translation.  plane = 0: the exact
 * least-squares closed form for the fixed correspondences (angle from the
 * cross-covariance projected on the plane normal to the axis; identity when
 * K = 0).  plane = 1: one Gauss-Newton step on (angle, translation) -- the
 * 6-DoF point-to-plane system restricted to 4 unknowns, the same |det| < 1e-6
 * guard (identity when it rejects), the exact rotation about the axis.  What a
 * context with visma_icp_set_rotation_axis solves. */
VISMA_ICP_API int visma_icp_solve_from_stats_axis(const double stats[VISMA_ICP_NSTATS],
                                                  int plane, const double axis[3],
                                                  double T_update[16]);

/* ---- rotation constrained to one axis (orientation constrained ICP) ----- */

/* visma_icp_set_rotation_axis(ctx, axis): from now on every solve of this
 * context rotates about `axis` only (in the target frame -- +Y for a scan whose
 * floor normal has been turned onto +Y) plus a free 3-D translation, through
 * every entry point: run, iterate, run_point_to_plane, both yaw sweeps, both
 * batches, run_batch_multi and run_corpus (whose contexts must all have the
 * same setting).  NULL clears it (the default: the unconstrained solves).  The
 * library normalises the axis; a zero, near-zero or non-finite one returns
 * VISMA_ICP_ERR_INVALID.  While it is set, solver GN_EULER / GN_EXPMAP and
 * with_scaling = 1 return VISMA_ICP_ERR_INVALID.
 * Invariant: R_result^T a = R_init^T a -- the tilt of `init` relative to the
 * axis is kept (start from a pose whose rotation fixes a, and every result
 * fixes it).
 * Sharded ranks do NOT take an axis: set_rotation_axis on a context that is
 * target-sharded or one of several ranks (comm_init, comm_ipc_init,
 * set_allreduce with nranks > 1), and those calls on a context with an axis
 * set, return VISMA_ICP_ERR_INVALID. */
VISMA_ICP_API int visma_icp_set_rotation_axis(visma_icp_ctx *ctx, const double axis[3]);
/* The unit axis in use (zeros when none) and *enabled = 0 / 1. */
VISMA_ICP_API int visma_icp_get_rotation_axis(const visma_icp_ctx *ctx, double axis_out[3],
                                              int *enabled);

/* ---- the full loop ------------------------------------------------------ */

/* open3d::RegistrationICP (O3D/Core/Registration/Registration.h:102-107,
 * .cpp:141-186) with estimator = cicp::TransformationEstimationPointToPoint4DoF
 * (include/constrained_ICP.h:14-30).  Same iteration/termination semantics:
 * max_iter+1 NN passes at most, stop when |dfitness| < rel_fitness and
 * |drmse| < rel_rmse, result fields from the last NN pass.  max_dist <= 0
 * returns OK with transformation = init and everything else 0
 * (Registration.cpp:148-151). */
VISMA_ICP_API int visma_icp_run(visma_icp_ctx *ctx, const double init[16],
                                double max_dist, int max_iter, double rel_fitness,
                                double rel_rmse, int solver, int with_scaling,
                                visma_icp_result *out);
/* Exactly `steps` fixed ICP iterations with no stop test: each step = one NN
 * pass at T, one reduction, one solve, T <- update * T (the body of the loop
 * at Registration.cpp:169-178).  T_inout is updated in place; out (may be NULL)
 * reports fitness / rmse / K of the LAST pass (taken at the T before the
 * final update).  This is the unit bench.py times. */
VISMA_ICP_API int visma_icp_iterate(visma_icp_ctx *ctx, double T_inout[16], double max_dist,
                                    int steps, int solver, int with_scaling,
                                    visma_icp_result *out);
/* Point-to-plane estimator (TransformationEstimation.cpp:61-103) on the same
 * reduction; needs set_target_normals_f64, else returns OK with
 * transformation = init (Registration.cpp:152-157). */
VISMA_ICP_API int visma_icp_run_point_to_plane(visma_icp_ctx *ctx, const double init[16],
                                               double max_dist, int max_iter,
                                               double rel_fitness, double rel_rmse,
                                               visma_icp_result *out);

/* feh::RegisterModelToScene (include/tool.h:40-42, src/annotation.cpp:29-64):
 * `level` yaw initialisations R_y(2 pi i / level), a full ICP from each (all
 * in flight together on the GPU), keep the first with strictly the most
 * correspondences.  per_level (may be NULL) receives all `level` results. */
VISMA_ICP_API int visma_icp_run_yaw_sweep(visma_icp_ctx *ctx, int level, double max_dist,
                                          int max_iter, double rel_fitness,
                                          double rel_rmse, int solver,
                                          visma_icp_result *best, int *best_level,
                                          visma_icp_result *per_level);

/* ---- trimmed ICP (Chetverikov, Svirko, Stepanov, Krsek: "The Trimmed Iterative Closest Point Algorithm",
 * ICPR 2002): of the K pairs a pass finds inside the radius only the m with the smallest distance enter the solve.
 * For a model registered against a PARTIAL scan: model points whose surface the scan never saw still find
 * partners inside the radius (the rim of the scanned part, the floor); those are the longest pairs of the pass.
 *
 *   keep in (0, 1]: the share of the SOURCE cloud expected to have a true partner (the paper's overlap).
 *   m = min(K, floor(keep * NS)), NS the number of source points; below 3, m = min(K, 3).  keep = 1: m = K.
 *   Kept are the m pairs with the smallest key (d2, source index): d2 the fp32 squared distance that
 *   visma_icp_get_correspondences reports for the pair -- in every search precision --, the caller's source
 *   index breaking exact ties.  The kept set is unique and does not depend on the order of execution.
 *
 * A keep BELOW the true overlap stalls the registration (the shortest pairs are the ones that are aligned
 * already): on a full-overlap pair keep = 0.5 ends at 5.9e-2 relative error after 60 iterations where the
 * plain run reaches 8e-4.  With keep at the overlap a radius several times the default becomes usable.
 *
 * The estimator is point-to-point: SOLVER_KABSCH with or without scaling, or, on a context with
 * visma_icp_set_rotation_axis, the axis-constrained closed form.  The Gauss-Newton point-to-point solvers and
 * point-to-plane are not offered trimmed (VISMA_ICP_ERR_INVALID).  Sharded contexts (comm_init, comm_ipc_init,
 * set_allreduce with more than one rank, set_target_shard): VISMA_ICP_ERR_INVALID -- an order statistic across
 * ranks does not exist yet. */
typedef struct {
    int64_t kept;          /* m */
    double trimmed_rmse;   /* sqrt(sum of |p - q|^2 over the kept pairs / m); 0 when m = 0 */
    double d2_cut;         /* the largest kept fp32 squared distance; 0 when m = 0 */
} visma_icp_trim_info;

/* The statistics of the last visma_icp_nn_pass over the kept pairs only (same layout and centred frame as
 * visma_icp_reduce: out_stats[0] = m, out_stats[1] = the sum of |p - q|^2 over them, ...). */
VISMA_ICP_API int visma_icp_reduce_trimmed(visma_icp_ctx *ctx, double keep, double out_stats[VISMA_ICP_NSTATS],
                                           visma_icp_trim_info *info);
/* RegistrationICP's loop (Registration.cpp:167-185) with the trimmed pass in place of the plain one.  Its stop
 * test compares fitness and TRIMMED rmse (the objective this loop minimises) of consecutive passes.
 * out->num_correspondences = K, out->fitness = K / NS and out->inlier_rmse (over all K) are the untrimmed values
 * of the last pass (callers pick yaw winners by them); what the trimming did is in *info (may be NULL).
 * One launch sequence per pass (search, select, masked reduction); never the persistent launch.  keep = 1 is
 * visma_icp_run, bit for bit. */
VISMA_ICP_API int visma_icp_run_trimmed(visma_icp_ctx *ctx, const double init[16], double max_dist, double keep,
                                        int max_iter, double rel_fitness, double rel_rmse, int solver,
                                        int with_scaling, visma_icp_result *out, visma_icp_trim_info *info);
/* visma_icp_run_yaw_sweep with every start a trimmed run (one after the other); the winner is the first start
 * with strictly the most correspondences K.  per_level / per_level_info / best_info may be NULL.  Afterwards the
 * context holds the last pass of the LAST start (get_correspondences, get_kept_mask). */
VISMA_ICP_API int visma_icp_run_yaw_sweep_trimmed(visma_icp_ctx *ctx, int level, double max_dist, double keep,
                                                  int max_iter, double rel_fitness, double rel_rmse, int solver,
                                                  visma_icp_result *best, int *best_level,
                                                  visma_icp_result *per_level, visma_icp_trim_info *best_info,
                                                  visma_icp_trim_info *per_level_info);
/* kept_per_src[i] = 1 iff source point i (caller's order, NS entries) was kept by the last trimmed pass.
 * visma_icp_get_correspondences keeps returning all K pairs. */
VISMA_ICP_API int visma_icp_get_kept_mask(visma_icp_ctx *ctx, uint8_t *kept_per_src);

/* ---- robust ICP: M-estimators by iteratively re-weighted least squares (Huber 1964; Beaton & Tukey 1974; the
 * Cauchy / Lorentzian kernel as in Fitzgibbon 2003; tuning constants of Holland & Welsch 1977).  Every pair a pass
 * finds inside the radius enters the solve with a weight w(r) of its own residual r; the scale c of the weight
 * function is the caller's or comes from the median residual of the pass.  Unlike trimmed ICP it takes no overlap
 * share: prefer it where the overlap is not known per object.
 *
 *   Pairs: those of the last visma_icp_nn_pass (all K pairs inside the radius).
 *   Residual r_i >= 0: point-to-point |p_i - q_i|; point-to-plane |(p_i - q_i) . n_i|, n_i the target normal; in
 *   f64 from the coordinates the plain reduction sums from (the f64 copies where the search ran on them).
 *   Weights, for a scale c:
 *     HUBER   w = 1 if r <= c, else c / r
 *     TUKEY   w = (1 - (r/c)^2)^2 if r < c, else 0
 *     CAUCHY  w = 1 / (1 + (r/c)^2)
 *     c == 0: every family gives w = 1 if r == 0, else 0 (no NaN is produced)
 *     L2      w = 1: the plain run, bit for bit (as keep = 1 is for trimmed ICP)
 *   Scale:
 *     scale > 0   c = scale, in the caller's units, fixed for the whole run
 *     scale == 0  per pass c = max(tune * 1.4826 * med, min_scale); med the LOWER median of the residuals: the m-th
 *                 smallest with m = (K + 1) / 2, med = sqrt((double)v) with v
 *                   point-to-point: the m-th smallest fp32 squared distance among the pairs, as
 *                                   visma_icp_get_correspondences reports them (the scale is a function of the
 *                                   pass's public output alone);
 *                   point-to-plane: the m-th smallest of (float)(r_i^2).
 *                 K == 0: c = min_scale.
 *     tune == 0   the family's 95 %-efficiency constant: Huber 1.345, Tukey 4.685, Cauchy 2.385
 *   A non-finite or negative scale, tune or min_scale, or an unknown kernel: VISMA_ICP_ERR_INVALID before any pass.
 *
 * The weighted statistics have the layout of visma_icp_reduce with every pair's contribution times w_i:
 * out_stats[0] = sum w, out_stats[1] = sum w |p - q|^2, ...  The solves take them as they are: sum w == 0 gives the
 * identity update (the rule for K == 0); the Gauss-Newton solve keeps the reference's |det| < 1e-6 guard as it is --
 * weights SHRINK J^T J, so a pass whose weights are small overall meets that guard sooner than the plain pass.
 *
 * Estimators: point-to-point with SOLVER_KABSCH, with or without scaling; point-to-plane (plane != 0; it needs
 * visma_icp_set_target_normals_f64 -- without normals the run returns init, Registration.cpp:152-157); both with or
 * without visma_icp_set_rotation_axis.  The point-to-plane statistics are in the caller's (world) frame.
 * NOT offered (VISMA_ICP_ERR_INVALID): sharded contexts (comm_init, comm_ipc_init, set_allreduce with more than one
 * rank, set_target_shard), batches and the corpus, the Gauss-Newton point-to-point solvers, and robust weights
 * together with keep < 1. */
enum {
    VISMA_ICP_ROBUST_L2 = 0,
    VISMA_ICP_ROBUST_HUBER = 1,
    VISMA_ICP_ROBUST_TUKEY = 2,
    VISMA_ICP_ROBUST_CAUCHY = 3
};
typedef struct {
    int kernel;            /* VISMA_ICP_ROBUST_* */
    double scale;          /* > 0: fixed c; 0: automatic, per pass */
    double tune;           /* automatic scale: c = tune * 1.4826 * median; 0: the family's constant */
    double min_scale;      /* automatic scale: lower bound of c */
} visma_icp_robust;
typedef struct {
    double scale;              /* c of the last pass */
    double median_residual;    /* automatic scale: med of the last pass; 0 with a fixed scale or K = 0 */
    double weight_sum;         /* sum w (= the statistics' [0]) */
    int64_t zero_weight;       /* pairs with w == 0 */
    double robust_rmse;        /* sqrt(sum w |p - q|^2 / sum w); 0 when sum w is not positive */
} visma_icp_robust_info;

/* The weighted statistics of the last visma_icp_nn_pass (plane == 0: centred frame as visma_icp_reduce; plane != 0:
 * point-to-plane rows in the world frame). */
VISMA_ICP_API int visma_icp_reduce_robust(visma_icp_ctx *ctx, const visma_icp_robust *cfg, int plane,
                                          double out_stats[VISMA_ICP_NSTATS], visma_icp_robust_info *info);
/* RegistrationICP's loop (Registration.cpp:167-185) with the weighted pass.  Its stop test compares fitness (K / NS,
 * unweighted) and the ROBUST rmse of consecutive passes.  out->num_correspondences = K, out->fitness and
 * out->inlier_rmse are the unweighted values of the last pass; *info (may be NULL) is what the weights did there.
 * One launch sequence per pass; never the persistent launch.  kernel = L2 is visma_icp_run, bit for bit. */
VISMA_ICP_API int visma_icp_run_robust(visma_icp_ctx *ctx, const double init[16], double max_dist,
                                       const visma_icp_robust *cfg, int plane, int max_iter, double rel_fitness,
                                       double rel_rmse, int with_scaling, visma_icp_result *out,
                                       visma_icp_robust_info *info);
/* visma_icp_run_yaw_sweep with every start a robust run (one after the other); the winner is the first start with
 * strictly the most correspondences K.  per_level / per_level_info / best_info may be NULL.  Afterwards the context
 * holds the last pass of the LAST start. */
VISMA_ICP_API int visma_icp_run_yaw_sweep_robust(visma_icp_ctx *ctx, int level, double max_dist,
                                                 const visma_icp_robust *cfg, int plane, int max_iter,
                                                 double rel_fitness, double rel_rmse, visma_icp_result *best,
                                                 int *best_level, visma_icp_result *per_level,
                                                 visma_icp_robust_info *best_info, visma_icp_robust_info *per_level_info);
/* w_per_src[i] = the weight of source point i (caller's order, NS entries) in the last robust pass, 0 where the
 * point has no pair.  VISMA_ICP_ERR_STATE before a robust pass.  (After an L2 run: 1 for every pair.) */
VISMA_ICP_API int visma_icp_get_pair_weights(visma_icp_ctx *ctx, double *w_per_src);

/* ---- generalized ICP (plane-to-plane; Segal, Haehnel, Thrun: "Generalized-ICP", RSS 2009).  Every pair's residual is
 * weighted by the inverse of the sum of both points' local surface covariances, so a source point may slide along
 * either surface at no cost.  The covariance of a surface element is a function of its normal alone,
 * C = I - (1 - epsilon) n n^T (a neighbourhood covariance with its eigenvalues replaced by (1, 1, epsilon)): the method
 * takes source normals, target normals and epsilon, no covariance arrays.  Prefer it where the source is a sampled
 * CAD model whose normals are exact.
 *
 *   Pairs: those of the last visma_icp_nn_pass (all K pairs inside the radius), (i, j) = (source, target).  In f64:
 *     p = T s_i as the robust pass forms it, q = t_j, d = p - q
 *     m = R n^s_i (the source normal turned by the rotation of T), n = n^t_j
 *     C = 2 I - (1 - epsilon)(n n^T + m m^T)
 *     M = C^-1 by the closed-form adjugate / determinant of a symmetric 3 x 3
 *     J = [ -[p]x | I ] (3 x 6); the unknowns x = [alpha beta gamma tx ty tz] as in the 6 x 6 point-to-plane path
 *   Frame and offset as visma_icp_reduce_robust with plane != 0: rows in the caller's (world) frame.
 *   Normals are used AS GIVEN: unit length is the caller's business (a longer normal makes C indefinite beyond
 *   |n|^2 = 2 / (1 - epsilon)).  A zero normal leaves its point isotropic (its share of C is I).  A non-finite normal
 *   reaches the sums only, never an index or an address.
 *   epsilon = 1 is point-to-point (M = I / 2); epsilon -> 0 with the source isotropic is point-to-plane.
 *
 * Statistics in the layout of visma_icp_reduce (the host solves take them unchanged):
 *   [0] = K   [1] = sum |d|^2 (unweighted: inlier_rmse is the plain one)
 *   [2:23] = upper triangle of sum J^T M J   [23:29] = sum J^T M d   [29:38] = 0
 * and in visma_icp_gicp_info: cost = sum d^T M d, mahalanobis_rmse = sqrt(cost / K), 0 when K = 0.
 * No floating-point atomics: a run is bit-identical to itself.
 *
 * The update solves A x = -b as visma_icp_solve_from_stats(VISMA_ICP_SOLVER_GN_EULER) does -- the reference's
 * |det A| < 1e-6 guard and its Rz Ry Rx map --, on a context with a rotation axis as
 * visma_icp_solve_from_stats_axis(plane = 1).  The eigenvalues of M lie in [1/2, 1/(2 epsilon)] for unit normals, so
 * det A >= det(J^T J of the point-to-point Gauss-Newton step) / 64: the guard rejects a pass no sooner than at 64 x
 * the determinant at which it rejects the point-to-point Gauss-Newton step over the same pairs.
 *
 * epsilon outside (0, 1] or not finite: VISMA_ICP_ERR_INVALID before any pass.  NOT offered (VISMA_ICP_ERR_INVALID):
 * sharded contexts (comm_init, comm_ipc_init, set_allreduce with more than one rank, set_target_shard).  Not
 * combined with robust weights or trimming; no batches, no corpus. */
typedef struct {
    double cost;               /* sum d^T M d of the last pass */
    double mahalanobis_rmse;   /* sqrt(cost / K); 0 when K = 0 */
} visma_icp_gicp_info;

/* Normals of the source, one per point in the caller's order (nxyz[i * stride + 0..2]), after the source is set; ns
 * must be the source's count (VISMA_ICP_ERR_INVALID).  A new source drops them, as a new target drops its normals. */
VISMA_ICP_API int visma_icp_set_source_normals_f64(visma_icp_ctx *ctx, const double *nxyz, int64_t ns, int stride);
/* The generalized statistics of the last visma_icp_nn_pass.  Without both sets of normals, or before a pass:
 * VISMA_ICP_ERR_STATE. */
VISMA_ICP_API int visma_icp_reduce_gicp(visma_icp_ctx *ctx, double epsilon, double out_stats[VISMA_ICP_NSTATS],
                                        visma_icp_gicp_info *info);
/* RegistrationICP's loop (Registration.cpp:167-185) with the generalized pass.  Its stop test compares fitness
 * (K / NS) and mahalanobis_rmse of consecutive passes.  out->num_correspondences = K, out->fitness and
 * out->inlier_rmse are the unweighted values of the last pass; *info (may be NULL) belongs to that pass.  Without both
 * sets of normals the run returns init (Registration.cpp:152-157, as point-to-plane does).  One launch sequence per
 * pass; never the persistent launch. */
VISMA_ICP_API int visma_icp_run_gicp(visma_icp_ctx *ctx, const double init[16], double max_dist, double epsilon,
                                     int max_iter, double rel_fitness, double rel_rmse, visma_icp_result *out,
                                     visma_icp_gicp_info *info);
/* visma_icp_run_yaw_sweep with every start a generalized run (one after the other); the winner is the first start
 * with strictly the most correspondences K.  per_level / per_level_info / best_info may be NULL.  Afterwards the
 * context holds the last pass of the LAST start. */
VISMA_ICP_API int visma_icp_run_yaw_sweep_gicp(visma_icp_ctx *ctx, int level, double max_dist, double epsilon,
                                               int max_iter, double rel_fitness, double rel_rmse,
                                               visma_icp_result *best, int *best_level, visma_icp_result *per_level,
                                               visma_icp_gicp_info *best_info, visma_icp_gicp_info *per_level_info);

/* ---- colored ICP (Park, Zhou, Koltun: "Colored Point Cloud Registration Revisited", ICCV 2017; the reference's
 * O3D/Core/Registration/ColoredICP.cpp).  Every pair enters the normal equations with two rows: the point-to-plane row and
 * a photometric row that compares the source point's intensity with the target's, carried along the target's colour
 * gradient to the source point's projection into the target's tangent plane.  A flat or smooth surface leaves the motion
 * inside the surface free for every geometric estimator (on a plane the point-to-plane 6 x 6 is singular and the
 * |det| < 1e-6 guard returns the identity); a texture pins it.  Prefer it for textured surfaces whose geometry leaves a
 * motion free.
 *
 *   Of a colour only the intensity I = (r + g + b) / 3.0 is kept (ColoredICP.cpp:94-95: f64, in that order), one f64 per
 *   point; there is no fp32 copy (k / 255 is not an fp32 number, and the photometric residual is a difference of nearby
 *   values).
 *
 *   The colour gradient g of target point k (ColoredICP.cpp:74-137), normal n, intensity I_k: neighbours by the Hybrid
 *   search (radius, max_nn) in the order of visma_icp_estimate_normals(search_type = 2); fewer than 3 list entries: g = 0.
 *   Else entry 0 is skipped whatever index it holds (the reference takes it for the point itself); every other entry a
 *   gives the row a' - p, a' = a - ((a - p).n) n, with the right side I_a - I_k; one more row (nn - 1) n, nn the list
 *   length, with the right side 0.  A^T A and A^T b are summed in f64 in list order; |det(A^T A)| < 1e-6 or a determinant
 *   that is not finite: g = 0 (Eigen.cpp:41-43); else the symmetric 3 x 3 is solved in closed form (the reference: LDLT --
 *   agreement to rounding, not to the bit).  max_nn outside [3, 170]: VISMA_ICP_ERR_INVALID (the lists live in LDS).
 *
 *   Pairs: those of the last visma_icp_nn_pass, (i, j) = (source, target).  In f64, lambda = lambda_geometric:
 *     p = T s_i as the generalized pass forms it, q = t_j, n = n_j, g = g_j
 *     r_g = sqrt(lambda) (p - q).n                      J_g = sqrt(lambda) [p x n | n]
 *     p' = p - ((p - q).n) n
 *     r_c = sqrt(1 - lambda) (I_s - (g.(p' - q) + I_t))  h = -(I - n n^T) g    J_c = sqrt(1 - lambda) [p x h | h]
 *   Frame and offset as visma_icp_reduce_gicp: rows in the caller's (world) frame.  Normals, colours and gradients are
 *   used AS GIVEN; a non-finite one reaches the sums only, never an index or an address.
 *
 * Statistics in the layout of visma_icp_reduce (the host solves take them unchanged: VISMA_ICP_SOLVER_GN_EULER, on a
 * context with a rotation axis visma_icp_solve_from_stats_axis(plane = 1)):
 *   [0] = K   [1] = sum |p - q|^2   [2:23] = upper triangle of sum (J_g^T J_g + J_c^T J_c)
 *   [23:29] = sum (J_g^T r_g + J_c^T r_c)   [29:38] = 0
 * and in visma_icp_colored_info the cost sum (r_g^2 + r_c^2) -- what the reference's ComputeRMSE returns
 * (ColoredICP.cpp:203-232) -- and its two parts.  No floating-point atomics: a run is bit-identical to itself.
 *
 * lambda_geometric outside [0, 1] or not finite becomes 0.968, as ColoredICP.cpp:54-55 does: NOT an error.
 * NOT offered: sharded contexts (VISMA_ICP_ERR_INVALID, as the generalized pass); a yaw sweep, batches or a corpus
 * (sampled CAD models carry no colour); a combination with trimming, robust weights or the generalized weights. */
typedef struct {
    double cost;               /* sum r_g^2 + r_c^2 of the last pass */
    double geometric_cost;     /* sum r_g^2 */
    double photometric_cost;   /* sum r_c^2 */
} visma_icp_colored_info;

/* Colours of the source / the target, one per point in the caller's order (rgb[i * stride + 0..2]), after the cloud is
 * set; the count must be the cloud's (VISMA_ICP_ERR_INVALID).  A new source or target drops its colours, as it drops
 * its normals. */
VISMA_ICP_API int visma_icp_set_source_colors_f64(visma_icp_ctx *ctx, const double *rgb, int64_t ns, int stride);
VISMA_ICP_API int visma_icp_set_target_colors_f64(visma_icp_ctx *ctx, const double *rgb, int64_t nt, int stride);
/* Computes the colour gradient of the context's target and keeps it on the device.  Without target normals and target
 * colours: VISMA_ICP_ERR_STATE.  A new target, new target normals or new target colours drop it.  The points and
 * normals are the copies the passes read: f64 where the context holds them, else fp32. */
VISMA_ICP_API int visma_icp_prepare_colored(visma_icp_ctx *ctx, double radius, int max_nn);
/* ... nt x 3 doubles in the caller's order; VISMA_ICP_ERR_STATE without a gradient. */
VISMA_ICP_API int visma_icp_get_color_gradient(visma_icp_ctx *ctx, double *out, int64_t nt);
/* The colored statistics of the last visma_icp_nn_pass.  Before a pass, or without target normals, target colours, source
 * colours or the gradient: VISMA_ICP_ERR_STATE. */
VISMA_ICP_API int visma_icp_reduce_colored(visma_icp_ctx *ctx, double lambda_geometric, double out_stats[VISMA_ICP_NSTATS],
                                           visma_icp_colored_info *info);
/* RegistrationColoredICP (ColoredICP.cpp:236-246): the gradient by visma_icp_prepare_colored(2 * max_dist, 30) unless one
 * for exactly these two values is held, then RegistrationICP's loop (Registration.cpp:159-185) with the colored pass.
 * Its stop test compares the plain fitness (K / NS) and the plain inlier_rmse of consecutive passes, as the reference's
 * loop does for every estimator -- not the colored cost.  *info (may be NULL) belongs to the last pass.  Without target
 * normals, target colours or source colours the run returns init (as visma_icp_run_gicp without normals).  One launch
 * sequence per pass; never the persistent launch. */
VISMA_ICP_API int visma_icp_run_colored(visma_icp_ctx *ctx, const double init[16], double max_dist, double lambda_geometric,
                                        int max_iter, double rel_fitness, double rel_rmse, visma_icp_result *out,
                                        visma_icp_colored_info *info);

/* ---- batched small problems (AnnotationTool loop, src/annotation.cpp:103-168) */

typedef struct {
    const double *src_xyz; int64_t ns; /* AoS f64, stride 3 */
    const double *tgt_xyz; int64_t nt;
    double init[16];
    double max_dist;
} visma_icp_problem;

/* The same sweep with the point-to-plane estimator (ICP.point_to_plane of cfg/tool.json,
 * src/annotation.cpp:45-50): needs target normals (visma_icp_set_target_normals_f64); without
 * them every start returns its initial transform, like Registration.cpp:152-157. */
VISMA_ICP_API int visma_icp_run_yaw_sweep_point_to_plane(visma_icp_ctx *ctx, int level,
                                                         double max_dist, int max_iter,
                                                         double rel_fitness, double rel_rmse,
                                                         visma_icp_result *best, int *best_level,
                                                         visma_icp_result *per_level);
/* n independent ICPs advanced in lock step, one grid launch per iteration. */
VISMA_ICP_API int visma_icp_run_batch(visma_icp_ctx *ctx, const visma_icp_problem *probs,
                                      int n, int max_iter, double rel_fitness,
                                      double rel_rmse, int solver,
                                      visma_icp_result *out);
/* The same batch over several WORKER contexts (any number on the same GPU -- each has its own stream -- and/or on
 * several GPUs): problems that pass the same target cloud stay together, the groups are dealt to the contexts by
 * size, every context runs its share as one visma_icp_run_batch on its own host thread, the shares side by side:
 * while one worker packs, uploads or solves, the others' searches have the GPU (config 3 on one MI355X: two workers
 * ~1.15x one).  out[] equals the single-context call's.  Returns the first error (message in errbuf). */
VISMA_ICP_API int visma_icp_run_batch_multi(visma_icp_ctx *const *ctxs, int n_ctx, const visma_icp_problem *probs, int n,
                                            int max_iter, double rel_fitness, double rel_rmse, int solver,
                                            visma_icp_result *out, char *errbuf, size_t errbuf_len);
/* The same with the point-to-plane estimator (TransformationEstimationPointToPlane,
 * O3D/Core/Registration/TransformationEstimation.cpp:101-134): tgt_normals[i] are the normals of
 * probs[i].tgt_xyz (AoS f64, stride 3; the same pointer wherever the same target pointer is
 * passed).  A problem whose target has no normals (NULL) returns its initial transform, like
 * Registration.cpp:152-157. */
VISMA_ICP_API int visma_icp_run_batch_point_to_plane(visma_icp_ctx *ctx, const visma_icp_problem *probs,
                                                     const double *const *tgt_normals, int n,
                                                     int max_iter, double rel_fitness, double rel_rmse,
                                                     visma_icp_result *out);

/* ---- the corpus: every (scene, CAD candidate) pair, one orientation-constrained registration each --------
 * The per-object loop of AnnotationTool (src/annotation.cpp:103-168: for each entry of objects.json ->
 * RegisterModelToScene(model, scan, config["ICP"])) over a whole corpus, as a native work queue: ONE HOST
 * THREAD PER CONTEXT (= per GPU) pulls chunks of `chunk` items from a counter, runs their `level` yaw starts
 * (src/annotation.cpp:35-39) as one batch (visma_icp_run_batch: clouds passed by several problems are uploaded
 * and gridded once) and keeps, per item, the first start with strictly the most correspondences
 * (src/annotation.cpp:59-61).  No collective, no exchange: replicas only.
 * `counter` (may be NULL: a private one) is advanced with atomic adds: ranks in OTHER processes can pull from
 * the same queue when it lives in shared memory (bench.py --workload c5 --gpus N: one process per GPU); it must
 * be 0 when the pass starts.  results[i].device is the index of the context that registered item i, -1 when
 * another process took it.  Returns the first error of any thread (message in errbuf). */
typedef struct {
    const double *model_xyz; int64_t n_model;   /* source: the sampled CAD model (AoS f64, stride 3) */
    const double *scene_xyz; int64_t n_scene;   /* target: the scan */
} visma_icp_corpus_item;
typedef struct {
    int level;               /* rotation_level (cfg/tool.json:17): yaw starts R_y(2 pi k / level) */
    double max_dist;         /* distance_threshold */
    int max_iter;            /* ICPConvergenceCriteria: 30 */
    double rel_fitness, rel_rmse;
    int solver;              /* VISMA_ICP_SOLVER_KABSCH = the reference's estimator */
    int chunk;               /* items per pull (<= 0: 8 -> 8 x 24 = 192 registrations in flight per launch) */
} visma_icp_corpus_params;
typedef struct {
    visma_icp_result best;   /* RegisterModelToScene's choice (transformation_ = what it returns) */
    int32_t best_level;      /* which start it was; -1: no start found a correspondence (best = identity) */
    int32_t device;          /* index into ctxs of the context that did it; -1: not done by this call */
    int64_t iterations_all_starts;   /* ICP iterations summed over the item's `level` registrations */
} visma_icp_corpus_result;
VISMA_ICP_API int visma_icp_run_corpus(visma_icp_ctx *const *ctxs, int n_ctx, const visma_icp_corpus_item *items,
                                       int64_t n_items, const visma_icp_corpus_params *params, int64_t *counter,
                                       visma_icp_corpus_result *results, char *errbuf, size_t errbuf_len);

/* ---- the gravity alignment and pose composition of feh::AnnotationTool (src/annotation.cpp:82-91, 111-153) --------
 * Host arithmetic (no context): the steps between the scan / the CAD model and RegisterModelToScene.
 *   visma_geom_find_plane_normal       feh::FindPlaneNormal (include/geometry.h:18-26): unit normal of the plane through
 *                                      n points = right singular vector of the smallest singular value of their
 *                                      covariance, WITH THE SIGN Eigen 3.3.2's JacobiSVD gives it (the reference turns
 *                                      this normal onto +Y: the sign decides which way up the scene ends)
 *   visma_geom_jacobi_svd3             Eigen::JacobiSVD<Matrix3d>(A, ComputeFullU | ComputeFullV), row-major 3x3
 *   visma_geom_rotation_between_vectors  feh::RotationBetweenVectors (core/utils.h:229-233) =
 *                                      Eigen::Quaterniond::FromTwoVectors(u, v).toRotationMatrix(), row-major 3x3
 *   visma_geom_centre_on_floor         (-mean_x, -min_y, -mean_z) of a cloud: the translation of T1 / T2
 *                                      (src/annotation.cpp:114-119, 128-132)
 *   visma_annot_total_pose             Ttot = (T1 T0)^-1 T3 T2 with the reference's rigid inverse (:147-153), row-major 4x4 */
VISMA_ICP_API int visma_geom_find_plane_normal(const double *xyz, int64_t n, double normal_out[3]);
VISMA_ICP_API int visma_geom_jacobi_svd3(const double A[9], double U[9], double S[3], double V[9]);
VISMA_ICP_API int visma_geom_rotation_between_vectors(const double u[3], const double v[3], double R[9]);
VISMA_ICP_API int visma_geom_centre_on_floor(const double *xyz, int64_t n, double t_out[3]);
VISMA_ICP_API int visma_annot_total_pose(const double T0[16], const double T1[16], const double T2[16], const double T3[16],
                                         double Ttot[16]);

/* ---- options / measurement --------------------------------------------- */
/* AUTO (default) uses the radius-cell grid whenever the target/radius make it
 * worthwhile and the LDS-tiled brute-force kernel otherwise; BRUTE / GRID force
 * one.  The grid is (re)built on the GPU when the target or the radius changes. */
VISMA_ICP_API int visma_icp_set_nn_mode(visma_icp_ctx *ctx, int nn_mode);
/* Arithmetic of the nearest-neighbour search.
 *   0            fp32 only: fp32 distances on the fp32-rounded clouds centred on the target
 *                centroid (the round-1 kernels).  Near-ties between two candidates, and
 *                candidates within ~1e-6 of the radius, can be decided differently from the
 *                reference's f64 KD-tree (about one query in 1e5); one flipped pair among K
 *                moves the update by ~(pair spacing)/K.
 *   1 (default)  exact: candidates are ranked in fp32, the best two are kept, and whenever
 *                the runner-up or the radius lies within the rounding band of the best
 *                (2.4e-7 (|p|_1 + r) + 4.8e-7 r on the distance, both operands fp32-rounded
 *                f64 coordinates) the candidates concerned are re-ranked in f64 with the
 *                reference's arithmetic: the f64 sum of squares of FLANN L2<double>, the
 *                strict d2 < (double)(float)(r*r) test, lowest index on exact ties.  Three
 *                candidates inside the band: the query rescans its cells in f64.  Source
 *                transform and statistics in f64 from the caller's f64 coordinates (shifted by
 *                the target centroid in f64 on upload).  The
 *                correspondences are those of mode 2 (and of the reference) for every input;
 *                every path has this flavour -- grid (single, sweep, batch), brute force,
 *                target-sharded.  Clouds given as fp32 are promoted on the device.
 *   2            f64 search: every candidate distance in f64.  Same results as 1, slower
 *                (+30 % at 64k -> 256k); kept as the in-library check of mode 1.
 * Takes effect at the next cloud upload.  Mode 1 runs at the speed of mode 0 (measured on MI355X,
 * profiles/r02_probe_keepq.txt: 56.3 vs 58.6 us per iteration at C4, 30.7 vs 29.0 at 64k -> 1M).
 * visma_icp_get_search_precision_used reports what the last run executed (0 / 1 / 2). */
VISMA_ICP_API int visma_icp_set_search_precision(visma_icp_ctx *ctx, int mode);
/* What the last pass ran: 0 fp32 ranking only, 1 exact (fp32 ranking + f64 re-rank), 2 f64. */
VISMA_ICP_API int visma_icp_get_search_precision_used(visma_icp_ctx *ctx, int *is_f64);
/* Which search the last nn_pass used (VISMA_ICP_NN_BRUTE or VISMA_ICP_NN_GRID). */
VISMA_ICP_API int visma_icp_get_nn_mode_used(visma_icp_ctx *ctx, int *nn_mode);
/* Kernel timing with HIP events on the context's stream (read with
 * visma_icp_get_timing).  0 = off, 1 = every launch, n > 1 = every n-th ICP pass
 * (the event records themselves cost ~3 us each; sampling keeps a timed run close
 * to an untimed one).  Candidate counting of the grid kernel follows the same switch. */
VISMA_ICP_API int visma_icp_set_profiling(visma_icp_ctx *ctx, int enabled);
VISMA_ICP_API int visma_icp_get_timing(visma_icp_ctx *ctx, visma_icp_timing *out,
                                       int reset);
/* The same for callers compiled against another revision of this header: at most `struct_size` bytes of the
 * structure are written (the structure only ever grows at its end; round 4 added persist_* -- a caller built against
 * round 3's header passes ITS sizeof and is not overrun).  visma_icp_get_timing(ctx, out, reset) is
 * visma_icp_get_timing_sized(ctx, out, sizeof(visma_icp_timing) OF THE LIBRARY'S BUILD, reset). */
VISMA_ICP_API int visma_icp_get_timing_sized(visma_icp_ctx *ctx, void *out, size_t struct_size, int reset);

/* ---- the persistent launch of a host loop -------------------------------------------------------------------------
 * visma_icp_run / visma_icp_iterate on one GPU (and source-sharded ranks on their own GPUs) keep ONE launch of the
 * search kernel alive for the passes of their loop: the next transform goes to the launch through a command block, the
 * statistics come back as always -- same results as one launch per pass, bit for bit.  Such a launch
 * needs every one of its workgroups resident at once and SPINS between passes: while a loop runs, the compute units it
 * holds are not available to other streams or processes.  An integrator decides with these three calls (they replace
 * nothing in the reference, which has no device to share):
 *  visma_icp_set_persistent(ctx, enabled, timeout_ms): 1 (default) / 0 = one launch per pass on this context (also
 *    VISMA_ICP_PERSIST=0).  timeout_ms > 0: how long the launch waits for the host's next command before it ends by
 *    itself (default 200; the loop then carries on with ordinary launches, same results).  After such an abort the
 *    context COOLS DOWN: its next 8 host loops launch once per pass, then persistent launches are tried again by
 *    themselves; visma_icp_set_persistent(ctx, 1, ...) re-arms them at once.
 *  visma_icp_set_persistent_cu_share(share): PER PROCESS, 0 < share <= 1 (default 1; also VISMA_ICP_PERSIST_CU_SHARE):
 *    the largest part of a device's workgroup slots a persistent launch may hold.  A loop whose launch would need
 *    more runs one launch per pass, which other streams' kernels interleave with (a 262,144-point source needs all
 *    slots of an MI355X; 65,536 points a quarter).  Queue workers of visma_icp_run_corpus / batches never start
 *    persistent launches.
 *  visma_icp_get_persistent_info(ctx, out): what happened so far on this context. */
typedef struct {
    int struct_size;               /* in: sizeof(visma_icp_persistent_info) of the caller's build */
    int enabled;                   /* the next host loop may start a persistent launch: the user's setting AND not cooling
                                      down (0 during the 8 loops after an abort, although the setting is still 1) */
    int last_loop_persistent;      /* the last finished host loop ran (part of) its passes in a persistent launch */
    int last_loop_passes;          /* ... that many of them */
    double launches, passes;       /* persistent launches / passes inside them since the context was created */
    double aborts;                 /* launches that ended by themselves or whose host came back too late */
    double timeout_ms;             /* the patience in force */
    double cu_share;               /* the process-wide share in force */
    int device_slots;              /* workgroups of this kernel the device holds at once (0: not asked yet) */
    int reserved;
} visma_icp_persistent_info;
VISMA_ICP_API int visma_icp_set_persistent(visma_icp_ctx *ctx, int enabled, double timeout_ms);
VISMA_ICP_API int visma_icp_set_persistent_cu_share(double share);
VISMA_ICP_API int visma_icp_get_persistent_info(visma_icp_ctx *ctx, visma_icp_persistent_info *out);

/* ---- radii that are large against the target's point spacing --------------------------------------------------------
 * The grid search lists the 27 radius-sized cells around a query (KDTreeFlann.cpp:164-189 asks for the nearest point
 * within the radius).  When such a cell holds hundreds of points -- a radius of tens of point spacings -- the library builds
 * cells of a few point spacings instead and searches them in rings of rows around the query, nearest first, bounded by the
 * best candidate so far and, after the first pass, by the previous winner (grid_ring.hip): the same correspondences, bit
 * for bit; the cost of a query follows the number of points nearer than its nearest neighbour, not the radius.
 *  visma_icp_set_ring_search(ctx, mode): -1 (default) by the occupancy of the radius-sized cells (>= 48 points per
 *    occupied cell for yaw sweeps, whose far-off starts leave most queries without a partner -- the ring walk's worst
 *    case --, >= 20 for one registration at a time; VISMA_ICP_RING_OCCUPANCY sets the first), 0 never, 1 whenever the f64 views exist and a finer table fits (also
 *    VISMA_ICP_RING=0/1 when the context is created).  Takes effect at the next grid build (new target or radius).
 *  visma_icp_get_ring_search(ctx, ...): what the current grid is: *rings > 0 = ring search with that many rings at most,
 *    *cell = the cell edge, *occupancy = points per occupied radius-sized cell as counted (0 = not counted).  Any pointer may
 *    be NULL.  Replaces nothing in the reference (FLANN's KD-tree has no such regime change). */
VISMA_ICP_API int visma_icp_set_ring_search(visma_icp_ctx *ctx, int mode);
VISMA_ICP_API int visma_icp_get_ring_search(visma_icp_ctx *ctx, int *rings, double *cell, double *occupancy);

/* ---- multi-GPU (one process per GPU; source-sharded) -------------------- */

#define VISMA_ICP_UNIQUE_ID_BYTES 128
/* Rank 0 creates the id, the host program broadcasts it (any transport), every
 * rank calls comm_init.  After that visma_icp_reduce / visma_icp_run sum the
 * per-shard statistics with ONE ncclAllReduce(38 x f64) per iteration over
 * xGMI; every rank solves the same system and holds the same transform.
 * RCCL is loaded at run time (dlopen) -- a single-GPU build needs none. */
VISMA_ICP_API int visma_icp_comm_unique_id(void *out_id /* 128 bytes */);
VISMA_ICP_API int visma_icp_comm_init(visma_icp_ctx *ctx, int rank, int nranks,
                                      const void *unique_id);
/* Peer-to-peer alternative on one node (preferred: ~3 us per iteration against ~30 us for a
 * 304-byte ncclAllReduce).  Every rank exports the handle of its mailbox (uncached device
 * memory), the host program all-gathers the handles (any transport), every rank calls
 * comm_ipc_init with ALL of them (nranks x VISMA_ICP_IPC_HANDLE_BYTES, rank order).  From then on
 * each iteration's 38 statistics are exchanged inside the search launch (by the workgroup that
 * finishes the fold; one small extra launch on the brute-force path): remote 16-byte stores
 * {value, sequence tag} into the peers' mailboxes over xGMI, every rank sums in rank order
 * (identical transforms on all ranks, bit for bit), the result goes straight to the host.
 * nranks <= 16; ranks may share a device (tests).  comm_ipc_init is COLLECTIVE: it ends with a
 * handshake (one all-reduce of known values, every rank must enter within tens of seconds) and
 * fails with VISMA_ICP_ERR_HIP when a peer's stores do not arrive -- fall back to
 * visma_icp_comm_init on every rank then.  comm_ipc_export starts a NEW session: it drops the mappings
 * of an earlier one, clears the mailbox and restarts the exchange count (which lives in device memory and
 * advances only when an exchange runs), so a retry after a failed handshake begins with export on every
 * rank again. */
#define VISMA_ICP_IPC_HANDLE_BYTES 64
VISMA_ICP_API int visma_icp_comm_ipc_export(visma_icp_ctx *ctx, void *out_handle /* 64 bytes */);
VISMA_ICP_API int visma_icp_comm_ipc_init(visma_icp_ctx *ctx, int rank, int nranks,
                                          const void *all_handles);
/* Alternative to RCCL: the host supplies the all-reduce (used by the CPU
 * `gloo` tests).  fn must sum `n` doubles in place across ranks. */
typedef int (*visma_icp_allreduce_fn)(void *user, double *inout, int n);
VISMA_ICP_API int visma_icp_set_allreduce(visma_icp_ctx *ctx, visma_icp_allreduce_fn fn,
                                          void *user, int rank, int nranks);
/* TARGET-sharded ranks (the literal reading of "the target cloud is sharded
 * across the GPUs"; for targets that exceed one GPU).  Every rank holds ALL source
 * points and target points [global_offset, global_offset + nt) of a target of
 * global_nt points (< 2^31).  Summing per-shard accumulators directly would count a
 * source point once per shard that has a neighbour of it, which is not the reference
 * algorithm (Registration.cpp:53-85 keeps ONE nearest neighbour); the exact scheme is
 * two collectives per iteration: a MIN all-reduce of NS packed keys
 * (fp32 d2 bits << 32 | global index: smallest distance, lowest index on ties), then
 * the owner of each winner accumulates it and the 38 statistics are summed as in the
 * source-sharded mode.  Correspondence indices are global.  `centre` must be the SAME
 * point on every rank (e.g. the centroid of the whole target); call this BEFORE
 * visma_icp_set_clouds_f64.  global_nt = 0 switches the mode off.  Needs
 * visma_icp_comm_init (RCCL) or both host callbacks below; the host loop only. */
VISMA_ICP_API int visma_icp_set_target_shard(visma_icp_ctx *ctx, int64_t global_offset,
                                             int64_t global_nt, const double centre[3]);
/* Host-supplied MIN all-reduce of n uint64 keys, in place (tests / other transports). */
typedef int (*visma_icp_minreduce_fn)(void *user, uint64_t *inout, int64_t n);
VISMA_ICP_API int visma_icp_set_minreduce(visma_icp_ctx *ctx, visma_icp_minreduce_fn fn, void *user);
/* Total source points over all ranks (fitness denominator); 0 = local ns. */
VISMA_ICP_API int visma_icp_set_global_source_count(visma_icp_ctx *ctx, int64_t ns_total);

/* open3d::VoxelDownSample (O3D/Core/Geometry/DownSample.cpp:179-220), the step
 * both callers run right before ICP (src/annotation.cpp:112,
 * src/evaluation.cpp:258).  AoS f64 in (stride 3; normals / colors may be NULL),
 * AoS f64 out (buffers of n rows).  Every output value is bit-identical to the
 * reference's (same f64 voxel index expression, sums taken in input order); the
 * ORDER of the voxels is ascending (ix,iy,iz) here, hash-map order there.
 * voxel_size <= 0, or voxel_size * INT_MAX < extent, give *n_out = 0 like the
 * reference. */
VISMA_ICP_API int visma_icp_voxel_down_sample(visma_icp_ctx *ctx, const double *xyz, int64_t n,
                                              const double *normals, const double *colors,
                                              double voxel_size, double *out_xyz,
                                              double *out_normals, double *out_colors,
                                              int64_t *n_out);

/* feh::SamplePointCloudFromMesh (include/geometry.h:29-64), the step that builds
 * the ICP source from a CAD mesh (src/evaluation.cpp:252, src/annotation.cpp:126).
 * V: nv x 3 f64, F: nf x 3 int32.  Sample i uses three uniforms (r, a, b): from
 * `uniforms` (3n doubles) when given, else from a counter-based Philox4x32-10
 * keyed by `seed` (the reference seeds std::knuth_b from the clock, so only its
 * mapping uniforms -> points can be matched).  reference_quirks != 0 reproduces
 * that mapping exactly: face k for r in [cdf[k], cdf[k+1]) (one face late, never
 * the last face, NO point for r < cdf[0]) and v0 + a(v1-v0) + b(v2-v0) over the
 * whole parallelogram -- about half of those points lie off the surface.
 * reference_quirks == 0 samples the triangles themselves, area-uniformly.
 * out_xyz holds n rows; *n_out <= n. */
VISMA_ICP_API int visma_icp_sample_mesh(visma_icp_ctx *ctx, const double *V, int64_t nv,
                                        const int32_t *F, int64_t nf, int64_t n,
                                        int reference_quirks, uint64_t seed,
                                        const double *uniforms, double *out_xyz, int64_t *n_out);
/* open3d::EstimateNormals (O3D/Core/Geometry/EstimateNormals.cpp:114-153; PointCloud.h:140-146) on the
 * GPU: the normal of every point from the covariance of its neighbours, found by one of KDTreeFlann's
 * three searches (KDTreeFlann.cpp:114-189) --
 *   search_type 0  KDTreeSearchParamKNN(knn)            the knn nearest points (the point itself included)
 *               1  KDTreeSearchParamRadius(radius)      every point with d2 < (double)(float)(radius^2)
 *               2  KDTreeSearchParamHybrid(radius, knn) the knn nearest of those
 * -- fewer than 3 neighbours: (0,0,1); normals_in (may be NULL) are the cloud's existing normals, whose
 * sign is kept (EstimateNormals.cpp:133-146).  n x 3 f64 in, n x 3 f64 out.  Any knn /
 * max_nn: lists of up to 170 entries live in LDS, longer ones (and dense Radius searches) in a heap per point in
 * global memory; Radius results are summed in the order of the reference's result list too.
 * The lists are in flann's order, ascending (d2, index), d2 flann's f64 sum; where distances tie exactly the lower index
 * comes first.  A neighbour at a NaN distance is never listed, in any search type: a point with a NaN coordinate is
 * nobody's neighbour and has none itself (its normal is (0,0,1)), every other point's normal is what it is on the cloud
 * without that point, and the result is a function of the input.  An infinite distance (a point with an infinite
 * coordinate) is a legitimate KNN entry, behind every finite one. */
VISMA_ICP_API int visma_icp_estimate_normals(visma_icp_ctx *ctx, const double *xyz, int64_t n,
                                             const double *normals_in, int search_type, int knn,
                                             double radius, double *normals_out);

/* The colour gradient per point of colored ICP (the block above visma_icp_colored_info states it) for any cloud:
 * xyz, normals, colors n x 3 f64 in, out_grad n x 3 f64.  max_nn outside [3, 170]: VISMA_ICP_ERR_INVALID. */
VISMA_ICP_API int visma_icp_color_gradient(visma_icp_ctx *ctx, const double *xyz, int64_t n, const double *normals,
                                           const double *colors, double radius, int max_nn, double *out_grad);

/* ---- registration without an initial pose: FPFH features, their matching, fast global registration -----------------
 * Every other registration of this header starts from a pose the caller supplies.  Where there is none: the FPFH of
 * both clouds, visma_icp_fast_global_registration on them, then any ICP of this header from the pose it returns
 * (INTEGRATION.md).
 *
 * open3d::ComputeFPFHFeature (O3D/Core/Registration/Feature.cpp:38-157) on the GPU: out[i * 33 + j] is the reference's
 * feature->data_(j, i).  xyz and normals n x 3 f64.  The neighbour lists are those of visma_icp_estimate_normals for
 *   search_type 0  KDTreeSearchParamKNN(knn)            (a neighbour at a NaN distance is never listed)
 *               2  KDTreeSearchParamHybrid(radius, knn)  (a radius that is not finite or <= 0: all zeros)
 * in flann's order, ascending (d2, index); search_type 1, and a list length knn (the point itself counted) outside
 * [2, 170] -- the lists live in LDS --: VISMA_ICP_ERR_INVALID.  f64 statement by statement: the SPFH pass skips entry 0
 * of the list whatever index it holds and bins every other pair's three angles with the weight 100 / (len - 1) -- the
 * zero 4-vector ComputePairFeatures returns for a zero distance or a zero cross product is binned too (bins 5, 16, 27);
 * a bin argument that is not finite goes to bin 0 --; the FPFH pass runs over the same list, skips entry 0 and entries
 * at distance 0, sums SPFH / d2 in list order, rescales each histogram to 100 where its sum is not 0 and adds the point's
 * own SPFH.  A list of length <= 1 leaves the column zero.  A non-finite normal or coordinate reaches sums only. */
#define VISMA_FPFH_DIM 33
VISMA_ICP_API int visma_icp_compute_fpfh(visma_icp_ctx *ctx, const double *xyz, int64_t n, const double *normals,
                                         int search_type, int knn, double radius, double *out /* n x 33, point-major */);
/* For every row of fb (nb x dim, row-major) the row of fa (na x dim) at the smallest squared distance: nn_of_b[k] in
 * [0, na), d2_of_b[k] (may be NULL) the distance.  d2 is flann's L2<double> to the bit (flann/algorithms/dist.h:150-177):
 * f64, plain differences, ascending j, whole groups of four added as result += ((s0 + s1) + s2) + s3, the last dim % 4
 * one by one.  Exact ties go to the lowest index.  A distance that is NaN or +inf never wins: a row of fb holding a NaN,
 * or na == 0, gets -1 and +inf, and a NaN row of fa is nobody's answer.  dim outside [1, 64]: VISMA_ICP_ERR_INVALID.  Up
 * to 2^31 - 1 rows each.  Brute force on the GPU (feature_match.hip). */
VISMA_ICP_API int visma_icp_match_features(visma_icp_ctx *ctx, const double *fa, int64_t na, const double *fb, int64_t nb,
                                           int dim, int32_t *nn_of_b /* nb */, double *d2_of_b /* nb, may be NULL */);

/* open3d::FastGlobalRegistration (Zhou, Park, Koltun: "Fast Global Registration", ECCV 2016;
 * O3D/Core/Registration/FastGlobalRegistration.cpp:42-375).  Clouds ns x 3 / nt x 3 f64, features n x 33 as
 * visma_icp_compute_fpfh writes them.  In the reference's order:
 *   normalize   both clouds minus their means, then divided by the larger max norm unless use_absolute_scale (:189-240)
 *   swap        so that i is the larger cloud (:47-58)
 *   match       visma_icp_match_features in both directions (:60-83)
 *   cross check (i, j) with nn(j) == i and nn(i) == j, ascending i (:98-123); n_mutual of them
 *   tuple test  100 * n_mutual trials at most (:126-174): a trial draws three indices into the cross-checked list, is
 *               accepted when all three edge ratios lie strictly inside (tuple_scale, 1 / tuple_scale), and pushes its
 *               three pairs; the loop ends once maximum_tuple_count trials have been accepted.  The reference seeds
 *               rand() from the clock, so only its mapping can be matched: trial t takes triples[3 t .. 3 t + 2] modulo
 *               n_mutual when `triples` is given (n_triples trials at most), else words 0..2 of the Philox4x32-10 of
 *               visma_icp_sample_mesh at counter (t, 0) keyed by `seed`, modulo n_mutual.
 *   un-swap     pairs are (source index, target index) again
 *   optimize    OptimizePairwiseRegistration (:242-325): s = (par / (|p - q|^2 + par))^2 per pair, three rows per pair,
 *               SolveLinearSystem(-JTJ, JTr) with its |det| < 1e-6 guard (zeros), TransformVector6dToMatrix4d,
 *               trans = delta * trans, par /= division_factor where itr % 4 == 0 && par > max_corr_dist (decrease_mu);
 *               par starts at scale_global, as the reference passes it.  Fewer than 10 pairs: the identity.
 *   map back    GetTransformationOriginalScale, then the inverse (:329-342, :373-374)
 * out_T is source-to-target, row-major, as RegistrationResult holds it.  A context with a rotation axis is not treated
 * specially: this is the 6-DoF method, there is no 4-DoF variant.  An empty cloud: VISMA_ICP_ERR_INVALID. */
typedef struct {
    double division_factor, max_corr_dist, tuple_scale;
    int use_absolute_scale, decrease_mu, iteration_number, maximum_tuple_count;
} visma_icp_fgr_option;   /* NULL where one is taken: 1.4, 0.025, 0.95, 0, 1, 64, 1000 (FastGlobalRegistration.h:44-50) */
typedef struct {
    int64_t n_mutual;         /* pairs that passed the cross check */
    int64_t n_tuple_corres;   /* pairs the tuple test pushed (3 per accepted trial): what the optimisation runs on */
    int64_t n_trials;         /* trials drawn */
} visma_icp_fgr_info;
/* Normalize, swap, match, cross check, tuple test, un-swap: the pairs into src_idx / tgt_idx (`capacity` entries each;
 * 3 * max(1, min(maximum_tuple_count, 100 * min(ns, nt))) always suffice, fewer: VISMA_ICP_ERR_INVALID when they do not),
 * *n_out of them.  info may be NULL. */
VISMA_ICP_API int visma_icp_fgr_correspondences(visma_icp_ctx *ctx, const double *src_xyz, int64_t ns, const double *src_fpfh,
                                                const double *tgt_xyz, int64_t nt, const double *tgt_fpfh,
                                                const visma_icp_fgr_option *opt, uint64_t seed, const int32_t *triples,
                                                int64_t n_triples, int32_t *src_idx, int32_t *tgt_idx, int64_t capacity,
                                                int64_t *n_out, visma_icp_fgr_info *info);
/* Normalize, optimize over the k given pairs, map back (host only, no context): out_T source-to-target; out_T_opt (may be
 * NULL) what OptimizePairwiseRegistration itself returned, in the normalized frame (it moves the target onto the source).
 * An index outside its cloud: VISMA_ICP_ERR_INVALID. */
VISMA_ICP_API int visma_icp_fgr_optimize(const double *src_xyz, int64_t ns, const double *tgt_xyz, int64_t nt,
                                         const int32_t *src_idx, const int32_t *tgt_idx, int64_t k,
                                         const visma_icp_fgr_option *opt, double out_T[16], double out_T_opt[16]);
/* The whole of it: visma_icp_fgr_correspondences, then visma_icp_fgr_optimize on its pairs. */
VISMA_ICP_API int visma_icp_fast_global_registration(visma_icp_ctx *ctx, const double *src_xyz, int64_t ns,
                                                     const double *src_fpfh, const double *tgt_xyz, int64_t nt,
                                                     const double *tgt_fpfh, const visma_icp_fgr_option *opt, uint64_t seed,
                                                     const int32_t *triples, int64_t n_triples, double out_T[16],
                                                     visma_icp_fgr_info *info);

/* ---- RANSAC global registration: the second method without an initial pose -----------------------------------------
 * open3d::RegistrationRANSACBasedOnFeatureMatching and ...BasedOnCorrespondence (O3D/Core/Registration/Registration.h:61-78,
 * 109-129; Registration.cpp:98-123, 188-353) with the three CorrespondenceCheckers (CorrespondenceChecker.cpp:35-89) and
 * RANSACConvergenceCriteria.  The trial loop runs on the GPU, one lane per trial (ransac.hip); the validation of the
 * trials that pass is EvaluateRegistration at many poses: visma_icp_run_batch with zero iterations.  The reference seeds
 * rand() from the clock and lets OpenMP threads race for total_validation; here the result is a function of the inputs and
 * `seed` (or `draws`).  Feature matching, as a serial loop:
 *   pair table  nn[i] = the target feature nearest to source feature i: ONE visma_icp_match_features(tgt_feat, src_feat)
 *               (num_similar_features == 1, :244): exact, ties to the lowest index, -1 for a NaN row
 *   trials      t = 0, 1, ... in order.  Trial t takes the ransac_n source indices draws[t * ransac_n + j] mod ns when
 *               `draws` is given (n_draw_trials trials at most), else word j mod 4 of the Philox4x32-10 of
 *               visma_icp_sample_mesh at counter (t, j / 4) keyed by `seed`, modulo ns (:273-293).  Duplicates are allowed,
 *               as in the reference.  ransac_n lies in [3, 8]: outside, VISMA_ICP_ERR_INVALID (:237 returns for < 3).
 *   no partner  a trial that draws a row with nn == -1 is rejected before alignment
 *   edge        (before alignment, every i < j, :35-53)  rejected when dis_source < dis_target * s || dis_target <
 *               dis_source * s, both plain norms
 *   solve       TransformationEstimationPointToPoint(false): Eigen::umeyama without scaling on the ransac_n pairs
 *   distance    (:55-68)  rejected when |target - T source| > distance_threshold for a pair
 *   normal      (:70-89)  rejected when target normal . (R source normal) < cos(normal_angle) for a pair; skipped when
 *               either cloud has no normals.  Every comparison is the reference's: one with a NaN is false and rejects
 *               nothing.  A trial that draws a point that is not finite solves R = I, t = NaN, as Eigen::umeyama does.
 *   validate    every trial that passes: EvaluateRegistration(source, target, max_dist, T) (:127-139)
 *   stop        after max_iteration trials, or once max_validation trials have been validated: the validated trials are the
 *               FIRST max_validation passing trials in trial order, whatever the launch geometry (max_validation <= 0:
 *               none -- the reference's racing counter would still validate one)
 *   best        strictly greater fitness, or equal fitness and strictly smaller rmse (:321-325); a full tie stays with the
 *               lowest trial.  No validated trial, or none with a correspondence: the reference's empty result (identity,
 *               fitness 0, rmse 0).
 * Then the context holds the pair (as after visma_icp_set_clouds_f64) and one ordinary pass at the best T: fitness, rmse and
 * count are those of visma_icp_run(init = T, max_iter = 0), and visma_icp_get_correspondences serves correspondence_set_.
 * A source point that is not finite takes part in the trials as it is and is never anybody's correspondence; a passing
 * trial whose T is not finite is validated to zero correspondences without a search.
 * Correspondences (:188-224): min(max_iteration, max_validation) trials (n_draw_trials at most); trial t draws ransac_n
 * entries of the K given pairs (same two draw sources, modulo K), solves, and scores the WHOLE list (:98-123): dis2 <
 * max_dist^2 strictly, fitness = good / K, rmse = sqrt(error2 / good); best as above; no checkers.  The result carries those
 * numbers (num_correspondences = good); the context's clouds are not touched.
 * Only the point-to-point estimator without scaling.  A context's rotation axis is not honoured: 6 degrees of freedom, as
 * visma_icp_fast_global_registration. */
typedef struct {
    int ransac_n;                    /* pairs per trial, [3, 8] */
    int max_iteration;               /* RANSACConvergenceCriteria::max_iteration_ */
    int max_validation;              /* ...::max_validation_ */
    double edge_length_similarity;   /* CorrespondenceCheckerBasedOnEdgeLength; <= 0 (or NaN): checker off */
    double distance_threshold;       /* CorrespondenceCheckerBasedOnDistance; <= 0: off */
    double normal_angle;             /* CorrespondenceCheckerBasedOnNormal, radians; <= 0: off */
    int chunk_trials;                /* trials per launch; 0: the library's choice.  Never changes a result. */
} visma_icp_ransac_option;           /* NULL where one is taken: 4, 1000, 1000, checkers off, 0 (Registration.h:61-78) */
typedef struct {
    int64_t n_trials;                /* trials consumed */
    int64_t n_rejected_before;       /* ... rejected before alignment (no partner, edge lengths) */
    int64_t n_rejected_after;        /* ... rejected after alignment (distance, normals) */
    int64_t n_validated;             /* ... validated */
    int64_t best_trial;              /* -1: none */
    double hypothesis_ms;            /* device time of the trial kernels and their compaction */
    double validation_ms;            /* host time of the validation (feature matching) or the scoring (correspondences) */
} visma_icp_ransac_info;
#define VISMA_RANSAC_PASS 0            /* verdicts of visma_icp_ransac_hypotheses: solved, every checker passed */
#define VISMA_RANSAC_REJECTED_BEFORE 1 /* rejected before alignment; its T is all zeros */
#define VISMA_RANSAC_REJECTED_AFTER 2  /* solved, rejected by the distance or the normal checker */
/* The hypothesis stage alone, trials [first_trial, first_trial + n_trials): verdict_out[n_trials], T_out[n_trials x 16]
 * row-major.  Pair k is (pair_src[k], pair_tgt[k]), or (k, pair_tgt[k]) where pair_src is NULL (a feature pair table:
 * n_pairs == ns); pair_tgt may hold -1.  Normals both or NULL.  `draws` (or NULL) holds ransac_n entries for every trial
 * from 0: (first_trial + n_trials) * ransac_n of them.  opt's max_iteration / max_validation play no part. */
VISMA_ICP_API int visma_icp_ransac_hypotheses(visma_icp_ctx *ctx, const double *src_xyz, int64_t ns, const double *tgt_xyz,
                                              int64_t nt, const double *src_normals, const double *tgt_normals,
                                              const int32_t *pair_src, const int32_t *pair_tgt, int64_t n_pairs,
                                              const visma_icp_ransac_option *opt, uint64_t seed, const int32_t *draws,
                                              int64_t first_trial, int64_t n_trials, int8_t *verdict_out, double *T_out);
/* The same on the host, no context: the very functions the kernels run (visma_amd/csrc/ransac.hpp). */
VISMA_ICP_API int visma_icp_ransac_hypotheses_host(const double *src_xyz, int64_t ns, const double *tgt_xyz, int64_t nt,
                                                   const double *src_normals, const double *tgt_normals,
                                                   const int32_t *pair_src, const int32_t *pair_tgt, int64_t n_pairs,
                                                   const visma_icp_ransac_option *opt, uint64_t seed, const int32_t *draws,
                                                   int64_t first_trial, int64_t n_trials, int8_t *verdict_out, double *T_out);
/* Features ns x dim / nt x dim, row-major, dim in [1, 64]; normals both or NULL; info may be NULL.  An empty cloud,
 * max_dist <= 0 (the reference's early return), ransac_n or dim out of range: VISMA_ICP_ERR_INVALID, before anything
 * reaches a device. */
VISMA_ICP_API int visma_icp_registration_ransac_feature_matching(visma_icp_ctx *ctx, const double *src_xyz, int64_t ns,
                                                                 const double *src_feat, const double *tgt_xyz, int64_t nt,
                                                                 const double *tgt_feat, int dim, const double *src_normals,
                                                                 const double *tgt_normals, double max_dist,
                                                                 const visma_icp_ransac_option *opt, uint64_t seed,
                                                                 const int32_t *draws, int64_t n_draw_trials,
                                                                 visma_icp_result *result, visma_icp_ransac_info *info);
/* K pairs (src_idx[c], tgt_idx[c]); an index outside its cloud, K < ransac_n: VISMA_ICP_ERR_INVALID. */
VISMA_ICP_API int visma_icp_registration_ransac_correspondence(visma_icp_ctx *ctx, const double *src_xyz, int64_t ns,
                                                               const double *tgt_xyz, int64_t nt, const int32_t *src_idx,
                                                               const int32_t *tgt_idx, int64_t K, double max_dist, int ransac_n,
                                                               int max_iteration, int max_validation, uint64_t seed,
                                                               const int32_t *draws, int64_t n_draw_trials,
                                                               visma_icp_result *result, visma_icp_ransac_info *info);

/* ---- multiway registration: the information matrix of an edge, pose-graph optimisation ------------------------------
 * (Choi, Zhou, Koltun: "Robust Reconstruction of Indoor Scenes", CVPR 2015; Kuemmerle et al.: "g2o", ICRA 2011; the
 * reference's GetInformationMatrixFromPointClouds, Registration.cpp:352-413, and GlobalOptimization.cpp.)
 *
 * N fragments are registered pairwise (odometry edges from ICP, loop closures from FGR or RANSAC); every edge is
 * weighted by its information matrix; the line-process optimisation drops the false loop closures and settles all
 * poses at once.
 *
 * The information matrix of an edge with transformation T: over the K pairs (i, j) of a nearest-neighbour pass at T
 * inside max_dist, with q = t_j the TARGET point in the caller's frame,
 *     G = [ 0  z -y 1 0 0 ;  -z 0 x 0 1 0 ;  y -x 0 0 0 1 ]       out = sum G^T G   (6 x 6, row-major)
 * i.e. [[sum hat(q)^T hat(q), sum hat(q)^T], [sum hat(q), K I]].  The kernel (information.hip) forms ten f64 sums
 * K, sum x y z, sum xx yy zz xy xz yz from q = (stored point) + (the context's centre) and the host lays them out.
 *
 * DEVIATION from the reference, on purpose: the reference starts GTG at the identity AND starts every OpenMP thread's
 * private copy at the identity, so it returns sum G^T G + (1 + P) I with P its number of threads (502 with one thread,
 * 504 with three, for K = 500).  This library returns the pure sum: out[35] == K exactly, which is what the
 * line-process weight of visma_icp_global_optimization reads it as, and the result does not depend on a thread count.
 *
 * No floating-point atomics: a run is bit-identical to itself, and an edge's matrix does not depend on what else a call
 * computed.  K = 0: the zero matrix, VISMA_ICP_OK.  A non-finite entry of T: the zero matrix and *k = 0 without a search
 * (as the RANSAC validation treats such a pose).  Non-finite points follow the rule at visma_icp_set_target, no error: a
 * non-finite SOURCE point has no pair (the matrix is that of the other pairs); a non-finite TARGET coordinate makes the
 * centroid visma_icp_set_clouds_f64 centres both clouds on non-finite, so nothing has a pair: K = 0, the zero matrix.
 * Clouds not set: VISMA_ICP_ERR_STATE.
 * Sharded contexts: VISMA_ICP_ERR_INVALID. */
VISMA_ICP_API int visma_icp_information_matrix(visma_icp_ctx *ctx, const double T[16], double max_dist, double out[36],
                                               int64_t *k);
/* The same over the pairs of the last visma_icp_nn_pass (as visma_icp_reduce_gicp reduces them).  Before a pass:
 * VISMA_ICP_ERR_STATE. */
VISMA_ICP_API int visma_icp_reduce_information(visma_icp_ctx *ctx, double out[36]);
/* Every edge of a pose graph in one call: probs[i].src_xyz / tgt_xyz are the edge's clouds, probs[i].init its
 * transformation, probs[i].max_dist its radius; out is n x 36, k (may be NULL) n counts.  A host loop over the edges
 * (upload, search, reduce; one reduction launch per edge): edges that pass the same target (pointer and count) are
 * handled one after the other and the target is uploaded once for them.  ONLY the upload is shared: a new source
 * invalidates the target's search grid on the engine, so every edge builds its own.  Every out[i] is bit-equal to what
 * visma_icp_set_clouds_f64 + visma_icp_information_matrix return for that edge, in whatever order the edges come.
 * Afterwards the context holds the clouds of the last edge handled (visma_icp_get_cloud_sizes: which sizes). */
VISMA_ICP_API int visma_icp_information_matrices(visma_icp_ctx *ctx, const visma_icp_problem *probs, int n, double *out,
                                                 int64_t *k);
/* The number of points of the source and of the target the context holds (0 for a cloud that is not set). */
VISMA_ICP_API int visma_icp_get_cloud_sizes(visma_icp_ctx *ctx, int64_t *ns, int64_t *nt);

/* ---- RGB-D odometry: the pose between two consecutive frames and the information matrix of that edge ------------------
 * (Steinbruecker, Sturm, Cremers: "Real-Time Visual Odometry from Dense RGB-D Images", ICCV workshops 2011 -- the colour
 * term; Park, Zhou, Koltun: "Colored Point Cloud Registration Revisited", ICCV 2017 -- the hybrid term; the reference's
 * ComputeRGBDOdometry, Odometry.cpp, RGBDOdometryJacobian.cpp.)  The odometry edges of the pose graph above.
 *
 * A frame is a gray image and a depth image (metres), both w x h single-channel fp32, row-major.  intrinsic = {fx, fy,
 * cx, cy}.  T maps SOURCE-camera coordinates to TARGET-camera coordinates.  The steps, each as the reference computes it
 * (odometry_image.hip, odometry.hip):
 *   both frames   Gaussian3 on the grays; depth outside [min_depth, max_depth] or <= 0 becomes NaN, then Gaussian3;
 *                 the pairs at `init` on the full-size depths; each gray times 0.5 / (its mean over those pairs);
 *                 n_levels pyramid levels (gray: Gaussian3 + down-sample, depth: down-sample only; level l has
 *                 floor(w / 2^l) x floor(h / 2^l) pixels and the camera matrix scaled by 2^-l); Sobel dx and dy of the
 *                 target's gray and depth; the source's xyz image.  The images are the reference's bit for bit.
 *   pairs at T    per source pixel (u, v) with depth d: uv = d K R K^-1 (u, v, 1) + K t in f64; u_t = (int)(uv.x / uv.z +
 *                 0.5), v_t likewise (truncation toward zero); inside the image, the target's depth d_t there not NaN,
 *                 |uv.z - d_t| <= max_depth_diff.
 *   one step      over the pairs, one row (COLOR) or two (HYBRID, weighted sqrt(1 - 0.968) and sqrt(0.968)) of a
 *                 Gauss-Newton system in f64; x = -(J^T J)^-1 J^T r unless |det J^T J| < 1e-6 or is not finite; the
 *                 update Rz(x2) Ry(x1) Rx(x0), translation x[3..6), applied on the left.
 *   the loop      iterations[0] steps on the COARSEST level, ..., iterations[n_levels - 1] on level 0.  A step without a
 *                 solution ends the run without success.
 *   information   over the pairs of the full-size processed depths at the result, the sum G^T G of the section above
 *                 with q the TARGET's xyz-image point.
 *
 * DEVIATIONS from the reference, on purpose:
 *   - a source pixel whose transformed depth uv.z is <= 0, or whose projection is not finite or beyond 2^30, has no
 *     pair: the reference casts such a value to int, which is undefined;
 *   - an all-zero init is the identity EVERYWHERE (the reference treats it so in the loop only, and places the pairs
 *     of the normalisation with the zero matrix);
 *   - the information matrix is the pure sum, as visma_icp_information_matrix returns it (the reference adds
 *     (1 + OpenMP threads) I here too: [5,5] = K + 2 with one thread, K + 4 with three), and the ZERO matrix when the
 *     run did not succeed (the reference: I);
 *   - no success is not an error: the call returns VISMA_ICP_OK with success = 0, T = I and the zero matrix.
 * No floating-point atomics: a run is bit-identical to itself.
 *
 * VISMA_ICP_ERR_INVALID, before anything reaches a device: a NULL pointer, w or h < 1, n_levels outside 1 .. 8, a level
 * that would have no pixels (min(w, h) >> (n_levels - 1) < 1), a negative iteration count, fx or fy zero or not finite,
 * an unknown method, a level or `which` out of range, a pairs_capacity above 0 and below the sum of the schedule.  A
 * step, correspondence, image or information call before a prepare: VISMA_ICP_ERR_STATE.  The order for such a call: a
 * NULL pointer, an unknown method, a `which` outside 0 .. 8 and a level outside 0 .. VISMA_ICP_ODOMETRY_MAX_LEVELS - 1
 * are INVALID whether or not frames are resident; then STATE without resident frames; then INVALID for a level at or
 * above the resident pyramid's n_levels.  Sharded contexts: VISMA_ICP_ERR_INVALID.  The frames are independent of the
 * clouds the context holds. */
#define VISMA_ICP_ODOMETRY_COLOR 0     /* RGBDOdometryJacobianFromColorTerm */
#define VISMA_ICP_ODOMETRY_HYBRID 1    /* RGBDOdometryJacobianFromHybridTerm (the reference's default) */
#define VISMA_ICP_ODOMETRY_MAX_LEVELS 8
typedef struct {                       /* OdometryOption; NULL where one is taken: 3 levels {20, 10, 5}, 0.03, 0, 4 */
    int n_levels;
    int iterations[VISMA_ICP_ODOMETRY_MAX_LEVELS];   /* coarsest level first, as in the reference */
    double max_depth_diff, min_depth, max_depth;
} visma_icp_odometry_option;
typedef struct {
    int success;
    int iterations;                    /* steps run, the failing one included */
    int64_t information_pairs;         /* K of the information matrix (0 without success) */
    int64_t *pairs;                    /* in: room for pairs_capacity counts, or NULL; out: the pairs of every step */
    int pairs_capacity;                /* 0: no counts wanted; otherwise at least the sum of option->iterations[0 .. n_levels),
                                          so that no count is ever cut off (less: VISMA_ICP_ERR_INVALID) */
} visma_icp_odometry_result;
/* the images of a level: visma_icp_odometry_get_image's `which` */
#define VISMA_ICP_ODOMETRY_SRC_GRAY 0
#define VISMA_ICP_ODOMETRY_SRC_DEPTH 1
#define VISMA_ICP_ODOMETRY_TGT_GRAY 2
#define VISMA_ICP_ODOMETRY_TGT_DEPTH 3
#define VISMA_ICP_ODOMETRY_TGT_GRAY_DX 4
#define VISMA_ICP_ODOMETRY_TGT_GRAY_DY 5
#define VISMA_ICP_ODOMETRY_TGT_DEPTH_DX 6
#define VISMA_ICP_ODOMETRY_TGT_DEPTH_DY 7
#define VISMA_ICP_ODOMETRY_SRC_XYZ 8   /* three floats per pixel */
VISMA_ICP_API int visma_icp_odometry_option_default(visma_icp_odometry_option *opt);
/* The whole of ComputeRGBDOdometry.  option may be NULL; out_info and out_result may be NULL. */
VISMA_ICP_API int visma_icp_rgbd_odometry(visma_icp_ctx *ctx, int w, int h, const float *src_gray, const float *src_depth,
                                          const float *tgt_gray, const float *tgt_depth, const double intrinsic[4],
                                          const double init[16], int method, const visma_icp_odometry_option *option,
                                          double out_T[16], double out_info[36], visma_icp_odometry_result *out_result);
/* The first half on its own: both processed pyramids of option->n_levels levels stay resident in the context until the
 * next prepare or visma_icp_rgbd_odometry (which prepares).  init only places the pairs of the normalisation. */
VISMA_ICP_API int visma_icp_odometry_prepare(visma_icp_ctx *ctx, int w, int h, const float *src_gray, const float *src_depth,
                                             const float *tgt_gray, const float *tgt_depth, const double intrinsic[4],
                                             const double init[16], const visma_icp_odometry_option *option);
/* A level of a resident pyramid: floor(w / 2^level) x floor(h / 2^level) floats (SRC_XYZ: times three). */
VISMA_ICP_API int visma_icp_odometry_get_image(visma_icp_ctx *ctx, int which, int level, float *out);
/* The pairs of a level at T: out_idx[v_s * w_l + u_s] = v_t * w_l + u_t or -1 (may be NULL), *out_k their number.  The
 * reference's correspondence list is the entries >= 0 in this (row-major source) order. */
VISMA_ICP_API int visma_icp_odometry_correspondences(visma_icp_ctx *ctx, int level, const double T[16], int32_t *out_idx,
                                                     int64_t *out_k);
/* One step's sums at T over those pairs, in the layout of visma_icp_reduce: {K, sum r^2, the 21 upper entries of J^T J
 * row by row, the 6 of J^T r, nine zeros}; visma_icp_solve_from_stats with VISMA_ICP_SOLVER_GN_EULER solves it.  out_k
 * and out_sum_r2 (either may be NULL) repeat the first two (the reference prints sum r^2 / rows as "Residual"). */
VISMA_ICP_API int visma_icp_odometry_step(visma_icp_ctx *ctx, int level, const double T[16], int method,
                                          double out_stats[VISMA_ICP_NSTATS], int64_t *out_k, double *out_sum_r2);
/* The information matrix of the resident frames at T (the last step of visma_icp_rgbd_odometry on its own). */
VISMA_ICP_API int visma_icp_odometry_information(visma_icp_ctx *ctx, const double T[16], double out[36], int64_t *out_k);

/* ---- TSDF integration: RGB-D frames with known poses fused into a truncated signed distance volume ---------------------
 * (Curless, Levoy: "A Volumetric Method for Building Complex Models from Range Images", SIGGRAPH 1996; the reference's
 * UniformTSDFVolume, Core/Integration/UniformTSDFVolume.cpp, and CreatePointCloudFromDepthImage / FromRGBDImage,
 * Core/Geometry/PointCloudFactory.cpp.)  The step behind odometry and the pose graph: with a pose per frame, the frames
 * become one de-noised cloud with normals and colours -- what the estimators above take as a target.
 *
 * A volume is an object owned by the context: several may live at once, each is resident on the device from its creation
 * to visma_icp_tsdf_destroy or the context's end.  It is a cube of `resolution`^3 voxels of side length / resolution whose
 * corner is `origin`; voxel (x, y, z) is at x R^2 + y R + z.  A frame is a depth image (metres, w x h fp32, row-major), a
 * colour image by the volume's colour type (RGB8: w x h x 3 bytes; GRAY32: w x h fp32; NONE: ignored, may be NULL),
 * the pinhole intrinsic {fx, fy, cx, cy} with ITS image size, and the extrinsic (world -> camera, 4 x 4 row-major).
 * Each step as the reference computes it (tsdf.hip):
 *   integrate   per voxel in fp32: the camera-space point of column (x, y) at z = 0, advanced along z by repeated
 *               addition of extrinsic(:, 2) * voxel_length; the pixel (int)(x fx / z + cx + 0.5), (int)(y fy / z + cy +
 *               0.5) inside [0.0001, size - 0.0001); its depth d > 0; sdf = (d - z) * sqrtf(xx^2 + yy^2 + 1) > -sdf_trunc;
 *               tsdf = (tsdf w + min(1, sdf / sdf_trunc)) / (w + 1), colour likewise, w += 1.  The volume is the
 *               reference's bit for bit.
 *   extract     ExtractPointCloud: for every voxel in [1, R - 2]^3 with w != 0 and tsdf in [-0.98, 0.98), and each axis
 *               whose +1 neighbour (index < R - 1) is such a voxel of the other sign: the point between them weighted by
 *               |tsdf|, its colour, and the normal from six trilinear samples 0.99 voxels away, in f64.  The order is the
 *               reference's: x, y, z, axis lexicographic.  ExtractVoxelPointCloud: every such voxel's centre, coloured
 *               (tsdf + 1) / 2.  Points and colours are the reference's bit for bit, normals within 1e-11.
 *   from depth  per pixel (u, v) of every stride-th row and column with d > 0: extrinsic^-1 ((u - cx) d / fx, (v - cy) d /
 *               fy, d, 1) in f64, row-major order; with colours rgb / 255 or (gray, gray, gray).
 *
 * DEVIATIONS from the reference, on purpose:
 *   - a frame that does not fit (its size differs from the intrinsic's, no colour image for a coloured volume) is
 *     VISMA_ICP_ERR_INVALID; the reference prints "Unsupported image format" and returns without integrating;
 *   - the extractions of a scalable volume come in a defined order (below); the reference's is a hash map's;
 *   - a scalable volume: a strided pixel touches no unit if its back-projected point has a coordinate that is not finite
 *     (a depth of inf; a huge depth times a pose), or if either of its unit indices floor((p -+ sdf_trunc) / unit length)
 *     lies outside +-2^30 on any axis; the rest of the frame integrates as usual, and a frame of nothing but such pixels
 *     opens no unit and is not an error.  (The reference converts such a floor to int, which is undefined behaviour; on
 *     x86-64 it opens one junk unit at index INT_MIN.)  A uniform volume needs no rule: a depth that is not > 0 (NaN, -inf,
 *     negative, 0) is skipped and a depth of +inf integrates as tsdf 1, as in the reference; the point clouds from a frame
 *     hold a row that is not finite for such a pixel, as the reference's do;
 *   - 16-bit depth is not provided;
 *   - ExtractTriangleMesh (below): the valid cubes, the edges that carry a vertex and every vertex's position and colour are
 *     the reference's bit for bit; THE ORDER of the vertices and triangles and THE CASE RULE -- how a cube's cut edges are
 *     joined into triangles -- are this library's.  The reference's case tables are its program text and are not part of
 *     this library; a rule made independently splits a cube's patch along other diagonals and joins the edges of a cube
 *     with a face of alternating signs in its own way, so the reference's triangle list is not reproduced index for index.
 *     Where no valid cube has such a face the two meshes have the same vertices, the same number of triangles, the same
 *     boundary and the same Euler characteristic, and the same winding.
 * No floating-point atomics: every voxel has one writer, and a run is bit-identical to itself.
 *
 * VISMA_ICP_ERR_INVALID, before anything reaches a device: a NULL pointer, resolution < 1, a volume of more than 2^31 - 1
 * voxels (resolution > 1290: too large for memory), length or sdf_trunc not positive and finite, an origin that is not
 * finite, an unknown colour type, w or h < 1, an image size that differs from the intrinsic's, fx or fy zero or not
 * finite, a missing colour image, stride < 1, a volume of another context, a get before its extract (VISMA_ICP_ERR_STATE) or
 * with another row count than the extract returned.  Sharded contexts: VISMA_ICP_ERR_INVALID.  A failed allocation is
 * VISMA_ICP_ERR_HIP and leaves no volume behind.  Volumes are independent of the clouds and of the odometry frames. */
#define VISMA_ICP_TSDF_COLOR_NONE 0    /* TSDFVolumeColorType::None */
#define VISMA_ICP_TSDF_COLOR_RGB8 1    /* TSDFVolumeColorType::RGB8: colour images of 3 x uint8 */
#define VISMA_ICP_TSDF_COLOR_GRAY32 2  /* TSDFVolumeColorType::Gray32: colour images of 1 x fp32 */
typedef struct visma_icp_tsdf visma_icp_tsdf;
/* UniformTSDFVolume(length, resolution, sdf_trunc, color_type, origin); origin may be NULL (zero) */
VISMA_ICP_API int visma_icp_tsdf_create_uniform(visma_icp_ctx *ctx, double length, int resolution, double sdf_trunc, int color_type,
                                                const double origin[3], visma_icp_tsdf **out);
VISMA_ICP_API int visma_icp_tsdf_destroy(visma_icp_ctx *ctx, visma_icp_tsdf *volume);
/* Reset(): a volume equal to a new one */
VISMA_ICP_API int visma_icp_tsdf_reset(visma_icp_ctx *ctx, visma_icp_tsdf *volume);
/* Integrate(): w x h is the images' size, intrinsic_w x intrinsic_h the intrinsic's; they must agree */
VISMA_ICP_API int visma_icp_tsdf_integrate(visma_icp_ctx *ctx, visma_icp_tsdf *volume, int w, int h, const float *depth,
                                           const void *color, const double intrinsic[4], int intrinsic_w, int intrinsic_h,
                                           const double extrinsic[16]);
/* ExtractPointCloud(): the cloud stays on the device, *out_n is its size; then the rows (n as returned; points, normals
 * and colors are n x 3 doubles, each may be NULL; colors is left untouched for a volume without colour) */
VISMA_ICP_API int visma_icp_tsdf_extract_point_cloud(visma_icp_ctx *ctx, visma_icp_tsdf *volume, int64_t *out_n);
VISMA_ICP_API int visma_icp_tsdf_get_point_cloud(visma_icp_ctx *ctx, visma_icp_tsdf *volume, double *points, double *normals,
                                                 double *colors, int64_t n);
/* ExtractVoxelPointCloud(), by the same pattern */
VISMA_ICP_API int visma_icp_tsdf_extract_voxel_point_cloud(visma_icp_ctx *ctx, visma_icp_tsdf *volume, int64_t *out_n);
VISMA_ICP_API int visma_icp_tsdf_get_voxel_point_cloud(visma_icp_ctx *ctx, visma_icp_tsdf *volume, double *points, double *colors,
                                                       int64_t n);
/* ExtractTriangleMesh(): marching cubes over the resident volume (tsdf.hip).  The mesh stays on the
 * device, *out_nv and *out_nt are its vertex and triangle counts; then the rows (nv, nt as returned; vertices and colors are
 * nv x 3 doubles, triangles nt x 3 int32 vertex indices; each may be NULL; colors is left untouched for a volume without
 * colour).  A get before its extract is VISMA_ICP_ERR_STATE; other counts than the extract returned, a volume of another
 * context or a sharded context are VISMA_ICP_ERR_INVALID before anything reaches a device.  resolution < 2, or a volume no
 * frame went into, gives an empty mesh and launches nothing.
 *   cubes      uniform: every (x, y, z) in [0, R - 2]^3; scalable: every voxel of every unit, a corner beyond the unit read
 *              from the unit next door, a missing unit reading weight 0.  A cube is VALID iff its eight weights are != 0
 *              (there is no tsdf range test here).  A corner is INSIDE iff tsdf < 0 (-0.0 is outside).  Cubes with all
 *              corners inside or all outside emit nothing.
 *   vertices   one per voxel edge (lower voxel, axis) whose two ends differ in sign and that lies on at least one valid cube,
 *              shared by the cubes around it.  In f64, in this order: each component half + voxel_length * index; the axis
 *              component += f0 * voxel_length / (f0 + f1) with f0 = |(double)tsdf(lower)|, f1 = |(double)tsdf(upper)|; a
 *              uniform volume then adds its origin, a scalable one uses global voxel indices.  Colour (f1 c0 + f0 c1) /
 *              (f0 + f1) in f64, c = (double)colour / 255.0 (RGB8) or (double)colour (GRAY32).  Bit for bit the reference's.
 *   THE ORDER  vertices ascend by (x, y, z, axis) of their edge -- ExtractPointCloud's order; a scalable volume's by the
 *              unit that owns the lower voxel, units in lexicographic index order, then (x, y, z, axis) in the unit.
 *              Triangles ascend by cube in the same order, within a cube in the order of the case rule.
 *   THE CASE RULE  bit i of a cube's case is its corner at offset (i & 1, (i >> 1) & 1, (i >> 2) & 1) being inside.  A cube
 *              edge is (lower corner, axis) with id 4 axis + j, j = the lower corner's two other coordinates, the earlier
 *              axis as bit 0 (0 .. 3: the x edges at (y, z) = (0,0) (1,0) (0,1) (1,1); 4 .. 7: the y edges at (x, z); 8 .. 11:
 *              the z edges at (x, y)).  On each face the cut edges are joined into segments that each cut off one group of
 *              inside corners connected along the face's edges; a face with four cut edges has two groups of one corner.
 *              Every cut edge then ends one segment and begins one; the segments close into loops; loops in the order of
 *              their lowest edge id, each started there and fanned from its start.  At most 5 triangles per cube.  The rule
 *              reads a face's four signs only: two cubes always agree on their common face, the mesh has no cracks.
 *   winding    the reference's: a triangle's normal (b - a) x (c - a) points towards increasing tsdf (free space).
 *   degenerate triangles (a vertex with f0 == 0 coincides with its neighbours') are kept, as in the reference.
 * Vertex indices are int32: a mesh of more than 2^31 - 1 vertices or triangles is VISMA_ICP_ERR_INVALID.
 * No atomics, one writer per row: a run is bit-identical to itself. */
VISMA_ICP_API int visma_icp_tsdf_extract_triangle_mesh(visma_icp_ctx *ctx, visma_icp_tsdf *volume, int64_t *out_nv, int64_t *out_nt);
VISMA_ICP_API int visma_icp_tsdf_get_triangle_mesh(visma_icp_ctx *ctx, visma_icp_tsdf *volume, double *vertices, double *colors,
                                                   int32_t *triangles, int64_t nv, int64_t nt);
/* The triangles of one case of THE CASE RULE as edge ids (host only, no context): cube_case in 0 .. 255, edge_ids has room
 * for 15 ints (5 triangles), *n_triangles is their number.  Anything else: VISMA_ICP_ERR_INVALID. */
VISMA_ICP_API int visma_icp_marching_cubes_case(int cube_case, int32_t *edge_ids, int *n_triangles);
/* tsdf_ and weight_ (R^3 floats) and color_ (R^3 x 3 floats, interleaved; untouched without colour) of a uniform volume
 * (unit_index NULL) or of the unit of a scalable volume with that index; each output may be NULL.  A unit_index for a
 * uniform volume, none for a scalable one, or an index no unit has: VISMA_ICP_ERR_INVALID. */
VISMA_ICP_API int visma_icp_tsdf_get_volume(visma_icp_ctx *ctx, visma_icp_tsdf *volume, const int32_t unit_index[3], float *tsdf,
                                            float *weight, float *color);
/* ScalableTSDFVolume(voxel_length, sdf_trunc, color_type, volume_unit_resolution, depth_sampling_stride): cubes of
 * volume_unit_resolution^3 voxels ("units", each a uniform volume of length voxel_length * resolution whose corner is index *
 * that length), opened where a frame's surface comes near.  Integrate back-projects every stride-th pixel (rows and
 * columns) with a depth to extrinsic^-1 ((u - cx) d / fx, (v - cy) d / fy, d) in f64 -- the inverse by cofactors on the
 * host --, opens every unit between floor((p - sdf_trunc) / unit length) and floor((p + sdf_trunc) / unit length) per
 * component (none for a pixel whose point is not finite or whose index lies beyond +-2^30: DEVIATIONS above), and
 * integrates the frame into each of those units as above.  The units live in a pool on the device of
 * initial_units units at first (0: 256) that doubles when it is full; a unit's place in it never changes.  Every unit a
 * frame touches is opened before its integration starts, and a pool that cannot grow is VISMA_ICP_ERR_HIP with the
 * volume as it was.  Reset() forgets the units.
 * THE ORDER of the extractions of a scalable volume is this library's definition -- the reference's is the iteration
 * order of an unordered_map, which means nothing: units in lexicographic order of their index (x, then y, then z), and
 * the reference's order within a unit (x, y, z, axis).  visma_icp_tsdf_get_units returns the indices in that order.  An
 * extracted point's +1 neighbour and the eight corners of a normal's samples are read across unit borders; a unit that
 * does not exist reads weight 0 and tsdf 0, as in the reference.
 * VISMA_ICP_ERR_INVALID: volume_unit_resolution < 1 or > 256, voxel_length or sdf_trunc not positive and finite, an
 * unknown colour type, depth_sampling_stride < 1, initial_units outside 0 .. 2^20. */
VISMA_ICP_API int visma_icp_tsdf_create_scalable(visma_icp_ctx *ctx, double voxel_length, double sdf_trunc, int color_type,
                                                 int volume_unit_resolution, int depth_sampling_stride, int initial_units,
                                                 visma_icp_tsdf **out);
/* The unit indices of a scalable volume, 3 ints per unit, in the order above: *out_n units; indices may be NULL for the
 * count alone, otherwise it has room for `capacity` units (less than *out_n: VISMA_ICP_ERR_INVALID, *out_n set). */
VISMA_ICP_API int visma_icp_tsdf_get_units(visma_icp_ctx *ctx, visma_icp_tsdf *volume, int32_t *indices, int64_t capacity,
                                           int64_t *out_n);
/* CreatePointCloudFromDepthImage (float depth) and CreatePointCloudFromRGBDImage (color_type RGB8 or GRAY32, as above).
 * extrinsic may be NULL (the identity).  *out_n is the number of points.  points (n x 3 doubles) may be NULL for the count
 * alone; otherwise points (and colors, which may be NULL) have room for `capacity` rows, at least ceil(w / stride) *
 * ceil(h / stride) (stride 1 for the RGB-D form): less is VISMA_ICP_ERR_INVALID before anything reaches a device. */
VISMA_ICP_API int visma_icp_point_cloud_from_depth(visma_icp_ctx *ctx, int w, int h, const float *depth, const double intrinsic[4],
                                                   const double extrinsic[16], int stride, double *points, int64_t capacity,
                                                   int64_t *out_n);
VISMA_ICP_API int visma_icp_point_cloud_from_rgbd(visma_icp_ctx *ctx, int w, int h, const float *depth, const void *color,
                                                  int color_type, const double intrinsic[4], const double extrinsic[16],
                                                  double *points, double *colors, int64_t capacity, int64_t *out_n);

/* ---- Color map optimization: camera poses refined against the vertices' intensities, then the vertices re-coloured ------
 *
 * Open3D's ColorMapOptimization (Zhou and Koltun, SIGGRAPH 2014; Core/ColorMap/ColorMapOptimization.cpp), the RIGID variant
 * (non_rigid_camera_coordinate == 0, Open3D's default).  The NON-RIGID variant has entry points of its own, further down
 * (visma_icp_color_map_create_non_rigid, visma_icp_color_map_optimization_non_rigid): the calls here answer an option with
 * that flag set with VISMA_ICP_ERR_INVALID and touch nothing.
 *
 * A color map is an object of its context (several may live at once; the context's end frees them all), resident on the
 * GPU (colormap.hip).  The staged calls, in order: create, set every image and the vertices, prepare, then
 * any of the getters, sums, step, run, and the colours.  A call before its stage is VISMA_ICP_ERR_INVALID; setting an image or
 * the vertices again asks for a new prepare.  Every argument check comes before a device is touched.
 *   images      gray = Gaussian3 of (0.2990f R + 0.5870f G + 0.1140f B) / 255.0f, dx and dy its Sobel3Dx and Sobel3Dy; the
 *               mask is 255 where the Sobel gradient of the depth exceeds depth_threshold_for_discontinuity_check, dilated by
 *               a square of half-size half_dilation_kernel_size_for_discontinuity_map.  Bit for bit the reference's.
 *   visibility  computed ONCE, by prepare, from the poses of that moment: z >= 0, the rounded pixel inside the image, its
 *               depth <= maximum_allowable_depth, its mask not 255, |z - depth| < depth_threshold_for_visiblity_check.
 *   iteration   per camera over its visible vertices inside the 10-pixel margin: the 6 x 6 system of the intensity residual
 *               against the vertex's proxy (the mean over its cameras), x = -JJ^-1 Jb, pose <- [Rz Ry Rx | t] pose; then the
 *               proxies anew.  All cameras in one launch, f64, no atomics: a run is bit-identical to itself.
 * Deviations from the reference:
 *   - the ORDER of visibility is defined: a camera's vertex list ascends in vertex id, a vertex's camera list ascends in
 *     camera id (the reference's per-vertex order is a race between its threads);
 *   - a camera with fewer than 6 accepted vertices, or with a singular JJ, KEEPS its pose for that iteration and reports
 *     its count (the reference inverts a zero matrix and turns the pose into NaN);
 *   - a vertex whose projection is not finite is not visible (undefined behaviour in the reference). */
typedef struct {                       /* ColorMapOptmizationOption, field for field */
    int32_t non_rigid_camera_coordinate;                       /* must be 0 here; the non-rigid entry points do not read it */
    int32_t number_of_vertical_anchors;                        /* 16; non-rigid only */
    double non_rigid_anchor_point_weight;                      /* 0.316; non-rigid only */
    double maximum_iteration;                                  /* 300 (a double in the reference) */
    double maximum_allowable_depth;                            /* 2.5 */
    double depth_threshold_for_visiblity_check;                /* 0.03 */
    double depth_threshold_for_discontinuity_check;            /* 0.1 */
    int32_t half_dilation_kernel_size_for_discontinuity_map;   /* 3; 0 .. 64 */
    int32_t reserved;
} visma_icp_color_map_option;
VISMA_ICP_API void visma_icp_color_map_option_default(visma_icp_color_map_option *option);
typedef struct visma_icp_color_map visma_icp_color_map;
#define VISMA_ICP_COLOR_MAP_GRAY 0
#define VISMA_ICP_COLOR_MAP_DX 1
#define VISMA_ICP_COLOR_MAP_DY 2
#define VISMA_ICP_COLOR_MAP_MASK 3     /* uint8; the others fp32 */
#define VISMA_ICP_COLOR_MAP_SUMS 29    /* per camera: the 21 upper entries of JJ row by row, Jb[6], rr, count */
/* n_images frames of w x h (both above 20: the margin leaves an interior), intrinsic = {fx, fy, cx, cy}; option NULL: the
 * defaults */
VISMA_ICP_API int visma_icp_color_map_create(visma_icp_ctx *ctx, int w, int h, int n_images, const double intrinsic[4],
                                             const visma_icp_color_map_option *option, visma_icp_color_map **out);
VISMA_ICP_API int visma_icp_color_map_destroy(visma_icp_ctx *ctx, visma_icp_color_map *map);
/* frame i: depth w x h fp32 in metres, color w x h x color_channels uint8 (color_channels must be 3: RGB8), extrinsic 4 x 4
 * row-major, world -> camera */
VISMA_ICP_API int visma_icp_color_map_set_image(visma_icp_ctx *ctx, visma_icp_color_map *map, int i, const float *depth,
                                                const uint8_t *color, int color_channels, const double extrinsic[16]);
VISMA_ICP_API int visma_icp_color_map_set_vertices(visma_icp_ctx *ctx, visma_icp_color_map *map, const double *vertices, int64_t n);
/* images, masks and visibility; visible_counts[n_images] (may be NULL) */
VISMA_ICP_API int visma_icp_color_map_prepare(visma_icp_ctx *ctx, visma_icp_color_map *map, int64_t *visible_counts);
/* which: VISMA_ICP_COLOR_MAP_*; out: w x h fp32, or uint8 for the mask */
VISMA_ICP_API int visma_icp_color_map_get_image(visma_icp_ctx *ctx, visma_icp_color_map *map, int i, int which, void *out);
/* camera i's visible vertices, ascending: *out_n of them; indices may be NULL for the count alone, else room for capacity */
VISMA_ICP_API int visma_icp_color_map_get_visible(visma_icp_ctx *ctx, visma_icp_color_map *map, int i, int32_t *indices,
                                                  int64_t capacity, int64_t *out_n);
/* the proxy intensities of the current poses: n doubles, n the vertex count */
VISMA_ICP_API int visma_icp_color_map_get_proxy(visma_icp_ctx *ctx, visma_icp_color_map *map, double *proxy, int64_t n);
/* sums[n_images x 29] at the current poses; no pose moves */
VISMA_ICP_API int visma_icp_color_map_sums(visma_icp_ctx *ctx, visma_icp_color_map *map, double *sums);
/* one iteration: rr[n_images] and count[n_images] of the poses BEFORE the step */
VISMA_ICP_API int visma_icp_color_map_step(visma_icp_ctx *ctx, visma_icp_color_map *map, double *rr, int64_t *count);
/* k iterations (k < 0: the option's maximum_iteration); residual[k] (may be NULL): the sum of rr over the cameras, per iteration */
VISMA_ICP_API int visma_icp_color_map_run(visma_icp_ctx *ctx, visma_icp_color_map *map, int k, double *residual);
/* n_images x 16 doubles, row-major */
VISMA_ICP_API int visma_icp_color_map_get_extrinsics(visma_icp_ctx *ctx, visma_icp_color_map *map, double *extrinsics);
VISMA_ICP_API int visma_icp_color_map_set_extrinsics(visma_icp_ctx *ctx, visma_icp_color_map *map, const double *extrinsics);
/* the colour average of the current poses: n x 3 doubles, n the vertex count */
VISMA_ICP_API int visma_icp_color_map_get_colors(visma_icp_ctx *ctx, visma_icp_color_map *map, double *colors, int64_t n);
/* Everything in one call: depth n_images x h x w fp32, color n_images x h x w x 3 uint8, extrinsics n_images x 16 in and out,
 * vertices n x 3, colors n x 3 out.  option->maximum_iteration iterations. */
VISMA_ICP_API int visma_icp_color_map_optimization(visma_icp_ctx *ctx, int w, int h, int n_images, const double intrinsic[4],
                                                   const float *depth, const uint8_t *color, double *extrinsics,
                                                   const double *vertices, int64_t n, const visma_icp_color_map_option *option,
                                                   double *colors);

/* ---- The NON-RIGID color map optimization: besides its pose, every image carries a bilinear warping field --------------
 *
 * Open3D's OptimizeImageCoorNonrigid (the method of Zhou and Koltun's paper): a rigid pose cannot absorb lens distortion,
 * rolling shutter or depth-dependent misregistration; a field of anchor_w x anchor_h anchors per image can.  GPU:
 * colormap_warp.hip, DESIGN.md 4.4c13.
 *   field       anchor_h = number_of_vertical_anchors, anchor_step = double(h) / (anchor_h - 1),
 *               anchor_w = int(ceil(double(w) / anchor_step) + 1); flow[(i + j anchor_w) 2 + {0, 1}] = {i step, j step} is the
 *               initial value and what the regulariser pulls toward.
 *   proxies and colours   the fp32 projection and its margin test as above; then the cell i = (int)(u / step), j likewise,
 *               p = (u - i step) / step, q likewise; the shift ((1-p)(1-q)) g00 + ((1-p) q) g01 + (p (1-q)) g10 + (p q) g11,
 *               the margin test on it, the pixel int(round(shift)).
 *   iteration   per camera over its visible list: u, v in f64, the cell and p, q, the shift (uu, vv), the margin test on
 *               it, gray / dx / dy there, the chain rule through the field, C[14] (6 of the pose, 2 per corner anchor),
 *               r = proxy - gray; the sums are kept PER CELL (121 each: the 105 upper entries of C C^T row by row, the 14
 *               of -r C, rr, count).  weight = non_rigid_anchor_point_weight * count / n_vertex; per flow entry
 *               JJ(d, d) += weight^2, Jb(d) += weight * weight (flow - flow_init), rr_reg += (weight (flow - flow_init))^2;
 *               x = -JJ^-1 Jb (on the host: a banded Cholesky with a border of six); the pose update as above, flow += x[6:].
 * Deviations from the reference:
 *   1. a visit whose cell (ii, jj) is outside [0, anchor_w - 2] x [0, anchor_h - 2], or whose u / step or v / step is not
 *      finite or reaches 2^30 in magnitude (compared as doubles, before the conversion to int), is SKIPPED: the reference
 *      indexes JJ out of bounds there.  (int) truncates toward zero: u in (-step, 0) is cell 0 with p < 0, in range, kept.
 *   2. a camera KEEPS its pose and its flow for that iteration, and reports its count, with fewer than 6 accepted visits,
 *      with a pivot of the factorisation that is not positive and finite, or with a step that is not finite (the reference
 *      continues only at count == 0);
 *   3. the ORDER is defined: within a camera the visits are summed cell by cell, within a cell in ascending vertex id.
 * The staged calls above serve both kinds of map (run's residual is the data residual); visma_icp_color_map_sums on a
 * non-rigid map is VISMA_ICP_ERR_INVALID, the calls below on a rigid one likewise. */
#define VISMA_ICP_COLOR_MAP_CELL_SUMS 121
/* the checks of visma_icp_color_map_create (the option's flag field is not read), and: 2 <= number_of_vertical_anchors <= 64,
 * anchor_w * anchor_h <= 8192, the weight finite and >= 0 */
VISMA_ICP_API int visma_icp_color_map_create_non_rigid(visma_icp_ctx *ctx, int w, int h, int n_images, const double intrinsic[4],
                                                       const visma_icp_color_map_option *option, visma_icp_color_map **out);
/* each output may be NULL */
VISMA_ICP_API int visma_icp_color_map_get_anchor_shape(visma_icp_ctx *ctx, visma_icp_color_map *map, int *anchor_w, int *anchor_h,
                                                       double *anchor_step);
/* n_images x anchor_w anchor_h 2 doubles, the reference's layout; set_flow invalidates the proxies, as set_extrinsics does */
VISMA_ICP_API int visma_icp_color_map_get_flow(visma_icp_ctx *ctx, visma_icp_color_map *map, double *flow);
VISMA_ICP_API int visma_icp_color_map_set_flow(visma_icp_ctx *ctx, visma_icp_color_map *map, const double *flow);
/* sums[n_images x (anchor_w - 1)(anchor_h - 1) x 121] at the current poses and fields, cell ii + jj (anchor_w - 1); nothing moves */
VISMA_ICP_API int visma_icp_color_map_cell_sums(visma_icp_ctx *ctx, visma_icp_color_map *map, double *sums);
/* one iteration: rr, rr_reg and count [n_images] of the state BEFORE the step */
VISMA_ICP_API int visma_icp_color_map_step_non_rigid(visma_icp_ctx *ctx, visma_icp_color_map *map, double *rr, double *rr_reg,
                                                     int64_t *count);
/* visma_icp_color_map_optimization with a field per image; flow (may be NULL): n_images x anchor_w anchor_h 2 out */
VISMA_ICP_API int visma_icp_color_map_optimization_non_rigid(visma_icp_ctx *ctx, int w, int h, int n_images, const double intrinsic[4],
                                                             const float *depth, const uint8_t *color, double *extrinsics,
                                                             const double *vertices, int64_t n,
                                                             const visma_icp_color_map_option *option, double *colors, double *flow);
/* Host only, no ctx, no GPU: one camera's system assembled from its (anchor_w - 1)(anchor_h - 1) cell rows, the regulariser
 * (weight_option: non_rigid_anchor_point_weight; n_vertex: the mesh's vertex count), and the solve.  flow, flow_init:
 * anchor_w anchor_h 2; x: 6 + anchor_w anchor_h 2 out (zero where the camera keeps: *kept = 1, deviation 2); rr_reg, kept may
 * be NULL. */
VISMA_ICP_API int visma_icp_color_map_solve_non_rigid(int anchor_w, int anchor_h, const double *cell_sums, int64_t n_vertex,
                                                      double weight_option, const double *flow, const double *flow_init, double *x,
                                                      double *rr_reg, int *kept);

/* The pose graph on plain arrays (pure functions; no ctx, no GPU).  Node i has a 4 x 4 pose (row-major, node to world);
 * an edge says: transformation maps the SOURCE node's cloud onto the TARGET node's (PoseGraph.h:52-86).  Odometry edges
 * are certain (uncertain = 0), loop closures uncertain; confidence is the line-process value in [0, 1]. */
typedef struct {
    int32_t source, target;
    double transformation[16];
    double information[36];
    int32_t uncertain;
    double confidence;
} visma_icp_pose_graph_edge;
typedef struct {                       /* GlobalOptimizationOption; NULL where one is taken: 0.075, 0.25, 1.0, -1 */
    double max_correspondence_distance;    /* < 0: 0.075 */
    double edge_prune_threshold;           /* outside [0, 1]: 0.25 */
    double preference_loop_closure;        /* < 0: 1.0 */
    int32_t reference_node;                /* the node whose pose is the same after the optimisation; outside the graph: none */
} visma_icp_global_optimization_option;
typedef struct {                       /* GlobalOptimizationConvergenceCriteria; NULL: 100, 1e-6 x 4, 20, 2/3, 1/3 */
    int32_t max_iteration;
    double min_relative_increment;
    double min_relative_residual_increment;
    double min_right_term;
    double min_residual;
    int32_t max_iteration_lm;
    double upper_scale_factor;             /* outside [0, 1]: 2/3 */
    double lower_scale_factor;             /* outside [0, 1]: 1/3 */
} visma_icp_global_optimization_criteria;
#define VISMA_ICP_GLOBAL_GAUSS_NEWTON 0
#define VISMA_ICP_GLOBAL_LEVENBERG_MARQUARDT 1
/* The clamping of the reference's constructors, in place. */
VISMA_ICP_API int visma_icp_global_optimization_option_clamp(visma_icp_global_optimization_option *opt);
VISMA_ICP_API int visma_icp_global_optimization_criteria_clamp(visma_icp_global_optimization_criteria *crit);
/* 1: every consecutive node pair (i, i + 1) has an edge and every edge names nodes of the graph; 0 otherwise
 * (ValidatePoseGraph); -VISMA_ICP_ERR_INVALID for NULL or negative arguments. */
VISMA_ICP_API int visma_icp_pose_graph_validate(int n_nodes, const visma_icp_pose_graph_edge *edges, int n_edges);
/* zeta (6 per edge): the linearised misalignment X^-1 Tt^-1 Ts of every edge (ComputeZeta).  An edge naming a node
 * outside the graph: VISMA_ICP_ERR_INVALID. */
VISMA_ICP_API int visma_icp_pose_graph_zeta(const double *poses, int n_nodes, const visma_icp_pose_graph_edge *edges,
                                            int n_edges, double *zeta_out);
/* H (6n x 6n, row-major) and b (6n) of the Gauss-Newton step at the given poses with the edges' confidences
 * (ComputeLinearSystem). */
VISMA_ICP_API int visma_icp_pose_graph_linear_system(const double *poses, int n_nodes, const visma_icp_pose_graph_edge *edges,
                                                     int n_edges, double *H_out, double *b_out);
/* ONE optimisation (GlobalOptimizationMethod::OptimizePoseGraph): no validation, no pruning, no compensation; poses and
 * the edges' confidences are updated.  An edge naming a node outside the graph: VISMA_ICP_ERR_INVALID.
 * Gauss-Newton solves the SINGULAR system of a graph without a fixed node, as the reference does: the rigid motion common
 * to all poses it returns is rounding noise there and here (0.13 between two builds on a 6-node graph); the poses
 * relative to one another are not.  Levenberg-Marquardt's damping fixes the common motion. */
VISMA_ICP_API int visma_icp_pose_graph_optimize(double *poses, int n_nodes, visma_icp_pose_graph_edge *edges, int n_edges,
                                                int method, const visma_icp_global_optimization_criteria *criteria,
                                                const visma_icp_global_optimization_option *option);
/* The whole of GlobalOptimization(): validation (an invalid graph comes back untouched, with VISMA_ICP_OK as the reference
 * returns nothing: ask visma_icp_pose_graph_validate),
 * the first optimisation, pruning (an uncertain edge with confidence <= edge_prune_threshold is dropped; the edges that
 * stay are moved to the front of `edges` in their order and *n_edges is their number), the second optimisation, the
 * compensation of reference_node.  Both methods restate the reference's stopping tests in the reference's order: the
 * right-hand side's largest coefficient (not its absolute value) below min_right_term, the relative increment, the
 * relative residual increment, the residual, the iteration limits; Levenberg-Marquardt with tau = 1e-5, rho with its
 * + 1e-3 and the scale factor clamped to [lower, upper].  Linear solves: a dense L D L^T with diagonal pivoting
 * throughout (the reference's sparse Cholesky inside Levenberg-Marquardt is an implementation detail).  information[35]
 * is read as the edge's number of correspondences (see the deviation above).  criteria / option may be NULL and are
 * clamped as the reference's constructors clamp.  poses: n_nodes x 16, in and out. */
VISMA_ICP_API int visma_icp_global_optimization(double *poses, int n_nodes, visma_icp_pose_graph_edge *edges, int *n_edges,
                                                int method, const visma_icp_global_optimization_criteria *criteria,
                                                const visma_icp_global_optimization_option *option);

/* Point -> triangle-mesh squared distance, face and closest point for np query
 * points: what igl::AABB::squared_distance returns inside feh::MeasureSurfaceError
 * (include/geometry.h:123-136).  face / closest may be NULL; exact ties go to the
 * lowest face index. */
VISMA_ICP_API int visma_icp_point_mesh_distance(visma_icp_ctx *ctx, const double *P, int64_t np,
                                                const double *V, int64_t nv, const int32_t *F,
                                                int64_t nf, double *d2, int32_t *face,
                                                double *closest);
/* open3d::ComputePointCloudToPointCloudDistance (O3D/Core/Geometry/PointCloud.cpp:122-142; PointCloud.h:161-167)
 * on the GPU: dist_out[i] = sqrt(min_j d2(src_i, tgt_j)), with no radius, for the ns source points (n x 3 f64,
 * caller's order).  d2 is flann's L2<double>, ((dx*dx) + dy*dy) + dz*dz in f64, and the result equals the
 * reference's bit for bit.  An empty target gives 0.0 for every query (the reference's SearchKNN fails on an
 * empty tree and its preset dists[0] = 0 comes back, KDTreeFlann.cpp:124-127); a row with a NaN coordinate leaves
 * the other rows unaffected, its own value unspecified.  Up to 2^31 - 1 points per cloud.  The context's clouds
 * and search state are not touched. */
VISMA_ICP_API int visma_icp_point_cloud_distance(visma_icp_ctx *ctx, const double *src_xyz, int64_t ns,
                                                 const double *tgt_xyz, int64_t nt, double *dist_out);
/* open3d::ComputePointCloudNearestNeighborDistance (PointCloud.cpp:200-219; PointCloud.h:180-183) on the GPU:
 * dist_out[i] = sqrt(min_{j != i} d2(xyz_i, xyz_j)) -- the reference's SearchKNN(p, 2) -> dists[1], so a duplicate
 * point gives 0 and a one-point cloud gives 0.0 (its `<= 1` branch).  Same arithmetic, limits and guarantees as
 * visma_icp_point_cloud_distance. */
VISMA_ICP_API int visma_icp_nearest_neighbor_distance(visma_icp_ctx *ctx, const double *xyz, int64_t n,
                                                      double *dist_out);
/* ---- KDTreeFlann: neighbour queries for ANY points against a cloud resident on the device --------------------------------
 * (the reference's Core/Geometry/KDTreeFlann.cpp: SearchKNN :117-140, SearchRadius :142-164, SearchHybrid :166-189.)
 * The exact search under normal estimation, the colour gradient and FPFH, handed to the caller: what an outlier filter, a
 * correspondence rule or a descriptor of the caller's own is built on.  A tree is an object owned by the context: the cloud
 * (n x 3 f64, n >= 1) is uploaded once and stays resident until visma_icp_kdtree_destroy or the context's end.
 *
 * Results, for every search: rows in the caller's query order; within a row ascending (d2, index) -- flann's result order
 * with the index deciding exact ties; d2 = ((dx dx) + dy dy) + dz dz in f64 (flann/algorithms/dist.h:159-176), equal to the
 * reference's to the bit.  Radius and Hybrid accept a neighbour iff d2 < (double)(float)(radius * radius), strictly
 * (KDTreeFlann.cpp:157-158, 184-185).  A neighbour at a NaN distance is never listed: a query with a NaN coordinate gets
 * empty lists and a point of the cloud with one is in no list; a query with an infinite coordinate is at d2 = +inf from every
 * finite point: KNN lists the lowest indices with d2 = +inf, Radius and Hybrid list nothing.  A second identical call
 * returns identical bytes.  Queries may lie anywhere: outside the cloud's bounding box, or far away from it.
 *   search_knn     idx, d2: nq x knn, cnt: nq.  A list holds min(knn, n) entries; behind cnt[i] entries row i is padded
 *                  with -1 and +inf.
 *   search_hybrid  the same layout with max_nn for knn: the max_nn nearest of those within the radius.
 *   search_radius  every neighbour within the radius, however many: the call counts, scans and writes the lists, which
 *                  STAY ON THE DEVICE; offsets (nq + 1) and *total come back.  visma_icp_kdtree_get_radius_result then
 *                  copies the *total entries out, in CSR order: query i owns [offsets[i], offsets[i + 1]).  It may be called
 *                  until the next search_radius on the tree; before any: VISMA_ICP_ERR_STATE.  A result of more than
 *                  VISMA_ICP_KDTREE_MAX_RADIUS_ENTRIES entries (12 bytes each on the device) is refused with
 *                  VISMA_ICP_ERR_INVALID, *total set and nothing kept: search fewer queries a call.
 * The grid: a tree searches a grid of cells built for the radius of the call (Radius and Hybrid share it) or sized for knn
 * (min(knn, n)).  It is KEPT for the next call that asks for the same parameter; a different radius or knn REBUILDS it (a
 * counting sort of the cloud, and for knn up to three more to size the cells).  A caller who alternates radii pays for a
 * rebuild each time: group the calls, or keep one tree per parameter.  The answers do not depend on the grid.
 * Memory: the cloud and its grid (about 100 bytes a point), the queries of a call, and the rows of at most 2^22 list entries
 * at a time (KNN and Hybrid go through the device in slabs of queries) plus, for lists longer than 170, as much again.
 *
 * VISMA_ICP_ERR_INVALID, before anything reaches a device: a NULL pointer, n < 1, nq < 0, knn < 1, max_nn < 1, a radius
 * that is not finite and > 0.  nq == 0 is not an error: nothing is written (offsets[0] = 0, *total = 0).  An error leaves
 * the tree usable.
 *
 * DEVIATIONS from the reference, on purpose:
 *   - three dimensions only: SetFeature and SetMatrixData with rows() != 3 are not provided (the 33-dimensional 1-NN of
 *     the feature matching is visma_icp_match_features);
 *   - the C ABI is stricter than the class: knn < 1, max_nn < 1 and a radius <= 0 are VISMA_ICP_ERR_INVALID, and a tree of
 *     no points cannot be made.  The class returns -1 from every search of an empty tree and for knn or max_nn < 0; it
 *     SQUARES a negative radius (the answer of its absolute value) and finds nothing below a radius of 0; with knn = 0 flann's
 *     KNNSimpleResultSet(0) writes dist_index_[-1] (flann/util/result_set.h:124), and with max_nn = 0 flann only counts and
 *     the class returns that count with vectors it has not filled.  The C++ shim (Core/Geometry/KDTreeFlann.h) returns what
 *     the class returns wherever that is defined -- -1 for an empty tree and for knn or max_nn < 0, the answer of |radius|,
 *     nothing for a radius of 0 -- and 0 with empty vectors for knn = 0 or max_nn = 0; a radius that is not finite finds
 *     nothing there (tests/golden/kdtree.npz records the reference's answers to the degenerate calls that are safe to make);
 *   - where distances tie exactly, the lower index comes first; flann's order among exact ties is its tree's. */
#define VISMA_ICP_KDTREE_MAX_RADIUS_ENTRIES 268435456ll   /* 2^28 */
typedef struct visma_icp_kdtree visma_icp_kdtree;
VISMA_ICP_API int visma_icp_kdtree_create(visma_icp_ctx *ctx, const double *xyz, int64_t n, visma_icp_kdtree **out);
VISMA_ICP_API int visma_icp_kdtree_destroy(visma_icp_kdtree *tree);
/* the number of points; 0 for NULL */
VISMA_ICP_API int64_t visma_icp_kdtree_size(const visma_icp_kdtree *tree);
VISMA_ICP_API int visma_icp_kdtree_search_knn(visma_icp_kdtree *tree, const double *queries, int64_t nq, int knn, int32_t *idx,
                                              double *d2, int32_t *cnt);
VISMA_ICP_API int visma_icp_kdtree_search_hybrid(visma_icp_kdtree *tree, const double *queries, int64_t nq, double radius,
                                                 int max_nn, int32_t *idx, double *d2, int32_t *cnt);
VISMA_ICP_API int visma_icp_kdtree_search_radius(visma_icp_kdtree *tree, const double *queries, int64_t nq, double radius,
                                                 int64_t *offsets, int64_t *total);
VISMA_ICP_API int visma_icp_kdtree_get_radius_result(visma_icp_kdtree *tree, int32_t *idx, double *d2);
/* Errors of a tree's calls are its context's: visma_icp_last_error(ctx). */

/* ---- TriangleMesh: normals, Purge, select, crop and Transform over a mesh resident on the device -------------------------
 * (the reference's Core/Geometry/TriangleMesh.cpp and .h, DownSample.cpp :107-177 and :256-274, Eigen's Dot.h for
 * normalize().)  What follows ExtractTriangleMesh in the reference pipeline, without a host round trip.  A mesh is an object
 * owned by its context; it lives until visma_icp_trimesh_destroy or the context's end and holds on the device: vertices
 * (nv x 3 f64), optional vertex normals and vertex colours (nv x 3 f64), triangles (nt x 3 int32), optional triangle
 * normals (nt x 3 f64).  "Has X" is the reference's HasX(): an attribute of no rows is not had.  Empty meshes are legal
 * everywhere and launch nothing.
 *
 * EVERY RESULT IS THE REFERENCE'S BIT FOR BIT, and a second identical call returns identical bytes: f64, every product,
 * difference and sum rounded on its own (no fused multiply-add: the reference is built for plain x86-64), correctly rounded
 * square root and division, every sum in the reference's serial order; no floating-point atomics, one writer per row.
 *   triangle normals  (v1 - v0) x (v2 - v0) by Eigen's component formula (y z' - z y', z x' - x z', x y' - y x').
 *   normalize_normals per vector, vertex and triangle normals alike: n2 = (x x + y y) + z z; if n2 > 0 every component is
 *                     divided by sqrt(n2), else the vector is left as it is (a zero vector stays zero; one whose n2 overflows
 *                     is divided by inf); then, if x -- and only x -- is NaN, the vector becomes (0, 0, 1): a vector whose
 *                     y alone is NaN stays.  compute_*_normals(normalized != 0) end in this call, which, as in the
 *                     reference, normalises BOTH kinds of normals the mesh has.
 *   vertex normals    every triangle's normal is added to its three corners in triangle order, then corner order: the sum of
 *                     a vertex has that fixed order (an incidence list by one stable radix sort; one lane per vertex walks
 *                     its list -- a vertex shared by very many triangles is summed by ONE lane: the price of the
 *                     reference's order).  A degenerate triangle (a, a, b) adds twice to a.  Two behaviours of the reference
 *                     are kept: triangle normals the mesh already HAS are used as they are (normalised or not), else
 *                     unnormalised ones are computed and kept; vertex normals the mesh already HAS are ADDED ONTO (the
 *                     reference's resize(n, Zero) does not reset), else the sums start from zero.
 *   remove_duplicated_vertices   two vertices are the same iff all three coordinates compare == as doubles (-0.0 == 0.0;
 *                     a vertex with a NaN coordinate equals nothing, itself included).  The lowest index of a group stays,
 *                     with its normal and colour; survivors keep their order; triangles are remapped.
 *   remove_duplicated_triangles  the key is the reference's rotation to the smallest index with its <= ties as written:
 *                     (0,1,2), (1,2,0), (2,0,1) share a key, (0,2,1) does not, and (0,1,0) and (0,0,1) do not although one
 *                     is a rotation of the other.  The first occurrence stays, with its corner order and its normal.
 *   remove_non_manifold_triangles  a triangle with two equal indices goes.
 *   remove_non_manifold_vertices   a vertex no triangle uses goes; triangles are remapped.
 *   purge             the four in this order; removed[4] in this order.
 *   select            a NEW mesh: the triangles whose three corners are among indices[] (duplicates change nothing), the
 *                     vertices those triangles use, order kept, attributes carried; then purged.
 *   crop              min_bound[k] > max_bound[k] for some k: an empty mesh.  Else select over the vertices with
 *                     min <= p <= max in every component, bounds included; a NaN, in a vertex or a bound, fails every test.
 *   transform         T row-major 4 x 4: a row is ((T_i0 x + T_i1 y) + T_i2 z) + T_i3 w, w = 1 for vertices and w = 0 for
 *                     both kinds of normals (T_i3 * 0 is added: a NaN or infinite translation reaches the normals, as in
 *                     the reference); the fourth row of T is not read.
 * from_tsdf copies the LAST EXTRACTED mesh of a volume device to device: the volume's colours become vertex colours, there
 * are no normals; VISMA_ICP_ERR_STATE before an extract (or after a frame or a reset), VISMA_ICP_ERR_INVALID for a volume
 * of another context.  get: each output may be NULL; counts other than the mesh's are VISMA_ICP_ERR_INVALID, asking for an
 * attribute the mesh does not have VISMA_ICP_ERR_STATE.  size: has_flags is a mask of VISMA_ICP_TRIMESH_HAS_*.
 *
 * DEVIATION from the reference, on purpose: every triangle index is checked on the device before a mesh exists, and every
 * selected index before a select; one outside [0, nv) is VISMA_ICP_ERR_INVALID (the reference reads out of bounds).  No
 * kernel indexes a vertex array with an index that has not passed that check.
 * Limits: nv, nt and 3 nt must each fit an int (the sorts take an int count), else VISMA_ICP_ERR_INVALID before anything is
 * allocated.  A sharded context: VISMA_ICP_ERR_INVALID, as for the TSDF volumes.  A mesh of another context:
 * VISMA_ICP_ERR_INVALID.  Memory: the mesh, and while a call runs about as much again (a compaction writes new arrays). */
#define VISMA_ICP_TRIMESH_HAS_VERTEX_NORMALS 1
#define VISMA_ICP_TRIMESH_HAS_VERTEX_COLORS 2
#define VISMA_ICP_TRIMESH_HAS_TRIANGLE_NORMALS 4
typedef struct visma_icp_trimesh visma_icp_trimesh;
VISMA_ICP_API int visma_icp_trimesh_create(visma_icp_ctx *ctx, const double *vertices, int64_t nv, const double *vertex_normals,
                                           const double *vertex_colors, const int32_t *triangles, int64_t nt,
                                           const double *triangle_normals, visma_icp_trimesh **out);
VISMA_ICP_API int visma_icp_trimesh_from_tsdf(visma_icp_ctx *ctx, visma_icp_tsdf *volume, visma_icp_trimesh **out);
VISMA_ICP_API int visma_icp_trimesh_destroy(visma_icp_ctx *ctx, visma_icp_trimesh *mesh);
VISMA_ICP_API int visma_icp_trimesh_size(const visma_icp_trimesh *mesh, int64_t *nv, int64_t *nt, int *has_flags);
VISMA_ICP_API int visma_icp_trimesh_get(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, double *vertices, double *vertex_normals,
                                        double *vertex_colors, int32_t *triangles, double *triangle_normals, int64_t nv, int64_t nt);
VISMA_ICP_API int visma_icp_trimesh_compute_triangle_normals(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, int normalized);
VISMA_ICP_API int visma_icp_trimesh_compute_vertex_normals(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, int normalized);
VISMA_ICP_API int visma_icp_trimesh_normalize_normals(visma_icp_ctx *ctx, visma_icp_trimesh *mesh);
/* the four steps of Purge; *removed (may be NULL): the rows the step removed */
VISMA_ICP_API int visma_icp_trimesh_remove_duplicated_vertices(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, int64_t *removed);
VISMA_ICP_API int visma_icp_trimesh_remove_duplicated_triangles(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, int64_t *removed);
VISMA_ICP_API int visma_icp_trimesh_remove_non_manifold_triangles(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, int64_t *removed);
VISMA_ICP_API int visma_icp_trimesh_remove_non_manifold_vertices(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, int64_t *removed);
VISMA_ICP_API int visma_icp_trimesh_purge(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, int64_t removed[4]);
VISMA_ICP_API int visma_icp_trimesh_select(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, const int64_t *indices, int64_t n,
                                           visma_icp_trimesh **out);
VISMA_ICP_API int visma_icp_trimesh_crop(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, const double min_bound[3],
                                         const double max_bound[3], visma_icp_trimesh **out);
VISMA_ICP_API int visma_icp_trimesh_transform(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, const double T[16]);

/* ---- PointCloud: a cloud resident on the device between the steps of a pipeline -------------------------------------------
 * (the reference's Core/Geometry/PointCloud.h and .cpp :47-198, DownSample.cpp :90-105 and :222-254, EstimateNormals.cpp
 * :158-204, Eigen's Dot.h and LU/InverseImpl.h.)  A cloud is an object owned by its context; it lives until
 * visma_icp_cloud_destroy or the context's end and holds on the device: points (n x 3 f64) and, optionally, normals and
 * colours (n x 3 f64).  "Has X" is the reference's HasX(): an attribute of no rows is not had.  n = 0 is a legal cloud
 * everywhere and launches nothing.  from_tsdf copies the LAST ExtractPointCloud (voxel_cloud 0: points, normals, and colours
 * unless the volume has none) or ExtractVoxelPointCloud (1: points and colours, no normals) of a volume device to device;
 * VISMA_ICP_ERR_STATE before that extract (or after a frame or a reset).
 *
 * EVERY RESULT IS THE REFERENCE'S BIT FOR BIT but for the stated deviations, and a second identical call returns identical
 * bytes: f64, every product, difference and sum rounded on its own (no fused multiply-add), correctly rounded square root and
 * division; no floating-point atomics, one writer per row.
 *   bounds            per axis std::min_element / max_element with a < b.  An empty cloud: zeros.  If the coordinate of
 *                     point 0 is NaN the result is that NaN; otherwise NaNs are skipped and, among equal values, the lowest
 *                     index wins: {0.0, -0.0} gives 0.0 and {-0.0, 0.0} gives -0.0.  (A reduction over (value, index)
 *                     pairs, exact in any order.)
 *   transform         T row-major 4 x 4: a row is ((T_i0 x + T_i1 y) + T_i2 z) + T_i3 w, w = 1 for points and w = 0 for
 *                     normals (T_i3 * 0 is added: a NaN or infinite translation reaches the normals); the fourth row of T
 *                     is not read.  Colours stay.  The kernel is the TriangleMesh's.
 *   normalize_normals per normal n2 = (x x + y y) + z z; if n2 > 0 every component is divided by sqrt(n2), else the normal
 *                     is left as it is.  The kernel is the TriangleMesh's WITHOUT its last step: PointCloud.h has no
 *                     "x is NaN -> (0, 0, 1)" rule, so a NaN normal stays and (inf, 1, 1) becomes (NaN, 0, 0).
 *   paint_uniform_color  every colour becomes rgb; an empty cloud stays without colours.
 *   append            operator+=.  other empty: NOTHING changes (the reference does not even clear the normals).  Else the
 *                     normals survive iff (this is empty or has normals) and other has them; colours by the same rule.
 *                     other may be the cloud itself: it doubles.
 *   select            a NEW cloud: the rows in the order of indices[], a repeated index repeats the row; normals and colours
 *                     are carried.  DEVIATION: an index outside [0, n) is VISMA_ICP_ERR_INVALID (the reference reads out of
 *                     bounds).
 *   uniform_down_sample  a NEW cloud: every_k == 0 gives an empty one (and VISMA_ICP_OK), else the rows 0, k, 2k, ...;
 *                     every_k < 0 is VISMA_ICP_ERR_INVALID (the reference's is a size_t).
 *   crop              a NEW cloud: min_bound[k] > max_bound[k] for some k gives an empty one.  Else the points with
 *                     min <= p <= max in every component, bounds included, in their order; a NaN, in a point or a bound,
 *                     fails every test.
 *   voxel_down_sample a NEW cloud: byte for byte what visma_icp_voxel_down_sample returns for the same rows.
 *   estimate_normals  in place; normals the cloud has keep their sign.  Byte for byte what visma_icp_estimate_normals returns
 *                     for the same rows and normals_in (the search grid's origin, the first point with three finite
 *                     coordinates, is found on the device).  knn < 3 (KNN, Hybrid) or radius <= 0 (Radius, Hybrid): every
 *                     normal is (0, 0, 1).
 *   orient_normals_to_align_with_direction   per normal: norm() == 0.0 -- that is sqrt((x x + y y) + z z) == 0.0, so a squared
 *                     norm that underflows counts as zero -- : the normal becomes ref; else if (x rx + y ry) + z rz < 0 it is
 *                     multiplied by -1.0.
 *   orient_normals_towards_camera_location   ref = camera - point per point; norm() == 0.0: the normal becomes ref,
 *                     normalised as above -- or (0, 0, 1) where ref's norm() == 0.0 too (the camera at the point); else the
 *                     sign rule.  DEVIATION, both: a cloud without normals is VISMA_ICP_ERR_STATE (the reference indexes an
 *                     empty vector).
 *   mean_and_covariance  an empty cloud: a zero mean and the identity.  Else the nine cumulants x, y, z, xx, xy, xz, yy, yz, zz
 *                     (products rounded, then added), divided by n; mean = the first three; cov(0,0) = c3 - c0 c0, ... as
 *                     PointCloud.cpp:164-178; cov row-major.  DEVIATION in the order of the sums, of the kind the centroid of
 *                     visma_icp_set_clouds_f64 has: they run serially over chunks of 16,384 consecutive points and the chunk
 *                     sums are added in chunk order.  A cloud of at most 16,384 points is summed in the reference's own order
 *                     and equals it to the bit; a larger one differs in the last bits but is a function of the input only.
 *   mahalanobis_distance  out[i] = sqrt((p^T C^-1) p), p = point - mean, with the mean and covariance above.  C^-1 is Eigen
 *                     3.3.2's 3 x 3 inverse on the host: the cofactors, det as the sum of the first cofactor column times
 *                     column 0, 1 / det, no invertibility test -- a singular covariance propagates inf and NaN, as in the
 *                     reference.  Three-term sums are (a0 + a1) + a2, as the compiled reference's.
 * get: each output may be NULL; n other than the cloud's is VISMA_ICP_ERR_INVALID, asking for an attribute the cloud does
 * not have VISMA_ICP_ERR_STATE.  size: has_flags is a mask of VISMA_ICP_CLOUD_HAS_*.
 * Limits: n must fit an int (also the sum of an append, and the number of selected indices), else VISMA_ICP_ERR_INVALID.
 * A sharded context: VISMA_ICP_ERR_INVALID.  A cloud or a volume of another context: VISMA_ICP_ERR_INVALID.  Every call
 * returns with the stream idle.  Memory: the cloud, and while a call runs about as much again. */
#define VISMA_ICP_CLOUD_HAS_NORMALS 1
#define VISMA_ICP_CLOUD_HAS_COLORS 2
typedef struct visma_icp_cloud visma_icp_cloud;
VISMA_ICP_API int visma_icp_cloud_create(visma_icp_ctx *ctx, const double *points, int64_t n, const double *normals,
                                         const double *colors, visma_icp_cloud **out);
VISMA_ICP_API int visma_icp_cloud_from_tsdf(visma_icp_ctx *ctx, visma_icp_tsdf *volume, int voxel_cloud, visma_icp_cloud **out);
VISMA_ICP_API int visma_icp_cloud_destroy(visma_icp_ctx *ctx, visma_icp_cloud *cloud);
VISMA_ICP_API int visma_icp_cloud_size(const visma_icp_cloud *cloud, int64_t *n, int *has_flags);
VISMA_ICP_API int visma_icp_cloud_get(visma_icp_ctx *ctx, visma_icp_cloud *cloud, double *points, double *normals, double *colors,
                                      int64_t n);
VISMA_ICP_API int visma_icp_cloud_transform(visma_icp_ctx *ctx, visma_icp_cloud *cloud, const double T[16]);
VISMA_ICP_API int visma_icp_cloud_normalize_normals(visma_icp_ctx *ctx, visma_icp_cloud *cloud);
VISMA_ICP_API int visma_icp_cloud_paint_uniform_color(visma_icp_ctx *ctx, visma_icp_cloud *cloud, const double rgb[3]);
VISMA_ICP_API int visma_icp_cloud_append(visma_icp_ctx *ctx, visma_icp_cloud *cloud, const visma_icp_cloud *other);
VISMA_ICP_API int visma_icp_cloud_bounds(visma_icp_ctx *ctx, visma_icp_cloud *cloud, double min_bound[3], double max_bound[3]);
VISMA_ICP_API int visma_icp_cloud_select(visma_icp_ctx *ctx, visma_icp_cloud *cloud, const int64_t *indices, int64_t n,
                                         visma_icp_cloud **out);
VISMA_ICP_API int visma_icp_cloud_uniform_down_sample(visma_icp_ctx *ctx, visma_icp_cloud *cloud, int64_t every_k,
                                                      visma_icp_cloud **out);
VISMA_ICP_API int visma_icp_cloud_crop(visma_icp_ctx *ctx, visma_icp_cloud *cloud, const double min_bound[3],
                                       const double max_bound[3], visma_icp_cloud **out);
VISMA_ICP_API int visma_icp_cloud_voxel_down_sample(visma_icp_ctx *ctx, visma_icp_cloud *cloud, double voxel_size,
                                                    visma_icp_cloud **out);
/* search_type, knn, radius: as visma_icp_estimate_normals */
VISMA_ICP_API int visma_icp_cloud_estimate_normals(visma_icp_ctx *ctx, visma_icp_cloud *cloud, int search_type, int knn,
                                                   double radius);
VISMA_ICP_API int visma_icp_cloud_orient_normals_to_align_with_direction(visma_icp_ctx *ctx, visma_icp_cloud *cloud,
                                                                         const double ref[3]);
VISMA_ICP_API int visma_icp_cloud_orient_normals_towards_camera_location(visma_icp_ctx *ctx, visma_icp_cloud *cloud,
                                                                         const double camera[3]);
VISMA_ICP_API int visma_icp_cloud_mean_and_covariance(visma_icp_ctx *ctx, visma_icp_cloud *cloud, double mean[3], double cov[9]);
/* out: n doubles on the host */
VISMA_ICP_API int visma_icp_cloud_mahalanobis_distance(visma_icp_ctx *ctx, visma_icp_cloud *cloud, double *out);

/* ---- Image: an image resident on the device between the steps of the RGB-D front end ---------------------------------------
 * (the reference's Core/Geometry/Image.h, Image.cpp, ImageFactory.cpp, RGBDImage.cpp and RGBDImageFactory.cpp.)  An image is
 * an object owned by its context; it lives until visma_icp_image_destroy or the context's end and holds on the device
 * width x height pixels of `channels` channels of 1, 2 or 4 bytes each, row-major, channels interleaved.  create takes 1 .. 4
 * channels (the reference's functions know 1 and 3).  An image of no pixels keeps its format (the reference's
 * PrepareImage(0, 0, 1, 4)) and launches nothing.  "The empty image" below is the reference's Image(): 0 x 0, 0 channels,
 * 0 bytes.  A function whose result is an image returns a NEW object; linear_transform and clip_intensity work in place, as
 * the reference's do.  The arithmetic is the reference's operation for operation: fp32 where it computes in fp32, f64 where
 * it widens, one rounding per operation, fp32 denormals kept.  Two runs give identical bytes.
 *
 *   to_float          CreateFloatImageFromImage: 1 channel: (float)p / 255.0f (1 byte), (float)p (2 bytes), p (float); 3
 *                     channels: Equal (a + b + c) / 3.0f, Weighted 0.2990f a + 0.5870f b + 0.1140f c, each / 255.0f for
 *                     1-byte channels only.  Any other channel count: the all-zero image.  An image without pixels: the empty
 *                     image.  A type that is neither: VISMA_ICP_ERR_INVALID.
 *   depth_to_float    ConvertDepthToFloatImage: to_float(Weighted), p /= (float)depth_scale in fp32, then 0 where
 *                     (double)p >= depth_trunc.
 *   from_float        CreateImageFromFloatImage<uint8_t> (bytes 1: (T)(p * 255.0f)) and <uint16_t> (bytes 2: (T)p); an input
 *                     that is not 1 x float: the empty image.  DEVIATION: the reference's static_cast is defined only where
 *                     the truncated value is representable; outside it this library SATURATES: NaN and negatives give 0,
 *                     values beyond the maximum the maximum.
 *   filter_horizontal FilterHorizontalImage: per tap the fp32 product pixel * (float)kernel[k], widened and added into an f64
 *                     sum in tap order, one cast to fp32; indices clamped at both borders; any odd length (a kernel longer
 *                     than a row is legal).  An even length, or an input that is not 1 x float: the empty image.
 *   filter_separable  FilterImage(dx, dy): horizontal(dx), transpose, horizontal(dy), transpose.
 *   filter            FilterImage(type), VISMA_ICP_IMAGE_GAUSSIAN3 .. SOBEL3DY; an unknown type: VISMA_ICP_ERR_INVALID.
 *   flip              FlipImage, which is a TRANSPOSE: the output is height x width.
 *   downsample        (p1 + p2 + p3 + p4) / 4.0f in fp32, in that order; floor(w / 2) x floor(h / 2), which may be 0 x 0.
 *   dilate            255 where a pixel == 255 lies in the (2k + 1)^2 window inside the image, else 0; k < 0: all zeros.  An
 *                     input that is not 1 x uint8: the empty image.
 *   linear_transform  p = (float)(scale * (double)p + offset).  clip_intensity: p > max -> (float)max, then p < min ->
 *                     (float)min, both compares in f64; a NaN stays.  Both leave an image that is not 1 x float as it is and
 *                     return VISMA_ICP_OK (the reference warns).
 *   pyramid           CreateImagePyramid: out[0] a copy, out[i] = downsample(filter(GAUSSIAN3)(out[i - 1])) or
 *                     downsample(out[i - 1]).  An input that is not 1 x float has NO levels: every out[i] is NULL.
 *   filter_pyramid    FilterImagePyramid: out[i] = filter(in[i], type).
 *   distance_multiplier  CreateDepthToCameraDistanceMultiplierFloatImage for intrinsic = {fx, fy, cx, cy} and w x h: the
 *                     image a TSDF volume integrates with (the same kernel).
 *   float_value_at    Image::FloatValueAt for n coordinates uv (n x 2 f64: u, v): ok[i] (0 / 1) and value[i].  DEVIATION: on
 *                     an image narrower or lower than 2 pixels the reference reads out of bounds, and with a NaN coordinate
 *                     it casts a NaN to int: both give (0, 0.0) here.
 *   rgbd              CreateRGBDImageFromColorAndDepth (COLOR_AND_DEPTH: the two doubles are read), ...FromRedwoodFormat
 *                     (1000, 4), ...FromTUMFormat (5000, 4), ...FromSUNFormat (each 16-bit depth rotated right by 3 bits,
 *                     then 1000, 7), ...FromNYUFormat (bytes swapped, 351.3 / (1092.5 - d), * 1000 rounded, then 1000, 7).
 *                     out_depth = depth_to_float, out_color = to_float(Weighted) or a copy.  Images of different sizes: both
 *                     outputs NULL and VISMA_ICP_OK (the reference's empty RGBDImage).  DEVIATIONS: the reference rewrites
 *                     the caller's SUN / NYU depth in place through a const reference; the resident input is left as it is.
 *                     NYU's (uint16_t)floor(xx * 1000 + 0.5) is undefined for swapped values 1088 .. 1092 (beyond 65535):
 *                     saturated to 65535 here, which the 7 m truncation turns into 0.  A SUN / NYU depth that is not
 *                     1 x uint16 (the reference reinterprets its bytes): VISMA_ICP_ERR_INVALID.
 *
 * Hand-offs: each takes the pixels device to device into the device core of the host-array entry point beside it, so the
 * results are that entry point's byte for byte for the same pixel bytes.
 *   visma_icp_tsdf_integrate_images    depth 1 x float; color of the volume's colour type (RGB8: 3 x uint8, GRAY32: 1 x float;
 *                     not read by a volume without colour).  Anything else: VISMA_ICP_ERR_INVALID, the volume untouched.
 *   visma_icp_odometry_prepare_images, visma_icp_rgbd_odometry_images   four 1 x float images of one size.
 *   visma_icp_cloud_from_depth_image   CreatePointCloudFromDepthImage into a resident visma_icp_cloud: a 1 x float depth as it is, a
 *                     1 x uint16 depth through depth_to_float(depth_scale, depth_trunc) first (the two doubles are read for it
 *                     only); the rows of visma_icp_point_cloud_from_depth.  visma_icp_cloud_from_rgbd_images: a 1 x float depth with
 *                     a 3 x uint8 or 1 x float colour; the rows of visma_icp_point_cloud_from_rgbd.  Any other format: an empty
 *                     cloud and VISMA_ICP_OK, as in the reference.  extrinsic NULL: the identity.
 *   visma_icp_image_from_odometry      a level of the resident odometry pyramid (which < VISMA_ICP_ODOMETRY_SRC_XYZ) as a
 *                     new image: the device-to-device counterpart of visma_icp_odometry_get_image.
 *
 * get: n_bytes other than the image's size is VISMA_ICP_ERR_INVALID.  A sharded context: VISMA_ICP_ERR_INVALID.  An image of
 * another context: VISMA_ICP_ERR_INVALID.  A context without the HIP engine: VISMA_ICP_ERR_STATE.  Every call returns with the
 * stream idle. */
#define VISMA_ICP_IMAGE_EQUAL 0
#define VISMA_ICP_IMAGE_WEIGHTED 1
#define VISMA_ICP_IMAGE_GAUSSIAN3 0
#define VISMA_ICP_IMAGE_GAUSSIAN5 1
#define VISMA_ICP_IMAGE_GAUSSIAN7 2
#define VISMA_ICP_IMAGE_SOBEL3DX 3
#define VISMA_ICP_IMAGE_SOBEL3DY 4
#define VISMA_ICP_RGBD_COLOR_AND_DEPTH 0
#define VISMA_ICP_RGBD_REDWOOD 1
#define VISMA_ICP_RGBD_TUM 2
#define VISMA_ICP_RGBD_SUN 3
#define VISMA_ICP_RGBD_NYU 4
typedef struct visma_icp_image visma_icp_image;
VISMA_ICP_API int visma_icp_image_create(visma_icp_ctx *ctx, int w, int h, int channels, int bytes_per_channel, const void *data,
                                         visma_icp_image **out);
VISMA_ICP_API int visma_icp_image_destroy(visma_icp_ctx *ctx, visma_icp_image *img);
VISMA_ICP_API int visma_icp_image_info(const visma_icp_image *img, int *w, int *h, int *channels, int *bytes_per_channel);
VISMA_ICP_API int visma_icp_image_get(visma_icp_ctx *ctx, visma_icp_image *img, void *bytes, int64_t n_bytes);
VISMA_ICP_API int visma_icp_image_copy(visma_icp_ctx *ctx, visma_icp_image *img, visma_icp_image **out);
VISMA_ICP_API int visma_icp_image_to_float(visma_icp_ctx *ctx, visma_icp_image *img, int type, visma_icp_image **out);
VISMA_ICP_API int visma_icp_image_depth_to_float(visma_icp_ctx *ctx, visma_icp_image *img, double depth_scale, double depth_trunc,
                                                 visma_icp_image **out);
VISMA_ICP_API int visma_icp_image_from_float(visma_icp_ctx *ctx, visma_icp_image *img, int bytes, visma_icp_image **out);
VISMA_ICP_API int visma_icp_image_filter(visma_icp_ctx *ctx, visma_icp_image *img, int type, visma_icp_image **out);
VISMA_ICP_API int visma_icp_image_filter_separable(visma_icp_ctx *ctx, visma_icp_image *img, const double *dx, int n_dx,
                                                   const double *dy, int n_dy, visma_icp_image **out);
VISMA_ICP_API int visma_icp_image_filter_horizontal(visma_icp_ctx *ctx, visma_icp_image *img, const double *kernel, int n,
                                                    visma_icp_image **out);
VISMA_ICP_API int visma_icp_image_flip(visma_icp_ctx *ctx, visma_icp_image *img, visma_icp_image **out);
VISMA_ICP_API int visma_icp_image_downsample(visma_icp_ctx *ctx, visma_icp_image *img, visma_icp_image **out);
VISMA_ICP_API int visma_icp_image_dilate(visma_icp_ctx *ctx, visma_icp_image *img, int half_kernel_size, visma_icp_image **out);
VISMA_ICP_API int visma_icp_image_linear_transform(visma_icp_ctx *ctx, visma_icp_image *img, double scale, double offset);
VISMA_ICP_API int visma_icp_image_clip_intensity(visma_icp_ctx *ctx, visma_icp_image *img, double min, double max);
/* out: room for `levels` pointers */
VISMA_ICP_API int visma_icp_image_pyramid(visma_icp_ctx *ctx, visma_icp_image *img, int levels, int with_gaussian_filter,
                                          visma_icp_image **out);
VISMA_ICP_API int visma_icp_image_filter_pyramid(visma_icp_ctx *ctx, visma_icp_image *const *in, int levels, int type,
                                                 visma_icp_image **out);
VISMA_ICP_API int visma_icp_image_distance_multiplier(visma_icp_ctx *ctx, const double intrinsic[4], int w, int h,
                                                      visma_icp_image **out);
VISMA_ICP_API int visma_icp_image_float_value_at(visma_icp_ctx *ctx, visma_icp_image *img, const double *uv, int64_t n, uint8_t *ok,
                                                 double *value);
VISMA_ICP_API int visma_icp_image_rgbd(visma_icp_ctx *ctx, visma_icp_image *color, visma_icp_image *depth, int format,
                                       double depth_scale, double depth_trunc, int convert_rgb_to_intensity,
                                       visma_icp_image **out_color, visma_icp_image **out_depth);
VISMA_ICP_API int visma_icp_tsdf_integrate_images(visma_icp_ctx *ctx, visma_icp_tsdf *volume, visma_icp_image *depth,
                                                  visma_icp_image *color, const double intrinsic[4], int intrinsic_w,
                                                  int intrinsic_h, const double extrinsic[16]);
VISMA_ICP_API int visma_icp_odometry_prepare_images(visma_icp_ctx *ctx, visma_icp_image *src_gray, visma_icp_image *src_depth,
                                                    visma_icp_image *tgt_gray, visma_icp_image *tgt_depth, const double intrinsic[4],
                                                    const double init[16], const visma_icp_odometry_option *option);
VISMA_ICP_API int visma_icp_rgbd_odometry_images(visma_icp_ctx *ctx, visma_icp_image *src_gray, visma_icp_image *src_depth,
                                                 visma_icp_image *tgt_gray, visma_icp_image *tgt_depth, const double intrinsic[4],
                                                 const double init[16], int method, const visma_icp_odometry_option *option,
                                                 double out_T[16], double out_info[36], visma_icp_odometry_result *out_result);
VISMA_ICP_API int visma_icp_image_from_odometry(visma_icp_ctx *ctx, int which, int level, visma_icp_image **out);
VISMA_ICP_API int visma_icp_cloud_from_depth_image(visma_icp_ctx *ctx, visma_icp_image *depth, const double intrinsic[4],
                                                   const double extrinsic[16], double depth_scale, double depth_trunc, int stride,
                                                   visma_icp_cloud **out);
VISMA_ICP_API int visma_icp_cloud_from_rgbd_images(visma_icp_ctx *ctx, visma_icp_image *depth, visma_icp_image *color,
                                                   const double intrinsic[4], const double extrinsic[16], visma_icp_cloud **out);

/* ---- The mesh renderer: a resident TriangleMesh seen through a pinhole camera, into resident Images ---------------------------
 * The counterpart of the reference's off-screen OpenGL renderer (render/renderer.h:41-160, renderer.cpp, edge_detection.frag):
 * a depth image, the visible triangle per pixel, a binary mask and a depth-edge image.  It is compute, not a graphics
 * pipeline, and its picture is a written rule, the same on the device, in visma_icp_render_host and in tests/render_spec.py:
 *
 *   camera       w x h pixels, intrinsic = [fx, fy, cx, cy] in Open3D's pixel convention (the sample of pixel (x, y) is the
 *                point (x, y): PinholeCameraIntrinsic, the TSDF volume and the odometry); extrinsic: world -> camera, row-major
 *                4 x 4, z forward and y down (the convention of visma_icp_tsdf_integrate); 0 < z_near < z_far
 *   vertex       P = R X + t in f64, ((R_i0 x + R_i1 y) + R_i2 z) + t_i as visma_icp_trimesh_transform computes it
 *   triangle     (a, b, c) with camera points A, B, C: n0 = B x C, n1 = C x A, n2 = A x B (a component is u_y v_z - u_z v_y:
 *                two products, one difference), det = (A_x n0_x + A_y n0_y) + A_z n0_z.  A triangle with a non-finite camera
 *                coordinate is not drawn
 *   box          the pixels a triangle is tested at, part of the rule and not an optimisation.  With k the number of its
 *                vertices at z >= z_near: nothing for k = 0; the whole image for k = 1 or 2; for k = 3 the projections
 *                u = fx (X / Z) + cx, v = fy (Y / Z) + cy of the three vertices, columns floor(min u) - 1 .. ceil(max u) + 1
 *                and rows likewise, clamped to the image (a non-finite min or max: the whole span; wholly off the image:
 *                nothing).  In exact arithmetic the box contains every pixel the triangle covers.  In f64 the edge values
 *                of a degenerate triangle are rounding noise and z = det / s is noise over noise, which can fall inside
 *                [z_near, z_far] anywhere: without the box, a triangle with its vertices on a line through the camera
 *                centre drew 114 pixels of a 32 x 24 image (exact arithmetic: 0), 215 of 1000 random ones of that family
 *                drew outside their box, and 1078 of 3000 scenes with every vertex a few ulps under z_near drew pixels
 *                (exact arithmetic: none)
 *   pixel        (of the box) d = ((x - cx) / fx, (y - cy) / fy, 1), e_i = (n_i.x d.x + n_i.y d.y) + n_i.z, s = (e0 + e1) + e2.
 *                Covered where s != 0 and all e_i >= 0 or all e_i <= 0 (both windings draw, the comparisons are inclusive);
 *                z = det / s; kept where z_near <= z <= z_far.  No clipping, no gap along a shared edge (the two triangles
 *                see exactly negated edge values there), and a function of the inputs alone
 *   winner       the smallest 64-bit key (bits of (float)z << 32) | triangle index: the nearest after the rounding to fp32,
 *                the lowest index among equals
 *   depth        1 x float: (float)z, 0 where nothing is drawn (VISMA_ICP_RENDER_METRIC); or the value of OpenGL's depth
 *                buffer, (float)(0.5 ((z_far + z_near) - 2 z_near z_far / z) / (z_far - z_near) + 0.5) from the winner's f64
 *                z, 1 where nothing is drawn (VISMA_ICP_RENDER_DEPTH_BUFFER): what visma_icp_linearize_depth inverts
 *   index        1 x int32: the winning triangle, -1 where nothing is drawn.  visma_icp_image_info reports 1 channel of 4
 *                bytes, visma_icp_image_is_int32 tells it from a float image; the operations on float images treat it as
 *                any format they do not know
 *   mask         1 x uint8: 255 where something is drawn, else 0
 *   edges        visma_icp_render_edges of a 1 x float METRIC depth image -> 1 x uint8.  v = depth where depth > 0, else
 *                -1.  0 for x < 5, x >= w - 5, y < 5, y >= h - 5 and where the centre has v = -1; else delta =
 *                0.25 (((|W - E| + |S - N|) + |NW - SE|) + |SW - NE|) in f64, c = 0 below 0.05, 1 from 0.10, (delta - 0.05) /
 *                0.05 between; the pixel is floor(255 c + 0.5)
 *
 * Deviations from the reference: samples sit at integer pixel coordinates (SetCamera's frustum samples at (i + 1/2)(w - 1)/w);
 * the depth buffer is not quantised to 24 bits; edges are taken on the true metric depth (the shader re-linearises with
 * the planes 0.05 / 2.0 fixed at construction, renderer.cpp:95-96, whatever the camera's are); the mask is 255 on covered
 * pixels (the reference reads back a colour channel no fragment shader writes); the OpenGL axis flips are dropped; a
 * triangle index outside [0, nv) is already an error of visma_icp_trimesh_create.
 *
 * VISMA_ICP_ERR_INVALID with a message and nothing written: w or h <= 0 or more than 2^30 pixels, fx or fy 0, z_near <= 0,
 * z_far <= z_near, a non-finite camera parameter or extrinsic entry, an unknown encoding, a mesh or image of another context,
 * an image that is not 1 x float for render_edges.  depth, index, mask: each may be NULL. */
enum { VISMA_ICP_RENDER_METRIC = 0, VISMA_ICP_RENDER_DEPTH_BUFFER = 1 };
VISMA_ICP_API int visma_icp_render(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, int w, int h, const double intrinsic[4],
                                   const double extrinsic[16], double z_near, double z_far, int encoding, visma_icp_image **depth,
                                   visma_icp_image **index, visma_icp_image **mask);
VISMA_ICP_API int visma_icp_render_edges(visma_icp_ctx *ctx, visma_icp_image *depth, visma_icp_image **edges);
/* the same arithmetic on host arrays: no context, no GPU.  vertices nv x 3, triangles nt x 3 (an index outside [0, nv):
 * VISMA_ICP_ERR_INVALID); depth, index, mask, edges: w x h each, each may be NULL.  edges is taken on the metric depth,
 * whatever `encoding` is. */
VISMA_ICP_API int visma_icp_render_host(const double *vertices, int64_t nv, const int32_t *triangles, int64_t nt, int w, int h,
                                        const double intrinsic[4], const double extrinsic[16], double z_near, double z_far,
                                        int encoding, float *depth, int32_t *index, uint8_t *mask, uint8_t *edges);
/* the edge rule alone on a host image (w x h floats, metric) */
VISMA_ICP_API int visma_icp_render_edges_host(const float *depth, int w, int h, uint8_t *edges);
/* LinearizeDepth (renderer.h:32-36): 2 z_near z_far / (z_far + z_near - (2 zb - 1)(z_far - z_near)), in f64 */
VISMA_ICP_API double visma_icp_linearize_depth(double zb, double z_near, double z_far);
/* *is_int32: 1 for the renderer's index image, 0 for every other image */
VISMA_ICP_API int visma_icp_image_is_int32(const visma_icp_image *img, int *is_int32);

/* feh::ComputeErrorMetric (include/geometry.h:85-101): out = mean, std, median
 * (sorted[n >> 1]), min, max.  Host only. */
VISMA_ICP_API int visma_icp_error_metric(const double *errors, int64_t n, double out[5]);
/* feh::MeasureSurfaceError (include/geometry.h:117-141): sample the source mesh,
 * distance of every sample to the target mesh, statistics of the distances. */
VISMA_ICP_API int visma_icp_measure_surface_error(visma_icp_ctx *ctx, const double *Vs, int64_t nvs,
                                                  const int32_t *Fs, int64_t nfs, const double *Vt,
                                                  int64_t nvt, const int32_t *Ft, int64_t nft,
                                                  int64_t num_samples, int reference_quirks,
                                                  uint64_t seed, double out[5]);


/* ---- SO(3) maps and their derivatives (host; the device versions are the same code) ----------
 * core/rodrigues.h of the reference on plain arrays.  3x3 matrices row-major; a derivative of
 * (or with respect to) a matrix indexes it by its ROW-MAJOR vectorisation, as the reference
 * (built with EIGEN_DEFAULT_TO_ROW_MAJOR) does:
 *   rodrigues      R = exp(hat(w)),  dR_dw[(3i+j)*3 + k] = dR(i,j)/dw(k)     (:143-182; th < 1e-8 -> I + hat(w))
 *   invrodrigues   w = log(R),       dw_dR[k*9 + 3i+j]   = dw(k)/dR(i,j)     (:184-226; tr -> 3 branch)
 *   project        U V^T of the SVD (projectSO3 :229-237, SO3Type::fitToSO3 core/se3.h:58-61)
 *   matrix_derivatives   dAB_dA, dAB_dB (:87-141), dAt_dA (:58-69), dhat (:17-35), dvee (:43-56);
 *                        any output may be NULL.
 * Jacobian arguments may be NULL. */
/* SE3Type of core/se3.h:79-169 as plain functions on g = [R | t], row-major 3x4: composition (:96-100),
 * action on a point (:103-106: what every search kernel applies to a source point), inverse (:108-110).
 * Host functions (visma_icp_testing.h: visma_icp_selftest_se3 runs the same code on the GPU).  Pinned by the outputs of
 * the reference header itself (tests/golden/se3.npz, oracle/ref_se3.cpp). */
VISMA_ICP_API int visma_se3_compose(const double a[12], const double b[12], double out[12]);
VISMA_ICP_API int visma_se3_act(const double g[12], const double v[3], double out[3]);
VISMA_ICP_API int visma_se3_inv(const double g[12], double out[12]);
VISMA_ICP_API int visma_so3_rodrigues(const double w[3], double R[9], double dR_dw[27]);
VISMA_ICP_API int visma_so3_invrodrigues(const double R[9], double w[3], double dw_dR[27]);
VISMA_ICP_API int visma_so3_project(const double A[9], double R[9]);
VISMA_ICP_API int visma_so3_matrix_derivatives(const double A[9], const double B[9],
                                               double dAB_dA[81], double dAB_dB[81],
                                               double dAt_dA[81], double dhat[27], double dvee[27]);

#ifdef __cplusplus
}
#endif
#endif /* VISMA_ICP_H */

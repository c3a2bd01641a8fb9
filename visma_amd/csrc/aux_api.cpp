// aux_api.cpp -- C ABI of the steps either side of the ICP loop: VoxelDownSample, EstimateNormals, mesh sampling
// and point-to-mesh distance, cloud-to-cloud and nearest-neighbour distances, FPFH / fast global registration / RANSAC global
// registration (no initial pose), the error metric, and the SO(3) / SE(3) functions (host + device self-tests).
#include "driver_ctx.hpp"
#include "plane_math.hpp"
#include "ransac.hpp"
#include "render_math.hpp"
#include "mc_table.h"

extern "C" {

int visma_icp_voxel_down_sample(visma_icp_ctx *ctx, const double *xyz, int64_t n, const double *normals,
                                const double *colors, double voxel_size, double *out_xyz,
                                double *out_normals, double *out_colors, int64_t *n_out)
{
    CTX_CHECK();
    if (!n_out || n < 0 || (n > 0 && (!xyz || !out_xyz)) || (normals && !out_normals) || (colors && !out_colors))
        return ctx->fail(VISMA_ICP_ERR_INVALID, "bad voxel_down_sample arguments");
    if (n > 0x7fffffff) return ctx->fail(VISMA_ICP_ERR_INVALID, "too many points for 32-bit indices");
    if (!ctx->eng->supports_device_loop())   // only the HIP engine owns a GPU
        return ctx->fail(VISMA_ICP_ERR_STATE, "voxel_down_sample needs the HIP engine");
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    hipError_t e = voxel_down_sample_device(xyz, normals, colors, n, voxel_size, out_xyz, out_normals,
                                            out_colors, n_out, ctx->eng->aux_stream());
    if (e != hipSuccess) return ctx->fail(VISMA_ICP_ERR_HIP, std::string("voxel_down_sample: ") + hipGetErrorString(e));
    return VISMA_ICP_OK;
}

int visma_icp_estimate_normals(visma_icp_ctx *ctx, const double *xyz, int64_t n, const double *normals_in,
                               int search_type, int knn, double radius, double *normals_out)
{
    CTX_CHECK();
    if (n < 0 || (n > 0 && (!xyz || !normals_out)) || search_type < 0 || search_type > 2)
        return ctx->fail(VISMA_ICP_ERR_INVALID, "bad estimate_normals arguments");
    if (n > 0x7fffffff) return ctx->fail(VISMA_ICP_ERR_INVALID, "too many points for 32-bit indices");
    if (!ctx->eng->supports_device_loop()) return ctx->fail(VISMA_ICP_ERR_STATE, "estimate_normals needs the HIP engine");
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    hipError_t e = estimate_normals_device(xyz, n, normals_in, search_type, knn, radius, normals_out,
                                           ctx->eng->aux_stream());
    if (e != hipSuccess) return ctx->fail(e == hipErrorInvalidValue ? VISMA_ICP_ERR_INVALID : VISMA_ICP_ERR_HIP,
                                          std::string("estimate_normals: ") + hipGetErrorString(e));
    return VISMA_ICP_OK;
}

int visma_icp_color_gradient(visma_icp_ctx *ctx, const double *xyz, int64_t n, const double *normals, const double *colors,
                             double radius, int max_nn, double *out_grad)
{
    CTX_CHECK();
    if (n < 0 || (n > 0 && (!xyz || !normals || !colors || !out_grad)) || std::isnan(radius))
        return ctx->fail(VISMA_ICP_ERR_INVALID, "bad color_gradient arguments");
    if (max_nn < 3 || max_nn > kNormalsMaxList) return ctx->fail(VISMA_ICP_ERR_INVALID, "color_gradient: max_nn must lie in [3, 170]");
    if (n > 0x7fffffff) return ctx->fail(VISMA_ICP_ERR_INVALID, "too many points for 32-bit indices");
    if (!ctx->eng->supports_device_loop()) return ctx->fail(VISMA_ICP_ERR_STATE, "color_gradient needs the HIP engine");
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    hipError_t e = color_gradient_device(xyz, n, normals, colors, radius, max_nn, out_grad, ctx->eng->aux_stream());
    if (e != hipSuccess) return ctx->fail(e == hipErrorInvalidValue ? VISMA_ICP_ERR_INVALID : VISMA_ICP_ERR_HIP,
                                          std::string("color_gradient: ") + hipGetErrorString(e));
    return VISMA_ICP_OK;
}

// ---- KDTreeFlann: a cloud resident on the device, searched for any query points (kdtree.hip) ----
#define TREE_CHECK()                                                                                  \
    if (!tree || !tree->ctx) { g_create_error = "tree is NULL"; return VISMA_ICP_ERR_INVALID; }      \
    visma_icp_ctx *const ctx = tree->ctx;

static int kdtree_fail(visma_icp_ctx *ctx, const char *what, hipError_t e)
{
    (void)hipGetLastError();
    return ctx->fail(VISMA_ICP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

static bool kdtree_radius_ok(double radius) { return std::isfinite(radius) && radius > 0.0; }

int visma_icp_kdtree_create(visma_icp_ctx *ctx, const double *xyz, int64_t n, visma_icp_kdtree **out)
{
    CTX_CHECK();
    if (!out) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    *out = nullptr;
    if (!xyz || n < 1) return ctx->fail(VISMA_ICP_ERR_INVALID, "kdtree_create: a cloud of at least one point");
    if (n > 0x7fffffff) return ctx->fail(VISMA_ICP_ERR_INVALID, "too many points for 32-bit indices");
    if (!ctx->eng->supports_device_loop()) return ctx->fail(VISMA_ICP_ERR_STATE, "kdtree needs the HIP engine");
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    std::unique_ptr<visma_icp_kdtree> t(new visma_icp_kdtree);
    t->ctx = ctx; t->n = n;
    const hipError_t e = kdtree_device_create(xyz, n, ctx->eng->aux_stream(), &t->dev);
    if (e != hipSuccess) return kdtree_fail(ctx, "kdtree_create", e);
    *out = t.get();
    ctx->trees.push_back(std::move(t));
    return VISMA_ICP_OK;
}

int visma_icp_kdtree_destroy(visma_icp_kdtree *tree)
{
    TREE_CHECK();
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    for (size_t i = 0; i < ctx->trees.size(); i++)
        if (ctx->trees[i].get() == tree) { ctx->trees.erase(ctx->trees.begin() + (std::ptrdiff_t)i); return VISMA_ICP_OK; }
    return ctx->fail(VISMA_ICP_ERR_INVALID, "no such tree");
}

int64_t visma_icp_kdtree_size(const visma_icp_kdtree *tree) { return tree ? tree->n : 0; }

static int kdtree_search_lists(visma_icp_kdtree *tree, bool knn, const double *queries, int64_t nq, double radius, int cap,
                               int32_t *idx, double *d2, int32_t *cnt)
{
    TREE_CHECK();
    const char *what = knn ? "kdtree_search_knn" : "kdtree_search_hybrid";
    if (nq < 0 || cap < 1 || (!knn && !kdtree_radius_ok(radius)))
        return ctx->fail(VISMA_ICP_ERR_INVALID, std::string(what) + (knn ? ": nq >= 0 and knn >= 1" : ": nq >= 0, max_nn >= 1 and a finite radius > 0"));
    if (nq > 0 && (!queries || !idx || !d2 || !cnt)) return ctx->fail(VISMA_ICP_ERR_INVALID, std::string(what) + ": NULL argument");
    if (nq > 0x7fffffff) return ctx->fail(VISMA_ICP_ERR_INVALID, "too many queries for one call");
    if (nq == 0) return VISMA_ICP_OK;
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    const hipError_t e = kdtree_device_search(tree->dev, knn, queries, nq, knn ? 0.0 : radius, cap, idx, d2, cnt, ctx->eng->aux_stream());
    return e == hipSuccess ? VISMA_ICP_OK : kdtree_fail(ctx, what, e);
}

int visma_icp_kdtree_search_knn(visma_icp_kdtree *tree, const double *queries, int64_t nq, int knn, int32_t *idx, double *d2,
                                int32_t *cnt)
{
    return kdtree_search_lists(tree, true, queries, nq, 0.0, knn, idx, d2, cnt);
}

int visma_icp_kdtree_search_hybrid(visma_icp_kdtree *tree, const double *queries, int64_t nq, double radius, int max_nn,
                                   int32_t *idx, double *d2, int32_t *cnt)
{
    return kdtree_search_lists(tree, false, queries, nq, radius, max_nn, idx, d2, cnt);
}

int visma_icp_kdtree_search_radius(visma_icp_kdtree *tree, const double *queries, int64_t nq, double radius, int64_t *offsets,
                                   int64_t *total)
{
    TREE_CHECK();
    if (nq < 0 || !kdtree_radius_ok(radius)) return ctx->fail(VISMA_ICP_ERR_INVALID, "kdtree_search_radius: nq >= 0 and a finite radius > 0");
    if (!offsets || !total || (nq > 0 && !queries)) return ctx->fail(VISMA_ICP_ERR_INVALID, "kdtree_search_radius: NULL argument");
    if (nq > 0x7fffffff) return ctx->fail(VISMA_ICP_ERR_INVALID, "too many queries for one call");
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    const hipError_t e = kdtree_device_search_radius(tree->dev, queries, nq, radius, offsets, total, ctx->eng->aux_stream());
    if (e == hipErrorOutOfMemory && *total > kKdTreeMaxRadiusEntries) {
        (void)hipGetLastError();
        return ctx->fail(VISMA_ICP_ERR_INVALID, "kdtree_search_radius: more than VISMA_ICP_KDTREE_MAX_RADIUS_ENTRIES entries; search fewer queries a call");
    }
    return e == hipSuccess ? VISMA_ICP_OK : kdtree_fail(ctx, "kdtree_search_radius", e);
}

int visma_icp_kdtree_get_radius_result(visma_icp_kdtree *tree, int32_t *idx, double *d2)
{
    TREE_CHECK();
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    const hipError_t e = kdtree_device_radius_result(tree->dev, idx, d2, ctx->eng->aux_stream());
    if (e == hipErrorNotReady) return ctx->fail(VISMA_ICP_ERR_STATE, "kdtree_get_radius_result: no radius search before it");
    if (e == hipErrorInvalidValue) return ctx->fail(VISMA_ICP_ERR_INVALID, "kdtree_get_radius_result: NULL argument");
    return e == hipSuccess ? VISMA_ICP_OK : kdtree_fail(ctx, "kdtree_get_radius_result", e);
}

// ---- TriangleMesh: a mesh resident on the device (trimesh.hip) ----
static int trimesh_enter(visma_icp_ctx *ctx, visma_icp_trimesh *mesh)
{
    if (mesh) {
        bool mine = false;
        for (const auto &m : ctx->meshes) mine = mine || m.get() == mesh;
        if (!mine) return ctx->fail(VISMA_ICP_ERR_INVALID, "not a mesh of this context");
    }
    if (ctx->sharded() || ctx->eng->is_sharded()) return ctx->fail(VISMA_ICP_ERR_INVALID, "a triangle mesh lives on one rank");
    if (!ctx->eng->supports_device_loop()) return ctx->fail(VISMA_ICP_ERR_STATE, "a triangle mesh needs the HIP engine");
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    return VISMA_ICP_OK;
}

static int trimesh_done(visma_icp_ctx *ctx, const char *what, hipError_t e)
{
    if (e == hipSuccess) return VISMA_ICP_OK;
    (void)hipGetLastError();
    if (e == hipErrorInvalidValue) return ctx->fail(VISMA_ICP_ERR_INVALID, std::string(what) + ": an index outside [0, nv)");
    return ctx->fail(VISMA_ICP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

static int trimesh_adopt(visma_icp_ctx *ctx, TriMeshDevice *dev, visma_icp_trimesh **out)
{
    std::unique_ptr<visma_icp_trimesh> m(new visma_icp_trimesh);
    m->ctx = ctx; m->dev = dev;
    *out = m.get();
    ctx->meshes.push_back(std::move(m));
    return VISMA_ICP_OK;
}

#define TRIMESH_CHECK(mesh)                                                                  \
    CTX_CHECK();                                                                             \
    if (!(mesh)) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL mesh");                      \
    if (int rc_ = trimesh_enter(ctx, (mesh))) return rc_;

// hipCUB's sorts take an int count: nv, nt and 3 nt must each fit one
static bool trimesh_counts_ok(int64_t nv, int64_t nt) { return nv >= 0 && nt >= 0 && nv <= 0x7fffffff && nt <= 0x7fffffff / 3; }

int visma_icp_trimesh_create(visma_icp_ctx *ctx, const double *vertices, int64_t nv, const double *vertex_normals,
                             const double *vertex_colors, const int32_t *triangles, int64_t nt, const double *triangle_normals,
                             visma_icp_trimesh **out)
{
    CTX_CHECK();
    if (!out) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    *out = nullptr;
    if (!trimesh_counts_ok(nv, nt)) return ctx->fail(VISMA_ICP_ERR_INVALID, "trimesh_create: nv, nt and 3 nt must each fit an int");
    if ((nv > 0 && !vertices) || (nt > 0 && !triangles)) return ctx->fail(VISMA_ICP_ERR_INVALID, "trimesh_create: NULL argument");
    if (int rc = trimesh_enter(ctx, nullptr)) return rc;
    TriMeshDevice *dev = nullptr;
    const hipError_t e = trimesh_device_create(vertices, nv, vertex_normals, vertex_colors, triangles, nt, triangle_normals, false,
                                               ctx->eng->aux_stream(), &dev);
    if (e != hipSuccess) return trimesh_done(ctx, "trimesh_create", e);
    return trimesh_adopt(ctx, dev, out);
}

int visma_icp_trimesh_from_tsdf(visma_icp_ctx *ctx, visma_icp_tsdf *volume, visma_icp_trimesh **out)
{
    CTX_CHECK();
    if (!out) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    *out = nullptr;
    bool mine = false;
    for (const auto &v : ctx->volumes) mine = mine || (volume && v.get() == volume);
    if (!mine) return ctx->fail(VISMA_ICP_ERR_INVALID, volume ? "not a volume of this context" : "NULL volume");
    if (int rc = trimesh_enter(ctx, nullptr)) return rc;
    if (volume->mesh_rows[0] < 0) return ctx->fail(VISMA_ICP_ERR_STATE, "no mesh: extract first");
    TsdfMeshView view;
    if (int rc = ctx->eng->tsdf_mesh_view(volume->id, &view)) return ctx->eng_fail(rc);
    if (!trimesh_counts_ok(view.nv, view.nt)) return ctx->fail(VISMA_ICP_ERR_INVALID, "trimesh_from_tsdf: nv, nt and 3 nt must each fit an int");
    TriMeshDevice *dev = nullptr;
    const hipError_t e = trimesh_device_create(view.vertices, view.nv, nullptr, view.colors, view.triangles, view.nt, nullptr, true,
                                               ctx->eng->aux_stream(), &dev);
    if (e != hipSuccess) return trimesh_done(ctx, "trimesh_from_tsdf", e);
    return trimesh_adopt(ctx, dev, out);
}

int visma_icp_trimesh_destroy(visma_icp_ctx *ctx, visma_icp_trimesh *mesh)
{
    CTX_CHECK();
    if (!mesh) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL mesh");
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    for (size_t i = 0; i < ctx->meshes.size(); i++)
        if (ctx->meshes[i].get() == mesh) { ctx->meshes.erase(ctx->meshes.begin() + (std::ptrdiff_t)i); return VISMA_ICP_OK; }
    return ctx->fail(VISMA_ICP_ERR_INVALID, "not a mesh of this context");
}

int visma_icp_trimesh_size(const visma_icp_trimesh *mesh, int64_t *nv, int64_t *nt, int *has_flags)
{
    if (!mesh || !mesh->dev) { g_create_error = "mesh is NULL"; return VISMA_ICP_ERR_INVALID; }
    int64_t v = 0, t = 0;
    int f = 0;
    trimesh_device_size(mesh->dev, &v, &t, &f);
    if (nv) *nv = v;
    if (nt) *nt = t;
    if (has_flags) *has_flags = f;
    return VISMA_ICP_OK;
}

int visma_icp_trimesh_get(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, double *vertices, double *vertex_normals, double *vertex_colors,
                          int32_t *triangles, double *triangle_normals, int64_t nv, int64_t nt)
{
    TRIMESH_CHECK(mesh);
    int64_t v = 0, t = 0;
    int f = 0;
    trimesh_device_size(mesh->dev, &v, &t, &f);
    if (nv != v || nt != t) return ctx->fail(VISMA_ICP_ERR_INVALID, "trimesh_get: nv or nt differs from the mesh's counts");
    if ((vertex_normals && !(f & kTriMeshVertexNormals)) || (vertex_colors && !(f & kTriMeshVertexColors)) ||
        (triangle_normals && !(f & kTriMeshTriangleNormals)))
        return ctx->fail(VISMA_ICP_ERR_STATE, "trimesh_get: the mesh does not have that attribute");
    return trimesh_done(ctx, "trimesh_get", trimesh_device_get(mesh->dev, vertices, vertex_normals, vertex_colors, triangles,
                                                               triangle_normals, ctx->eng->aux_stream()));
}

int visma_icp_trimesh_compute_triangle_normals(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, int normalized)
{
    TRIMESH_CHECK(mesh);
    return trimesh_done(ctx, "trimesh_compute_triangle_normals",
                        trimesh_device_compute_triangle_normals(mesh->dev, normalized != 0, ctx->eng->aux_stream()));
}

int visma_icp_trimesh_compute_vertex_normals(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, int normalized)
{
    TRIMESH_CHECK(mesh);
    return trimesh_done(ctx, "trimesh_compute_vertex_normals",
                        trimesh_device_compute_vertex_normals(mesh->dev, normalized != 0, ctx->eng->aux_stream()));
}

int visma_icp_trimesh_normalize_normals(visma_icp_ctx *ctx, visma_icp_trimesh *mesh)
{
    TRIMESH_CHECK(mesh);
    return trimesh_done(ctx, "trimesh_normalize_normals", trimesh_device_normalize_normals(mesh->dev, ctx->eng->aux_stream()));
}

static int trimesh_remove(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, int step, int64_t *removed)
{
    TRIMESH_CHECK(mesh);
    int64_t r = 0;
    const hipError_t e = trimesh_device_remove(mesh->dev, step, &r, ctx->eng->aux_stream());
    if (removed) *removed = r;
    return trimesh_done(ctx, "trimesh_remove", e);
}

int visma_icp_trimesh_remove_duplicated_vertices(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, int64_t *removed) { return trimesh_remove(ctx, mesh, 0, removed); }
int visma_icp_trimesh_remove_duplicated_triangles(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, int64_t *removed) { return trimesh_remove(ctx, mesh, 1, removed); }
int visma_icp_trimesh_remove_non_manifold_triangles(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, int64_t *removed) { return trimesh_remove(ctx, mesh, 2, removed); }
int visma_icp_trimesh_remove_non_manifold_vertices(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, int64_t *removed) { return trimesh_remove(ctx, mesh, 3, removed); }

int visma_icp_trimesh_purge(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, int64_t removed[4])
{
    TRIMESH_CHECK(mesh);
    int64_t r[4] = {0, 0, 0, 0};
    const hipError_t e = trimesh_device_purge(mesh->dev, r, ctx->eng->aux_stream());
    if (removed) std::copy(r, r + 4, removed);
    return trimesh_done(ctx, "trimesh_purge", e);
}

int visma_icp_trimesh_select(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, const int64_t *indices, int64_t n, visma_icp_trimesh **out)
{
    CTX_CHECK();
    if (!out) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    *out = nullptr;
    if (!mesh) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL mesh");
    if (n < 0 || (n > 0 && !indices)) return ctx->fail(VISMA_ICP_ERR_INVALID, "trimesh_select: n >= 0 indices");
    if (int rc = trimesh_enter(ctx, mesh)) return rc;
    TriMeshDevice *dev = nullptr;
    const hipError_t e = trimesh_device_select(mesh->dev, indices, n, ctx->eng->aux_stream(), &dev);
    if (e != hipSuccess) return trimesh_done(ctx, "trimesh_select", e);
    return trimesh_adopt(ctx, dev, out);
}

int visma_icp_trimesh_crop(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, const double min_bound[3], const double max_bound[3],
                           visma_icp_trimesh **out)
{
    CTX_CHECK();
    if (!out) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    *out = nullptr;
    if (!mesh || !min_bound || !max_bound) return ctx->fail(VISMA_ICP_ERR_INVALID, "trimesh_crop: NULL argument");
    if (int rc = trimesh_enter(ctx, mesh)) return rc;
    TriMeshDevice *dev = nullptr;
    const hipError_t e = trimesh_device_crop(mesh->dev, min_bound, max_bound, ctx->eng->aux_stream(), &dev);
    if (e != hipSuccess) return trimesh_done(ctx, "trimesh_crop", e);
    return trimesh_adopt(ctx, dev, out);
}

int visma_icp_trimesh_transform(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, const double T[16])
{
    TRIMESH_CHECK(mesh);
    if (!T) return ctx->fail(VISMA_ICP_ERR_INVALID, "trimesh_transform: NULL argument");
    return trimesh_done(ctx, "trimesh_transform", trimesh_device_transform(mesh->dev, T, ctx->eng->aux_stream()));
}

// ---- PointCloud: a cloud resident on the device (cloud.hip) ----
static int cloud_enter(visma_icp_ctx *ctx, const visma_icp_cloud *cloud)
{
    if (cloud) {
        bool mine = false;
        for (const auto &c : ctx->clouds) mine = mine || c.get() == cloud;
        if (!mine) return ctx->fail(VISMA_ICP_ERR_INVALID, "not a cloud of this context");
    }
    if (ctx->sharded() || ctx->eng->is_sharded()) return ctx->fail(VISMA_ICP_ERR_INVALID, "a point cloud lives on one rank");
    if (!ctx->eng->supports_device_loop()) return ctx->fail(VISMA_ICP_ERR_STATE, "a point cloud needs the HIP engine");
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    return VISMA_ICP_OK;
}

static int cloud_done(visma_icp_ctx *ctx, const char *what, hipError_t e)
{
    if (e == hipSuccess) return VISMA_ICP_OK;
    (void)hipGetLastError();
    if (e == hipErrorInvalidValue) return ctx->fail(VISMA_ICP_ERR_INVALID, std::string(what) + ": an index outside [0, n), or more rows than an int holds");
    return ctx->fail(VISMA_ICP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

static int cloud_adopt(visma_icp_ctx *ctx, CloudDevice *dev, visma_icp_cloud **out)
{
    std::unique_ptr<visma_icp_cloud> c(new visma_icp_cloud);
    c->ctx = ctx; c->dev = dev;
    *out = c.get();
    ctx->clouds.push_back(std::move(c));
    return VISMA_ICP_OK;
}

#define CLOUD_CHECK(cloud)                                                                   \
    CTX_CHECK();                                                                             \
    if (!(cloud)) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL cloud");                    \
    if (int rc_ = cloud_enter(ctx, (cloud))) return rc_;

// an operation that makes a new cloud: the checks before it
#define CLOUD_NEW_CHECK(cloud)                                                               \
    CTX_CHECK();                                                                             \
    if (!out) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");                       \
    *out = nullptr;                                                                          \
    if (!(cloud)) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL cloud");                    \
    if (int rc_ = cloud_enter(ctx, (cloud))) return rc_;

int visma_icp_cloud_create(visma_icp_ctx *ctx, const double *points, int64_t n, const double *normals, const double *colors,
                           visma_icp_cloud **out)
{
    CTX_CHECK();
    if (!out) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    *out = nullptr;
    if (n < 0 || n > 0x7fffffff) return ctx->fail(VISMA_ICP_ERR_INVALID, "cloud_create: n must fit an int");
    if (n > 0 && !points) return ctx->fail(VISMA_ICP_ERR_INVALID, "cloud_create: NULL argument");
    if (int rc = cloud_enter(ctx, nullptr)) return rc;
    CloudDevice *dev = nullptr;
    const hipError_t e = cloud_device_create(points, n, normals, colors, false, ctx->eng->aux_stream(), &dev);
    if (e != hipSuccess) return cloud_done(ctx, "cloud_create", e);
    return cloud_adopt(ctx, dev, out);
}

int visma_icp_cloud_from_tsdf(visma_icp_ctx *ctx, visma_icp_tsdf *volume, int voxel_cloud, visma_icp_cloud **out)
{
    CTX_CHECK();
    if (!out) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    *out = nullptr;
    bool mine = false;
    for (const auto &v : ctx->volumes) mine = mine || (volume && v.get() == volume);
    if (!mine) return ctx->fail(VISMA_ICP_ERR_INVALID, volume ? "not a volume of this context" : "NULL volume");
    if (voxel_cloud != 0 && voxel_cloud != 1) return ctx->fail(VISMA_ICP_ERR_INVALID, "cloud_from_tsdf: voxel_cloud is 0 or 1");
    if (int rc = cloud_enter(ctx, nullptr)) return rc;
    if (volume->rows[voxel_cloud] < 0) return ctx->fail(VISMA_ICP_ERR_STATE, "no extraction: extract first");
    TsdfCloudView view;
    if (int rc = ctx->eng->tsdf_cloud_view(volume->id, voxel_cloud, &view)) return ctx->eng_fail(rc);
    if (view.n > 0x7fffffff) return ctx->fail(VISMA_ICP_ERR_INVALID, "cloud_from_tsdf: n must fit an int");
    CloudDevice *dev = nullptr;
    const hipError_t e = cloud_device_create(view.points, view.n, view.normals, view.colors, true, ctx->eng->aux_stream(), &dev);
    if (e != hipSuccess) return cloud_done(ctx, "cloud_from_tsdf", e);
    return cloud_adopt(ctx, dev, out);
}

int visma_icp_cloud_destroy(visma_icp_ctx *ctx, visma_icp_cloud *cloud)
{
    CTX_CHECK();
    if (!cloud) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL cloud");
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    for (size_t i = 0; i < ctx->clouds.size(); i++)
        if (ctx->clouds[i].get() == cloud) { ctx->clouds.erase(ctx->clouds.begin() + (std::ptrdiff_t)i); return VISMA_ICP_OK; }
    return ctx->fail(VISMA_ICP_ERR_INVALID, "not a cloud of this context");
}

int visma_icp_cloud_size(const visma_icp_cloud *cloud, int64_t *n, int *has_flags)
{
    if (!cloud || !cloud->dev) { g_create_error = "cloud is NULL"; return VISMA_ICP_ERR_INVALID; }
    int64_t rows = 0;
    int f = 0;
    cloud_device_size(cloud->dev, &rows, &f);
    if (n) *n = rows;
    if (has_flags) *has_flags = f;
    return VISMA_ICP_OK;
}

int visma_icp_cloud_get(visma_icp_ctx *ctx, visma_icp_cloud *cloud, double *points, double *normals, double *colors, int64_t n)
{
    CLOUD_CHECK(cloud);
    int64_t rows = 0;
    int f = 0;
    cloud_device_size(cloud->dev, &rows, &f);
    if (n != rows) return ctx->fail(VISMA_ICP_ERR_INVALID, "cloud_get: n differs from the cloud's count");
    if ((normals && !(f & kCloudNormals)) || (colors && !(f & kCloudColors)))
        return ctx->fail(VISMA_ICP_ERR_STATE, "cloud_get: the cloud does not have that attribute");
    return cloud_done(ctx, "cloud_get", cloud_device_get(cloud->dev, points, normals, colors, ctx->eng->aux_stream()));
}

int visma_icp_cloud_transform(visma_icp_ctx *ctx, visma_icp_cloud *cloud, const double T[16])
{
    CLOUD_CHECK(cloud);
    if (!T) return ctx->fail(VISMA_ICP_ERR_INVALID, "cloud_transform: NULL argument");
    return cloud_done(ctx, "cloud_transform", cloud_device_transform(cloud->dev, T, ctx->eng->aux_stream()));
}

int visma_icp_cloud_normalize_normals(visma_icp_ctx *ctx, visma_icp_cloud *cloud)
{
    CLOUD_CHECK(cloud);
    return cloud_done(ctx, "cloud_normalize_normals", cloud_device_normalize_normals(cloud->dev, ctx->eng->aux_stream()));
}

int visma_icp_cloud_paint_uniform_color(visma_icp_ctx *ctx, visma_icp_cloud *cloud, const double rgb[3])
{
    CLOUD_CHECK(cloud);
    if (!rgb) return ctx->fail(VISMA_ICP_ERR_INVALID, "cloud_paint_uniform_color: NULL argument");
    return cloud_done(ctx, "cloud_paint_uniform_color", cloud_device_paint_uniform_color(cloud->dev, rgb, ctx->eng->aux_stream()));
}

int visma_icp_cloud_append(visma_icp_ctx *ctx, visma_icp_cloud *cloud, const visma_icp_cloud *other)
{
    CLOUD_CHECK(cloud);
    if (!other) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL cloud");
    if (int rc = cloud_enter(ctx, other)) return rc;
    return cloud_done(ctx, "cloud_append", cloud_device_append(cloud->dev, other->dev, ctx->eng->aux_stream()));
}

int visma_icp_cloud_bounds(visma_icp_ctx *ctx, visma_icp_cloud *cloud, double min_bound[3], double max_bound[3])
{
    CLOUD_CHECK(cloud);
    if (!min_bound || !max_bound) return ctx->fail(VISMA_ICP_ERR_INVALID, "cloud_bounds: NULL argument");
    return cloud_done(ctx, "cloud_bounds", cloud_device_bounds(cloud->dev, min_bound, max_bound, ctx->eng->aux_stream()));
}

int visma_icp_cloud_select(visma_icp_ctx *ctx, visma_icp_cloud *cloud, const int64_t *indices, int64_t n, visma_icp_cloud **out)
{
    CLOUD_NEW_CHECK(cloud);
    if (n < 0 || n > 0x7fffffff || (n > 0 && !indices)) return ctx->fail(VISMA_ICP_ERR_INVALID, "cloud_select: 0 <= n indices, n fits an int");
    CloudDevice *dev = nullptr;
    const hipError_t e = cloud_device_select(cloud->dev, indices, n, ctx->eng->aux_stream(), &dev);
    if (e != hipSuccess) return cloud_done(ctx, "cloud_select", e);
    return cloud_adopt(ctx, dev, out);
}

int visma_icp_cloud_uniform_down_sample(visma_icp_ctx *ctx, visma_icp_cloud *cloud, int64_t every_k, visma_icp_cloud **out)
{
    CLOUD_NEW_CHECK(cloud);
    if (every_k < 0) return ctx->fail(VISMA_ICP_ERR_INVALID, "cloud_uniform_down_sample: every_k >= 0");
    CloudDevice *dev = nullptr;
    const hipError_t e = cloud_device_uniform_down_sample(cloud->dev, every_k, ctx->eng->aux_stream(), &dev);
    if (e != hipSuccess) return cloud_done(ctx, "cloud_uniform_down_sample", e);
    return cloud_adopt(ctx, dev, out);
}

int visma_icp_cloud_crop(visma_icp_ctx *ctx, visma_icp_cloud *cloud, const double min_bound[3], const double max_bound[3],
                         visma_icp_cloud **out)
{
    CLOUD_NEW_CHECK(cloud);
    if (!min_bound || !max_bound) return ctx->fail(VISMA_ICP_ERR_INVALID, "cloud_crop: NULL argument");
    CloudDevice *dev = nullptr;
    const hipError_t e = cloud_device_crop(cloud->dev, min_bound, max_bound, ctx->eng->aux_stream(), &dev);
    if (e != hipSuccess) return cloud_done(ctx, "cloud_crop", e);
    return cloud_adopt(ctx, dev, out);
}

int visma_icp_cloud_voxel_down_sample(visma_icp_ctx *ctx, visma_icp_cloud *cloud, double voxel_size, visma_icp_cloud **out)
{
    CLOUD_NEW_CHECK(cloud);
    CloudDevice *dev = nullptr;
    const hipError_t e = cloud_device_voxel_down_sample(cloud->dev, voxel_size, ctx->eng->aux_stream(), &dev);
    if (e != hipSuccess) return cloud_done(ctx, "cloud_voxel_down_sample", e);
    return cloud_adopt(ctx, dev, out);
}

int visma_icp_cloud_estimate_normals(visma_icp_ctx *ctx, visma_icp_cloud *cloud, int search_type, int knn, double radius)
{
    CLOUD_CHECK(cloud);
    if (search_type < 0 || search_type > 2) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad estimate_normals arguments");
    return cloud_done(ctx, "cloud_estimate_normals",
                      cloud_device_estimate_normals(cloud->dev, search_type, knn, radius, ctx->eng->aux_stream()));
}

static int cloud_orient(visma_icp_ctx *ctx, visma_icp_cloud *cloud, bool camera, const double ref[3])
{
    CLOUD_CHECK(cloud);
    if (!ref) return ctx->fail(VISMA_ICP_ERR_INVALID, "cloud_orient_normals: NULL argument");
    int64_t rows = 0;
    int f = 0;
    cloud_device_size(cloud->dev, &rows, &f);
    if (!(f & kCloudNormals)) return ctx->fail(VISMA_ICP_ERR_STATE, "cloud_orient_normals: the cloud has no normals");   // (the reference indexes an empty vector)
    return cloud_done(ctx, "cloud_orient_normals", cloud_device_orient_normals(cloud->dev, camera, ref, ctx->eng->aux_stream()));
}

int visma_icp_cloud_orient_normals_to_align_with_direction(visma_icp_ctx *ctx, visma_icp_cloud *cloud, const double ref[3])
{
    return cloud_orient(ctx, cloud, false, ref);
}

int visma_icp_cloud_orient_normals_towards_camera_location(visma_icp_ctx *ctx, visma_icp_cloud *cloud, const double camera[3])
{
    return cloud_orient(ctx, cloud, true, camera);
}

int visma_icp_cloud_mean_and_covariance(visma_icp_ctx *ctx, visma_icp_cloud *cloud, double mean[3], double cov[9])
{
    CLOUD_CHECK(cloud);
    if (!mean || !cov) return ctx->fail(VISMA_ICP_ERR_INVALID, "cloud_mean_and_covariance: NULL argument");
    return cloud_done(ctx, "cloud_mean_and_covariance",
                      cloud_device_mean_and_covariance(cloud->dev, kHostChunk, mean, cov, ctx->eng->aux_stream()));
}

// Eigen 3.3.2's inverse of a 3 x 3 matrix (LU/InverseImpl.h:126-169), row-major m -> r: the cofactors, the determinant as
// the sum of the first cofactor column times column 0, 1 / det, no invertibility test
static void inverse3_eigen(const double m[9], double r[9])
{
    const double c0 = m[4] * m[8] - m[5] * m[7];
    const double c1 = m[7] * m[2] - m[8] * m[1];
    const double c2 = m[1] * m[5] - m[2] * m[4];
    const double det = (c0 * m[0] + c1 * m[3]) + c2 * m[6];
    const double invdet = 1.0 / det;
    r[0] = c0 * invdet; r[1] = c1 * invdet; r[2] = c2 * invdet;
    r[3] = (m[5] * m[6] - m[3] * m[8]) * invdet;
    r[4] = (m[8] * m[0] - m[6] * m[2]) * invdet;
    r[5] = (m[2] * m[3] - m[0] * m[5]) * invdet;
    r[6] = (m[3] * m[7] - m[4] * m[6]) * invdet;
    r[7] = (m[6] * m[1] - m[7] * m[0]) * invdet;
    r[8] = (m[0] * m[4] - m[1] * m[3]) * invdet;
}

int visma_icp_cloud_mahalanobis_distance(visma_icp_ctx *ctx, visma_icp_cloud *cloud, double *out)
{
    CLOUD_CHECK(cloud);
    int64_t rows = 0;
    int f = 0;
    cloud_device_size(cloud->dev, &rows, &f);
    if (rows > 0 && !out) return ctx->fail(VISMA_ICP_ERR_INVALID, "cloud_mahalanobis_distance: NULL argument");
    double mean[3], cov[9], inv[9];
    hipError_t e = cloud_device_mean_and_covariance(cloud->dev, kHostChunk, mean, cov, ctx->eng->aux_stream());
    if (e != hipSuccess) return cloud_done(ctx, "cloud_mahalanobis_distance", e);
    inverse3_eigen(cov, inv);
    return cloud_done(ctx, "cloud_mahalanobis_distance", cloud_device_mahalanobis(cloud->dev, mean, inv, out, ctx->eng->aux_stream()));
}

// ---- Image: an image resident on the device (image.hip) ----
static int image_enter(visma_icp_ctx *ctx, const visma_icp_image *img)
{
    if (img && !ctx->owns(img)) return ctx->fail(VISMA_ICP_ERR_INVALID, "not an image of this context");
    if (ctx->sharded() || ctx->eng->is_sharded()) return ctx->fail(VISMA_ICP_ERR_INVALID, "an image lives on one rank");
    if (!ctx->eng->supports_device_loop()) return ctx->fail(VISMA_ICP_ERR_STATE, "an image needs the HIP engine");
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    return VISMA_ICP_OK;
}

static int image_done(visma_icp_ctx *ctx, const char *what, hipError_t e)
{
    if (e == hipSuccess) return VISMA_ICP_OK;
    (void)hipGetLastError();
    return ctx->fail(VISMA_ICP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

static int image_adopt(visma_icp_ctx *ctx, const char *what, hipError_t e, ImageDevice *dev, visma_icp_image **out)
{
    if (e != hipSuccess) return image_done(ctx, what, e);
    *out = ctx->adopt(dev);
    return VISMA_ICP_OK;
}

#define IMAGE_CHECK(img)                                                                     \
    CTX_CHECK();                                                                             \
    if (!(img)) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL image");                      \
    if (int rc_ = image_enter(ctx, (img))) return rc_;

// an operation that makes a new image: the checks before it
#define IMAGE_NEW_CHECK(img)                                                                 \
    CTX_CHECK();                                                                             \
    if (!out) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");                       \
    *out = nullptr;                                                                          \
    if (!(img)) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL image");                      \
    if (int rc_ = image_enter(ctx, (img))) return rc_;

static bool image_is_float(const visma_icp_image *img)
{
    int w, h, ch, bpc;
    image_device_info(img->dev, &w, &h, &ch, &bpc);
    return ch == 1 && bpc == 4 && !image_device_is_integer(img->dev);
}

int visma_icp_image_create(visma_icp_ctx *ctx, int w, int h, int channels, int bytes_per_channel, const void *data, visma_icp_image **out)
{
    CTX_CHECK();
    if (!out) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    *out = nullptr;
    if (w < 0 || h < 0 || (int64_t)w * h > (int64_t)1 << 30) return ctx->fail(VISMA_ICP_ERR_INVALID, "image_create: 0 <= w, h and at most 2^30 pixels");
    if (channels < 1 || channels > 4) return ctx->fail(VISMA_ICP_ERR_INVALID, "image_create: 1 .. 4 channels");
    if (bytes_per_channel != 1 && bytes_per_channel != 2 && bytes_per_channel != 4)
        return ctx->fail(VISMA_ICP_ERR_INVALID, "image_create: 1, 2 or 4 bytes per channel");
    if ((int64_t)w * h > 0 && !data) return ctx->fail(VISMA_ICP_ERR_INVALID, "image_create: NULL argument");
    if (int rc = image_enter(ctx, nullptr)) return rc;
    ImageDevice *dev = nullptr;
    const hipError_t e = image_device_create(w, h, channels, bytes_per_channel, data, false, ctx->eng->aux_stream(), &dev);
    return image_adopt(ctx, "image_create", e, dev, out);
}

int visma_icp_image_destroy(visma_icp_ctx *ctx, visma_icp_image *img)
{
    CTX_CHECK();
    if (!img) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL image");
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    for (size_t i = 0; i < ctx->images.size(); i++)
        if (ctx->images[i].get() == img) { ctx->images.erase(ctx->images.begin() + (std::ptrdiff_t)i); return VISMA_ICP_OK; }
    return ctx->fail(VISMA_ICP_ERR_INVALID, "not an image of this context");
}

int visma_icp_image_info(const visma_icp_image *img, int *w, int *h, int *channels, int *bytes_per_channel)
{
    if (!img || !img->dev) { g_create_error = "image is NULL"; return VISMA_ICP_ERR_INVALID; }
    int v[4];
    image_device_info(img->dev, &v[0], &v[1], &v[2], &v[3]);
    if (w) *w = v[0];
    if (h) *h = v[1];
    if (channels) *channels = v[2];
    if (bytes_per_channel) *bytes_per_channel = v[3];
    return VISMA_ICP_OK;
}

int visma_icp_image_get(visma_icp_ctx *ctx, visma_icp_image *img, void *bytes, int64_t n_bytes)
{
    IMAGE_CHECK(img);
    int w, h, ch, bpc;
    image_device_info(img->dev, &w, &h, &ch, &bpc);
    const int64_t have = (int64_t)w * h * ch * bpc;
    if (n_bytes != have) return ctx->fail(VISMA_ICP_ERR_INVALID, "image_get: n_bytes differs from the image's size");
    if (have > 0 && !bytes) return ctx->fail(VISMA_ICP_ERR_INVALID, "image_get: NULL argument");
    return image_done(ctx, "image_get", image_device_get(img->dev, bytes, ctx->eng->aux_stream()));
}

int visma_icp_image_copy(visma_icp_ctx *ctx, visma_icp_image *img, visma_icp_image **out)
{
    IMAGE_NEW_CHECK(img);
    ImageDevice *dev = nullptr;
    return image_adopt(ctx, "image_copy", image_device_copy(img->dev, ctx->eng->aux_stream(), &dev), dev, out);
}

int visma_icp_image_to_float(visma_icp_ctx *ctx, visma_icp_image *img, int type, visma_icp_image **out)
{
    IMAGE_NEW_CHECK(img);
    if (type != VISMA_ICP_IMAGE_EQUAL && type != VISMA_ICP_IMAGE_WEIGHTED) return ctx->fail(VISMA_ICP_ERR_INVALID, "image_to_float: unknown conversion type");
    ImageDevice *dev = nullptr;
    const hipError_t e = image_device_to_float(img->dev, type == VISMA_ICP_IMAGE_WEIGHTED, ctx->eng->aux_stream(), &dev);
    return image_adopt(ctx, "image_to_float", e, dev, out);
}

int visma_icp_image_depth_to_float(visma_icp_ctx *ctx, visma_icp_image *img, double depth_scale, double depth_trunc, visma_icp_image **out)
{
    IMAGE_NEW_CHECK(img);
    ImageDevice *dev = nullptr;
    const hipError_t e = image_device_depth_to_float(img->dev, depth_scale, depth_trunc, ctx->eng->aux_stream(), &dev);
    return image_adopt(ctx, "image_depth_to_float", e, dev, out);
}

int visma_icp_image_from_float(visma_icp_ctx *ctx, visma_icp_image *img, int bytes, visma_icp_image **out)
{
    IMAGE_NEW_CHECK(img);
    if (bytes != 1 && bytes != 2) return ctx->fail(VISMA_ICP_ERR_INVALID, "image_from_float: 1 or 2 bytes");
    ImageDevice *dev = nullptr;
    return image_adopt(ctx, "image_from_float", image_device_from_float(img->dev, bytes, ctx->eng->aux_stream(), &dev), dev, out);
}

// Image.cpp:32-37
static bool image_filter_kernels(int type, const double **dx, const double **dy, int *n)
{
    static const double g3[3] = {0.25, 0.5, 0.25}, g5[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
    static const double g7[7] = {0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125};
    static const double s31[3] = {-1.0, 0.0, 1.0}, s32[3] = {1.0, 2.0, 1.0};
    switch (type) {
    case VISMA_ICP_IMAGE_GAUSSIAN3: *dx = g3; *dy = g3; *n = 3; return true;
    case VISMA_ICP_IMAGE_GAUSSIAN5: *dx = g5; *dy = g5; *n = 5; return true;
    case VISMA_ICP_IMAGE_GAUSSIAN7: *dx = g7; *dy = g7; *n = 7; return true;
    case VISMA_ICP_IMAGE_SOBEL3DX: *dx = s31; *dy = s32; *n = 3; return true;
    case VISMA_ICP_IMAGE_SOBEL3DY: *dx = s32; *dy = s31; *n = 3; return true;
    default: return false;
    }
}

int visma_icp_image_filter(visma_icp_ctx *ctx, visma_icp_image *img, int type, visma_icp_image **out)
{
    IMAGE_NEW_CHECK(img);
    const double *dx = nullptr, *dy = nullptr;
    int n = 0;
    if (!image_filter_kernels(type, &dx, &dy, &n)) return ctx->fail(VISMA_ICP_ERR_INVALID, "image_filter: unknown filter type");
    ImageDevice *dev = nullptr;
    const hipError_t e = image_device_filter_separable(img->dev, ctx->image_scratch(), dx, n, dy, n, ctx->eng->aux_stream(), &dev);
    return image_adopt(ctx, "image_filter", e, dev, out);
}

int visma_icp_image_filter_separable(visma_icp_ctx *ctx, visma_icp_image *img, const double *dx, int n_dx, const double *dy, int n_dy,
                                     visma_icp_image **out)
{
    IMAGE_NEW_CHECK(img);
    if (n_dx < 0 || n_dy < 0 || (n_dx > 0 && !dx) || (n_dy > 0 && !dy)) return ctx->fail(VISMA_ICP_ERR_INVALID, "image_filter_separable: bad kernel arguments");
    ImageDevice *dev = nullptr;
    const hipError_t e = image_device_filter_separable(img->dev, ctx->image_scratch(), dx, n_dx, dy, n_dy, ctx->eng->aux_stream(), &dev);
    return image_adopt(ctx, "image_filter_separable", e, dev, out);
}

int visma_icp_image_filter_horizontal(visma_icp_ctx *ctx, visma_icp_image *img, const double *kernel, int n, visma_icp_image **out)
{
    IMAGE_NEW_CHECK(img);
    if (n < 0 || (n > 0 && !kernel)) return ctx->fail(VISMA_ICP_ERR_INVALID, "image_filter_horizontal: bad kernel arguments");
    ImageDevice *dev = nullptr;
    const hipError_t e = image_device_filter_horizontal(img->dev, ctx->image_scratch(), kernel, n, ctx->eng->aux_stream(), &dev);
    return image_adopt(ctx, "image_filter_horizontal", e, dev, out);
}

int visma_icp_image_flip(visma_icp_ctx *ctx, visma_icp_image *img, visma_icp_image **out)
{
    IMAGE_NEW_CHECK(img);
    ImageDevice *dev = nullptr;
    return image_adopt(ctx, "image_flip", image_device_flip(img->dev, ctx->eng->aux_stream(), &dev), dev, out);
}

int visma_icp_image_downsample(visma_icp_ctx *ctx, visma_icp_image *img, visma_icp_image **out)
{
    IMAGE_NEW_CHECK(img);
    ImageDevice *dev = nullptr;
    return image_adopt(ctx, "image_downsample", image_device_downsample(img->dev, ctx->eng->aux_stream(), &dev), dev, out);
}

int visma_icp_image_dilate(visma_icp_ctx *ctx, visma_icp_image *img, int half_kernel_size, visma_icp_image **out)
{
    IMAGE_NEW_CHECK(img);
    ImageDevice *dev = nullptr;
    return image_adopt(ctx, "image_dilate", image_device_dilate(img->dev, ctx->image_scratch(), half_kernel_size, ctx->eng->aux_stream(), &dev), dev, out);
}

int visma_icp_image_linear_transform(visma_icp_ctx *ctx, visma_icp_image *img, double scale, double offset)
{
    IMAGE_CHECK(img);
    return image_done(ctx, "image_linear_transform", image_device_linear_transform(img->dev, scale, offset, ctx->eng->aux_stream()));
}

int visma_icp_image_clip_intensity(visma_icp_ctx *ctx, visma_icp_image *img, double min, double max)
{
    IMAGE_CHECK(img);
    return image_done(ctx, "image_clip_intensity", image_device_clip_intensity(img->dev, min, max, ctx->eng->aux_stream()));
}

// the levels made so far are destroyed where a later one fails
static int image_drop_levels(visma_icp_ctx *ctx, visma_icp_image **out, int levels, int rc)
{
    for (int l = 0; l < levels; l++)
        if (out[l]) { visma_icp_image_destroy(ctx, out[l]); out[l] = nullptr; }
    return rc;
}

// ImageFactory.cpp:150-182
int visma_icp_image_pyramid(visma_icp_ctx *ctx, visma_icp_image *img, int levels, int with_gaussian_filter, visma_icp_image **out)
{
    CTX_CHECK();
    if (levels < 0 || (levels > 0 && !out)) return ctx->fail(VISMA_ICP_ERR_INVALID, "image_pyramid: bad arguments");
    for (int l = 0; l < levels; l++) out[l] = nullptr;
    if (!img) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL image");
    if (int rc = image_enter(ctx, img)) return rc;
    if (!image_is_float(img)) return VISMA_ICP_OK;           // no levels
    for (int l = 0; l < levels; l++) {
        int rc;
        if (l == 0) {
            rc = visma_icp_image_copy(ctx, img, &out[0]);
        } else if (with_gaussian_filter) {
            visma_icp_image *blurred = nullptr;
            rc = visma_icp_image_filter(ctx, out[l - 1], VISMA_ICP_IMAGE_GAUSSIAN3, &blurred);
            if (!rc) {
                rc = visma_icp_image_downsample(ctx, blurred, &out[l]);
                const std::string err = ctx->err;
                visma_icp_image_destroy(ctx, blurred);
                if (rc) ctx->err = err;
            }
        } else {
            rc = visma_icp_image_downsample(ctx, out[l - 1], &out[l]);
        }
        if (rc) return image_drop_levels(ctx, out, levels, rc);
    }
    return VISMA_ICP_OK;
}

// Image.cpp:259-268
int visma_icp_image_filter_pyramid(visma_icp_ctx *ctx, visma_icp_image *const *in, int levels, int type, visma_icp_image **out)
{
    CTX_CHECK();
    if (levels < 0 || (levels > 0 && (!in || !out))) return ctx->fail(VISMA_ICP_ERR_INVALID, "image_filter_pyramid: bad arguments");
    for (int l = 0; l < levels; l++) out[l] = nullptr;
    for (int l = 0; l < levels; l++)
        if (int rc = visma_icp_image_filter(ctx, in[l], type, &out[l])) return image_drop_levels(ctx, out, levels, rc);
    return VISMA_ICP_OK;
}

int visma_icp_image_distance_multiplier(visma_icp_ctx *ctx, const double intrinsic[4], int w, int h, visma_icp_image **out)
{
    CTX_CHECK();
    if (!out) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    *out = nullptr;
    if (!intrinsic) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL argument");
    if (w < 0 || h < 0 || (int64_t)w * h > (int64_t)1 << 30) return ctx->fail(VISMA_ICP_ERR_INVALID, "image_distance_multiplier: 0 <= w, h and at most 2^30 pixels");
    if (int rc = image_enter(ctx, nullptr)) return rc;
    ImageDevice *dev = nullptr;
    return image_adopt(ctx, "image_distance_multiplier", image_device_distance_multiplier(w, h, intrinsic, ctx->eng->aux_stream(), &dev), dev, out);
}

int visma_icp_image_float_value_at(visma_icp_ctx *ctx, visma_icp_image *img, const double *uv, int64_t n, uint8_t *ok, double *value)
{
    IMAGE_CHECK(img);
    if (n < 0 || n > 0x7fffffff || (n > 0 && (!uv || !ok || !value))) return ctx->fail(VISMA_ICP_ERR_INVALID, "image_float_value_at: bad arguments");
    return image_done(ctx, "image_float_value_at", image_device_float_value_at(img->dev, uv, n, ok, value, ctx->eng->aux_stream()));
}

// RGBDImageFactory.cpp
int visma_icp_image_rgbd(visma_icp_ctx *ctx, visma_icp_image *color, visma_icp_image *depth, int format, double depth_scale, double depth_trunc,
                         int convert_rgb_to_intensity, visma_icp_image **out_color, visma_icp_image **out_depth)
{
    CTX_CHECK();
    if (!out_color || !out_depth) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL output");
    *out_color = *out_depth = nullptr;
    if (!color || !depth) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL image");
    if (format < VISMA_ICP_RGBD_COLOR_AND_DEPTH || format > VISMA_ICP_RGBD_NYU) return ctx->fail(VISMA_ICP_ERR_INVALID, "image_rgbd: unknown format");
    if (int rc = image_enter(ctx, color)) return rc;
    if (int rc = image_enter(ctx, depth)) return rc;
    int cw, chh, cch, cb, dw, dh, dch, db;
    image_device_info(color->dev, &cw, &chh, &cch, &cb);
    image_device_info(depth->dev, &dw, &dh, &dch, &db);
    if (cw != dw || chh != dh) return VISMA_ICP_OK;          // the reference's empty RGBDImage
    const bool decode = format == VISMA_ICP_RGBD_SUN || format == VISMA_ICP_RGBD_NYU;
    if (decode && (dch != 1 || db != 2)) return ctx->fail(VISMA_ICP_ERR_INVALID, "image_rgbd: a SUN or NYU depth is a 1 x uint16 image");
    switch (format) {
    case VISMA_ICP_RGBD_REDWOOD: depth_scale = 1000.0; depth_trunc = 4.0; break;
    case VISMA_ICP_RGBD_TUM: depth_scale = 5000.0; depth_trunc = 4.0; break;
    case VISMA_ICP_RGBD_SUN: case VISMA_ICP_RGBD_NYU: depth_scale = 1000.0; depth_trunc = 7.0; break;
    default: break;
    }
    hipStream_t s = ctx->eng->aux_stream();
    ImageDevice *decoded = nullptr, *d = nullptr, *c = nullptr;
    hipError_t e = hipSuccess;
    if (decode) e = image_device_decode_depth(depth->dev, format == VISMA_ICP_RGBD_NYU, s, &decoded);
    if (e == hipSuccess) e = image_device_depth_to_float(decoded ? decoded : depth->dev, depth_scale, depth_trunc, s, &d);
    image_device_destroy(decoded);
    if (e == hipSuccess) e = convert_rgb_to_intensity ? image_device_to_float(color->dev, 1, s, &c) : image_device_copy(color->dev, s, &c);
    if (e != hipSuccess) { image_device_destroy(d); image_device_destroy(c); return image_done(ctx, "image_rgbd", e); }
    *out_depth = ctx->adopt(d);
    *out_color = ctx->adopt(c);
    return VISMA_ICP_OK;
}

// ---- FPFH, feature matching, fast global registration ----

int visma_icp_compute_fpfh_probe(visma_icp_ctx *ctx, const double *xyz, int64_t n, const double *normals, int search_type,
                                 int knn, double radius, double *out, int second_pass, double ms[3])
{
    CTX_CHECK();
    if (n < 0 || (n > 0 && (!xyz || !normals || !out)) || second_pass < 0 || second_pass > 2)
        return ctx->fail(VISMA_ICP_ERR_INVALID, "bad compute_fpfh arguments");
    if (search_type != 0 && search_type != 2)
        return ctx->fail(VISMA_ICP_ERR_INVALID, "compute_fpfh: search_type must be 0 (KNN) or 2 (Hybrid)");
    if (knn < 2 || knn > kNormalsMaxList) return ctx->fail(VISMA_ICP_ERR_INVALID, "compute_fpfh: knn must lie in [2, 170]");
    if (n > 0x7fffffff) return ctx->fail(VISMA_ICP_ERR_INVALID, "too many points for 32-bit indices");
    if (!ctx->eng->supports_device_loop()) return ctx->fail(VISMA_ICP_ERR_STATE, "compute_fpfh needs the HIP engine");
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    hipError_t e = compute_fpfh_device(xyz, n, normals, search_type, knn, radius, out, second_pass, ms, ctx->eng->aux_stream());
    if (e != hipSuccess) return ctx->fail(e == hipErrorInvalidValue ? VISMA_ICP_ERR_INVALID : VISMA_ICP_ERR_HIP,
                                          std::string("compute_fpfh: ") + hipGetErrorString(e));
    return VISMA_ICP_OK;
}

int visma_icp_compute_fpfh(visma_icp_ctx *ctx, const double *xyz, int64_t n, const double *normals, int search_type, int knn,
                           double radius, double *out)
{
    return visma_icp_compute_fpfh_probe(ctx, xyz, n, normals, search_type, knn, radius, out, 0, nullptr);
}

int visma_icp_match_features_probe(visma_icp_ctx *ctx, const double *fa, int64_t na, const double *fb, int64_t nb, int dim,
                                   int32_t *nn_of_b, double *d2_of_b, double *kernel_ms)
{
    CTX_CHECK();
    if (dim < 1 || dim > 64) return ctx->fail(VISMA_ICP_ERR_INVALID, "match_features: dim must lie in [1, 64]");
    if (na < 0 || nb < 0 || (na > 0 && !fa) || (nb > 0 && (!fb || !nn_of_b)))
        return ctx->fail(VISMA_ICP_ERR_INVALID, "bad match_features arguments");
    if (na > 0x7fffffff || nb > 0x7fffffff) return ctx->fail(VISMA_ICP_ERR_INVALID, "too many rows for 32-bit indices");
    if (kernel_ms) *kernel_ms = 0.0;
    if (nb == 0) return VISMA_ICP_OK;
    if (!ctx->eng->supports_device_loop()) return ctx->fail(VISMA_ICP_ERR_STATE, "match_features needs the HIP engine");
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    hipError_t e = match_features_device(fa, na, fb, nb, dim, nn_of_b, d2_of_b, kernel_ms, ctx->eng->aux_stream());
    if (e != hipSuccess) return ctx->fail(e == hipErrorInvalidValue ? VISMA_ICP_ERR_INVALID : VISMA_ICP_ERR_HIP,
                                          std::string("match_features: ") + hipGetErrorString(e));
    return VISMA_ICP_OK;
}

int visma_icp_match_features(visma_icp_ctx *ctx, const double *fa, int64_t na, const double *fb, int64_t nb, int dim,
                             int32_t *nn_of_b, double *d2_of_b)
{
    return visma_icp_match_features_probe(ctx, fa, na, fb, nb, dim, nn_of_b, d2_of_b, nullptr);
}

static FgrOption fgr_option_of(const visma_icp_fgr_option *opt)
{
    FgrOption o;
    if (opt) {
        o.division_factor = opt->division_factor; o.max_corr_dist = opt->max_corr_dist; o.tuple_scale = opt->tuple_scale;
        o.use_absolute_scale = opt->use_absolute_scale; o.decrease_mu = opt->decrease_mu;
        o.iteration_number = opt->iteration_number; o.maximum_tuple_count = opt->maximum_tuple_count;
    }
    return o;
}

// steps 0-3 of AdvancedMatching on the normalized clouds; pairs (source index, target index)
static int fgr_correspondences_impl(visma_icp_ctx *ctx, const double *src_xyz, int64_t ns, const double *src_fpfh,
                                    const double *tgt_xyz, int64_t nt, const double *tgt_fpfh, const FgrOption &o, uint64_t seed,
                                    const int32_t *triples, int64_t n_triples, std::vector<int32_t> &oi, std::vector<int32_t> &oj,
                                    visma_icp_fgr_info *info)
{
    const FgrNormalized N = fgr_normalize(src_xyz, ns, tgt_xyz, nt, o.use_absolute_scale != 0);
    const bool swapped = nt > ns;                                 // i is the larger cloud (:51-58)
    const int fi = swapped ? 1 : 0, fj = swapped ? 0 : 1;
    const double *feat[2] = {src_fpfh, tgt_fpfh};
    const int64_t cnt[2] = {ns, nt};
    std::vector<int32_t> nn_i_of_j((size_t)cnt[fj]), nn_j_of_i((size_t)cnt[fi]);
    if (int rc = visma_icp_match_features(ctx, feat[fi], cnt[fi], feat[fj], cnt[fj], VISMA_FPFH_DIM, nn_i_of_j.data(), nullptr)) return rc;
    if (int rc = visma_icp_match_features(ctx, feat[fj], cnt[fj], feat[fi], cnt[fi], VISMA_FPFH_DIM, nn_j_of_i.data(), nullptr)) return rc;
    std::vector<int32_t> ci, cj, ti, tj;
    fgr_cross_check(nn_i_of_j.data(), cnt[fj], nn_j_of_i.data(), cnt[fi], ci, cj);
    const int64_t trials = fgr_tuple_test(N.xyz[fi].data(), N.xyz[fj].data(), ci, cj, o.tuple_scale, o.maximum_tuple_count, seed,
                                          triples, n_triples, ti, tj);
    if (swapped) ti.swap(tj);
    oi.swap(ti); oj.swap(tj);
    if (info) {
        info->n_mutual = (int64_t)ci.size();
        info->n_tuple_corres = (int64_t)oi.size();
        info->n_trials = trials;
    }
    return VISMA_ICP_OK;
}

int visma_icp_fgr_correspondences(visma_icp_ctx *ctx, const double *src_xyz, int64_t ns, const double *src_fpfh,
                                  const double *tgt_xyz, int64_t nt, const double *tgt_fpfh, const visma_icp_fgr_option *opt,
                                  uint64_t seed, const int32_t *triples, int64_t n_triples, int32_t *src_idx, int32_t *tgt_idx,
                                  int64_t capacity, int64_t *n_out, visma_icp_fgr_info *info)
{
    CTX_CHECK();
    if (ns <= 0 || nt <= 0 || !src_xyz || !tgt_xyz || !src_fpfh || !tgt_fpfh || !n_out || capacity < 0 ||
        (capacity > 0 && (!src_idx || !tgt_idx)) || n_triples < 0 || (n_triples > 0 && !triples))
        return ctx->fail(VISMA_ICP_ERR_INVALID, "bad fgr_correspondences arguments");
    if (ns > 0x7fffffff || nt > 0x7fffffff) return ctx->fail(VISMA_ICP_ERR_INVALID, "too many points for 32-bit indices");
    std::vector<int32_t> oi, oj;
    if (int rc = fgr_correspondences_impl(ctx, src_xyz, ns, src_fpfh, tgt_xyz, nt, tgt_fpfh, fgr_option_of(opt), seed,
                                          n_triples > 0 ? triples : nullptr, n_triples, oi, oj, info))
        return rc;
    if ((int64_t)oi.size() > capacity) return ctx->fail(VISMA_ICP_ERR_INVALID, "fgr_correspondences: the index buffers are too small");
    std::copy(oi.begin(), oi.end(), src_idx);
    std::copy(oj.begin(), oj.end(), tgt_idx);
    *n_out = (int64_t)oi.size();
    return VISMA_ICP_OK;
}

int visma_icp_fgr_optimize(const double *src_xyz, int64_t ns, const double *tgt_xyz, int64_t nt, const int32_t *src_idx,
                           const int32_t *tgt_idx, int64_t k, const visma_icp_fgr_option *opt, double out_T[16],
                           double out_T_opt[16])
{
    if (ns <= 0 || nt <= 0 || !src_xyz || !tgt_xyz || k < 0 || (k > 0 && (!src_idx || !tgt_idx)) || !out_T)
        return VISMA_ICP_ERR_INVALID;
    for (int64_t c = 0; c < k; c++)
        if (src_idx[c] < 0 || src_idx[c] >= ns || tgt_idx[c] < 0 || tgt_idx[c] >= nt) return VISMA_ICP_ERR_INVALID;
    const FgrOption o = fgr_option_of(opt);
    const FgrNormalized N = fgr_normalize(src_xyz, ns, tgt_xyz, nt, o.use_absolute_scale != 0);
    const Mat4 t = fgr_optimize(N.xyz[0].data(), N.xyz[1].data(), src_idx, tgt_idx, k, o, N.scale_global);
    const Mat4 T = fgr_map_back(t, N);
    memcpy(out_T, T.m, sizeof(T.m));
    if (out_T_opt) memcpy(out_T_opt, t.m, sizeof(t.m));
    return VISMA_ICP_OK;
}

int visma_icp_fast_global_registration(visma_icp_ctx *ctx, const double *src_xyz, int64_t ns, const double *src_fpfh,
                                       const double *tgt_xyz, int64_t nt, const double *tgt_fpfh, const visma_icp_fgr_option *opt,
                                       uint64_t seed, const int32_t *triples, int64_t n_triples, double out_T[16],
                                       visma_icp_fgr_info *info)
{
    CTX_CHECK();
    if (ns <= 0 || nt <= 0 || !src_xyz || !tgt_xyz || !src_fpfh || !tgt_fpfh || !out_T || n_triples < 0 ||
        (n_triples > 0 && !triples))
        return ctx->fail(VISMA_ICP_ERR_INVALID, "bad fast_global_registration arguments");
    if (ns > 0x7fffffff || nt > 0x7fffffff) return ctx->fail(VISMA_ICP_ERR_INVALID, "too many points for 32-bit indices");
    std::vector<int32_t> oi, oj;
    if (int rc = fgr_correspondences_impl(ctx, src_xyz, ns, src_fpfh, tgt_xyz, nt, tgt_fpfh, fgr_option_of(opt), seed,
                                          n_triples > 0 ? triples : nullptr, n_triples, oi, oj, info))
        return rc;
    if (visma_icp_fgr_optimize(src_xyz, ns, tgt_xyz, nt, oi.data(), oj.data(), (int64_t)oi.size(), opt, out_T, nullptr))
        return ctx->fail(VISMA_ICP_ERR_INVALID, "fast_global_registration: optimize rejected its pairs");
    return VISMA_ICP_OK;
}

// ---- RANSAC global registration (include/visma_icp.h; trial arithmetic: ransac.hpp; kernels: ransac.hip) ----

static const visma_icp_ransac_option kRansacDefaults = {4, 1000, 1000, 0.0, 0.0, 0.0, 0};
constexpr int64_t kRansacChunk = 1 << 19;             // trials per launch: 48 MB of T slots

// the arguments every entry point shares; NULL: fine, else the message
static const char *ransac_check(const double *src, int64_t ns, const double *tgt, int64_t nt, const double *sn, const double *tn,
                                const visma_icp_ransac_option &o, const int32_t *draws, int64_t n_draw_trials)
{
    if (ns <= 0 || nt <= 0 || !src || !tgt) return "ransac: an empty cloud";
    if (ns > 0x7fffffff || nt > 0x7fffffff) return "too many points for 32-bit indices";
    if ((sn == nullptr) != (tn == nullptr)) return "ransac: normals for both clouds or for none";
    if (o.ransac_n < kRansacMinN || o.ransac_n > kRansacMaxN) return "ransac: ransac_n must lie in [3, 8]";
    if (o.chunk_trials < 0 || o.chunk_trials > (1 << 22)) return "ransac: chunk_trials must lie in [0, 4194304]";
    if (n_draw_trials < 0 || (n_draw_trials > 0 && !draws)) return "ransac: bad draws";
    return nullptr;
}

static RansacProblem ransac_problem(const double *src, int64_t ns, const double *tgt, int64_t nt, const double *sn, const double *tn,
                                    const int32_t *pair_src, const int32_t *pair_tgt, int64_t n_pairs,
                                    const visma_icp_ransac_option &o, uint64_t seed, const int32_t *draws, int64_t n_draw_trials)
{
    RansacProblem p;
    p.src = src; p.ns = ns; p.tgt = tgt; p.nt = nt; p.src_n = sn; p.tgt_n = tn;
    p.pair_src = pair_src; p.pair_tgt = pair_tgt; p.n_pairs = n_pairs;
    p.draws = draws; p.n_draw_trials = draws ? n_draw_trials : 0;
    p.seed = seed; p.ransac_n = o.ransac_n;
    p.use_edge = o.edge_length_similarity > 0.0; p.edge = o.edge_length_similarity;
    p.use_dist = o.distance_threshold > 0.0; p.dist = o.distance_threshold;
    p.use_normal = o.normal_angle > 0.0; p.cos_normal = std::cos(o.normal_angle);
    return p;
}

static RansacView ransac_host_view(const RansacProblem &p)
{
    RansacView v;
    v.src = p.src; v.tgt = p.tgt; v.src_n = p.src_n; v.tgt_n = p.tgt_n;
    v.pair_src = p.pair_src; v.pair_tgt = p.pair_tgt; v.n_pairs = p.n_pairs;
    v.draws = p.draws; v.seed = p.seed;
    v.edge = p.edge; v.dist = p.dist; v.cos_normal = p.cos_normal;
    v.use_edge = p.use_edge; v.use_dist = p.use_dist; v.use_normal = p.use_normal;
    return v;
}

static int ransac_trial_host(const RansacView &v, int n, long long t, double T[12])
{
    switch (n) {
    case 3: return ransac_trial<3>(v, t, T);
    case 4: return ransac_trial<4>(v, t, T);
    case 5: return ransac_trial<5>(v, t, T);
    case 6: return ransac_trial<6>(v, t, T);
    case 7: return ransac_trial<7>(v, t, T);
    default: return ransac_trial<8>(v, t, T);
    }
}

static const char *ransac_check_hypotheses(const double *src, int64_t ns, const double *tgt, int64_t nt, const double *sn,
                                           const double *tn, const int32_t *pair_src, const int32_t *pair_tgt, int64_t n_pairs,
                                           const visma_icp_ransac_option &o, const int32_t *draws, int64_t first_trial,
                                           int64_t n_trials, const int8_t *verdict_out, const double *T_out)
{
    if (const char *m = ransac_check(src, ns, tgt, nt, sn, tn, o, draws, 0)) return m;
    if (!pair_tgt || n_pairs <= 0 || n_pairs > 0x7fffffff || (!pair_src && n_pairs != ns)) return "ransac_hypotheses: bad pair table";
    if (first_trial < 0 || n_trials < 0 || (n_trials > 0 && (!verdict_out || !T_out))) return "bad ransac_hypotheses arguments";
    for (int64_t k = 0; k < n_pairs; k++)
        if (pair_tgt[k] < -1 || pair_tgt[k] >= nt || (pair_src && (pair_src[k] < 0 || pair_src[k] >= ns)))
            return "ransac_hypotheses: a pair outside its cloud";
    return nullptr;
}

int visma_icp_ransac_hypotheses_host(const double *src, int64_t ns, const double *tgt, int64_t nt, const double *sn, const double *tn,
                                     const int32_t *pair_src, const int32_t *pair_tgt, int64_t n_pairs,
                                     const visma_icp_ransac_option *opt, uint64_t seed, const int32_t *draws, int64_t first_trial,
                                     int64_t n_trials, int8_t *verdict_out, double *T_out)
{
    const visma_icp_ransac_option o = opt ? *opt : kRansacDefaults;
    if (ransac_check_hypotheses(src, ns, tgt, nt, sn, tn, pair_src, pair_tgt, n_pairs, o, draws, first_trial, n_trials, verdict_out, T_out))
        return VISMA_ICP_ERR_INVALID;
    const RansacView v = ransac_host_view(ransac_problem(src, ns, tgt, nt, sn, tn, pair_src, pair_tgt, n_pairs, o, seed, draws,
                                                         first_trial + n_trials));
    parallel_for(n_trials, 256, [&](int64_t i) {
        double T[12];
        const int r = ransac_trial_host(v, o.ransac_n, first_trial + i, T);
        verdict_out[i] = (int8_t)r;
        double *out = T_out + 16 * i;
        for (int c = 0; c < 12; c++) out[c] = T[c];
        out[12] = out[13] = out[14] = 0.0;
        out[15] = r == kRansacBefore ? 0.0 : 1.0;
    });
    return VISMA_ICP_OK;
}

struct RansacDeviceHolder {
    RansacDevice *d = nullptr;
    ~RansacDeviceHolder() { ransac_device_destroy(d); }
};

int visma_icp_ransac_hypotheses(visma_icp_ctx *ctx, const double *src, int64_t ns, const double *tgt, int64_t nt, const double *sn,
                                const double *tn, const int32_t *pair_src, const int32_t *pair_tgt, int64_t n_pairs,
                                const visma_icp_ransac_option *opt, uint64_t seed, const int32_t *draws, int64_t first_trial,
                                int64_t n_trials, int8_t *verdict_out, double *T_out)
{
    CTX_CHECK();
    const visma_icp_ransac_option o = opt ? *opt : kRansacDefaults;
    if (const char *m = ransac_check_hypotheses(src, ns, tgt, nt, sn, tn, pair_src, pair_tgt, n_pairs, o, draws, first_trial, n_trials,
                                                verdict_out, T_out))
        return ctx->fail(VISMA_ICP_ERR_INVALID, m);
    if (n_trials == 0) return VISMA_ICP_OK;
    if (!ctx->eng->supports_device_loop()) return ctx->fail(VISMA_ICP_ERR_STATE, "ransac_hypotheses needs the HIP engine");
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    const int64_t chunk = std::min<int64_t>(o.chunk_trials > 0 ? o.chunk_trials : kRansacChunk, n_trials);
    RansacDeviceHolder H;
    hipError_t e = ransac_device_create(ransac_problem(src, ns, tgt, nt, sn, tn, pair_src, pair_tgt, n_pairs, o, seed, draws,
                                                       first_trial + n_trials), chunk, ctx->eng->aux_stream(), &H.d);
    for (int64_t t = 0; e == hipSuccess && t < n_trials; t += chunk)
        e = ransac_device_chunk(H.d, first_trial + t, std::min(chunk, n_trials - t),
                                verdict_out + t, T_out + 16 * t, nullptr, nullptr, nullptr);
    if (e != hipSuccess) return ctx->fail(e == hipErrorInvalidValue ? VISMA_ICP_ERR_INVALID : VISMA_ICP_ERR_HIP,
                                          std::string("ransac_hypotheses: ") + hipGetErrorString(e));
    return VISMA_ICP_OK;
}

int visma_icp_ransac_hypotheses_probe(visma_icp_ctx *ctx, const double *src, int64_t ns, const double *tgt, int64_t nt, const double *sn,
                                      const double *tn, const int32_t *pair_src, const int32_t *pair_tgt, int64_t n_pairs,
                                      const visma_icp_ransac_option *opt, uint64_t seed, int64_t n_trials, int64_t counts[3], double *ms)
{
    CTX_CHECK();
    const visma_icp_ransac_option o = opt ? *opt : kRansacDefaults;
    int8_t none = 0;
    double noT = 0.0;
    if (const char *m = ransac_check_hypotheses(src, ns, tgt, nt, sn, tn, pair_src, pair_tgt, n_pairs, o, nullptr, 0, n_trials, &none, &noT))
        return ctx->fail(VISMA_ICP_ERR_INVALID, m);
    if (!counts || !ms || n_trials <= 0) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad ransac_hypotheses_probe arguments");
    if (!ctx->eng->supports_device_loop()) return ctx->fail(VISMA_ICP_ERR_STATE, "ransac_hypotheses_probe needs the HIP engine");
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    const int64_t chunk = std::min<int64_t>(o.chunk_trials > 0 ? o.chunk_trials : kRansacChunk, n_trials);
    RansacDeviceHolder H;
    hipError_t e = ransac_device_create(ransac_problem(src, ns, tgt, nt, sn, tn, pair_src, pair_tgt, n_pairs, o, seed, nullptr, 0), chunk,
                                        ctx->eng->aux_stream(), &H.d);
    std::vector<int8_t> verdict((size_t)chunk);
    counts[0] = counts[1] = counts[2] = 0;
    *ms = 0.0;
    for (int64_t t = 0; e == hipSuccess && t < n_trials; t += chunk) {
        const int64_t m = std::min(chunk, n_trials - t);
        e = ransac_device_chunk(H.d, t, m, verdict.data(), nullptr, nullptr, nullptr, ms);
        for (int64_t i = 0; e == hipSuccess && i < m; i++) {
            const int8_t r = verdict[(size_t)i];
            if (r < 0 || r > kRansacAfter) { e = hipErrorUnknown; break; }           // (no trial leaves another verdict)
            counts[r]++;
        }
    }
    if (e != hipSuccess) return ctx->fail(e == hipErrorInvalidValue ? VISMA_ICP_ERR_INVALID : VISMA_ICP_ERR_HIP,
                                          std::string("ransac_hypotheses_probe: ") + hipGetErrorString(e));
    return VISMA_ICP_OK;
}

static void ransac_empty_result(visma_icp_result *r)
{
    std::memset(r, 0, sizeof(*r));
    const Mat4 I = Mat4::identity();
    std::memcpy(r->transformation, I.m, sizeof(I.m));
}

static double ransac_now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The source as the searches see it: a point that is not finite (the trials read it as it is) is moved where no transform
// of this call can bring it within max_dist of the target.  Every T solved here maps the mean of its source sample onto
// the mean of its target sample and is rigid, so |T far - (a target point)| >= |far - (a source point)| - (target extent).
static const double *ransac_search_source(const double *src, int64_t ns, const double *tgt, int64_t nt, double max_dist,
                                          std::vector<double> &copy)
{
    bool clean = true;
    for (int64_t i = 0; clean && i < 3 * ns; i++) clean = std::isfinite(src[i]);
    if (clean) return src;
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, ext = 0.0;
    bool first = true;
    auto grow = [&](const double *p) {
        if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) return;
        for (int a = 0; a < 3; a++) {
            if (first || p[a] < lo[a]) lo[a] = p[a];
            if (first || p[a] > hi[a]) hi[a] = p[a];
        }
        first = false;
    };
    for (int64_t i = 0; i < ns; i++) grow(src + 3 * i);
    for (int64_t i = 0; i < nt; i++) grow(tgt + 3 * i);
    for (int a = 0; a < 3; a++) ext += hi[a] - lo[a];
    const double far = 1000.0 * (ext + max_dist);
    copy.assign(src, src + 3 * ns);
    for (int64_t i = 0; i < ns; i++) {
        double *p = &copy[(size_t)(3 * i)];
        if (std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2])) continue;
        for (int a = 0; a < 3; a++) p[a] = hi[a] + far;
    }
    return copy.data();
}

// EvaluateRegistration at every T (16 doubles each) through the batch path: one upload and one grid of the pair per
// sub-batch, the poses as its initial transforms, zero iterations.  A T that is not finite: zero correspondences.
static int ransac_validate(visma_icp_ctx *ctx, const double *src, int64_t ns, const double *tgt, int64_t nt, double max_dist,
                           const std::vector<double> &Ts, std::vector<visma_icp_result> &out)
{
    const int64_t n = (int64_t)(Ts.size() / 16);
    out.assign((size_t)n, visma_icp_result());
    std::vector<int64_t> finite;
    for (int64_t i = 0; i < n; i++) {
        bool ok = true;
        for (int c = 0; c < 16; c++) ok = ok && std::isfinite(Ts[(size_t)(16 * i + c)]);
        std::memset(&out[(size_t)i], 0, sizeof(visma_icp_result));
        std::memcpy(out[(size_t)i].transformation, &Ts[(size_t)(16 * i)], 16 * sizeof(double));
        if (ok) finite.push_back(i);
    }
    // (the split never changes a result: every problem of a batch is searched and reduced on its own)
    const int64_t per = std::max<int64_t>(1, std::min<int64_t>(64, (int64_t)(8 << 20) / std::max<int64_t>(ns, 1)));
    std::vector<visma_icp_problem> pb;
    std::vector<visma_icp_result> rs;
    for (size_t b = 0; b < finite.size(); b += (size_t)per) {
        const size_t m = std::min(finite.size() - b, (size_t)per);
        pb.assign(m, visma_icp_problem());
        rs.assign(m, visma_icp_result());
        for (size_t k = 0; k < m; k++) {
            pb[k].src_xyz = src; pb[k].ns = ns; pb[k].tgt_xyz = tgt; pb[k].nt = nt; pb[k].max_dist = max_dist;
            std::memcpy(pb[k].init, &Ts[(size_t)(16 * finite[b + k])], 16 * sizeof(double));
        }
        if (int rc = visma_icp_run_batch(ctx, pb.data(), (int)m, 0, 0.0, 0.0, VISMA_ICP_SOLVER_KABSCH, rs.data())) return rc;
        for (size_t k = 0; k < m; k++) out[(size_t)finite[b + k]] = rs[k];
    }
    return VISMA_ICP_OK;
}

// Registration.cpp:215-219 / :321-325 over the trials in order; -1: nobody beat the empty result
static int64_t ransac_best(const std::vector<double> &fitness, const std::vector<double> &rmse)
{
    int64_t best = -1;
    double bf = 0.0, br = 0.0;
    for (size_t i = 0; i < fitness.size(); i++)
        if (fitness[i] > bf || (fitness[i] == bf && rmse[i] < br)) { best = (int64_t)i; bf = fitness[i]; br = rmse[i]; }
    return best;
}

int visma_icp_registration_ransac_feature_matching(visma_icp_ctx *ctx, const double *src, int64_t ns, const double *src_feat,
                                                   const double *tgt, int64_t nt, const double *tgt_feat, int dim, const double *sn,
                                                   const double *tn, double max_dist, const visma_icp_ransac_option *opt,
                                                   uint64_t seed, const int32_t *draws, int64_t n_draw_trials,
                                                   visma_icp_result *result, visma_icp_ransac_info *info)
{
    CTX_CHECK();
    const visma_icp_ransac_option o = opt ? *opt : kRansacDefaults;
    if (const char *m = ransac_check(src, ns, tgt, nt, sn, tn, o, draws, n_draw_trials)) return ctx->fail(VISMA_ICP_ERR_INVALID, m);
    if (!src_feat || !tgt_feat || !result) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad registration_ransac_feature_matching arguments");
    if (dim < 1 || dim > 64) return ctx->fail(VISMA_ICP_ERR_INVALID, "registration_ransac_feature_matching: dim must lie in [1, 64]");
    if (!(max_dist > 0.0)) return ctx->fail(VISMA_ICP_ERR_INVALID, "registration_ransac_feature_matching: max_dist must be positive");
    if (!ctx->eng->supports_device_loop())
        return ctx->fail(VISMA_ICP_ERR_STATE, "registration_ransac_feature_matching needs the HIP engine");
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    ransac_empty_result(result);
    visma_icp_ransac_info I = {0, 0, 0, 0, -1, 0.0, 0.0};
    int64_t trials = std::max(o.max_iteration, 0);
    if (draws) trials = std::min(trials, n_draw_trials);
    const int64_t want = std::max(o.max_validation, 0);
    if (want == 0) trials = 0;
    std::vector<int64_t> pass_trial;
    std::vector<double> pass_T;
    if (trials > 0) {
        std::vector<int32_t> nn((size_t)ns);
        if (int rc = visma_icp_match_features(ctx, tgt_feat, nt, src_feat, ns, dim, nn.data(), nullptr)) return rc;
        const int64_t chunk = std::min<int64_t>(o.chunk_trials > 0 ? o.chunk_trials : kRansacChunk, trials);
        RansacDeviceHolder H;
        hipError_t e = ransac_device_create(ransac_problem(src, ns, tgt, nt, sn, tn, nullptr, nn.data(), ns, o, seed, draws, trials),
                                            chunk, ctx->eng->aux_stream(), &H.d);
        std::vector<int8_t> verdict((size_t)chunk);
        int64_t done = 0;
        while (e == hipSuccess && done < trials && (int64_t)pass_trial.size() < want) {
            const int64_t m = std::min(chunk, trials - done);
            e = ransac_device_chunk(H.d, done, m, verdict.data(), nullptr, &pass_trial, &pass_T, &I.hypothesis_ms);
            if (e != hipSuccess) break;
            // the serial loop stops with the trial that was validated last: count the chunk up to there
            int64_t upto = m;
            if ((int64_t)pass_trial.size() >= want) {
                pass_trial.resize((size_t)want);
                pass_T.resize((size_t)(16 * want));
                upto = pass_trial.back() + 1 - done;
            }
            for (int64_t i = 0; i < upto; i++) {
                I.n_rejected_before += verdict[(size_t)i] == kRansacBefore;
                I.n_rejected_after += verdict[(size_t)i] == kRansacAfter;
            }
            done += upto;
        }
        if (e != hipSuccess) return ctx->fail(e == hipErrorInvalidValue ? VISMA_ICP_ERR_INVALID : VISMA_ICP_ERR_HIP,
                                              std::string("registration_ransac_feature_matching: ") + hipGetErrorString(e));
        I.n_trials = done;
        I.n_validated = (int64_t)pass_trial.size();
    }
    if (!pass_trial.empty()) {
        const double t0 = ransac_now_ms();
        std::vector<double> copy;
        const double *ssrc = ransac_search_source(src, ns, tgt, nt, max_dist, copy);
        std::vector<visma_icp_result> rs;
        if (int rc = ransac_validate(ctx, ssrc, ns, tgt, nt, max_dist, pass_T, rs)) return rc;
        std::vector<double> fit(rs.size()), rmse(rs.size());
        for (size_t i = 0; i < rs.size(); i++) { fit[i] = rs[i].fitness; rmse[i] = rs[i].inlier_rmse; }
        const int64_t b = ransac_best(fit, rmse);
        I.validation_ms = ransac_now_ms() - t0;
        if (b >= 0) {
            I.best_trial = pass_trial[(size_t)b];
            if (int rc = visma_icp_set_clouds_f64(ctx, ssrc, ns, 3, tgt, nt, 3)) return rc;
            // twice: the first pass after an upload searches cold, every later one starts from the previous pass's winners and
            // folds its sums in another order (rmse may differ in the last bit).  The numbers returned are those of the state
            // the context is left in: the ones visma_icp_run(init = T, max_iter = 0) repeats.
            for (int pass = 0; pass < 2; pass++)
                if (int rc = visma_icp_run(ctx, &pass_T[(size_t)(16 * b)], max_dist, 0, 0.0, 0.0, VISMA_ICP_SOLVER_KABSCH, 0, result)) return rc;
        }
    }
    if (info) *info = I;
    return VISMA_ICP_OK;
}

int visma_icp_registration_ransac_correspondence(visma_icp_ctx *ctx, const double *src, int64_t ns, const double *tgt, int64_t nt,
                                                 const int32_t *src_idx, const int32_t *tgt_idx, int64_t K, double max_dist,
                                                 int ransac_n, int max_iteration, int max_validation, uint64_t seed,
                                                 const int32_t *draws, int64_t n_draw_trials, visma_icp_result *result,
                                                 visma_icp_ransac_info *info)
{
    CTX_CHECK();
    visma_icp_ransac_option o = kRansacDefaults;
    o.ransac_n = ransac_n; o.max_iteration = max_iteration; o.max_validation = max_validation;
    if (const char *m = ransac_check(src, ns, tgt, nt, nullptr, nullptr, o, draws, n_draw_trials)) return ctx->fail(VISMA_ICP_ERR_INVALID, m);
    if (!src_idx || !tgt_idx || !result || K > 0x7fffffff) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad registration_ransac_correspondence arguments");
    if (K < ransac_n) return ctx->fail(VISMA_ICP_ERR_INVALID, "registration_ransac_correspondence: fewer pairs than ransac_n");
    if (!(max_dist > 0.0)) return ctx->fail(VISMA_ICP_ERR_INVALID, "registration_ransac_correspondence: max_dist must be positive");
    for (int64_t c = 0; c < K; c++)
        if (src_idx[c] < 0 || src_idx[c] >= ns || tgt_idx[c] < 0 || tgt_idx[c] >= nt)
            return ctx->fail(VISMA_ICP_ERR_INVALID, "registration_ransac_correspondence: a pair outside its cloud");
    if (!ctx->eng->supports_device_loop())
        return ctx->fail(VISMA_ICP_ERR_STATE, "registration_ransac_correspondence needs the HIP engine");
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    ransac_empty_result(result);
    visma_icp_ransac_info I = {0, 0, 0, 0, -1, 0.0, 0.0};
    int64_t trials = std::max(std::min(max_iteration, max_validation), 0);
    if (draws) trials = std::min(trials, n_draw_trials);
    if (trials > 0) {
        const int64_t chunk = std::min<int64_t>(kRansacChunk, trials);
        RansacDeviceHolder H;
        hipError_t e = ransac_device_create(ransac_problem(src, ns, tgt, nt, nullptr, nullptr, src_idx, tgt_idx, K, o, seed, draws, trials),
                                            chunk, ctx->eng->aux_stream(), &H.d);
        std::vector<int8_t> verdict((size_t)chunk);
        std::vector<int64_t> pass_trial;
        std::vector<double> pass_T;
        for (int64_t t = 0; e == hipSuccess && t < trials; t += chunk)
            e = ransac_device_chunk(H.d, t, std::min(chunk, trials - t), verdict.data(), nullptr, &pass_trial,
                                    &pass_T, &I.hypothesis_ms);
        const double t0 = ransac_now_ms();
        std::vector<int64_t> good(pass_trial.size());
        std::vector<double> err2(pass_trial.size());
        if (e == hipSuccess) e = ransac_score_device(H.d, pass_T.data(), (int64_t)pass_trial.size(), max_dist, good.data(), err2.data());
        if (e != hipSuccess) return ctx->fail(e == hipErrorInvalidValue ? VISMA_ICP_ERR_INVALID : VISMA_ICP_ERR_HIP,
                                              std::string("registration_ransac_correspondence: ") + hipGetErrorString(e));
        std::vector<double> fit(good.size()), rmse(good.size());
        for (size_t i = 0; i < good.size(); i++) {
            fit[i] = good[i] == 0 ? 0.0 : (double)good[i] / (double)K;
            rmse[i] = good[i] == 0 ? 0.0 : std::sqrt(err2[i] / (double)good[i]);
        }
        const int64_t b = ransac_best(fit, rmse);
        I.validation_ms = ransac_now_ms() - t0;
        I.n_trials = trials;
        I.n_validated = (int64_t)pass_trial.size();
        if (b >= 0) {
            I.best_trial = pass_trial[(size_t)b];
            std::memcpy(result->transformation, &pass_T[(size_t)(16 * b)], 16 * sizeof(double));
            result->fitness = fit[(size_t)b];
            result->inlier_rmse = rmse[(size_t)b];
            result->num_correspondences = good[(size_t)b];
        }
    }
    if (info) *info = I;
    return VISMA_ICP_OK;
}

// ---- the pose graph (host_math.hpp; pure functions) ---------------------------------------------------------------------
int visma_icp_global_optimization_option_clamp(visma_icp_global_optimization_option *o)
{
    if (!o) return VISMA_ICP_ERR_INVALID;
    // (the reference's comparisons, so a NaN stays what the caller gave)
    if (o->max_correspondence_distance < 0.0) o->max_correspondence_distance = 0.075;
    if (o->edge_prune_threshold < 0.0 || o->edge_prune_threshold > 1.0) o->edge_prune_threshold = 0.25;
    if (o->preference_loop_closure < 0.0) o->preference_loop_closure = 1.0;
    return VISMA_ICP_OK;
}

int visma_icp_global_optimization_criteria_clamp(visma_icp_global_optimization_criteria *c)
{
    if (!c) return VISMA_ICP_ERR_INVALID;
    if (c->upper_scale_factor < 0.0 || c->upper_scale_factor > 1.0) c->upper_scale_factor = 2. / 3.;
    if (c->lower_scale_factor < 0.0 || c->lower_scale_factor > 1.0) c->lower_scale_factor = 1. / 3.;
    return VISMA_ICP_OK;
}

static bool pose_graph_args_ok(const double *poses, int n_nodes, const visma_icp_pose_graph_edge *edges, int n_edges)
{
    return n_nodes >= 0 && n_edges >= 0 && (n_nodes == 0 || poses) && (n_edges == 0 || edges);
}

static PoseGraphData pose_graph_of(const double *poses, int n_nodes, const visma_icp_pose_graph_edge *edges, int n_edges)
{
    PoseGraphData g;
    g.nodes.resize((size_t)n_nodes);
    for (int i = 0; i < n_nodes; i++) g.nodes[(size_t)i] = Mat4::from(poses + (size_t)i * 16);
    g.edges.resize((size_t)n_edges);
    for (int e = 0; e < n_edges; e++) {
        PgEdge &t = g.edges[(size_t)e];
        t.source = edges[e].source; t.target = edges[e].target;
        t.X = Mat4::from(edges[e].transformation);
        std::memcpy(t.info, edges[e].information, sizeof(t.info));
        t.uncertain = edges[e].uncertain != 0;
        t.confidence = edges[e].confidence;
    }
    return g;
}

static bool pose_graph_ids_ok(const PoseGraphData &g)
{
    const int n = (int)g.nodes.size();
    for (const PgEdge &t : g.edges)
        if (t.source < 0 || t.source >= n || t.target < 0 || t.target >= n) return false;
    return true;
}

int visma_icp_pose_graph_validate(int n_nodes, const visma_icp_pose_graph_edge *edges, int n_edges)
{
    if (n_nodes < 0 || n_edges < 0 || (n_edges > 0 && !edges)) return -VISMA_ICP_ERR_INVALID;
    PoseGraphData g;
    g.nodes.resize((size_t)n_nodes);
    g.edges.resize((size_t)n_edges);
    for (int e = 0; e < n_edges; e++) { g.edges[(size_t)e].source = edges[e].source; g.edges[(size_t)e].target = edges[e].target; }
    return pg_validate(g) ? 1 : 0;
}

int visma_icp_pose_graph_zeta(const double *poses, int n_nodes, const visma_icp_pose_graph_edge *edges, int n_edges, double *zeta_out)
{
    if (!pose_graph_args_ok(poses, n_nodes, edges, n_edges) || (n_edges > 0 && !zeta_out)) return VISMA_ICP_ERR_INVALID;
    const PoseGraphData g = pose_graph_of(poses, n_nodes, edges, n_edges);
    if (!pose_graph_ids_ok(g)) return VISMA_ICP_ERR_INVALID;
    std::vector<double> zeta;
    pg_zeta(g, zeta);
    if (!zeta.empty()) std::memcpy(zeta_out, zeta.data(), sizeof(double) * zeta.size());
    return VISMA_ICP_OK;
}

int visma_icp_pose_graph_linear_system(const double *poses, int n_nodes, const visma_icp_pose_graph_edge *edges, int n_edges,
                                       double *H_out, double *b_out)
{
    if (!pose_graph_args_ok(poses, n_nodes, edges, n_edges) || (n_nodes > 0 && (!H_out || !b_out))) return VISMA_ICP_ERR_INVALID;
    const PoseGraphData g = pose_graph_of(poses, n_nodes, edges, n_edges);
    if (!pose_graph_ids_ok(g)) return VISMA_ICP_ERR_INVALID;
    std::vector<double> zeta, H, b;
    pg_zeta(g, zeta);
    pg_linear_system(g, zeta, H, b);
    if (!H.empty()) std::memcpy(H_out, H.data(), sizeof(double) * H.size());
    if (!b.empty()) std::memcpy(b_out, b.data(), sizeof(double) * b.size());
    return VISMA_ICP_OK;
}

static int pose_graph_run(bool whole, double *poses, int n_nodes, visma_icp_pose_graph_edge *edges, int *n_edges, int method,
                          const visma_icp_global_optimization_criteria *criteria, const visma_icp_global_optimization_option *option)
{
    if (!n_edges || !pose_graph_args_ok(poses, n_nodes, edges, *n_edges)) return VISMA_ICP_ERR_INVALID;
    if (method != VISMA_ICP_GLOBAL_GAUSS_NEWTON && method != VISMA_ICP_GLOBAL_LEVENBERG_MARQUARDT) return VISMA_ICP_ERR_INVALID;
    visma_icp_global_optimization_option o = {0.075, 0.25, 1.0, -1};
    visma_icp_global_optimization_criteria c = {100, 1e-6, 1e-6, 1e-6, 1e-6, 20, 2. / 3., 1. / 3.};
    if (option) o = *option;
    if (criteria) c = *criteria;
    visma_icp_global_optimization_option_clamp(&o);
    visma_icp_global_optimization_criteria_clamp(&c);
    PgOption po;
    po.max_corr_dist = o.max_correspondence_distance; po.edge_prune_threshold = o.edge_prune_threshold;
    po.preference_loop_closure = o.preference_loop_closure; po.reference_node = o.reference_node;
    PgCriteria pc;
    pc.max_iteration = c.max_iteration; pc.min_relative_increment = c.min_relative_increment;
    pc.min_relative_residual_increment = c.min_relative_residual_increment; pc.min_right_term = c.min_right_term;
    pc.min_residual = c.min_residual; pc.max_iteration_lm = c.max_iteration_lm;
    pc.upper_scale_factor = c.upper_scale_factor; pc.lower_scale_factor = c.lower_scale_factor;
    PoseGraphData g = pose_graph_of(poses, n_nodes, edges, *n_edges);
    if (whole) {
        if (!pg_global_optimization(g, method, pc, po)) return VISMA_ICP_OK;     // an invalid graph: untouched
    } else {
        if (!pose_graph_ids_ok(g)) return VISMA_ICP_ERR_INVALID;
        pg_optimize(g, method, pc, po);
    }
    for (int i = 0; i < n_nodes; i++) std::memcpy(poses + (size_t)i * 16, g.nodes[(size_t)i].m, sizeof(double) * 16);
    for (size_t e = 0; e < g.edges.size(); e++) {
        const PgEdge &t = g.edges[e];
        visma_icp_pose_graph_edge &d = edges[e];
        d.source = t.source; d.target = t.target;
        std::memcpy(d.transformation, t.X.m, sizeof(d.transformation));
        std::memcpy(d.information, t.info, sizeof(d.information));
        d.uncertain = t.uncertain;
        d.confidence = t.confidence;
    }
    *n_edges = (int)g.edges.size();
    return VISMA_ICP_OK;
}

int visma_icp_global_optimization(double *poses, int n_nodes, visma_icp_pose_graph_edge *edges, int *n_edges, int method,
                                  const visma_icp_global_optimization_criteria *criteria,
                                  const visma_icp_global_optimization_option *option)
{
    return pose_graph_run(true, poses, n_nodes, edges, n_edges, method, criteria, option);
}

int visma_icp_pose_graph_optimize(double *poses, int n_nodes, visma_icp_pose_graph_edge *edges, int n_edges, int method,
                                  const visma_icp_global_optimization_criteria *criteria,
                                  const visma_icp_global_optimization_option *option)
{
    return pose_graph_run(false, poses, n_nodes, edges, &n_edges, method, criteria, option);
}

int visma_icp_point_mesh_distance(visma_icp_ctx *ctx, const double *P, int64_t np, const double *V,
                                  int64_t nv, const int32_t *F, int64_t nf, double *d2, int32_t *face,
                                  double *closest)
{
    CTX_CHECK();
    if (np < 0 || nv < 0 || nf < 0 || (np > 0 && (!P || !d2)) || (nf > 0 && (!V || !F)))
        return ctx->fail(VISMA_ICP_ERR_INVALID, "bad point_mesh_distance arguments");
    if (!ctx->eng->supports_device_loop()) return ctx->fail(VISMA_ICP_ERR_STATE, "needs the HIP engine");
    float ms = 0.f, bms = 0.f;
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    hipError_t e = point_mesh_distance_device(P, np, V, nv, F, nf, ctx->mesh_method, d2, face, closest, &ms, &bms,
                                              ctx->eng->aux_stream());
    if (e != hipSuccess) return ctx->fail(e == hipErrorInvalidValue ? VISMA_ICP_ERR_INVALID : VISMA_ICP_ERR_HIP,
                                          std::string("point_mesh_distance: ") + hipGetErrorString(e));
    ctx->last_aux_kernel_ms = ms;
    ctx->last_aux_build_ms = bms;
    return VISMA_ICP_OK;
}

int visma_icp_point_cloud_distance(visma_icp_ctx *ctx, const double *src_xyz, int64_t ns, const double *tgt_xyz,
                                   int64_t nt, double *dist_out)
{
    CTX_CHECK();
    if (ns < 0 || nt < 0 || (ns > 0 && (!src_xyz || !dist_out)) || (nt > 0 && !tgt_xyz))
        return ctx->fail(VISMA_ICP_ERR_INVALID, "bad point_cloud_distance arguments");
    if (ns > 0x7fffffff || nt > 0x7fffffff) return ctx->fail(VISMA_ICP_ERR_INVALID, "too many points for 32-bit indices");
    if (ns == 0) return VISMA_ICP_OK;
    if (!ctx->eng->supports_device_loop()) return ctx->fail(VISMA_ICP_ERR_STATE, "needs the HIP engine");
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    hipError_t e = point_cloud_distance_device(src_xyz, ns, tgt_xyz, nt, dist_out, ctx->eng->aux_stream());
    if (e != hipSuccess) return ctx->fail(e == hipErrorInvalidValue ? VISMA_ICP_ERR_INVALID : VISMA_ICP_ERR_HIP,
                                          std::string("point_cloud_distance: ") + hipGetErrorString(e));
    return VISMA_ICP_OK;
}

int visma_icp_nearest_neighbor_distance(visma_icp_ctx *ctx, const double *xyz, int64_t n, double *dist_out)
{
    CTX_CHECK();
    if (n < 0 || (n > 0 && (!xyz || !dist_out)))
        return ctx->fail(VISMA_ICP_ERR_INVALID, "bad nearest_neighbor_distance arguments");
    if (n > 0x7fffffff) return ctx->fail(VISMA_ICP_ERR_INVALID, "too many points for 32-bit indices");
    if (n == 0) return VISMA_ICP_OK;
    if (!ctx->eng->supports_device_loop()) return ctx->fail(VISMA_ICP_ERR_STATE, "needs the HIP engine");
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    hipError_t e = nearest_neighbor_distance_device(xyz, n, dist_out, ctx->eng->aux_stream());
    if (e != hipSuccess) return ctx->fail(e == hipErrorInvalidValue ? VISMA_ICP_ERR_INVALID : VISMA_ICP_ERR_HIP,
                                          std::string("nearest_neighbor_distance: ") + hipGetErrorString(e));
    return VISMA_ICP_OK;
}

int visma_icp_last_mesh_kernel_ms(visma_icp_ctx *ctx, double *query_ms, double *build_ms)
{
    CTX_CHECK();
    if (query_ms) *query_ms = ctx->last_aux_kernel_ms;
    if (build_ms) *build_ms = ctx->last_aux_build_ms;
    return VISMA_ICP_OK;
}

int visma_icp_set_mesh_search(visma_icp_ctx *ctx, int method)
{
    CTX_CHECK();
    if (method < 0 || method > 2) return ctx->fail(VISMA_ICP_ERR_INVALID, "mesh search method must be 0, 1 or 2");
    ctx->mesh_method = method;
    return VISMA_ICP_OK;
}

int visma_icp_sample_mesh(visma_icp_ctx *ctx, const double *V, int64_t nv, const int32_t *F, int64_t nf,
                          int64_t n, int reference_quirks, uint64_t seed, const double *uniforms,
                          double *out_xyz, int64_t *n_out)
{
    CTX_CHECK();
    if (!n_out || n < 0 || nv < 0 || nf < 0 || (n > 0 && !out_xyz) || (nf > 0 && (!V || !F)))
        return ctx->fail(VISMA_ICP_ERR_INVALID, "bad sample_mesh arguments");
    if (n > 0x7fffffff) return ctx->fail(VISMA_ICP_ERR_INVALID, "too many samples for 32-bit indices");
    if (!ctx->eng->supports_device_loop()) return ctx->fail(VISMA_ICP_ERR_STATE, "needs the HIP engine");
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    hipError_t e = sample_mesh_device(V, nv, F, nf, n, reference_quirks, (unsigned long long)seed, uniforms,
                                      out_xyz, n_out, ctx->eng->aux_stream());
    if (e != hipSuccess) return ctx->fail(e == hipErrorInvalidValue ? VISMA_ICP_ERR_INVALID : VISMA_ICP_ERR_HIP,
                                          std::string("sample_mesh: ") + hipGetErrorString(e));
    return VISMA_ICP_OK;
}

int visma_icp_error_metric(const double *errors, int64_t n, double out[5])
{
    if (!out || n <= 0 || !errors) return VISMA_ICP_ERR_INVALID;   // the reference indexes errors[n >> 1]
    // feh::ComputeErrorMetric (include/geometry.h:85-101), same accumulation order
    double mean = 0.0, sq = 0.0, mn = std::numeric_limits<double>::max(), mx = std::numeric_limits<double>::lowest();
    for (int64_t i = 0; i < n; i++) {
        mean += errors[i];
        sq += errors[i] * errors[i];
        mn = std::min(mn, errors[i]);
        mx = std::max(mx, errors[i]);
    }
    mean /= (double)n;
    // sorted[n >> 1] (geometry.h:96-97) without the full sort
    std::vector<double> s(errors, errors + n);
    if (n > 0) std::nth_element(s.begin(), s.begin() + (n >> 1), s.end());
    out[0] = mean;
    out[1] = std::sqrt(sq / (double)n - mean * mean);
    out[2] = n > 0 ? s[(size_t)n >> 1] : 0.0;
    out[3] = mn;
    out[4] = mx;
    return VISMA_ICP_OK;
}

int visma_icp_measure_surface_error(visma_icp_ctx *ctx, const double *Vs, int64_t nvs, const int32_t *Fs,
                                    int64_t nfs, const double *Vt, int64_t nvt, const int32_t *Ft,
                                    int64_t nft, int64_t num_samples, int reference_quirks, uint64_t seed,
                                    double out[5])
{
    CTX_CHECK();
    if (!out || num_samples <= 0) return ctx->fail(VISMA_ICP_ERR_INVALID, "bad measure_surface_error arguments");
    if (nvs < 0 || nfs < 0 || nvt < 0 || nft < 0 || (nfs > 0 && (!Vs || !Fs)) || (nft > 0 && (!Vt || !Ft)))
        return ctx->fail(VISMA_ICP_ERR_INVALID, "bad measure_surface_error arguments");
    if (!ctx->eng->supports_device_loop()) return ctx->fail(VISMA_ICP_ERR_STATE, "needs the HIP engine");
    std::vector<double> dist((size_t)num_samples);
    int64_t m = 0;
    float ms = 0.f, bms = 0.f;
    if (int rc = ctx->eng->bind_device()) return ctx->eng_fail(rc);
    hipError_t e = surface_distances_device(Vs, nvs, Fs, nfs, Vt, nvt, Ft, nft, num_samples, reference_quirks,
                                            (unsigned long long)seed, ctx->mesh_method, dist.data(), &m, &ms, &bms,
                                            ctx->eng->aux_stream());
    if (e != hipSuccess) return ctx->fail(e == hipErrorInvalidValue ? VISMA_ICP_ERR_INVALID : VISMA_ICP_ERR_HIP,
                                          std::string("measure_surface_error: ") + hipGetErrorString(e));
    ctx->last_aux_kernel_ms = ms;
    ctx->last_aux_build_ms = bms;
    if (m == 0) return ctx->fail(VISMA_ICP_ERR_INVALID, "no sample could be drawn from the source mesh");
    return visma_icp_error_metric(dist.data(), m, out);
}

int visma_icp_selftest_so3(const double *w, double *R, double *w_back, int n)
{
    if (!w || !R || !w_back || n <= 0) return VISMA_ICP_ERR_INVALID;
    DevBufs bufs;
    double *dw = nullptr, *dR = nullptr, *dw2 = nullptr;
    if (bufs.alloc(&dw, 3 * (size_t)n) == hipSuccess && bufs.alloc(&dR, 9 * (size_t)n) == hipSuccess &&
        bufs.alloc(&dw2, 3 * (size_t)n) == hipSuccess &&
        hipMemcpy(dw, w, sizeof(double) * 3 * n, hipMemcpyHostToDevice) == hipSuccess &&
        launch_so3_selftest(dw, dR, dw2, n, nullptr) == hipSuccess &&
        hipMemcpy(R, dR, sizeof(double) * 9 * n, hipMemcpyDeviceToHost) == hipSuccess &&
        hipMemcpy(w_back, dw2, sizeof(double) * 3 * n, hipMemcpyDeviceToHost) == hipSuccess)
        return VISMA_ICP_OK;
    g_create_error = "so3 selftest: HIP call failed (no GPU?)";
    return VISMA_ICP_ERR_HIP;
}

int visma_se3_compose(const double a[12], const double b[12], double out[12])
{
    if (!a || !b || !out) return VISMA_ICP_ERR_INVALID;
    se3_compose(a, b, out);
    return VISMA_ICP_OK;
}

int visma_se3_act(const double g[12], const double v[3], double out[3])
{
    if (!g || !v || !out) return VISMA_ICP_ERR_INVALID;
    se3_act(g, v, out);
    return VISMA_ICP_OK;
}

int visma_se3_inv(const double g[12], double out[12])
{
    if (!g || !out) return VISMA_ICP_ERR_INVALID;
    se3_inv(g, out);
    return VISMA_ICP_OK;
}

int visma_icp_selftest_se3(const double *g, const double *h, const double *v, int n, double *gh, double *gv, double *gi)
{
    if (n < 0 || (n > 0 && (!g || !h || !v || !gh || !gv || !gi))) return VISMA_ICP_ERR_INVALID;
    if (n == 0) return VISMA_ICP_OK;
    DevBufs bufs;
    double *d[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const size_t sz[6] = {12, 12, 3, 12, 3, 12};
    const double *in[3] = {g, h, v};
    double *outp[3] = {gh, gv, gi};
    bool ok = true;
    for (int k = 0; k < 6 && ok; k++) ok = bufs.alloc(&d[k], sz[k] * (size_t)n) == hipSuccess;
    for (int k = 0; k < 3 && ok; k++) ok = hipMemcpy(d[k], in[k], sizeof(double) * sz[k] * (size_t)n, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && launch_se3_selftest(d[0], d[1], d[2], n, d[3], d[4], d[5], nullptr) == hipSuccess;
    for (int k = 0; k < 3 && ok; k++) ok = hipMemcpy(outp[k], d[3 + k], sizeof(double) * sz[3 + k] * (size_t)n, hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); g_create_error = "se3 selftest: HIP call failed (no GPU?)"; return VISMA_ICP_ERR_HIP; }
    return VISMA_ICP_OK;
}

int visma_so3_rodrigues(const double w[3], double R[9], double dR_dw[27])
{
    if (!w || !R) return VISMA_ICP_ERR_INVALID;
    double D[27];
    rodrigues_jac(w, R, D);
    if (dR_dw) std::memcpy(dR_dw, D, sizeof(D));
    return VISMA_ICP_OK;
}

int visma_so3_invrodrigues(const double R[9], double w[3], double dw_dR[27])
{
    if (!w || !R) return VISMA_ICP_ERR_INVALID;
    double D[27];
    invrodrigues_jac(R, w, D);
    if (dw_dR) std::memcpy(dw_dR, D, sizeof(D));
    return VISMA_ICP_OK;
}

int visma_so3_project(const double A[9], double R[9])
{
    if (!A || !R) return VISMA_ICP_ERR_INVALID;
    project_so3(A, R);
    return VISMA_ICP_OK;
}

int visma_so3_matrix_derivatives(const double A[9], const double B[9], double dAB_dA_out[81], double dAB_dB_out[81],
                                 double dAt_dA_out[81], double dhat_out[27], double dvee_out[27])
{
    if (dAB_dA_out) { if (!B) return VISMA_ICP_ERR_INVALID; dAB_dA(B, dAB_dA_out); }
    if (dAB_dB_out) { if (!A) return VISMA_ICP_ERR_INVALID; dAB_dB(A, dAB_dB_out); }
    if (dAt_dA_out) dAt_dA(dAt_dA_out);
    if (dhat_out) dhat(dhat_out);
    if (dvee_out) dvee(dvee_out);
    return VISMA_ICP_OK;
}

int visma_icp_selftest_so3_jac(const double *w, int n, double *R, double *dR_dw, double *w_back, double *dw_dR,
                               double *proj)
{
    if (!w || !R || !dR_dw || !w_back || !dw_dR || !proj || n <= 0) return VISMA_ICP_ERR_INVALID;
    DevBufs bufs;
    double *d[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const size_t sz[6] = {3, 9, 27, 3, 27, 9};
    bool ok = true;
    for (int k = 0; k < 6 && ok; k++) ok = bufs.alloc(&d[k], sz[k] * (size_t)n) == hipSuccess;
    ok = ok && hipMemcpy(d[0], w, sizeof(double) * 3 * n, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && launch_so3_selftest_jac(d[0], n, d[1], d[2], d[3], d[4], d[5], nullptr) == hipSuccess;
    double *out[6] = {nullptr, R, dR_dw, w_back, dw_dR, proj};
    for (int k = 1; k < 6 && ok; k++) ok = hipMemcpy(out[k], d[k], sizeof(double) * sz[k] * n, hipMemcpyDeviceToHost) == hipSuccess;
    if (ok) return VISMA_ICP_OK;
    g_create_error = "so3 selftest: HIP call failed (no GPU?)";
    return VISMA_ICP_ERR_HIP;
}

int visma_icp_selftest_neighbor_lists(const double *xyz, int64_t n, int search_type, int cap, double radius, int list_kind,
                                      int32_t *idx, double *d2, int32_t *cnt)
{
    const bool lists = search_type != 1;
    if (!xyz || !cnt || n <= 0 || n > 0x7fffffff || search_type < 0 || search_type > 2 || cap < 1 || list_kind < 0 ||
        list_kind > 1 || (list_kind == 0 && cap > kNormalsMaxList) || (lists && (!idx || !d2)) ||
        (search_type != 0 && (!(radius > 0.0) || !std::isfinite(radius))))
        return VISMA_ICP_ERR_INVALID;
    const hipError_t e = nn_selftest_lists_device(xyz, n, search_type, cap, radius, list_kind, idx, d2, cnt, nullptr);
    if (e == hipSuccess) return VISMA_ICP_OK;
    (void)hipGetLastError();
    g_create_error = std::string("neighbor lists selftest: ") + hipGetErrorString(e);
    return VISMA_ICP_ERR_HIP;
}

// ---- the gravity alignment and pose composition of feh::AnnotationTool (src/annotation.cpp:82-91, 111-153): host
// code (plane_math.hpp); the clouds it looks at are the ones about to be uploaded
int visma_geom_find_plane_normal(const double *xyz, int64_t n, double normal_out[3])
{
    if (!normal_out || n < 0 || (n > 0 && !xyz)) return VISMA_ICP_ERR_INVALID;
    visma::plane::find_plane_normal(xyz, n, normal_out);
    return VISMA_ICP_OK;
}

int visma_geom_jacobi_svd3(const double A[9], double U[9], double S[3], double V[9])
{
    if (!A || !U || !S || !V) return VISMA_ICP_ERR_INVALID;
    visma::plane::jacobi_svd3(A, U, S, V);
    return VISMA_ICP_OK;
}

int visma_geom_rotation_between_vectors(const double u[3], const double v[3], double R[9])
{
    if (!u || !v || !R) return VISMA_ICP_ERR_INVALID;
    const double lu = u[0] * u[0] + u[1] * u[1] + u[2] * u[2], lv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    if (!(lu > 0.0) || !(lv > 0.0)) return VISMA_ICP_ERR_INVALID;
    visma::plane::rotation_between_vectors(u, v, R);
    return VISMA_ICP_OK;
}

int visma_geom_centre_on_floor(const double *xyz, int64_t n, double t_out[3])
{
    if (!t_out || n <= 0 || !xyz) return VISMA_ICP_ERR_INVALID;
    visma::plane::centre_on_floor(xyz, n, t_out);
    return VISMA_ICP_OK;
}

// Ttot = (T1 T0)^-1 T3 T2 with the reference's rigid inverse (rotation transposed, t <- -R^T t), row-major 4x4
int visma_annot_total_pose(const double T0[16], const double T1[16], const double T2[16], const double T3[16], double Ttot[16])
{
    if (!T0 || !T1 || !T2 || !T3 || !Ttot) return VISMA_ICP_ERR_INVALID;
    auto mul = [](const double *a, const double *b, double *c) {
        double r[16];
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) {
                double v = 0.0;
                for (int k = 0; k < 4; k++) v += a[4 * i + k] * b[4 * k + j];
                r[4 * i + j] = v;
            }
        for (int i = 0; i < 16; i++) c[i] = r[i];
    };
    double A[16], Ai[16];
    mul(T1, T0, A);
    for (int i = 0; i < 16; i++) Ai[i] = A[i];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Ai[4 * i + j] = A[4 * j + i];      // block<3,3>.transposeInPlace()
    for (int i = 0; i < 3; i++) Ai[4 * i + 3] = -(Ai[4 * i] * A[3] + Ai[4 * i + 1] * A[7] + Ai[4 * i + 2] * A[11]);
    mul(Ai, T3, A);
    mul(A, T2, Ttot);
    return VISMA_ICP_OK;
}

int visma_icp_marching_cubes_case(int cube_case, int32_t *edge_ids, int *n_triangles)
{
    if (cube_case < 0 || cube_case > 255 || !edge_ids || !n_triangles) return VISMA_ICP_ERR_INVALID;
    const visma::McCase &c = visma::mc_table().c[cube_case];
    if (c.n > visma::kMcMaxTriangles) return VISMA_ICP_ERR_STATE;     // (the rule gave more than the table holds: never)
    *n_triangles = c.n;
    for (int i = 0; i < 3 * c.n; i++) edge_ids[i] = c.edge[i];
    return VISMA_ICP_OK;
}

// ---- the mesh renderer (render.hip, render_math.hpp) ----
static const char *render_check_camera(int w, int h, const double *intrinsic, const double *extrinsic, double z_near, double z_far, int encoding)
{
    if (!intrinsic || !extrinsic) return "render: NULL argument";
    if (w <= 0 || h <= 0 || (int64_t)w * h > (int64_t)1 << 30) return "render: 0 < w, h and at most 2^30 pixels";
    for (int k = 0; k < 4; k++) if (!std::isfinite(intrinsic[k])) return "render: a non-finite camera parameter";
    for (int k = 0; k < 16; k++) if (!std::isfinite(extrinsic[k])) return "render: a non-finite extrinsic entry";
    if (!std::isfinite(z_near) || !std::isfinite(z_far)) return "render: a non-finite camera parameter";
    if (intrinsic[0] == 0.0 || intrinsic[1] == 0.0) return "render: fx or fy is 0";
    if (!(z_near > 0.0)) return "render: z_near <= 0";
    if (!(z_far > z_near)) return "render: z_far <= z_near";
    if (encoding != VISMA_ICP_RENDER_METRIC && encoding != VISMA_ICP_RENDER_DEPTH_BUFFER) return "render: unknown encoding";
    return nullptr;
}

static RenderCamera render_camera(int w, int h, const double *k, double z_near, double z_far)
{
    RenderCamera c;
    c.w = w; c.h = h; c.fx = k[0]; c.fy = k[1]; c.cx = k[2]; c.cy = k[3]; c.z_near = z_near; c.z_far = z_far;
    return c;
}

int visma_icp_render(visma_icp_ctx *ctx, visma_icp_trimesh *mesh, int w, int h, const double intrinsic[4], const double extrinsic[16],
                     double z_near, double z_far, int encoding, visma_icp_image **depth, visma_icp_image **index, visma_icp_image **mask)
{
    CTX_CHECK();
    if (depth) *depth = nullptr;
    if (index) *index = nullptr;
    if (mask) *mask = nullptr;
    if (!mesh) return ctx->fail(VISMA_ICP_ERR_INVALID, "NULL mesh");
    if (const char *m = render_check_camera(w, h, intrinsic, extrinsic, z_near, z_far, encoding)) return ctx->fail(VISMA_ICP_ERR_INVALID, m);
    if (int rc = trimesh_enter(ctx, mesh)) return rc;
    ImageDevice *d = nullptr, *i = nullptr, *k = nullptr;
    const hipError_t e = render_device_render(ctx->render_scratch(), mesh->dev, render_camera(w, h, intrinsic, z_near, z_far), extrinsic,
                                              encoding, ctx->eng->aux_stream(), depth ? &d : nullptr, index ? &i : nullptr,
                                              mask ? &k : nullptr);
    if (e != hipSuccess) return image_done(ctx, "render", e);
    if (depth) *depth = ctx->adopt(d);
    if (index) *index = ctx->adopt(i);
    if (mask) *mask = ctx->adopt(k);
    return VISMA_ICP_OK;
}

int visma_icp_render_edges(visma_icp_ctx *ctx, visma_icp_image *depth, visma_icp_image **out)
{
    IMAGE_NEW_CHECK(depth);
    if (!image_is_float(depth)) return ctx->fail(VISMA_ICP_ERR_INVALID, "render_edges: the depth is a 1 x float image");
    ImageDevice *dev = nullptr;
    return image_adopt(ctx, "render_edges", render_device_edges(depth->dev, ctx->eng->aux_stream(), &dev), dev, out);
}

int visma_icp_render_edges_host(const float *depth, int w, int h, uint8_t *edges)
{
    if (!depth || !edges || w <= 0 || h <= 0) { g_create_error = "render_edges_host: bad arguments"; return VISMA_ICP_ERR_INVALID; }
    parallel_for(h, 16, [&](int64_t y) {
        for (int x = 0; x < w; x++) edges[y * w + x] = render_edge(depth, w, h, x, (int)y);
    });
    return VISMA_ICP_OK;
}

int visma_icp_render_host(const double *vertices, int64_t nv, const int32_t *triangles, int64_t nt, int w, int h, const double intrinsic[4],
                          const double extrinsic[16], double z_near, double z_far, int encoding, float *depth, int32_t *index,
                          uint8_t *mask, uint8_t *edges)
{
    if (const char *m = render_check_camera(w, h, intrinsic, extrinsic, z_near, z_far, encoding)) { g_create_error = m; return VISMA_ICP_ERR_INVALID; }
    if (nv < 0 || nt < 0 || nt > 0x7fffffff || (nv > 0 && !vertices) || (nt > 0 && !triangles)) {
        g_create_error = "render_host: bad mesh arguments";
        return VISMA_ICP_ERR_INVALID;
    }
    for (int64_t k = 0; k < 3 * nt; k++)
        if (triangles[k] < 0 || triangles[k] >= nv) { g_create_error = "render_host: an index outside [0, nv)"; return VISMA_ICP_ERR_INVALID; }
    const RenderCamera c = render_camera(w, h, intrinsic, z_near, z_far);
    std::vector<double> cam(3 * (size_t)nv);
    for (int64_t i = 0; i < nv; i++) render_camera_point(extrinsic, vertices + 3 * i, cam.data() + 3 * i);
    std::vector<RenderTri> tris((size_t)nt);
    std::vector<unsigned long long> keys((size_t)w * (size_t)h, kRenderNoKey);
    for (int64_t i = 0; i < nt; i++) {
        RenderTri &t = tris[(size_t)i];
        render_setup(cam.data() + 3 * (size_t)triangles[3 * i], cam.data() + 3 * (size_t)triangles[3 * i + 1],
                     cam.data() + 3 * (size_t)triangles[3 * i + 2], c, t);
        for (int y = t.y0; y <= t.y1; y++)
            for (int x = t.x0; x <= t.x1; x++) {
                const unsigned long long key = render_key(t, c, x, y, (unsigned)i);
                unsigned long long &at = keys[(size_t)y * (size_t)w + (size_t)x];
                if (key < at) at = key;
            }
    }
    std::vector<float> metric(edges ? keys.size() : 0);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t p = (size_t)y * (size_t)w + (size_t)x;
            float d;
            int32_t idx;
            uint8_t m;
            render_resolve(keys[p], tris.data(), c, x, y, encoding, &d, &idx, &m);
            if (depth) depth[p] = d;
            if (index) index[p] = idx;
            if (mask) mask[p] = m;
            if (edges) {
                if (encoding != VISMA_ICP_RENDER_METRIC) render_resolve(keys[p], tris.data(), c, x, y, VISMA_ICP_RENDER_METRIC, &d, &idx, &m);
                metric[p] = d;
            }
        }
    if (edges)
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) edges[(size_t)y * (size_t)w + (size_t)x] = render_edge(metric.data(), w, h, x, y);
    return VISMA_ICP_OK;
}

double visma_icp_linearize_depth(double zb, double z_near, double z_far) { return render_linearize_depth(zb, z_near, z_far); }

int visma_icp_image_is_int32(const visma_icp_image *img, int *is_int32)
{
    if (!img || !img->dev || !is_int32) { g_create_error = "image is NULL"; return VISMA_ICP_ERR_INVALID; }
    *is_int32 = image_device_is_integer(img->dev) ? 1 : 0;
    return VISMA_ICP_OK;
}

}  // extern "C"

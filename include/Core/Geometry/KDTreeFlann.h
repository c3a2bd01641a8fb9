// Core/Geometry/KDTreeFlann.h -- neighbour queries against a cloud resident on the GPU (shape of
// O3D/Core/Geometry/KDTreeFlann.h:45-86).  The methods are defined in visma_icp_open3d.hpp (visma_icp.h, "KDTreeFlann": the
// results, the grid a tree keeps, and the deviations from the reference).  Not flann and not a k-d tree: the exact grid search
// of the library, with the reference's results -- its lists, its order, its d2 to the bit, its return values:
//   -1       an empty tree (no SetGeometry / SetMatrixData yet, or one that failed), knn < 0, max_nn < 0, a query that has
//            not three rows
//   the number of neighbours otherwise, `indices` and `distance2` resized to it.  A negative radius is squared, as the
//   reference squares it: the answer of its absolute value.
// Where the class differs: three dimensions only (SetMatrixData with rows() != 3 returns false; no SetFeature: the
// 33-dimensional 1-NN of feature matching is visma_icp_match_features); knn = 0 and max_nn = 0 return 0 (the reference runs
// flann's result sets with no capacity); a radius of 0 or one that is not finite finds nothing; and this stand-alone set has
// no Geometry base class: the constructor and SetGeometry are overloaded for PointCloud and for TriangleMesh (its vertices).
//
// One Search is a launch and a round trip to the device.  For many queries use the batch overloads in open3d::cicp
// (visma_icp_open3d.hpp: KDTreeSearchKNN, KDTreeSearchHybrid, KDTreeSearchRadius), which take all of them in one call.
#pragma once

#include <Eigen/Core>
#include <vector>

#include "KDTreeSearchParam.h"
#include "PointCloud.h"
#include "TriangleMesh.h"

struct visma_icp_ctx;
struct visma_icp_kdtree;

namespace open3d {

class KDTreeFlann {
public:
    // on this thread's context (which the tree must not outlive) ...
    KDTreeFlann() {}
    explicit KDTreeFlann(const Eigen::MatrixXd &data) { SetMatrixData(data); }
    explicit KDTreeFlann(const PointCloud &geometry) { SetGeometry(geometry); }
    explicit KDTreeFlann(const TriangleMesh &geometry) { SetGeometry(geometry); }
    // ... or on a context of the caller's
    explicit KDTreeFlann(visma_icp_ctx *ctx) : ctx_(ctx) {}
    KDTreeFlann(visma_icp_ctx *ctx, const PointCloud &geometry) : ctx_(ctx) { SetGeometry(geometry); }
    KDTreeFlann(visma_icp_ctx *ctx, const TriangleMesh &geometry) : ctx_(ctx) { SetGeometry(geometry); }
    ~KDTreeFlann();
    KDTreeFlann(const KDTreeFlann &) = delete;
    KDTreeFlann &operator=(const KDTreeFlann &) = delete;

    // 3 x n, column j the point j; false (and an empty tree) for rows() != 3 or no columns
    bool SetMatrixData(const Eigen::MatrixXd &data);
    bool SetGeometry(const PointCloud &geometry);
    bool SetGeometry(const TriangleMesh &geometry);

    template <typename T>
    int Search(const T &query, const KDTreeSearchParam &param, std::vector<int> &indices, std::vector<double> &distance2) const;
    template <typename T>
    int SearchKNN(const T &query, int knn, std::vector<int> &indices, std::vector<double> &distance2) const;
    template <typename T>
    int SearchRadius(const T &query, double radius, std::vector<int> &indices, std::vector<double> &distance2) const;
    template <typename T>
    int SearchHybrid(const T &query, double radius, int max_nn, std::vector<int> &indices, std::vector<double> &distance2) const;

    // (the batch overloads) the context and the tree on it, NULL while the tree is empty; the number of points
    visma_icp_ctx *context() const { return ctx_; }
    visma_icp_kdtree *handle() const { return tree_; }
    size_t size() const { return dataset_size_; }

private:
    bool SetRawData(const double *xyz, size_t n);
    visma_icp_ctx *ctx_ = nullptr;
    visma_icp_kdtree *tree_ = nullptr;
    size_t dataset_size_ = 0;
};

}  // namespace open3d

// Core/Registration/Feature.h -- one feature vector per point as the columns of a matrix
// (shape of O3D/Core/Registration/Feature.h:37-55), and the FPFH of a cloud with normals.
#pragma once

#include <Eigen/Core>
#include <memory>

#include "../Geometry/KDTreeSearchParam.h"

namespace open3d {

class PointCloud;

class Feature {
public:
    void Resize(int dim, int n) { data_.resize(dim, n); data_.setZero(); }
    size_t Dimension() const { return data_.rows(); }
    size_t Num() const { return data_.cols(); }

    Eigen::MatrixXd data_;
};

inline std::shared_ptr<Feature> ComputeFPFHFeature(const PointCloud &input,
                                                   const KDTreeSearchParam &search_param = KDTreeSearchParamKNN());

}  // namespace open3d

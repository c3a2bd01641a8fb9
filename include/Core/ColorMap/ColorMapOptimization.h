// Core/ColorMap/ColorMapOptimization.h -- color map optimization (Q.-Y. Zhou and V. Koltun, Color Map Optimization for 3D
// Reconstruction with Consumer Depth Cameras, SIGGRAPH 2014; shape of O3D/Core/ColorMap/ColorMapOptimization.h).  The
// rigid variant runs on the GPU (visma_icp_open3d.hpp) as ColorMapOptimization; the non-rigid one -- a warping field per
// image -- as cicp::ColorMapOptimizationNonRigid, a function of its own: ColorMapOptimization with
// non_rigid_camera_coordinate_ set throws std::invalid_argument and says so.  Stand-alone and header-only.
#pragma once

#include <vector>

#include "../Camera/PinholeCameraTrajectory.h"
#include "../Geometry/PointCloud.h"
#include "../Geometry/RGBDImage.h"
#include "../Geometry/TriangleMesh.h"

namespace open3d {

class ColorMapOptmizationOption {        // (the reference's spelling)
public:
    ColorMapOptmizationOption(bool non_rigid_camera_coordinate = false, int number_of_vertical_anchors = 16,
                              double non_rigid_anchor_point_weight = 0.316, double maximum_iteration = 300,
                              double maximum_allowable_depth = 2.5, double depth_threshold_for_visiblity_check = 0.03,
                              double depth_threshold_for_discontinuity_check = 0.1,
                              int half_dilation_kernel_size_for_discontinuity_map = 3)
        : non_rigid_camera_coordinate_(non_rigid_camera_coordinate), number_of_vertical_anchors_(number_of_vertical_anchors),
          non_rigid_anchor_point_weight_(non_rigid_anchor_point_weight), maximum_iteration_(maximum_iteration),
          maximum_allowable_depth_(maximum_allowable_depth), depth_threshold_for_visiblity_check_(depth_threshold_for_visiblity_check),
          depth_threshold_for_discontinuity_check_(depth_threshold_for_discontinuity_check),
          half_dilation_kernel_size_for_discontinuity_map_(half_dilation_kernel_size_for_discontinuity_map) {}

    bool non_rigid_camera_coordinate_;
    int number_of_vertical_anchors_;
    double non_rigid_anchor_point_weight_;
    double maximum_iteration_;
    double maximum_allowable_depth_;
    double depth_threshold_for_visiblity_check_;
    double depth_threshold_for_discontinuity_check_;
    int half_dilation_kernel_size_for_discontinuity_map_;
};

// Refines camera.extrinsic_ in place and writes mesh.vertex_colors_.  images_rgbd: float depth in metres and an RGB8 colour
// image per frame, all of the intrinsic's size; any other format throws std::invalid_argument.  Reads nothing of the mesh
// but vertices_.  On the GPU, in visma_icp_open3d.hpp (this thread's context; cicp::ColorMapOptimization takes one).
inline void ColorMapOptimization(TriangleMesh &mesh, const std::vector<RGBDImage> &images_rgbd, PinholeCameraTrajectory &camera,
                                 const ColorMapOptmizationOption &option = ColorMapOptmizationOption());
// (A caller who sets non_rigid_camera_coordinate_ calls cicp::ColorMapOptimizationNonRigid(mesh or cloud, images_rgbd, camera,
//  option[, ctx first]) of visma_icp_open3d.hpp instead: number_of_vertical_anchors_ and non_rigid_anchor_point_weight_ are read
//  there whatever the flag says.)

}  // namespace open3d

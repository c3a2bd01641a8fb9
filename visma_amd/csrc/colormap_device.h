// colormap_device.h -- what colormap.hip (the rigid color map optimization) and colormap_warp.hip (the non-rigid one) share:
// the device object, the camera, the margin test and the warping field's bilinear shift.  Internal to the two files.  The
// shared types live in the NAMED namespace visma::cm: both files see one ColorMapDevice made of the same types.
#pragma once

#include "kernels.h"
#include "dev_mem.h"

#include <vector>

namespace visma {

namespace cm {

constexpr double kCmMargin = 10.0;                       // IMAGE_BOUNDARY_MARGIN

struct CmCamera { double fx, fy, cx, cy; int w, h; };

// TestImageBoundary(u, v, 10) on doubles; a NaN fails
__device__ __forceinline__ bool cm_inside(double u, double v, const CmCamera &K)
{
    return u >= kCmMargin && u < (double)K.w - kCmMargin && v >= kCmMargin && v < (double)K.h - kCmMargin;
}

// the four anchors of cell (i, j) of one image's field (flow: 2 aw ah doubles): QueryFlow(i, j), (i, j + 1), (i + 1, j), (i + 1, j + 1)
struct CmWarpCell { double x00, y00, x01, y01, x10, y10, x11, y11; };

__device__ __forceinline__ CmWarpCell cm_warp_cell(const double *__restrict__ flow, int aw, int i, int j)
{
    const double *a = flow + 2 * ((long long)i + (long long)j * aw), *b = a + 2 * (long long)aw;
    CmWarpCell g;
    g.x00 = a[0]; g.y00 = a[1]; g.x10 = a[2]; g.y10 = a[3];
    g.x01 = b[0]; g.y01 = b[1]; g.x11 = b[2]; g.y11 = b[3];
    return g;
}

// GetImageWarpingField: every scalar weight formed first, the four terms added left to right
__device__ __forceinline__ void cm_warp_shift(const CmWarpCell &g, double p, double q, double *su, double *sv)
{
    const double w00 = (1 - p) * (1 - q), w01 = (1 - p) * q, w10 = p * (1 - q), w11 = p * q;
    *su = ((w00 * g.x00 + w01 * g.x01) + w10 * g.x10) + w11 * g.x11;
    *sv = ((w00 * g.y00 + w01 * g.y01) + w10 * g.y10) + w11 * g.y11;
}

}  // namespace cm

using namespace cm;

struct ColorMapDevice {
    ColorMapConfig cfg;
    hipStream_t stream = nullptr;
    CmCamera K;
    long long plane = 0, nv = 0, nvp = 0;
    int words = 0, blocks = 1;
    // the frames
    DeviceBuf<float> depth;
    DeviceBuf<unsigned char> rgb, mask;
    DeviceBuf<float4> texels;
    DeviceBuf<double> extrinsics;    // the CURRENT poses; host_extr is their copy
    DeviceBuf<double> extr0;         // the poses of prepare (what visibility read)
    std::vector<double> host_extr;
    // per image scratch: five fp32 planes and two mask planes
    DeviceBuf<float> tmp[5];
    DeviceBuf<unsigned char> mtmp[2];
    // the vertices and what hangs off them
    DeviceBuf<double> vertices, proxy, colors;
    DeviceBuf<unsigned> bits;
    DeviceBuf<int32_t> list;
    DeviceBuf<long long> offsets;
    std::vector<long long> host_offsets;
    Compactor compactor;             // the visibility lists' compaction (compact.h, in colormap.hip)
    // the iteration
    DeviceBuf<double> partials, sums;
    DeviceBuf<unsigned> tickets;
    bool proxy_valid = false;
    // the non-rigid map (cfg.anchors > 0; colormap_warp.hip): a warping field per image
    bool warp = false;
    int aw = 0, ah = 0;
    double step = 0.0;
    DeviceBuf<double> flow;          // n_images x 2 aw ah, the CURRENT fields; host_flow is their copy
    std::vector<double> host_flow, host_flow_init;       // (host_flow_init: one field, 2 aw ah)
    DeviceBuf<int32_t> keys, sorted;                     // per visit of the concatenated list: its cell; the vertex ids by cell
    DeviceBuf<int> hist;             // n_images x bins x tiles: the tiles' histograms
    DeviceBuf<int> hist_scan;        // their exclusive scan, camera by camera: where (bin, tile) begins in the camera's list
    DeviceBuf<double> cell_sums;     // n_images x cells x 121
    long long warp_tiles = 0, warp_rows = 0;
};

// (colormap.hip) the poses -- and the fields of a non-rigid map -- on the device and the proxies of them
hipError_t cm_refresh_proxy(ColorMapDevice *D);
// (colormap_warp.hip) the field's buffers at create, the sort's at prepare
hipError_t color_map_warp_create(ColorMapDevice *D);
hipError_t color_map_warp_prepare(ColorMapDevice *D);
hipError_t color_map_warp_upload_flow(ColorMapDevice *D);

}  // namespace visma

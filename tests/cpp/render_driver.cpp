// render_driver.cpp -- a caller of the renderer written against the stand-alone header set.  Two modes:
//   renderer IN OUT   vertices, faces, a camera, a pose and a model -> feh::gpu::Renderer with the reference's members:
//                     SetCamera (both forms), SetMesh (the pointer, vector or Eigen form), RenderDepth, RenderMask, RenderEdge;
//                     the three images, the accessors and LinearizeDepth of every depth value out
//   chain IN OUT      a depth frame, intrinsic, extrinsic -> UniformTSDFVolume::Integrate, the volume's mesh device to device,
//                     cicp::RenderDepth at the frame's pose, the resident depth into a second volume and through
//                     cicp::RenderEdges: depth, index, mask, edges, tsdf and weight out, with one download each
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "constrained_ICP.h"
#include "visma_geometry.hpp"

using namespace open3d;
static FILE *f, *o;
static double rd() { double v; if (fread(&v, 8, 1, f) != 1) std::exit(2); return v; }
static int ri() { return (int)rd(); }

static int renderer()
{
    const int form = ri(), nv = ri();
    std::vector<float> V(3 * (size_t)nv);
    for (auto &x : V) x = (float)rd();
    const int nf = ri();
    std::vector<int> F(3 * (size_t)nf);
    for (auto &x : F) x = ri();
    const int w = ri(), h = ri();
    float k[4];
    for (auto &x : k) x = (float)rd();
    const float zn = (float)rd(), zf = (float)rd();
    Eigen::Matrix<float, 4, 4, Eigen::ColMajor> pose, model;
    for (int i = 0; i < 16; i++) pose(i / 4, i % 4) = (float)rd();
    for (int i = 0; i < 16; i++) model(i / 4, i % 4) = (float)rd();
    feh::gpu::RendererPtr r = std::make_shared<feh::gpu::Renderer>(h, w);
    if (form == 0) r->SetCamera(zn, zf, k); else r->SetCamera(zn, zf, k[0], k[1], k[2], k[3]);
    r->SetCamera(pose);
    if (form == 0) {
        r->SetMesh(V.data(), nv, F.data(), nf);
    } else if (form == 1) {
        r->SetMesh(V, F);
    } else {
        Eigen::Matrix<float, Eigen::Dynamic, 3, Eigen::RowMajor> Vm(nv, 3);
        Eigen::Matrix<int, Eigen::Dynamic, 3, Eigen::RowMajor> Fm(nf, 3);
        for (int i = 0; i < 3 * nv; i++) Vm(i / 3, i % 3) = V[i];
        for (int i = 0; i < 3 * nf; i++) Fm(i / 3, i % 3) = F[i];
        r->SetMesh(Vm, Fm);
    }
    if (r->rows() != h || r->cols() != w || r->height() != h || r->width() != w || r->fx() != k[0] || r->fy() != k[1] || r->cx() != k[2] ||
        r->cy() != k[3] || r->z_near() != zn || r->z_far() != zf || r->id() != r->name() || r->name().empty())
        return 5;
    const size_t px = (size_t)w * h;
    std::vector<float> depth(px), metres(px);
    std::vector<uint8_t> mask(px), edge(px);
    r->RenderDepth(model, depth.data());
    r->RenderMask(model, mask.data());
    r->RenderEdge(model, edge.data());
    for (size_t i = 0; i < px; i++) metres[i] = feh::gpu::LinearizeDepth(depth[i], zn, zf);
    fwrite(depth.data(), 4, px, o);
    fwrite(mask.data(), 1, px, o);
    fwrite(edge.data(), 1, px, o);
    fwrite(metres.data(), 4, px, o);
    return 0;
}

static int chain()
{
    const int w = ri(), h = ri();
    Image depth;
    depth.PrepareImage(w, h, 1, 4);
    if (fread(depth.data_.data(), 1, depth.data_.size(), f) != depth.data_.size()) return 2;
    const double fx = rd(), fy = rd(), cx = rd(), cy = rd();
    Eigen::Matrix4d E;
    for (int i = 0; i < 16; i++) E(i / 4, i % 4) = rd();
    PinholeCameraIntrinsic cam(w, h, fx, fy, cx, cy);
    UniformTSDFVolume a(2.0, 32, 0.1, TSDFVolumeColorType::None, Eigen::Vector3d(-1.0, -1.0, -1.0));
    UniformTSDFVolume b(2.0, 32, 0.1, TSDFVolumeColorType::None, Eigen::Vector3d(-1.0, -1.0, -1.0));
    a.Integrate(cicp::DeviceImage(a.Context(), depth), nullptr, cam, E);
    int64_t nv = 0, nt = 0;
    if (visma_icp_tsdf_extract_triangle_mesh(a.Context(), a.Handle(), &nv, &nt) != VISMA_ICP_OK) return 3;
    cicp::DeviceTriangleMesh mesh = cicp::DeviceTriangleMesh::FromVolume(a);
    cicp::DeviceImage index(a.Context(), (visma_icp_image *)nullptr), mask(a.Context(), (visma_icp_image *)nullptr);
    cicp::DeviceImage d = cicp::RenderDepth(mesh, cam, E, 0.05, 10.0, false, &index, &mask);
    cicp::DeviceImage e = cicp::RenderEdges(d);
    b.Integrate(d, nullptr, cam, E);                       // device to device
    bool refused = false;
    try { b.Integrate(index, nullptr, cam, E); } catch (const std::invalid_argument &) { refused = true; }   // no depth
    if (!refused) return 6;
    refused = false;
    try { cicp::RenderDepth(mesh, PinholeCameraIntrinsic(w, h, 0.0, fy, cx, cy), E); } catch (const std::invalid_argument &) { refused = true; }
    if (!refused) return 7;
    for (const cicp::DeviceImage *img : {&d, &index, &mask, &e}) {
        const std::shared_ptr<Image> host = img->Download();
        const int info[4] = {host->width_, host->height_, host->num_of_channels_, host->bytes_per_channel_};
        fwrite(info, 4, 4, o);
        fwrite(host->data_.data(), 1, host->data_.size(), o);
    }
    std::vector<float> tsdf, weight;
    std::vector<Eigen::Vector3f> col;
    b.Download(tsdf, weight, col);
    const int n = (int)tsdf.size();
    fwrite(&n, 4, 1, o);
    fwrite(tsdf.data(), 4, tsdf.size(), o);
    fwrite(weight.data(), 4, weight.size(), o);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 4) return 1;
    f = fopen(argv[2], "rb");
    o = fopen(argv[3], "wb");
    if (!f || !o) return 1;
    int rc = 1;
    try {
        if (!strcmp(argv[1], "renderer")) rc = renderer();
        else if (!strcmp(argv[1], "chain")) rc = chain();
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        rc = 4;
    }
    fclose(o);
    return rc;
}

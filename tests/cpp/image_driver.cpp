// image_driver.cpp -- a caller of the reference's image front end, written against the stand-alone header set
// (Core/Geometry/Image.h, RGBDImage.h) with the reference's names and signatures.  Three modes:
//   cases IN OUT      a program of tests/image_cases.py (its encode()) through the stock names; the registers and results out
//   chain IN OUT      color (3 x uint8) and depth (1 x uint16) -> cicp::DeviceImage: RGBD(TUM), a 3-level pyramid of the gray,
//                     Gaussian5, LinearTransform, ClipIntensity, FromFloat(1) per level: one upload each, one download per level
//   integrate IN OUT  depth (1 x float), color (3 x uint8), intrinsic, extrinsic -> UniformTSDFVolume::Integrate of DeviceImages;
//                     tsdf and weight out
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "constrained_ICP.h"

using namespace open3d;
static FILE *f, *o;
static double rd() { double v; if (fread(&v, 8, 1, f) != 1) std::exit(2); return v; }
static int ri() { return (int)rd(); }
static std::vector<double> rvec() { std::vector<double> v((size_t)rd()); for (auto &x : v) x = rd(); return v; }
static Image rimage()
{
    Image m;
    const int w = ri(), h = ri(), ch = ri(), b = ri();
    m.PrepareImage(w, h, ch, b);
    if (!m.data_.empty() && fread(m.data_.data(), 1, m.data_.size(), f) != m.data_.size()) std::exit(2);
    return m;
}
static void wimage(const Image &m)
{
    const int info[4] = {m.width_, m.height_, m.num_of_channels_, m.bytes_per_channel_};
    fwrite(info, 4, 4, o);
    if (!m.data_.empty()) fwrite(m.data_.data(), 1, m.data_.size(), o);
}
static void wall(const std::vector<Image> &r, const std::vector<double> &results)
{
    const int n = (int)r.size(), nr = (int)results.size();
    fwrite(&n, 4, 1, o);
    for (auto &m : r) wimage(m);
    fwrite(&nr, 4, 1, o);
    if (nr) fwrite(results.data(), 8, (size_t)nr, o);
}

static int cases()
{
    std::vector<Image> r;
    std::vector<double> results;
    const int n_in = ri();
    for (int k = 0; k < n_in; k++) r.push_back(rimage());
    const int nops = ri();
    for (int k = 0; k < nops; k++) {
        const int op = ri();
        switch (op) {
        case 0: { const int s = ri(), t = ri();
                  r.push_back(*CreateFloatImageFromImage(r[s], t == 0 ? Image::ColorToIntensityConversionType::Equal
                                                                      : Image::ColorToIntensityConversionType::Weighted)); break; }
        case 1: { const int s = ri(); const double a = rd(), b = rd(); r.push_back(*ConvertDepthToFloatImage(r[s], a, b)); break; }
        case 2: { const int s = ri(), b = ri();
                  r.push_back(b == 1 ? *CreateImageFromFloatImage<uint8_t>(r[s]) : *CreateImageFromFloatImage<uint16_t>(r[s])); break; }
        case 3: { const int s = ri(), t = ri(); r.push_back(*FilterImage(r[s], (Image::FilterType)t)); break; }
        case 4: { const int s = ri(); const std::vector<double> dx = rvec(), dy = rvec(); r.push_back(*FilterImage(r[s], dx, dy)); break; }
        case 5: { const int s = ri(); const std::vector<double> kk = rvec(); r.push_back(*FilterHorizontalImage(r[s], kk)); break; }
        case 6: { const int s = ri(); r.push_back(*FlipImage(r[s])); break; }
        case 7: { const int s = ri(); r.push_back(*DownsampleImage(r[s])); break; }
        case 8: { const int s = ri(), kk = ri(); r.push_back(*DilateImage(r[s], kk)); break; }
        case 9: { const int s = ri(); const double a = rd(), b = rd(); LinearTransformImage(r[s], a, b); break; }
        case 10: { const int s = ri(); const double a = rd(), b = rd(); ClipIntensityImage(r[s], a, b); break; }
        case 11: { const int s = ri(), levels = ri(), g = ri();
                   for (auto &m : CreateImagePyramid(r[s], (size_t)levels, g != 0)) r.push_back(*m);
                   break; }
        case 12: { const int first = ri(), count = ri(), t = ri();
                   ImagePyramid in;
                   for (int i = 0; i < count; i++) in.push_back(std::make_shared<Image>(r[first + i]));
                   for (auto &m : FilterImagePyramid(in, (Image::FilterType)t)) r.push_back(*m);
                   break; }
        case 13: { const double fx = rd(), fy = rd(), cx = rd(), cy = rd(); const int w = ri(), h = ri();
                   PinholeCameraIntrinsic cam(w, h, fx, fy, cx, cy);
                   r.push_back(*CreateDepthToCameraDistanceMultiplierFloatImage(cam)); break; }
        case 14: { const int s = ri(); const std::vector<double> uv = rvec();
                   std::vector<double> ok, val;
                   for (size_t i = 0; i + 1 < uv.size(); i += 2) {
                       if (!r[s].TestImageBoundary(0.0, 0.0) && r[s].width_ > 0 && r[s].height_ > 0) return 4;
                       auto p = r[s].FloatValueAt(uv[i], uv[i + 1]);
                       ok.push_back(p.first ? 1.0 : 0.0); val.push_back(p.second);
                   }
                   results.insert(results.end(), ok.begin(), ok.end());
                   results.insert(results.end(), val.begin(), val.end());
                   break; }
        case 15: { const int c = ri(), d = ri(), fmt = ri(); const double a = rd(), b = rd(); const bool conv = ri() != 0;
                   std::shared_ptr<RGBDImage> p;
                   const Image before = r[d];
                   switch (fmt) {
                   case 0: p = CreateRGBDImageFromColorAndDepth(r[c], r[d], a, b, conv); break;
                   case 1: p = CreateRGBDImageFromRedwoodFormat(r[c], r[d], conv); break;
                   case 2: p = CreateRGBDImageFromTUMFormat(r[c], r[d], conv); break;
                   case 3: p = CreateRGBDImageFromSUNFormat(r[c], r[d], conv); break;
                   default: p = CreateRGBDImageFromNYUFormat(r[c], r[d], conv); break;
                   }
                   if (before.data_ != r[d].data_) return 5;  // the caller's depth stays as it is
                   r.push_back(p->color_); r.push_back(p->depth_);
                   break; }
        case 16: { const int s = ri(); r.push_back(r[s]); break; }
        default: return 3;
        }
    }
    wall(r, results);
    return 0;
}

static int chain()
{
    const Image color = rimage(), depth = rimage();
    cicp::DeviceImage c(color), d(depth);                    // the two uploads
    std::pair<cicp::DeviceImage, cicp::DeviceImage> rgbd = cicp::DeviceImage::RGBD(c, d, VISMA_ICP_RGBD_TUM);
    std::vector<Image> r;
    for (cicp::DeviceImage &level : rgbd.first.Pyramid(3, true)) {
        cicp::DeviceImage g = level.Filter(Image::FilterType::Gaussian5);
        r.push_back(*g.LinearTransform(4.0, -1.5).ClipIntensity(0.0, 1.0).FromFloat(1).Download());
    }
    r.push_back(*rgbd.second.Download());
    // ... and the RGB-D pyramid of the stock names on the same frame
    auto host = CreateRGBDImageFromTUMFormat(color, depth);
    RGBDImagePyramid pyramid = FilterRGBDImagePyramid(CreateRGBDImagePyramid(*host, 2), Image::FilterType::Gaussian3);
    for (auto &level : pyramid) { r.push_back(level->color_); r.push_back(level->depth_); }
    wall(r, std::vector<double>());
    return 0;
}

static int integrate()
{
    const Image depth = rimage(), color = rimage();
    const double fx = rd(), fy = rd(), cx = rd(), cy = rd();
    Eigen::Matrix4d E;
    for (int i = 0; i < 16; i++) E(i / 4, i % 4) = rd();
    PinholeCameraIntrinsic cam(depth.width_, depth.height_, fx, fy, cx, cy);
    UniformTSDFVolume a(2.0, 32, 0.1, TSDFVolumeColorType::RGB8, Eigen::Vector3d(-1.0, -1.0, -1.0));
    ScalableTSDFVolume s(2.0 / 32, 0.1, TSDFVolumeColorType::RGB8, 8, 4);
    cicp::DeviceImage d(a.Context(), depth), c(a.Context(), color);
    a.Integrate(d, &c, cam, E);
    cicp::DeviceImage ds(s.Context(), depth), cs(s.Context(), color);
    s.Integrate(ds, &cs, cam, E);
    bool refused = false;
    try { a.Integrate(c, &d, cam, E); } catch (const std::invalid_argument &) { refused = true; }      // the formats swapped
    if (!refused) return 6;
    std::vector<float> tsdf, weight;
    std::vector<Eigen::Vector3f> col;
    a.Download(tsdf, weight, col);
    const int n = (int)tsdf.size();
    fwrite(&n, 4, 1, o);
    fwrite(tsdf.data(), 4, tsdf.size(), o);
    fwrite(weight.data(), 4, weight.size(), o);
    auto cloud = s.ExtractPointCloud();
    const int np = (int)cloud->points_.size();
    fwrite(&np, 4, 1, o);
    for (auto &p : cloud->points_) fwrite(p.data(), 8, 3, o);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    f = std::fopen(argv[2], "rb"); o = std::fopen(argv[3], "wb");
    if (!f || !o) return 2;
    int rc = 3;
    try {
        if (!std::strcmp(argv[1], "cases")) rc = cases();
        else if (!std::strcmp(argv[1], "chain")) rc = chain();
        else if (!std::strcmp(argv[1], "integrate")) rc = integrate();
    } catch (const std::exception &e) {
        std::fprintf(stderr, "image_driver: %s\n", e.what());
        rc = 7;
    }
    std::fclose(o);
    return rc;
}

// cloud_distance_driver.cpp -- the cloud-to-cloud and nearest-neighbour distances called the way an Open3D caller
// does, through the stock names of the stand-alone header set and through open3d::cicp::.
// Usage: cloud_distance_driver <in.bin> <out.bin>
//   in : int64 ns, int64 nt, ns*3 doubles (source), nt*3 doubles (target)
//   out: ns doubles each of open3d::ComputePointCloudToPointCloudDistance(source, target),
//        cicp::ComputePointCloudToPointCloudDistance(source, target), open3d::ComputePointCloudNearestNeighborDistance(
//        source), cicp::ComputePointCloudNearestNeighborDistance(source)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "constrained_ICP.h"

using namespace open3d;

static void read_cloud(FILE *f, std::vector<Eigen::Vector3d> &v, int64_t n)
{
    v.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        double p[3];
        if (fread(p, 8, 3, f) != 3) std::exit(2);
        v[(size_t)i] = Eigen::Vector3d(p[0], p[1], p[2]);
    }
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t ns, nt;
    if (fread(&ns, 8, 1, f) != 1 || fread(&nt, 8, 1, f) != 1) return 2;
    PointCloud source, target;
    read_cloud(f, source.points_, ns);
    read_cloud(f, target.points_, nt);
    std::fclose(f);
    std::vector<std::vector<double>> out;
    try {
        out.push_back(ComputePointCloudToPointCloudDistance(source, target));
        out.push_back(cicp::ComputePointCloudToPointCloudDistance(source, target));
        out.push_back(ComputePointCloudNearestNeighborDistance(source));
        out.push_back(cicp::ComputePointCloudNearestNeighborDistance(source));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    for (const auto &d : out)
        if (d.size() != (size_t)ns || (ns > 0 && fwrite(d.data(), 8, d.size(), o) != d.size())) return 4;
    std::fclose(o);
    return 0;
}

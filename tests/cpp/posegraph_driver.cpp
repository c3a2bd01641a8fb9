// posegraph_driver.cpp -- multiway registration called the way an Open3D caller does, against the stand-alone header set.
// Usage: posegraph_driver graph|info <in.bin> <out.bin>
//   graph (no GPU): open3d::GlobalOptimization on a PoseGraph.
//     in : int64 n_nodes, int64 n_edges, int32 method (0 Gauss-Newton, 1 Levenberg-Marquardt), double max_correspondence_distance,
//          edge_prune_threshold, preference_loop_closure, int32 reference_node, n_nodes * 16 doubles (poses, row-major), per
//          edge: int32 source, target, uncertain, 16 doubles transformation, 36 doubles information, double confidence
//     out: double n_edges after the optimisation, n_nodes * 16 doubles, per edge: source, target, uncertain, confidence,
//          the 16 of its transformation and information(0, 0) (doubles); then the same for ONE OptimizePoseGraph of the method on the input (no pruning: the input's edges)
//   info (GPU): cicp::GetInformationMatrixFromPointClouds on one pair and on every edge of a graph.
//     in : int64 n_clouds, per cloud int64 n and n * 3 doubles; double max_correspondence_distance; int64 n_edges, per edge
//          int32 source, target and 16 doubles transformation
//     out: per edge 36 doubles from the batched overload, then per edge 36 doubles from the single call
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "constrained_ICP.h"

using namespace open3d;

static void rd(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) std::exit(2); }
static void wd(FILE *o, double v) { if (fwrite(&v, 8, 1, o) != 1) std::exit(4); }
static Eigen::Matrix4d read4(FILE *f)
{
    double p[16];
    rd(f, p, sizeof(p));
    Eigen::Matrix4d T;
    for (int i = 0; i < 16; i++) T(i / 4, i % 4) = p[i];
    return T;
}

static void write_graph(FILE *o, const PoseGraph &g)
{
    wd(o, (double)g.edges_.size());
    for (const PoseGraphNode &n : g.nodes_)
        for (int i = 0; i < 16; i++) wd(o, n.pose_(i / 4, i % 4));
    for (const PoseGraphEdge &e : g.edges_) {
        wd(o, e.source_node_id_); wd(o, e.target_node_id_); wd(o, e.uncertain_ ? 1.0 : 0.0); wd(o, e.confidence_);
        for (int i = 0; i < 16; i++) wd(o, e.transformation_(i / 4, i % 4));
        wd(o, e.information_(0, 0));
    }
}

int main(int argc, char **argv)
{
    if (argc != 4) return 1;
    FILE *f = std::fopen(argv[2], "rb"), *o = std::fopen(argv[3], "wb");
    if (!f || !o) return 2;
    if (!std::strcmp(argv[1], "graph")) {
        int64_t nn, ne; int32_t method, ref; double op[3];
        rd(f, &nn, 8); rd(f, &ne, 8); rd(f, &method, 4); rd(f, op, 24); rd(f, &ref, 4);
        PoseGraph g;
        for (int64_t i = 0; i < nn; i++) g.nodes_.push_back(PoseGraphNode(read4(f)));
        for (int64_t e = 0; e < ne; e++) {
            int32_t id[3]; rd(f, id, 12);
            const Eigen::Matrix4d T = read4(f);
            double I[36], conf; rd(f, I, sizeof(I)); rd(f, &conf, 8);
            Eigen::Matrix6d info;
            for (int i = 0; i < 36; i++) info(i / 6, i % 6) = I[i];
            g.edges_.push_back(PoseGraphEdge(id[0], id[1], T, info, id[2] != 0, conf));
        }
        const GlobalOptimizationOption option(op[0], op[1], op[2], ref);
        const GlobalOptimizationConvergenceCriteria criteria;
        const GlobalOptimizationGaussNewton gn;
        const GlobalOptimizationLevenbergMarquardt lm;
        const GlobalOptimizationMethod &m = method == 0 ? static_cast<const GlobalOptimizationMethod &>(gn) : lm;
        PoseGraph whole = g, once = g;
        GlobalOptimization(whole, m, criteria, option);
        write_graph(o, whole);
        m.OptimizePoseGraph(once, criteria, option);
        write_graph(o, once);
    } else if (!std::strcmp(argv[1], "info")) {
        int64_t nc;
        rd(f, &nc, 8);
        std::vector<PointCloud> clouds((size_t)nc);
        for (int64_t c = 0; c < nc; c++) {
            int64_t n; rd(f, &n, 8);
            clouds[(size_t)c].points_.resize((size_t)n);
            for (int64_t i = 0; i < n; i++) { double p[3]; rd(f, p, 24); clouds[(size_t)c].points_[(size_t)i] = Eigen::Vector3d(p[0], p[1], p[2]); }
        }
        double max_dist; int64_t ne;
        rd(f, &max_dist, 8); rd(f, &ne, 8);
        PoseGraph g;
        g.nodes_.resize((size_t)nc);
        for (int64_t e = 0; e < ne; e++) {
            int32_t id[2]; rd(f, id, 8);
            g.edges_.push_back(PoseGraphEdge(id[0], id[1], read4(f)));
        }
        std::vector<const PointCloud *> ptr;
        for (const PointCloud &c : clouds) ptr.push_back(&c);
        cicp::GetInformationMatrixFromPointClouds(g, ptr, max_dist);
        for (const PoseGraphEdge &e : g.edges_)
            for (int i = 0; i < 36; i++) wd(o, e.information_(i / 6, i % 6));
        for (const PoseGraphEdge &e : g.edges_) {
            const Eigen::Matrix6d G = GetInformationMatrixFromPointClouds(clouds[(size_t)e.source_node_id_], clouds[(size_t)e.target_node_id_],
                                                                          max_dist, e.transformation_);
            for (int i = 0; i < 36; i++) wd(o, G(i / 6, i % 6));
        }
    } else {
        return 1;
    }
    std::fclose(o);
    return 0;
}

// kdtree_driver.cpp -- open3d::KDTreeFlann of the stand-alone header set (Core/Geometry/KDTreeFlann.h) and the batch overloads
// of open3d::cicp, for tests/test_kdtree_shim.py.  in.bin: n, the points, nq, the queries, knn, radius, max_nn.  out.bin,
// all doubles: for a tree on a PointCloud (this thread's context) and one on a TriangleMesh (a context of the driver's), per
// query the three Search kinds (k, the indices, the distances), then the three batch overloads; then the return values of the
// degenerate calls.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <Core/Core.h>

#include "visma_icp_open3d.hpp"

using namespace open3d;

static void rd(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) std::exit(2); }
static void wd(FILE *o, double v) { fwrite(&v, 8, 1, o); }
static std::vector<Eigen::Vector3d> points(FILE *f)
{
    int n; rd(f, &n, 4);
    std::vector<Eigen::Vector3d> v((size_t)n);
    for (auto &p : v) { double x[3]; rd(f, x, 24); p = Eigen::Vector3d(x[0], x[1], x[2]); }
    return v;
}
static void wlist(FILE *o, int k, const std::vector<int> &idx, const std::vector<double> &d2)
{
    wd(o, (double)k);
    if (k < 0) return;
    if ((size_t)k != idx.size() || (size_t)k != d2.size()) std::exit(4);     // the vectors are resized to the count
    for (int i : idx) wd(o, (double)i);
    for (double d : d2) wd(o, d);
}

static void searches(FILE *o, const KDTreeFlann &tree, const std::vector<Eigen::Vector3d> &queries, int knn, double radius, int max_nn)
{
    std::vector<int> idx, cnt; std::vector<double> d2; std::vector<int64_t> off;
    for (auto &q : queries) {
        wlist(o, tree.Search(q, KDTreeSearchParamKNN(knn), idx, d2), idx, d2);
        wlist(o, tree.Search(q, KDTreeSearchParamRadius(radius), idx, d2), idx, d2);
        wlist(o, tree.Search(q, KDTreeSearchParamHybrid(radius, max_nn), idx, d2), idx, d2);
    }
    wd(o, (double)cicp::KDTreeSearchKNN(tree, queries, knn, idx, d2, cnt));
    for (int c : cnt) wd(o, (double)c);
    for (int i : idx) wd(o, (double)i);
    for (double d : d2) wd(o, d);
    wd(o, (double)cicp::KDTreeSearchHybrid(tree, queries, radius, max_nn, idx, d2, cnt));
    for (int c : cnt) wd(o, (double)c);
    for (int i : idx) wd(o, (double)i);
    for (double d : d2) wd(o, d);
    wd(o, (double)cicp::KDTreeSearchRadius(tree, queries, radius, off, idx, d2));
    for (int64_t v : off) wd(o, (double)v);
    for (int i : idx) wd(o, (double)i);
    for (double d : d2) wd(o, d);
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = std::fopen(argv[1], "rb"), *o = std::fopen(argv[2], "wb");
    if (!f || !o) return 2;
    PointCloud pc; TriangleMesh mesh;
    pc.points_ = points(f);
    mesh.vertices_ = pc.points_;
    const std::vector<Eigen::Vector3d> queries = points(f);
    int knn, max_nn; double radius;
    rd(f, &knn, 4); rd(f, &radius, 8); rd(f, &max_nn, 4);
    {
        KDTreeFlann tree(pc);                                       // this thread's context
        searches(o, tree, queries, knn, radius, max_nn);
    }
    visma_icp_ctx *ctx = nullptr;
    if (visma_icp_create(&ctx, 0) != VISMA_ICP_OK) return 3;
    {
        KDTreeFlann tree(ctx);
        if (!tree.SetGeometry(mesh)) return 5;                      // by its vertices
        searches(o, tree, queries, knn, radius, max_nn);
        // the degenerate calls
        std::vector<int> idx(7, 1), cnt; std::vector<double> d2(7, 1.0); std::vector<int64_t> off;
        const Eigen::Vector3d q = queries[0];
        KDTreeFlann empty;
        wd(o, empty.SearchKNN(q, knn, idx, d2)); wd(o, empty.SearchRadius(q, radius, idx, d2)); wd(o, empty.SearchHybrid(q, radius, max_nn, idx, d2));
        wd(o, cicp::KDTreeSearchKNN(empty, queries, knn, idx, d2, cnt)); wd(o, cicp::KDTreeSearchRadius(empty, queries, radius, off, idx, d2));
        wd(o, tree.SearchKNN(q, -1, idx, d2)); wd(o, tree.SearchHybrid(q, radius, -1, idx, d2));
        wd(o, cicp::KDTreeSearchKNN(tree, queries, -1, idx, d2, cnt)); wd(o, cicp::KDTreeSearchHybrid(tree, queries, radius, -1, idx, d2, cnt));
        wd(o, (double)idx.size());                                  // 7: a call that returns -1 leaves the vectors alone
        wd(o, tree.SearchKNN(q, 0, idx, d2)); wd(o, (double)idx.size());
        wd(o, tree.SearchHybrid(q, radius, 0, idx, d2)); wd(o, tree.SearchRadius(q, 0.0, idx, d2));
        wlist(o, tree.SearchRadius(q, -radius, idx, d2), idx, d2);  // a negative radius: the answer of its absolute value
        wlist(o, tree.SearchHybrid(q, -radius, max_nn, idx, d2), idx, d2);
        wlist(o, tree.SearchKNN(q, (int)pc.points_.size() + 5, idx, d2), idx, d2);      // knn > n: the list holds n
        Eigen::MatrixXd two(2, 4), three(3, (Eigen::Index)pc.points_.size());
        two.setZero();
        for (size_t j = 0; j < pc.points_.size(); j++) three.col((Eigen::Index)j) = pc.points_[j];
        KDTreeFlann m(ctx);
        wd(o, m.SetMatrixData(two) ? 1.0 : 0.0); wd(o, m.SearchKNN(q, knn, idx, d2));
        wd(o, m.SetMatrixData(three) ? 1.0 : 0.0);
        wlist(o, m.SearchKNN(q, knn, idx, d2), idx, d2);
        wd(o, m.SetGeometry(PointCloud()) ? 1.0 : 0.0); wd(o, m.SearchKNN(q, knn, idx, d2));     // no data: an empty tree again
        Eigen::VectorXd q4(4); q4.setZero();
        wd(o, tree.SearchKNN(q4, knn, idx, d2));                    // a query that has not three rows
    }
    visma_icp_destroy(ctx);
    std::fclose(o);
    return 0;
}

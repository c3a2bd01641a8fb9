// render.hip -- the off-screen mesh renderer (visma_icp_render, visma_icp_render_edges): a resident TriangleMesh, a pinhole
// camera and a pose in; a depth image, the visible triangle per pixel, a mask and a depth-edge image out, all resident
// Images.  The counterpart of the reference's OpenGL renderer (render/renderer.cpp, edge_detection.frag) as plain compute.
// The arithmetic is render_math.hpp's, shared with visma_icp_render_host: f64, unfused, one written order.
//
//   rn_vertices     P = R X + t per vertex into a camera-space scratch
//   rn_setup        per triangle: the three edge normals, det and the screen box it is drawn in
//   rn_cover_small  one lane per triangle whose box has at most kSmallArea pixels (a fused TSDF mesh: hundreds of
//                   thousands of triangles of about a pixel each), the box walked by that lane
//   rn_cover_large  the other triangles, cut into chunks of kChunk box pixels through ONE ordered compaction (compact.h:
//                   a triangle emits ceil(area / kChunk) items); one workgroup per item, lanes on neighbouring pixels of
//                   a row.  A CAD model that fills a 640 x 480 frame with a few triangles becomes 75 items per triangle
//   rn_resolve      the key buffer into the depth, index and mask images
//   rn_edges        the edge image of a depth image
//
// Coverage: 64-bit integer atomicMin on a w x h key buffer behind a plain-load pre-test (as kernels.hip's winner search
// does in 32 bits).  The key (fp32 depth bits << 32 | triangle) makes the minimum the nearest triangle, the lowest index
// among equals; an integer minimum does not depend on arrival order, so the pictures do not depend on scheduling.  No
// floating-point atomic anywhere.  The pre-test reads a value that only ever falls: a stale read costs one atomic, never
// a result.  Lanes of the large path hit 64 consecutive keys (512 contiguous bytes per wave instruction); lanes of the
// small path scatter, one or a few atomics each.  The binned alternative (triangles to screen tiles, an LDS z-buffer per
// tile) trades the atomics for a sort of triangle-tile pairs and a second read of every set-up triangle; it was not
// built, and neither was measured against the other.
#include "compact.h"
#include "kernels.h"
#include "render_math.hpp"

#include <memory>

namespace visma {

namespace {

constexpr int kSmallArea = 64;                           // box pixels up to which one lane walks a triangle
constexpr int kChunk = 16 * kThreads;                    // box pixels per item of the large path

struct RenderPose { double m[12]; };

__global__ __launch_bounds__(kThreads) void rn_vertices(const double *__restrict__ v, long long nv, RenderPose T, double *__restrict__ cam)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < nv; i += (long long)gridDim.x * kThreads) {
        const double X[3] = {v[3 * i], v[3 * i + 1], v[3 * i + 2]};
        double P[3];
        render_camera_point(T.m, X, P);
        cam[3 * i] = P[0]; cam[3 * i + 1] = P[1]; cam[3 * i + 2] = P[2];
    }
}

__global__ __launch_bounds__(kThreads) void rn_setup(const double *__restrict__ cam, const int *__restrict__ tri, long long nt, RenderCamera c,
                                                     RenderTri *__restrict__ out)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < nt; i += (long long)gridDim.x * kThreads) {
        const int a = tri[3 * i], b = tri[3 * i + 1], d = tri[3 * i + 2];   // (inside [0, nv): trimesh_device_create checked)
        const double A[3] = {cam[3 * (long long)a], cam[3 * (long long)a + 1], cam[3 * (long long)a + 2]};
        const double B[3] = {cam[3 * (long long)b], cam[3 * (long long)b + 1], cam[3 * (long long)b + 2]};
        const double C[3] = {cam[3 * (long long)d], cam[3 * (long long)d + 1], cam[3 * (long long)d + 2]};
        RenderTri t;
        render_setup(A, B, C, c, t);
        out[i] = t;
    }
}

__device__ __forceinline__ void rn_offer(unsigned long long *keys, long long p, unsigned long long key)
{
    if (key != kRenderNoKey && key < keys[p]) atomicMin(&keys[p], key);
}

__global__ __launch_bounds__(kThreads) void rn_cover_small(const RenderTri *__restrict__ tris, long long nt, RenderCamera c,
                                                           unsigned long long *keys)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < nt; i += (long long)gridDim.x * kThreads) {
        const RenderTri t = tris[i];
        const long long area = render_box_area(t);
        if (area == 0 || area > kSmallArea) continue;
        for (int y = t.y0; y <= t.y1; y++)
            for (int x = t.x0; x <= t.x1; x++) rn_offer(keys, (long long)y * c.w + x, render_key(t, c, x, y, (unsigned)i));
    }
}

// the items of the large path: (triangle, chunk of its box)
struct LargeItems {
    const RenderTri *tris;
    int *item_tri, *item_chunk;
    __device__ int count(long long i) const
    {
        const long long area = render_box_area(tris[i]);
        return area > kSmallArea ? (int)((area + kChunk - 1) / kChunk) : 0;
    }
    __device__ void emit(long long i, long long row) const
    {
        const int n = count(i);
        for (int k = 0; k < n; k++) { item_tri[row + k] = (int)i; item_chunk[row + k] = k; }
    }
};

__global__ __launch_bounds__(kThreads) void rn_cover_large(const RenderTri *__restrict__ tris, const int *__restrict__ item_tri,
                                                           const int *__restrict__ item_chunk, long long items, RenderCamera c,
                                                           unsigned long long *keys)
{
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int i = item_tri[it];
        const RenderTri t = tris[i];
        const int bw = t.x1 - t.x0 + 1;
        const long long area = render_box_area(t), first = (long long)item_chunk[it] * kChunk;
        for (int k = 0; k < kChunk / kThreads; k++) {
            const long long q = first + (long long)k * kThreads + threadIdx.x;
            if (q >= area) break;
            const int y = t.y0 + (int)(q / bw), x = t.x0 + (int)(q % bw);
            rn_offer(keys, (long long)y * c.w + x, render_key(t, c, x, y, (unsigned)i));
        }
    }
}

__global__ __launch_bounds__(kThreads) void rn_resolve(const unsigned long long *__restrict__ keys, const RenderTri *__restrict__ tris,
                                                       RenderCamera c, int encoding, float *__restrict__ depth, int32_t *__restrict__ index,
                                                       uint8_t *__restrict__ mask)
{
    const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (p >= (long long)c.w * c.h) return;
    const int y = (int)(p / c.w), x = (int)(p - (long long)y * c.w);
    float d;
    int32_t idx;
    uint8_t m;
    render_resolve(keys[p], tris, c, x, y, encoding, &d, &idx, &m);
    if (depth) depth[p] = d;
    if (index) index[p] = idx;
    if (mask) mask[p] = m;
}

__global__ __launch_bounds__(kThreads) void rn_edges(const float *__restrict__ depth, int w, int h, uint8_t *__restrict__ out)
{
    const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (p >= (long long)w * h) return;
    const int y = (int)(p / w), x = (int)(p - (long long)y * w);
    out[p] = render_edge(depth, w, h, x, y);
}

inline unsigned pixel_blocks(long long n) { return (unsigned)((n + kThreads - 1) / kThreads); }

struct ImageHolder {
    ImageDevice *p = nullptr;
    ~ImageHolder() { image_device_destroy(p); }
    ImageDevice *release() { ImageDevice *r = p; p = nullptr; return r; }
};

}  // namespace

// what a render works in, one per context, grow-only.  Every call returns with the stream idle
struct RenderScratch {
    DeviceBuf<double> cam;
    DeviceBuf<RenderTri> tris;
    DeviceBuf<unsigned long long> keys;
    DeviceBuf<int> item_tri, item_chunk;
    Compactor comp;
};

RenderScratch *render_scratch_create() { return new RenderScratch; }
void render_scratch_destroy(RenderScratch *W) { delete W; }

hipError_t render_device_render(RenderScratch *W, const TriMeshDevice *M, const RenderCamera &c, const double E[16], int encoding,
                                hipStream_t stream, ImageDevice **depth, ImageDevice **index, ImageDevice **mask)
{
    if (depth) *depth = nullptr;
    if (index) *index = nullptr;
    if (mask) *mask = nullptr;
    int64_t nv = 0, nt = 0;
    const double *v = nullptr;
    const int *tri = nullptr;
    trimesh_device_arrays(M, &nv, &nt, &v, &tri);
    const long long px = (long long)c.w * c.h;
    ImageHolder D, I, K;
    if (depth) VISMA_TRY(image_device_alloc(c.w, c.h, 1, 4, false, &D.p));
    if (index) VISMA_TRY(image_device_alloc(c.w, c.h, 1, 4, true, &I.p));
    if (mask) VISMA_TRY(image_device_alloc(c.w, c.h, 1, 1, false, &K.p));
    DEV_RESERVE(W->keys, (size_t)px);
    DEV_RESERVE(W->cam, 3 * (size_t)nv);
    DEV_RESERVE(W->tris, (size_t)nt);
    VISMA_TRY(hipMemsetAsync(W->keys.get(), 0xff, sizeof(unsigned long long) * (size_t)px, stream));
    if (nt > 0) {
        RenderPose T;
        for (int k = 0; k < 12; k++) T.m[k] = E[k];
        rn_vertices<<<capped_blocks(nv), kThreads, 0, stream>>>(v, nv, T, W->cam.get());
        rn_setup<<<capped_blocks(nt), kThreads, 0, stream>>>(W->cam.get(), tri, nt, c, W->tris.get());
        VISMA_TRY(hipGetLastError());
        LargeItems src{W->tris.get(), nullptr, nullptr};
        long long items = 0;
        VISMA_TRY(compact_count(W->comp, src, nt, stream, &items));
        rn_cover_small<<<capped_blocks(nt), kThreads, 0, stream>>>(W->tris.get(), nt, c, W->keys.get());
        if (items > 0) {
            DEV_RESERVE(W->item_tri, (size_t)items);
            DEV_RESERVE(W->item_chunk, (size_t)items);
            src.item_tri = W->item_tri.get(); src.item_chunk = W->item_chunk.get();
            VISMA_TRY(compact_write(W->comp, src, nt, stream));
            const unsigned blocks = (unsigned)std::min<long long>(items, 1 << 20);
            rn_cover_large<<<blocks, kThreads, 0, stream>>>(W->tris.get(), W->item_tri.get(), W->item_chunk.get(), items, c, W->keys.get());
        }
        VISMA_TRY(hipGetLastError());
    }
    rn_resolve<<<pixel_blocks(px), kThreads, 0, stream>>>(W->keys.get(), W->tris.get(), c, encoding,
                                                         D.p ? (float *)image_device_pixels_rw(D.p) : nullptr,
                                                         I.p ? (int32_t *)image_device_pixels_rw(I.p) : nullptr,
                                                         K.p ? (uint8_t *)image_device_pixels_rw(K.p) : nullptr);
    VISMA_TRY(hipGetLastError());
    VISMA_TRY(hipStreamSynchronize(stream));
    if (depth) *depth = D.release();
    if (index) *index = I.release();
    if (mask) *mask = K.release();
    return hipSuccess;
}

// `depth`: 1 x float (the caller checked)
hipError_t render_device_edges(const ImageDevice *depth, hipStream_t stream, ImageDevice **out)
{
    *out = nullptr;
    int w, h, ch, bpc;
    image_device_info(depth, &w, &h, &ch, &bpc);
    ImageHolder O;
    VISMA_TRY(image_device_alloc(w, h, 1, 1, false, &O.p));
    const long long px = (long long)w * h;
    if (px > 0) {
        rn_edges<<<pixel_blocks(px), kThreads, 0, stream>>>((const float *)image_device_pixels(depth), w, h, (uint8_t *)image_device_pixels_rw(O.p));
        VISMA_TRY(hipGetLastError());
    }
    VISMA_TRY(hipStreamSynchronize(stream));
    *out = O.release();
    return hipSuccess;
}

}  // namespace visma

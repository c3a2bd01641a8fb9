// compact.h -- count, scan, write: the ordered compaction tsdf.hip (extraction, frame clouds) and colormap.hip (the visible
// vertex lists) share.  The kernels and the two passes; each including file gets its own copy (unnamed namespace).  The
// buffers they work in are dev_mem.h's Compactor.
#pragma once

#include "dev_mem.h"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace visma {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;                         // memory-bound passes: the grid is capped and strides
constexpr int kScanThreads = 1024;

inline unsigned capped_blocks(long long n) { return (unsigned)std::min<long long>((n + kThreads - 1) / kThreads, kMaxBlocks); }

// ---- count, scan, write: an ordered compaction over n items in tiles of kThreads ----
// A Source has  __device__ int count(long long i) const  (rows item i emits) and
//               __device__ void emit(long long i, long long row) const  (writes them at row, row + 1, ...).
template <class Source>
__global__ __launch_bounds__(kThreads) void count_kernel(Source s, long long n, long long tiles, int *tile_count)
{
    __shared__ int wave_sum[kThreads / 64];
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long i = tile * kThreads + threadIdx.x;
        int c = i < n ? s.count(i) : 0;
        for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
        if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) {
            int t = 0;
            for (int k = 0; k < kThreads / 64; k++) t += wave_sum[k];
            tile_count[tile] = t;
        }
        __syncthreads();
    }
}

// exclusive scan of tile_count[0 .. tiles) into tile_offset, the total into *total: ONE workgroup, chunk by chunk with a carry
__global__ __launch_bounds__(kScanThreads) void scan_kernel(const int *tile_count, long long tiles, long long *tile_offset, long long *total)
{
    __shared__ long long buf[kScanThreads];
    __shared__ long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (long long at = 0; at < tiles; at += kScanThreads) {
        const long long i = at + threadIdx.x;
        const long long v = i < tiles ? (long long)tile_count[i] : 0;
        buf[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < kScanThreads; o <<= 1) {                     // Hillis-Steele, inclusive
            const long long add = (int)threadIdx.x >= o ? buf[threadIdx.x - o] : 0;
            __syncthreads();
            buf[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < tiles) tile_offset[i] = carry + buf[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == kScanThreads - 1) carry += buf[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

template <class Source>
__global__ __launch_bounds__(kThreads) void write_kernel(Source s, long long n, long long tiles, const long long *tile_offset)
{
    __shared__ int buf[kThreads];
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long i = tile * kThreads + threadIdx.x;
        const int c = i < n ? s.count(i) : 0;
        buf[threadIdx.x] = c;
        __syncthreads();
        for (int o = 1; o < kThreads; o <<= 1) {
            const int add = (int)threadIdx.x >= o ? buf[threadIdx.x - o] : 0;
            __syncthreads();
            buf[threadIdx.x] += add;
            __syncthreads();
        }
        if (c > 0) s.emit(i, tile_offset[tile] + (long long)(buf[threadIdx.x] - c));
        __syncthreads();
    }
}

// the count pass and the scan over c's buffers (dev_mem.h: grow-only); *rows on the host (one wait)
template <class Source>
hipError_t compact_count(Compactor &c, const Source &s, long long n, hipStream_t stream, long long *rows)
{
    *rows = 0;
    if (n <= 0) return hipSuccess;                       // nothing is launched over nothing
    const long long tiles = (n + kThreads - 1) / kThreads;
    hipError_t e = c.ensure(tiles);
    if (e != hipSuccess) return e;
    count_kernel<Source><<<(unsigned)std::min<long long>(tiles, kMaxBlocks), kThreads, 0, stream>>>(s, n, tiles, c.tile_count);
    scan_kernel<<<1, kScanThreads, 0, stream>>>(c.tile_count, tiles, c.tile_offset, c.total);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(rows, c.total, sizeof(long long), hipMemcpyDeviceToHost, stream);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(stream);
}
// ... and the write pass behind it (the Source now holds its output pointers)
template <class Source>
hipError_t compact_write(const Compactor &c, const Source &s, long long n, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const long long tiles = (n + kThreads - 1) / kThreads;
    write_kernel<Source><<<(unsigned)std::min<long long>(tiles, kMaxBlocks), kThreads, 0, stream>>>(s, n, tiles, c.tile_offset);
    return hipGetLastError();
}

}  // namespace

}  // namespace visma

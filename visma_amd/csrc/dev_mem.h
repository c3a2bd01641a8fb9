// dev_mem.h -- the device allocator under every DevBuf<T> (dev_buf.h) outside the engine, and what turns a buffer's return
// code into a hipError_t.  dev_buf.h itself stays free of HIP (its stand-alone driver runs it against malloc); this header is
// where the two meet.
#pragma once

#include "dev_buf.h"

#include <hip/hip_runtime.h>

namespace visma {

using drv::DevBuf;

// hipMalloc / hipFree.  A request for zero bytes gives a real block (one byte): reset(0) leaves a pointer that a launch, a
// copy or a view may be handed.  A failure leaves no sticky error behind and *p == nullptr.
inline int device_alloc(void **p, size_t bytes)
{
    const hipError_t e = hipMalloc(p, bytes ? bytes : 1);
    if (e != hipSuccess) { *p = nullptr; (void)hipGetLastError(); }
    return (int)e;
}
inline void device_free(void *p) { (void)hipFree(p); }
inline drv::RawAlloc device_memory() { return drv::RawAlloc{&device_alloc, &device_free}; }

// a DevBuf bound to device_memory() from its declaration on: what members, arrays of members and locals are declared as
template <class T>
struct DeviceBuf : DevBuf<T> {
    DeviceBuf() : DevBuf<T>(device_memory()) {}
};

// inside a function that returns hipError_t: grow-only, and free-then-allocate-exactly
#define DEV_RESERVE(buf, count) do { if (int rc_ = (buf).reserve(count)) return (hipError_t)rc_; } while (0)
#define DEV_RESET(buf, count) do { if (int rc_ = (buf).reset(count)) return (hipError_t)rc_; } while (0)

// What compact.h's ordered compaction works in, grow-only.  The kernels and the two passes are compact.h's (a copy per
// including file); the buffers stand here, in the named namespace, so that an object two files share holds one by value.
struct Compactor {
    DeviceBuf<int> tile_count;
    DeviceBuf<long long> tile_offset, total;
    hipError_t ensure(long long tiles)
    {
        DEV_RESERVE(total, 1);
        DEV_RESERVE(tile_count, (size_t)tiles);
        DEV_RESERVE(tile_offset, (size_t)tiles);
        return hipSuccess;
    }
};

}  // namespace visma

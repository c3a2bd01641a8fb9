// dev_buf.h -- who owns the engine's device and pinned memory: one pool (DevPool) and one owning buffer type (DevBuf<T>).
// Host-only, no HIP header: the raw allocator is a pair of plain functions, so tests/cpp/dev_buf_driver.cpp runs all of
// it against a malloc-backed fake.
//
// The invariant every caller relies on: after a FAILED reserve / reset the buffer is empty (get() == nullptr,
// count() == 0), so the next call with the same size allocates again instead of trusting a capacity that no memory backs.
#pragma once
#include <algorithm>
#include <cstddef>
#include <unordered_map>
#include <utility>
#include <vector>

namespace visma {
namespace drv {

// alloc: 0 and the block in *p, or the runtime's error code (never 0) and *p == nullptr.  The engine passes thin wrappers
// of hipMalloc / hipFree (device memory) and of hipHostMalloc / hipHostFree (pinned host memory, never pooled).
struct RawAlloc {
    int (*alloc)(void **p, size_t bytes);
    void (*free)(void *p);
};

// Cloud-sized device buffers are recycled: a registration after another of about the same size (every caller's loop)
// re-uses them instead of paying a free + an allocation (a device sync and ~0.5 ms per 100 MB).
class DevPool {
public:
    explicit DevPool(const RawAlloc &raw) : raw_(raw) {}
    DevPool(const DevPool &) = delete;
    DevPool &operator=(const DevPool &) = delete;
    ~DevPool() { trim(0); }                                   // (its buffers went first: nothing is live any more)
    const RawAlloc &raw() const { return raw_; }
    size_t free_blocks() const { return free_.size(); }
    size_t live_blocks() const { return live_.size(); }

    int alloc(void **p, size_t bytes)
    {
        *p = nullptr;
        bytes = std::max<size_t>(bytes, 256);
        int best = -1;
        for (int i = 0; i < (int)free_.size(); i++)
            if (free_[i].second >= bytes && free_[i].second <= 2 * bytes + (1u << 20) &&
                (best < 0 || free_[i].second < free_[best].second))
                best = i;
        if (best >= 0) {
            *p = free_[best].first;
            live_[*p] = free_[best].second;
            free_.erase(free_.begin() + best);
            return 0;
        }
        size_t got = bytes + bytes / 8;                        // a little head-room: the next cloud is rarely the same size
        if (raw_.alloc(p, got) != 0) {
            trim(0);                                           // give the recycled blocks back and try the exact size
            got = bytes;
            const int rc = raw_.alloc(p, got);
            if (rc != 0) { *p = nullptr; return rc; }
        }
        live_[*p] = got;
        return 0;
    }
    void free(void *p)
    {
        auto it = live_.find(p);
        if (it == live_.end()) return;                         // (not one of ours: never happens through DevBuf)
        free_.push_back({p, it->second});
        live_.erase(it);
        trim(10);
    }
    void trim(size_t keep)                                     // the oldest free blocks go first
    {
        while (free_.size() > keep) {
            raw_.free(free_.front().first);
            free_.erase(free_.begin());
        }
    }

private:
    RawAlloc raw_;
    std::unordered_map<void *, size_t> live_;
    std::vector<std::pair<void *, size_t>> free_;
};

// An owning, typed, move-only buffer.  Whether it is pooled is decided once, by what it is constructed with.
// count() is the number of elements asked for; `slack` elements beyond them are allocated but not counted (rows that
// kernels read past the end of).
template <class T>
class DevBuf {
public:
    explicit DevBuf(DevPool &pool) : raw_(pool.raw()), pool_(&pool) {}
    explicit DevBuf(const RawAlloc &raw) : raw_(raw) {}
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : raw_(o.raw_), pool_(o.pool_), p_(o.p_), n_(o.n_), bytes_(o.bytes_) { o.forget(); }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            raw_ = o.raw_; pool_ = o.pool_; p_ = o.p_; n_ = o.n_; bytes_ = o.bytes_;
            o.forget();
        }
        return *this;
    }
    ~DevBuf() { release(); }

    // grow-only: nothing happens while n <= count().  *grew is SET when the buffer was reallocated (never cleared: the
    // buffers of a group share one flag).  Returns 0 or the allocator's error code; empty after an error.
    int reserve(size_t n, bool *grew = nullptr, size_t slack = 0)
    {
        if (n <= n_) return 0;
        if (grew) *grew = true;
        return reset(n, slack);
    }
    // free, then allocate exactly n (+ slack) elements -- through the pool's rules when pooled
    int reset(size_t n, size_t slack = 0)
    {
        release();
        const size_t bytes = (n + slack) * sizeof(T);
        void *p = nullptr;
        const int rc = pool_ ? pool_->alloc(&p, bytes) : raw_.alloc(&p, bytes);
        if (rc != 0) return rc;
        p_ = static_cast<T *>(p); n_ = n; bytes_ = bytes;
        return 0;
    }
    // takes over n elements that the raw allocator's own allocate call made elsewhere (never a pooled buffer)
    void adopt(T *p, size_t n)
    {
        release();
        if (p) { p_ = p; n_ = n; bytes_ = n * sizeof(T); }
    }
    void release()
    {
        if (p_) { if (pool_) pool_->free(p_); else raw_.free(p_); }
        forget();
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    size_t count() const { return n_; }
    size_t bytes() const { return bytes_; }                    // (count() + slack) * sizeof(T)

private:
    void forget() { p_ = nullptr; n_ = 0; bytes_ = 0; }
    RawAlloc raw_;
    DevPool *pool_ = nullptr;
    T *p_ = nullptr;
    size_t n_ = 0, bytes_ = 0;
};

}  // namespace drv
}  // namespace visma

// dev_buf_driver.cpp -- DevPool and DevBuf<T> (visma_amd/csrc/dev_buf.h) against a malloc-backed allocator that counts
// its live blocks, records every size it was asked for and fails the k-th request on demand.  A program of its own: no
// library, no HIP, no GPU.  Built with -fsanitize=address,undefined (build_dev_buf.py): a block freed twice or written
// past its end aborts the run, and the leak check at exit is part of the verdict.
#include "dev_buf.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

using visma::drv::DevBuf;
using visma::drv::DevPool;
using visma::drv::RawAlloc;

namespace {

struct Fake {
    std::set<void *> live;
    std::vector<size_t> asked;       // every request, failed ones included
    int fail_at = 0, fail_n = 1;     // fail_at > 0: from the fail_at-th request from now on, fail_n requests in a row fail
    int frees = 0;
    bool bad_free = false;
};
Fake g_dev, g_pin;

int fake_alloc(Fake &f, void **p, size_t bytes)
{
    f.asked.push_back(bytes);
    *p = nullptr;
    if (f.fail_at > 1) f.fail_at--;
    else if (f.fail_at == 1) {                                 // (2: hipErrorOutOfMemory's value; any non-zero code does)
        if (--f.fail_n == 0) { f.fail_at = 0; f.fail_n = 1; }
        return 2;
    }
    *p = std::malloc(bytes ? bytes : 1);
    std::memset(*p, 0xA5, bytes);                              // (touch every byte: ASan sees a block shorter than asked for)
    f.live.insert(*p);
    return 0;
}
void fake_free(Fake &f, void *p)
{
    f.frees++;
    if (!f.live.erase(p)) { f.bad_free = true; return; }      // freed twice, or never ours
    std::free(p);
}
int dev_alloc(void **p, size_t b) { return fake_alloc(g_dev, p, b); }
void dev_free(void *p) { fake_free(g_dev, p); }
int pin_alloc(void **p, size_t b) { return fake_alloc(g_pin, p, b); }
void pin_free(void *p) { fake_free(g_pin, p); }
const RawAlloc kDev{&dev_alloc, &dev_free}, kPin{&pin_alloc, &pin_free};

int g_failed = 0, g_cases = 0;
bool g_ok = true;
#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) { std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); g_ok = false; } \
    } while (0)

void begin()
{
    g_ok = true;
    CHECK(g_dev.live.empty() && g_pin.live.empty());          // (every case starts, and so the one before ended, with nothing live)
    g_dev = Fake();
    g_pin = Fake();
}
void end(const char *name)
{
    CHECK(g_dev.live.empty() && g_pin.live.empty());
    CHECK(!g_dev.bad_free && !g_pin.bad_free);
    g_cases++;
    if (!g_ok) g_failed++;
    std::printf("%s: %s\n", name, g_ok ? "ok" : "FAILED");
}

constexpr size_t MiB = 1u << 20;

void reserve_grows_only()
{
    begin();
    {
        DevBuf<double> b(kDev);
        CHECK(!b && b.get() == nullptr && b.count() == 0 && b.bytes() == 0);
        bool grew = false;
        CHECK(b.reserve(0, &grew) == 0 && !grew && g_dev.asked.empty());      // nothing asked, nothing made
        CHECK(b.reserve(100, &grew) == 0 && grew && b.count() == 100 && b.bytes() == 800);
        CHECK(g_dev.asked.size() == 1 && g_dev.asked[0] == 800 && g_dev.frees == 0);
        double *p = b;
        grew = false;
        CHECK(b.reserve(100, &grew) == 0 && !grew && b.get() == p);
        CHECK(b.reserve(7, &grew) == 0 && !grew && b.get() == p && b.count() == 100);
        CHECK(g_dev.asked.size() == 1 && g_dev.frees == 0);                   // no allocator call at all
        CHECK(b.reserve(101, &grew) == 0 && grew && b.count() == 101);
        CHECK(g_dev.asked.size() == 2 && g_dev.asked[1] == 808 && g_dev.frees == 1 && g_dev.live.size() == 1);
        grew = true;
        CHECK(b.reserve(50, &grew) == 0 && grew);                             // the flag is only ever set: groups share it
        // slack: allocated, not counted
        DevBuf<float> s(kDev);
        CHECK(s.reserve(10, nullptr, 6) == 0 && s.count() == 10 && s.bytes() == 64 && g_dev.asked.back() == 64);
        const size_t calls = g_dev.asked.size();
        CHECK(s.reserve(10, nullptr, 6) == 0 && g_dev.asked.size() == calls);
        s[15] = 1.0f;                                                         // (the last slack element is there)
    }
    end("reserve");
}

void reset_is_exact()
{
    begin();
    {
        DevBuf<int> b(kDev);
        CHECK(b.reset(1000) == 0 && b.count() == 1000 && g_dev.asked.back() == 4000);
        CHECK(b.reset(10) == 0 && b.count() == 10 && g_dev.asked.back() == 40);   // shrinks: always a new block
        CHECK(b.reset(10) == 0 && g_dev.asked.size() == 3 && g_dev.frees == 2 && g_dev.live.size() == 1);
        CHECK(b.reset(4, 4) == 0 && b.count() == 4 && b.bytes() == 32 && g_dev.asked.back() == 32);
        b.release();
        CHECK(!b && b.count() == 0 && b.bytes() == 0 && g_dev.live.empty());
        b.release();                                                          // (twice: nothing to free)
        CHECK(g_dev.frees == 4);
        // pooled: the pool's rules decide the block, the buffer still counts what was asked for
        DevPool pool(kDev);
        DevBuf<int> q(pool);
        CHECK(q.reset(1000) == 0 && q.count() == 1000 && q.bytes() == 4000 && g_dev.asked.back() == 4000 + 500);
        CHECK(q.reset(1000) == 0 && g_dev.asked.back() == 4500 && g_dev.live.size() == 1);   // its own block, recycled
        CHECK(g_dev.asked.size() == 5);
        // adopt: a block the raw allocator made elsewhere
        void *raw = nullptr;
        CHECK(dev_alloc(&raw, 48) == 0);
        b.adopt(static_cast<int *>(raw), 12);
        CHECK(b && b.count() == 12 && b.bytes() == 48);
    }
    end("reset");
}

// three buffers that grow together, as the engine's groups do: the k-th allocation fails
int group(DevBuf<int> &a, DevBuf<float> &b, DevBuf<double> &c, size_t n, bool *grew)
{
    int rc = a.reserve(n, grew);
    if (rc == 0) rc = b.reserve(n, grew);
    if (rc == 0) rc = c.reserve(n, grew, 8);
    return rc;
}
void failure_leaves_buffers_empty()
{
    for (int pooled = 0; pooled < 2; pooled++)
        for (int k = 1; k <= 3; k++) {
            begin();
            {
                DevPool pool(kDev);
                DevBuf<int> a = pooled ? DevBuf<int>(pool) : DevBuf<int>(kDev);
                DevBuf<float> b = pooled ? DevBuf<float>(pool) : DevBuf<float>(kDev);
                DevBuf<double> c = pooled ? DevBuf<double>(pool) : DevBuf<double>(kDev);
                bool grew = false;
                CHECK(group(a, b, c, 64, &grew) == 0 && grew);                // a first, healthy round
                const void *pb = b.get();
                // the k-th buffer's allocation fails (pooled: the head-room request and the retry at the exact size)
                g_dev.fail_at = k;
                g_dev.fail_n = pooled ? 2 : 1;
                grew = false;
                CHECK(group(a, b, c, 4096, &grew) == 2 && grew);
                // who completed is consistent, who did not is empty, who was not reached is as before
                CHECK(k == 1 ? (!a && a.count() == 0 && a.bytes() == 0) : (a && a.count() == 4096));
                CHECK(k == 1 ? (b.get() == pb && b.count() == 64) : k == 2 ? (!b && b.count() == 0) : (b && b.count() == 4096));
                CHECK(k == 3 ? (!c && c.count() == 0 && c.bytes() == 0) : (c && c.count() == 64 && c.bytes() == 8 * 72));
                if (pooled) CHECK(pool.free_blocks() == 0);                   // (trimmed before the retry)
                // the same request with the allocator healthy: what is missing is made, nothing else
                const size_t before = g_dev.asked.size();
                grew = false;
                CHECK(group(a, b, c, 4096, &grew) == 0 && grew);
                CHECK(g_dev.asked.size() - before == (size_t)(4 - k));
                CHECK(a && b && c && a.count() == 4096 && b.count() == 4096 && c.count() == 4096 && c.bytes() == 8 * 4104);
                a[4095] = 1; b[4095] = 1.f; c[4103] = 1.0;
                CHECK(pooled ? pool.live_blocks() == 3 : g_dev.live.size() == 3);
                grew = false;
                CHECK(group(a, b, c, 4096, &grew) == 0 && !grew);             // ... and a third time: nothing at all
            }
            char name[64];
            std::snprintf(name, sizeof name, "failure %s k=%d", pooled ? "(pooled)" : "(raw)", k);
            end(name);
        }
}

void pool_rules()
{
    begin();
    {
        DevPool pool(kDev);
        DevBuf<char> a(pool), b(pool), c(pool);
        // the 256-byte floor, and 1/8 head-room on a fresh block
        CHECK(a.reset(1) == 0 && g_dev.asked.back() == 256 + 32 && a.count() == 1);
        CHECK(b.reset(8000) == 0 && g_dev.asked.back() == 9000);
        // best fit: the smallest free block that holds the request
        CHECK(c.reset(16000) == 0 && g_dev.asked.back() == 18000);
        char *pb = b, *pc = c;
        b.release(); c.release();
        CHECK(pool.free_blocks() == 2 && g_dev.frees == 0);                   // returned to the pool, not to the allocator
        const size_t calls = g_dev.asked.size();
        DevBuf<char> d(pool);
        CHECK(d.reset(8500) == 0 && d.get() == pb && g_dev.asked.size() == calls);   // 9000 fits and is the smaller one
        CHECK(c.reset(8500) == 0 && c.get() == pc && g_dev.asked.size() == calls);   // 18000 <= 2 * 8500 + 1 MiB
        // the bound: a 10 MiB block is not handed to a 1 MiB request (2 * 1 MiB + 1 MiB < 10 MiB) ...
        DevBuf<char> big(pool), small(pool);
        CHECK(big.reset(10 * MiB) == 0);
        big.release();
        CHECK(small.reset(1 * MiB) == 0 && g_dev.asked.back() == MiB + MiB / 8 && pool.free_blocks() == 1);
        // ... and just inside it is: a block of exactly 2 * bytes + 1 MiB
        DevBuf<char> edge(pool), fits(pool);
        pool.trim(0);
        CHECK(edge.reset(3 * MiB) == 0);                                      // a block of 3 MiB + 3/8 MiB
        const size_t blk = g_dev.asked.back();
        edge.release();
        const size_t calls2 = g_dev.asked.size();
        CHECK(fits.reset((blk - MiB + 1) / 2) == 0 && g_dev.asked.size() == calls2);       // 2 * bytes + 1 MiB >= blk
        fits.release();
        CHECK(fits.reset((blk - MiB) / 2 - 1) == 0 && g_dev.asked.size() == calls2 + 1);   // 2 * bytes + 1 MiB < blk
    }
    end("pool: floor, head-room, best fit, bound");
    begin();
    {
        // the head-room request fails: the pool gives its free blocks back, then asks for the exact size
        DevPool pool(kDev);
        DevBuf<char> keep(pool), a(pool);
        CHECK(keep.reset(1000) == 0);
        keep.release();
        CHECK(pool.free_blocks() == 1 && g_dev.live.size() == 1);
        g_dev.asked.clear();
        g_dev.fail_at = 1;
        CHECK(a.reset(8 * MiB) == 0 && a.count() == 8 * MiB);
        CHECK(g_dev.asked.size() == 2 && g_dev.asked[0] == 9 * MiB && g_dev.asked[1] == 8 * MiB);
        CHECK(pool.free_blocks() == 0 && g_dev.live.size() == 1 && g_dev.frees == 1);
        a[8 * MiB - 1] = 1;
    }
    end("pool: exact size after a failed head-room request");
    begin();
    {
        // at most 10 free blocks are kept; the oldest goes first
        DevPool pool(kDev);
        std::vector<DevBuf<char>> v;
        for (int i = 0; i < 12; i++) { v.emplace_back(pool); CHECK(v.back().reset(1000 * (size_t)(i + 1)) == 0); }
        std::vector<void *> p;
        for (auto &b : v) p.push_back(b.get());
        for (auto &b : v) b.release();
        CHECK(pool.free_blocks() == 10 && pool.live_blocks() == 0 && g_dev.frees == 2 && g_dev.live.size() == 10);
        CHECK(!g_dev.live.count(p[0]) && !g_dev.live.count(p[1]) && g_dev.live.count(p[2]) && g_dev.live.count(p[11]));
        // a buffer that is not pooled never enters the pool, whatever pool stands next to it
        DevBuf<char> raw(kDev), pin(kPin);
        CHECK(raw.reset(1000) == 0 && g_dev.asked.back() == 1000);            // the exact size: no floor, no head-room, no recycling
        CHECK(pin.reset(10) == 0 && g_pin.asked.size() == 1 && g_pin.asked[0] == 10);
        const int frees = g_dev.frees;
        raw.release(); pin.release();
        CHECK(g_dev.frees == frees + 1 && g_pin.frees == 1 && pool.free_blocks() == 10 && g_pin.live.empty());
        pool.trim(0);
        CHECK(pool.free_blocks() == 0 && g_dev.live.empty());
    }
    end("pool: ten free blocks, unpooled buffers");
}

void moves_and_teardown()
{
    begin();
    {
        DevPool pool(kDev);
        DevBuf<int> a(pool);
        CHECK(a.reset(100) == 0);
        int *p = a;
        DevBuf<int> b(std::move(a));                                           // move construction
        CHECK(!a && a.count() == 0 && a.bytes() == 0 && b.get() == p && b.count() == 100);
        DevBuf<int> c(kDev);
        CHECK(c.reset(5) == 0);
        c = std::move(b);                                                     // move assignment: c's own block goes first
        CHECK(!b && b.count() == 0 && c.get() == p && c.count() == 100 && g_dev.frees == 1 && g_dev.live.size() == 1);
        c.release();
        CHECK(pool.free_blocks() == 1);                                       // (the binding moved with the block: back to the pool)
        CHECK(a.reset(10) == 0 && b.reset(10) == 0);                          // moved-from buffers are empty buffers, still bound
    }
    end("moves");
    for (int order = 0; order < 3; order++) {
        begin();
        {
            DevPool pool(kDev);
            DevBuf<char> *b[3];
            for (int i = 0; i < 3; i++) { b[i] = new DevBuf<char>(pool); CHECK(b[i]->reset(5000 * (size_t)(i + 1)) == 0); }
            static const int seq[3][3] = {{0, 1, 2}, {2, 1, 0}, {1, 2, 0}};
            for (int i = 0; i < 3; i++) delete b[seq[order][i]];
            CHECK(pool.live_blocks() == 0 && pool.free_blocks() == 3 && g_dev.live.size() == 3 && g_dev.frees == 0);
        }                                                                      // the pool goes after its buffers ...
        CHECK(g_dev.live.empty() && g_dev.frees == 3);                         // ... and nothing is left, nothing freed twice
        end("teardown");
    }
}

}  // namespace

int main()
{
    reserve_grows_only();
    reset_is_exact();
    failure_leaves_buffers_empty();
    pool_rules();
    moves_and_teardown();
    std::printf("%d cases, %d failed\n", g_cases, g_failed);
    if (g_failed == 0) std::printf("all passed\n");
    return g_failed == 0 ? 0 : 1;
}

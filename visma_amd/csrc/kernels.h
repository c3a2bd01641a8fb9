// kernels.h -- launch interface of the gfx950 ICP kernels (kernels.hip).
#pragma once

#include "dev_buf.h"

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

namespace visma {

// ---- the device memory and events of one host-in, host-out call (the neighbourhood features, feature_match.hip, ransac.hip)
#define VISMA_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)
// every allocation is freed with the object
struct DevBufs {
    std::vector<void *> ptrs;
    DevBufs() = default;
    DevBufs(const DevBufs &) = delete;
    DevBufs &operator=(const DevBufs &) = delete;
    ~DevBufs() { for (void *p : ptrs) (void)hipFree(p); }
    template <class T>
    hipError_t alloc(T **out, size_t count)
    {
        void *p = nullptr;
        VISMA_TRY(hipMalloc(&p, sizeof(T) * (count ? count : 1)));
        ptrs.push_back(p);
        *out = (T *)p;
        return hipSuccess;
    }
};
// ... and N events for the calls that report device time
template <int N>
struct DevEvents {
    hipEvent_t ev[N] = {};
    DevEvents() = default;
    DevEvents(const DevEvents &) = delete;
    DevEvents &operator=(const DevEvents &) = delete;
    ~DevEvents()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    hipError_t create()
    {
        for (hipEvent_t &e : ev) VISMA_TRY(hipEventCreate(&e));
        return hipSuccess;
    }
    hipEvent_t operator[](int k) const { return ev[k]; }
};

// ---- compile-time tile constants (reported by visma_icp_get_tile_config) ----
constexpr int kBlock = 256;         // threads per workgroup (4 wave64)
constexpr int kSptLarge = 8;        // source points per thread, large clouds
constexpr int kSptSmall = 2;        // ... small clouds (more workgroups)
constexpr int kSTile = kBlock * kSptLarge;  // S_TILE = 2048 source points / workgroup
constexpr int kTChunk = 512;        // target points staged per LDS fill
constexpr int kSub = 64;            // sub-chunk whose winner id is tracked
constexpr int kReduceAcc = 29;      // per-thread f64 accumulators (max over modes)
constexpr int kNStats = 38;

struct Xform32 { float m[12]; };    // row-major 3x4, fp32 (NN search)
struct Xform64 { double m[12]; };   // row-major 3x4, f64  (statistics)
struct Offset64 { double v[3]; };   // frame shift applied to p and q in the statistics
// A point in f64 for the double-precision search (32 B: x, y, z, original index).
struct Pt64 {
    double x, y, z;
    unsigned long long w;
};

// State of one ICP problem advanced entirely on the device (icp_loop.hip): the
// NN / reduction kernels read the current transform from it, the one-thread
// solve kernel updates it, the host only reads it back at the end.
struct DevIcpState {
    double Tc[12];       // current transform, centred frame (row-major 3x4)
    double centre[3];    // cloud centre (frame offset of GN / point-to-plane statistics)
    double stats[kNStats];
    double fit, rmse, fit_prev, rmse_prev, K;
    double rel_fit, rel_rmse;
    long long ns_total;  // fitness denominator (all ranks)
    int iter;            // solves performed
    int passes;          // NN passes performed
    int active;          // 1 while the loop is still running
    int max_iter, solver, scaling, plane, world_frame, check_stop;
    float r2f;
    int have_prev;       // Tc_prev holds the transform of the previous NN pass (the certificate of grid_coop.hip)
    double Tc_prev[12];
    double axis[3];      // use_axis: every update rotates about this unit axis only (host_math.hpp: *_axis_from_stats)
    int use_axis;
    int pad_axis;        // (the state is copied as 8-byte words)
};

// The fold of the partial rows inside the search launch (device_common.h: fused_fold).
// Rows per first-level group (launches of more than kFoldSingle rows fold in two levels).  16 since the end of round 4
// (32 before): the last arrivers of the groups -- the slowest workgroups of a launch by construction -- sum half as many
// rows, and the level-2 sum of 64 rows is still one batch of eight loads per thread: C4 22.2 vs 24.2 us per iteration
// in the persistent launch, 25.9 vs 27.8 with one launch per pass (64: 26.4 in the persistent launch; 8: as 16).
#ifndef VISMA_FOLD_GROUP
#define VISMA_FOLD_GROUP 16
#endif
constexpr int kFoldGroup = VISMA_FOLD_GROUP;
constexpr int kIpcMaxRanks = 16;
constexpr long long kIpcSpinLimit = 200000000ll;    // polls of the own mailbox before a peer counts as lost (minutes)
constexpr long long kIpcHandshakeSpins = 15000000ll;  // ... in the handshake of visma_icp_comm_ipc_init (tens of seconds)
struct IpcPeers { void *box[kIpcMaxRanks]; };     // box[r]: rank r's mailbox as mapped HERE (box[rank] = own)

struct FoldArgs {
    unsigned *tickets;            // ticket_stride words per problem, zero; NULL = fold in a separate launch
    double *partials2;            // ticket_stride rows of kReduceAcc per problem
    int ticket_stride;            // >= 1 + ceil(workgroups per problem / 32)
    double *stats_out;            // the 38 statistics of problem b at stats_out + b * stats_stride
    long long stats_stride;
    double *host_out;             // mapped host memory for tagged publication (or NULL)
    unsigned long long seq;
    // source-sharded ranks with peer-to-peer mailboxes (ipc_n > 1): the folding workgroup exchanges the 38
    // statistics with the peers itself before it publishes (no separate all-reduce launch)
    IpcPeers peers;
    int ipc_rank, ipc_n;
    unsigned long long *ipc_seq_dev;   // exchanges performed so far, in DEVICE memory: it advances only when an
                                       // exchange really runs (a launch that returns because its loop has ended
                                       // must not burn a number: the two mailbox halves alternate by it)
    int *ipc_flag;
    long long ipc_spins;
    void *const *peer_table;           // the same mailboxes as `peers`, as a table in DEVICE memory: what the persistent
                                       // kernel's fold reads (a by-value table indexed in a loop would live in scratch there)
    // the POLLED fold of persistent launches (device_common.h: polled_fold): rows and group rows as self-validating
    // granules {low half, tag, high half, tag}, 32 per row; NULL = the ticket fold
    void *rows_tagged, *rows2_tagged;
    unsigned long long *dead_flag;     // the launch's "somebody left" word (kernels.h: kPersistDead)
    long long poll_ticks;              // how long a reducer waits for a row (wall_clock64 ticks) before it gives the launch up
    // device-resident loops with the closed-form (Kabsch) update (round 5): the workgroup that completes problem b's fold
    // advances solve[b] right there (icp_state.h: advance_state<true>) -- no solve launch between two search launches.
    // NULL: the statistics are left in the state and solve_state_kernel advances it (Gauss-Newton modes, point-to-plane,
    // ranks that exchange first).  Honoured by the kernels batches and sweeps run (grid.hip, grid_wave.hip), NOT by
    // the certificate kernels of grid_coop.hip (launch_nn_coop refuses a fold that sets it for them).  Compiled in only
    // with -DVISMA_SOLVE_IN_FOLD=1 (kSolveInFold): it measured slower than the solve launch and its
    // inlined one-thread solve costs the default search kernels scratch and LDS -- default builds carry none of it.
    DevIcpState *solve;
    // (round 6) the PERSISTENT SWEEP launch (grid_wave.hip: nn_wave_kernel_sweep): the workgroup that completes problem b's
    // fold advances solve[b] and hands the next pass's transform to the problem's other workgroups through
    // sweep_relay + 32 b: kPersistWords 8-byte words {half of a double | tag << 32} + the command word (GO / STOP), every
    // word carrying sweep_tag -- the tag of the pass that is due next.  NULL: not that launch.
    unsigned long long *sweep_relay;
    unsigned sweep_tag;
    int sweep_passes;                  // DevIcpState::passes of solve[b] before this pass's update (validates the state read)
};
#ifndef VISMA_SOLVE_IN_FOLD
#define VISMA_SOLVE_IN_FOLD 0
#endif
constexpr bool kSolveInFold = VISMA_SOLVE_IN_FOLD != 0;

// The tag the granule rows of the polled fold validate themselves with: the pass's sequence number folded into
// 1 .. 2^32 - 1 -- never 0 (a cleared buffer validates nothing), the same value again only 2^32 - 1 passes later (the
// host clears the rows before a session whose numbers run through that wrap: hip_engine_passes.cpp).
constexpr unsigned long long kFoldTagPeriod = 0xFFFFFFFFull;
#if defined(__HIPCC__)
__host__ __device__
#endif
inline unsigned fold_row_tag(unsigned long long seq) { return (unsigned)(seq % kFoldTagPeriod) + 1u; }

// The PERSISTENT form of the certificate kernel (grid_coop.hip, round 4b): ONE launch runs up to max_passes ICP
// passes of one registration.  After a pass the workgroup that finished the fold (and published the statistics to
// the host) polls a command block in mapped host memory for the next transform, re-publishes it in device memory
// (relay) for the other workgroups, and everybody runs the next pass -- no relaunch, no dispatch ramp, source and
// state re-read from a warm L2.  Command block / relay: kPersistWords 8-byte words {low or high half of a double |
// tag << 32}, each word validating itself (no fence anywhere): words 0..23 = the 3 x 4 transform, word 24 = command.
// Every wait is bounded by the 100 MHz wall clock: a launch whose host went away ends by itself.
constexpr int kPersistWords = 25;
constexpr int kPersistPublished = 31;   // relay word: the tag of the pass whose statistics have been published
constexpr int kPersistDead = 29;        // relay word: nonzero once a workgroup of this launch has left early (the launch can never fold again)
constexpr int kPersistStarted = 30;     // relay word: workgroups of this launch that have begun (zeroed on the stream before the launch)
constexpr unsigned kPersistGo = 1u, kPersistStop = 2u, kPersistAbort = 3u;
struct PersistArgs {
    const unsigned long long *host_cmd;   // mapped, coherent host memory (device pointer), kPersistWords words -- or, `direct`,
                                          // fine-grained DEVICE memory the host stores into through the PCIe BAR: then every
                                          // workgroup polls it itself (no PCIe read per poll, no relay hop)
    int direct;
    unsigned long long *relay;            // device memory, kPersistWords words
    unsigned *host_flag;                  // mapped host memory: set to the pass count reached when a wait ran out
    int max_passes;                       // passes this launch may run (>= 1); the first needs no command
    unsigned tag0;                        // the command for pass p (1-based after the first) carries tag0 + p - 1
    long long wait_ticks;                 // how long a workgroup waits for a command AFTER the pass's statistics were published
                                          // (wall_clock64 ticks, 100 MHz).  The HOST never posts GO later than a quarter of
                                          // this after it saw the statistics (it posts STOP and carries on with ordinary
                                          // launches), so no command can arrive while some workgroups have given up already
    long long start_ticks;                // how long a workgroup waits for the launch's OTHER workgroups to begin (round 5:
                                          // 5 ms by default -- when another stream's kernels hold compute units the launch
                                          // cannot complete its residency, and waiting the four patiences of wait_ticks for
                                          // that cost 0.8 s per attempt); 0: wait_ticks
    long long hard_ticks;                 // ... and before that publication (the pass is still running somewhere): a cap that
                                          // only a lost workgroup could reach -- unless not every workgroup of the launch has
                                          // begun by then (another process's persistent launch holds the rest of the compute
                                          // units and waits for ours): then wait_ticks
    unsigned long long *timeline;         // measurement (VISMA_ICP_PERSIST_TIMELINE), else NULL: per pass and workgroup the
    int timeline_passes;                  // 100 MHz clock when the pass began and when its body (fold ticket included) was done
    int wait_first;                       // (round 6) the launch was queued BEHIND the registration's cold pass, before its
                                          // statistics were out: the transform of the launch's first pass is not in the
                                          // kernel arguments -- it comes as a command with tag0 like every later one (which
                                          // then carry tag0 + p instead of tag0 + p - 1), and the launch waits for it first
};

struct NNLaunch {
    int src_tiles;
    int tgt_splits;
    int spt;
};

// Pick the launch geometry for ns source points against nt_pad/kTChunk chunks.
NNLaunch nn_plan(int64_t ns, int64_t nt_pad);

// Fused transform + brute-force nearest neighbour.  tgt must be padded to a
// multiple of kTChunk with +inf points.  keys: [splits][ns_pad] 64-bit
// (d2 bits << 32 | sub-chunk id), no initialisation needed.
hipError_t launch_nn_brute(const float4 *src, int64_t ns, const float4 *tgt,
                           int64_t nt_pad, const Xform32 &T, float r2f,
                           unsigned long long *keys, int64_t ns_pad,
                           const NNLaunch &plan, const DevIcpState *st, hipStream_t stream,
                           const Pt64 *src64 = nullptr, const Xform64 *T64 = nullptr, float *second = nullptr);
// src64 + T64 + second ([splits][ns_pad] floats): the exact flavour (see nn_brute_kernel)

// Merge the per-split keys, recover the exact target index inside the winning
// sub-chunk, then accumulate the per-correspondence Jacobian/residual
// statistics; per-workgroup partials go to `partials`, `finalize` folds them
// (fixed order) into the 38 statistics at `stats_out` (device or mapped host).
// idx_out/d2_out (ns) receive the final correspondence per source point.
// the exact flavour of the brute-force path: f64 clouds (source in engine order, target in the caller's
// order) and the runner-up array written by launch_nn_brute
// Queries whose winner cannot be decided inside the winning sub-chunk (another sub-chunk reaches into the
// rounding band: about one in a thousand) are listed by the reduce kernel and resolved together by two
// passes of ALL workgroups over the target (brute_rescan_kernel), not by a scan of their own.
constexpr int kBrutePendCap = 4096;       // more pending queries than this: the wave scans in place (slow, exact)
struct BrutePend {
    int *count;                           // [0] pending queries (may exceed the capacity)
    float4 *q32;                          // (px, py, pz, L): fp32 query and its squared fp32 filter radius
    Pt64 *q64;                            // f64 query, w = source slot
    unsigned long long *best;             // f64 bits of the best d2 (order preserving), r2d bits = none
    unsigned *best_idx;                   // lowest index among the targets at that distance
};
struct BruteExact {
    const Pt64 *src64, *tgt64, *nrm64;
    const float *second;
    int64_t nt;
    BrutePend pend;                       // pend.count == NULL: every scan in place
};
hipError_t launch_reduce(const float4 *src, int64_t ns, const float4 *tgt,
                         const float4 *tgt_normals, const unsigned long long *keys,
                         int nsplits, int64_t ns_pad, const Xform32 &T32,
                         const Xform64 &T64, const double frame_offset[3], float r2f,
                         int point_to_plane,
                         int32_t *idx_out, float *d2_out, double *partials,
                         int max_partial_blocks, double *stats_out, const DevIcpState *st,
                         int *nblocks_out, hipStream_t stream, double *host_out = nullptr,
                         unsigned long long seq = 0, const BruteExact *ex = nullptr);

int reduce_max_blocks();
constexpr int kSortedSlack = 64;   // entries allocated past the end of a cell-sorted target: the exact grid
                                   // search loads whole batches (<= U*G slots) from a run's first slot
// one-shot all-reduce of the 38 statistics through IPC-mapped mailboxes (kernels.hip)
hipError_t launch_ipc_allreduce(const double *stats_in, double *stats_out, const IpcPeers &peers, int rank,
                                int nranks, unsigned long long *seq_dev, double *host_out, unsigned long long host_seq,
                                int *timeout_flag, hipStream_t stream, long long max_spins = kIpcSpinLimit);
// target-sharded ranks: keys of the local winners / moments of the global winners owned here
hipError_t launch_shard_keys(const int32_t *idx, const float *d2, int64_t ns, unsigned offset,
                             unsigned long long *keys, hipStream_t stream);
hipError_t launch_shard_accumulate(const float4 *src, int64_t ns, const unsigned long long *keys,
                                   const float4 *tgt, int64_t nt_local, unsigned offset,
                                   const float4 *tgt_normals, const Xform64 &T64,
                                   const double frame_offset[3], float r2f, int point_to_plane,
                                   int32_t *idx_out, float *d2_out, double *partials,
                                   int max_partial_blocks, int *nblocks_out, hipStream_t stream);
// ... the same in f64 (exact search on every shard): key 1 = bits of the local f64 d2 (MIN over ranks =
// the global nearest), key 2 = global index of the shards that hold it (MIN = lowest index on exact
// ties); the owner accumulates from the f64 coordinates
hipError_t launch_shard_keys64(const int32_t *idx, const double *d64, int64_t ns, unsigned long long *keys,
                               hipStream_t stream);
hipError_t launch_shard_claim64(const int32_t *idx, const double *d64, const unsigned long long *gkeys, int64_t ns,
                                unsigned offset, unsigned long long *claim, hipStream_t stream);
hipError_t launch_shard_accumulate64(const Pt64 *src64, int64_t ns, const unsigned long long *gkeys,
                                     const unsigned long long *claim, const Pt64 *tgt64, int64_t nt_local,
                                     unsigned offset, const float4 *tgt_normals, const Pt64 *nrm64,
                                     const Xform64 &T64, const double frame_offset[3], double r2d,
                                     int point_to_plane, int32_t *idx_out, float *d2_out, double *partials,
                                     int max_partial_blocks, int *nblocks_out, hipStream_t stream,
                                     const DevIcpState *st = nullptr);
// stats (device) -> host_out[0..37] (mapped host memory), then host_out[38] = seq (u64 bits)
hipError_t launch_publish_stats(const double *stats, double *host_out, unsigned long long seq,
                                hipStream_t stream);

// Fold `nblocks` partial rows into the 38 statistics (one workgroup, fixed order).
// host_out (mapped host memory, may be NULL): also publish the 38 statistics there
// and then raise host_out[38] = seq (u64 bits) -- see launch_publish_stats.
hipError_t launch_finalize(const double *partials, int nblocks, int point_to_plane,
                           double *stats_out, hipStream_t stream, double *host_out = nullptr,
                           unsigned long long seq = 0);
// On-device loop (icp_loop.hip): fold + solve + stop test, no host round trip.
//  launch_finalize_solve : single GPU (fold partials, then advance the state)
//  launch_finalize_state : fold partials into st->stats only (an all-reduce follows)
//  launch_solve_state    : advance the state from st->stats
// nprob problems: workgroup b folds rows [b*nblocks, (b+1)*nblocks) into st[b]
hipError_t launch_finalize_solve(const double *partials, int nblocks, DevIcpState *st, int plane,
                                 int nprob, hipStream_t stream);
hipError_t launch_finalize_state(const double *partials, int nblocks, DevIcpState *st, int plane,
                                 hipStream_t stream);
hipError_t launch_solve_state(DevIcpState *st, int nprob, hipStream_t stream);

// ---- radius-cell uniform grid (grid.hip) -------------------------------------

struct GridParams {
    float mn[3];      // lower corner of the target's bounding box
    float h, inv_h;   // cell edge along x (>= 1.001 * max_dist) and its reciprocal
    int dim[3];       // cells per axis (y and z counted in cells of edge h / sub)
    int sub;          // 1, or 2: rows (y,z) at half pitch -- 25 thinner rows instead of 9
    float hs, inv_hs; // h / sub and its reciprocal
    int ring;         // 0: cells at least as large as the search radius (27-cell neighbourhoods); > 0: cells SMALLER than
                      // the radius, searched in rings of rows (grid_ring.hip) -- the largest ring a radius can reach, + 1
                      // (in the 4 bytes the alignment of ncell left free: the structure every search kernel takes by value
                      //  has the size it had -- 8 bytes more cost the persistent launch 0.25 us per pass)
    int64_t ncell;
};
static_assert(sizeof(GridParams) == 56, "GridParams is a kernel argument of every search kernel");
// one row of the ring search's visiting order: its offset from the query's row and the squared distance (in cells) that
// every point of it is at least away from any point of the query's cell row: max(|dy| - 1, 0)^2 + max(|dz| - 1, 0)^2
struct RingRow { short dy, dz; float base; };
// ... the whole order for a grid with g.ring rings: (2 ring + 1)^2 entries, nearest first (device memory)
struct RingTable { const RingRow *rows; int nrows; };
constexpr int kRingMaxRings = 64;   // cells are enlarged until a radius spans no more rings than this
constexpr int64_t kGridMaxCells = 64ll * 1024 * 1024;        // at sub = 1
constexpr int64_t kGridMaxCellsFine = 256ll * 1024 * 1024;   // at sub = 2 (1 GiB table)
constexpr int kGridMaxDim = 2048;   // per axis at sub = 1: keeps the fp32 binning error < 1e-3 cell

// One problem of a batch with its OWN clouds (offsets into concatenated arrays).
struct ProbDesc {
    long long src_off, sorted_off, start_off, out_off;
    int ns, first_block, nblocks, pad_;
    GridParams g;
};

#ifdef VISMA_WITH_TILE   /* experiment, side build only (see HipEngine::use_tile) */
// ---- streamed radius-cell search with exact (f64) tie-breaks and fused fold (tile.hip) ------
struct TileArgs {
    const Pt64 *src64;            // source, f64 (centred), Morton order
    int ns;
    const float4 *sorted;         // cell-sorted target, fp32 view (w = original index)
    const Pt64 *sorted64;         // ... and the f64 points in the same slots
    const unsigned *start;        // cell table
    GridParams g;
    const float4 *nrm;            // target normals by original index (point-to-plane)
    const Pt64 *nrm64;
    Xform64 T64;
    Offset64 off;
    float r2f;
    int *idx_out;
    float *d2_out;
    double *partials;             // one row of kReduceAcc per workgroup
    double *partials2;            // ticket_stride rows per problem (level-2 rows of the fused fold)
    unsigned *tickets;            // ticket_stride words per problem, zero; NULL = no fused fold
    int ticket_stride;            // >= 1 + ceil(workgroups per problem / 32)
    double *stats_out;            // the 38 statistics of problem b at stats_out + b * stats_stride
    long long stats_stride;
    double *host_out;             // mapped host memory for tagged publication (or NULL)
    unsigned long long seq;
    unsigned long long *stats;    // profiling counters, 512 x 8 (or NULL)
    const DevIcpState *st;        // device loop state (or NULL)
    int bpp;                      // workgroups per problem (shared clouds)
    long long out_stride;
    const ProbDesc *descs;        // problems with their own clouds (or NULL)
    int nprob;
    int force_fallback;           // testing: search from global memory in every workgroup
};
// workgroup size of a tile configuration (queries per workgroup)
int tile_threads(int config);
// total_blocks = sum over problems of ceil(ns / tile_threads(config))
hipError_t launch_nn_tile_reduce(const TileArgs &a, int point_to_plane, int config, int total_blocks,
                                 hipStream_t stream);
#endif
// float4 (x, y, z, .) -> Pt64 (x, y, z, index): f64 view of clouds uploaded as fp32
hipError_t launch_promote_pt64(const float4 *src, Pt64 *dst, int64_t n, hipStream_t stream);
// order.hip: the source cloud (caller's f64 points, already on the device) into Morton order
size_t order_source_scratch_bytes(int64_t n);
hipError_t order_source_device(const double *d_xyz, int64_t n, const double c[3], float4 *d_src, Pt64 *d_src64,
                               int32_t *d_order, void *scratch, size_t scratch_bytes, hipStream_t stream);
// raw f64 xyz (3 doubles per point) -> f4[j] = ((float)(x - c), .., 0) and, when p8 != NULL, p8[j] = {x - c, .., j}
hipError_t launch_expand_f64(const double *xyz, int64_t n, const double c[3], float4 *f4, Pt64 *p8, hipStream_t stream,
                             int64_t index0 = 0);
// ... the same from values fp32 holds exactly (3 floats per point): p8[j].w = index0 + j
hipError_t launch_expand_f32(const float *xyz, int64_t n, int64_t index0, const double c[3], float4 *f4, Pt64 *p8,
                             hipStream_t stream);

hipError_t launch_grid_bbox(const float4 *tgt, int64_t nt, unsigned *box6, hipStream_t stream);
hipError_t launch_pack12(const float4 *src, float *dst, int64_t n, hipStream_t stream);   // (x,y,z,w) -> packed (x,y,z)
void grid_decode_bbox(const unsigned box6[6], float mn[3], float mx[3]);
GridParams grid_plan(const float mn[3], const float mx[3], double max_dist, int64_t max_cells, int max_sub = 1);
// the same table with cells of edge `cell` < max_dist (enlarged until the table fits), for the ring search (grid_ring.hip)
GridParams grid_plan_ring(const float mn[3], const float mx[3], double max_dist, double cell, int64_t max_cells);
int grid_scan_blocks(int64_t ncell);

// ---- mesh steps (mesh.hip): host arrays in, host arrays out -------------------
// method: 0 = choose, 1 = brute force (LDS-tiled scan of all faces), 2 = BVH
hipError_t point_mesh_distance_device(const double *h_P, int64_t np, const double *h_V, int64_t nv,
                                      const int32_t *h_F, int64_t nf, int method, double *h_d2, int32_t *h_face,
                                      double *h_closest, float *kernel_ms, float *build_ms, hipStream_t stream);
hipError_t sample_mesh_transformed_device(const double *h_V, int64_t nv, const int32_t *h_F, int64_t nf, int64_t n,
                                          int quirks, unsigned long long seed, const double *T16, double *d_out,
                                          int64_t room, int64_t *m_out, hipStream_t stream);
hipError_t sample_mesh_device(const double *h_V, int64_t nv, const int32_t *h_F, int64_t nf, int64_t n,
                              int quirks, unsigned long long seed, const double *h_uniforms,
                              double *h_out, int64_t *n_out, hipStream_t stream);
hipError_t surface_distances_device(const double *h_Vs, int64_t nvs, const int32_t *h_Fs, int64_t nfs,
                                    const double *h_Vt, int64_t nvt, const int32_t *h_Ft, int64_t nft, int64_t n,
                                    int quirks, unsigned long long seed, int method, double *h_dist,
                                    int64_t *n_out, float *kernel_ms, float *build_ms, hipStream_t stream);

// ---- cloud-to-cloud distances (cloud_distance.hip): host arrays in, host arrays out ----
// exact unbounded nearest-neighbour distance of every source point to the target (0 for an empty target), and of
// every point to the nearest other point of its own cloud (0 for a one-point cloud); own buffers, the given stream
hipError_t point_cloud_distance_device(const double *h_src, int64_t ns, const double *h_tgt, int64_t nt,
                                       double *h_dist, hipStream_t stream);
hipError_t nearest_neighbor_distance_device(const double *h_xyz, int64_t n, double *h_dist, hipStream_t stream);

// ---- normal estimation (normals.hip): host arrays in, host arrays out ----------
// open3d::EstimateNormals; search_type 0 KNN(knn) | 1 Radius(radius) | 2 Hybrid(radius, max_nn = knn)
constexpr int kNormalsMaxList = 170;     // longer result lists live in global memory (a heap per point) instead of LDS
hipError_t estimate_normals_device(const double *h_xyz, int64_t n, const double *h_nrm_in, int search_type,
                                   int knn, double radius, double *h_out, hipStream_t stream);
// ... the device part alone (resident input and output; origin: nn_binning_origin's point of the cloud), not for the trivial
// case (fewer than 3 neighbours for every point: every normal is (0, 0, 1), which the caller fills in)
bool estimate_normals_trivial(int search_type, int knn, double radius);
hipError_t estimate_normals_core(const double *d_xyz, int64_t n, const double *d_nrm_in, const double origin[3], int search_type,
                                 int knn, double radius, double *d_out, hipStream_t stream);

// ---- voxel down-sampling (voxel.hip): host arrays in, host arrays out ---------
hipError_t voxel_down_sample_device(const double *h_xyz, const double *h_nrm, const double *h_col,
                                    int64_t n, double voxel, double *h_out_xyz, double *h_out_nrm,
                                    double *h_out_col, int64_t *n_out, hipStream_t stream);
// ... the device part alone (resident input; the resident output in the caller's buffers, d_onrm / d_ocol or NULL), and the
// centroid of resident points with the host's summation order (centroid_f64): what the device-resident caller pipeline uses
hipError_t voxel_down_sample_core(const double *d_xyz, const double *d_nrm, const double *d_col, int64_t n, double voxel,
                                  drv::DevBuf<double> &d_oxyz, drv::DevBuf<double> *d_onrm, drv::DevBuf<double> *d_ocol,
                                  int64_t *n_out, hipStream_t stream);
hipError_t centroid_device(const double *d_xyz, int64_t n, int64_t chunk, double *d_part, double *d_out, hipStream_t stream);
// counting sort of the target by cell: start[ncell+1], sorted[nt] = (x,y,z, bits(orig index))
// tgt64 / sorted64 (both or neither): the f64 copy of the target is scattered in the same order
size_t exclusive_scan_u32_tmp_bytes(long long n);
hipError_t launch_exclusive_scan_u32_lib(const unsigned *in, long long n, unsigned *out, void *tmp, size_t tmp_bytes,
                                         hipStream_t stream);
// (cell_of: 2 * nt words; bsum: grid_scan_blocks(g.ncell) + 1 words)
hipError_t launch_grid_build(const float4 *tgt, int64_t nt, const GridParams &g,
                             unsigned *cell_of, unsigned *count, unsigned *bsum,
                             unsigned *start, float4 *sorted, hipStream_t stream,
                             const Pt64 *tgt64 = nullptr, Pt64 *sorted64 = nullptr);
// ---- the grid searches (grid.hip, grid_coop.hip, grid_wave.hip, grid_ring.hip) -----------------------------------
// fused transform + grid NN + Jacobian/residual + reduction to partial rows (launch_finalize folds them, or the
// launch itself: SearchArgs::fold); also writes idx_out / d2_out.
// The exact search with the candidates of a wave flattened over its lanes (grid_coop.hip; grid_wave.hip: round 3's
// kernel behind the same code, for batches and sweeps): the lanes code G = 1, U = 99.  launch_nn_grid_reduce falls back
// to the lane-serial kernel (1, 8) where it does not apply (fp32-only / all-f64 search, half-pitch rows, no wst_io).
constexpr int kCoopLanes = 9901;
// The bits of SearchArgs::warm -- a kernel argument of the flattened searches: the values are fixed.
enum : int {
    kWarmRead = 1,       // wst_io holds the winners of the previous pass over the SAME source order and target: start from them
    kWarmMap = 2,        // batches: a workgroup -> problem map (one int per workgroup) follows descs[nprob]
    kWarmTprev = 4,      // Tprev is valid (launch_nn_coop sets / clears it from SearchArgs::Tprev, device loops from
                         // DevIcpState::have_prev): queries whose winner provably cannot have changed skip the search
    kWarmNoCert = 8,     // certificates switched off (VISMA_ICP_CERT=0, A/B timing) -- the wave kernel's no-partner one too
    kWarmPrioShift = 5, kWarmPrioMask = 3   // bits 5-6: VISMA_ICP_PERSIST_PRIO 1 / 2 of a persistent launch (experiment)
};
// The persistent form of the batch / sweep search over SHARED clouds (grid_wave.hip, round 6): ONE launch runs up to
// max_passes warm passes of nprob problems of bpp workgroups each -- search, fold, closed-form update, compose and stop
// test inside the launch (fused_fold<..., LOOPED, SOLVE>), the next transform handed to the problem's workgroups through
// `relay` (32 words per problem, device memory, zeroed by the caller).  Every workgroup must be resident at once
// (nn_wave_sweep_capacity()).  `dead`: one word, zeroed by the caller; nonzero afterwards = a wait ran out (somebody's
// workgroups were not resident): the states hold what was completed, the caller carries on with ordinary launches.
struct SweepArgs {
    unsigned long long *relay;
    unsigned long long *dead;
    int max_passes;
    unsigned tag0;             // the command for pass p (p >= 1) carries tag0 + p; pass 0 reads the state itself
    int passes0;               // DevIcpState::passes of every problem when the launch begins (its first pass makes it passes0 + 1)
    long long wait_ticks;      // how long a workgroup waits for its problem's next transform (100 MHz ticks)
};

// What a search launch is given (host side only: the launchers spread it over the kernels' own argument lists).
// Shared clouds (descs == NULL): nprob problems search the same source against the same target.  Batches (descs):
// every problem has its own clouds at offsets into concatenated arrays, its grid in descs[] and its transform, frame
// offset and radius in st[] -- ns, g, ring, T32, T64, off, r2f, r2d, max_blocks, out_stride, d64_out stay as they are here.
struct SearchArgs {
    // ---- source
    int64_t ns = 0;
    const float4 *src = nullptr;
    const Pt64 *src64 = nullptr;           // f64 views of source and target: both or neither (fp32-only search)
    // ---- target
    const float4 *sorted = nullptr;        // cell-sorted, w = original index: the fp32-only and the all-f64 search
    const float *sorted12 = nullptr;       // ... its packed copy, 12 bytes per point: what the exact search ranks on
    const Pt64 *sorted64 = nullptr;
    const unsigned *start = nullptr;       // cell table
    GridParams g{};
    RingTable ring{nullptr, 0};            // the visiting order of a grid with g.ring > 0 (grid_ring.hip)
    const float4 *nrm = nullptr;           // target normals by ORIGINAL index (batches: concatenated like the unsorted
    const Pt64 *nrm64 = nullptr;           // targets) -> the point-to-plane estimator
    // ---- problems
    const ProbDesc *descs = nullptr;       // device: every problem's offsets / grid / workgroup range
    int nprob = 1;
    int max_blocks = 1;                    // shared clouds: cap of the workgroups per problem (search_blocks)
    int total_blocks = 0;                  // batches: sum of descs[].nblocks
    int one_per_lane = 0;                  // batches: no problem has more than G queries per lane group
    int64_t out_stride = 0;                // shared clouds: problem b writes idx_out / d2_out / wst_io at b * out_stride
    // ---- the pass
    Xform32 T32{};
    Xform64 T64{};
    Offset64 off{};
    float r2f = 0.f;
    double r2d = 0.0;
    int point_to_plane = 0;
    int exact = 0;                         // with the f64 views: fp32 ranking + f64 re-rank (1) or f64 throughout (0)
    int lanes = 0;                         // lanes code G + 100 U (lanes per query, loads in flight per lane), or kCoopLanes
    DevIcpState *st = nullptr;             // device loops: the problems' states (transform, radius, frame offset from there)
    int warm = 0;                          // kWarm* bits
    const Xform64 *Tprev = nullptr;        // the transform of the pass that left wst_io (host-driven passes; see kWarmTprev)
    FoldArgs fold{};                       // fold.tickets == NULL: the partial rows are folded by a separate launch
    const PersistArgs *persist = nullptr;  // run the launch as the persistent certificate kernel: one problem, one query
                                           // per lane, fused fold with host publication; hipErrorInvalidValue where that
                                           // does not apply -- ask coop_persist_capacity first
    // ---- outputs and per-query state
    int32_t *idx_out = nullptr;
    float *d2_out = nullptr;
    double *d64_out = nullptr;             // f64 squared distances (target-sharded ranks compare shards in f64), or NULL
    double *partials = nullptr;            // one row of kReduceAcc per workgroup
    unsigned long long *cand_count = nullptr;   // profiling counters, or NULL
    Pt64 *wst_io = nullptr;                // one per query, laid out like idx_out: the exact searches leave their winners
                                           // there (f64 point, original index | LB << 32 -- grid_coop.hip; NaN coordinates =
                                           // none, all bits set = nothing known); read when warm & kWarmRead
    Pt64 *ru_io = nullptr;                 // the runner-up half of that state (-DVISMA_COOP_RU=1 builds), or NULL

    // which candidate array the kernels read: sorted12 (true) or sorted
    bool packed() const { return src64 != nullptr && exact != 0; }
};
// workgroups per problem of a pass over shared clouds: one lane group of G = lanes % 100 per query up to the cap
inline int search_blocks(int64_t ns, int lanes, int max_blocks)
{
    const int64_t want = (ns * (lanes % 100) + kBlock - 1) / kBlock;
    const int nb = (int)(want > max_blocks ? max_blocks : want);
    return nb < 1 ? 1 : nb;
}
// the geometry launch_nn_grid_reduce hands to the launchers behind it
struct SearchGeom {
    int total_blocks, bpp;                 // workgroups of the launch / per problem (batches: 1)
    int one;                               // at most one query per lane
};
// Every kind of pass: the ring search (g.ring > 0), the flattened exact search (lanes == kCoopLanes) or the lane-serial
// kernel of the (G, U) pairs the policies use; shared clouds run nprob * search_blocks(ns, lanes, max_blocks) workgroups.
hipError_t launch_nn_grid_reduce(const SearchArgs &a, hipStream_t stream);
hipError_t launch_nn_coop(const SearchArgs &a, const SearchGeom &geo, hipStream_t stream);
hipError_t launch_nn_wave(const SearchArgs &a, const SearchGeom &geo, hipStream_t stream);
// the ring search over cells smaller than the radius: a.lanes % 100 = 1, 2, 4, 8 lanes per query, `nblocks` workgroups
// per problem; candidates ranked in fp32 on sorted12 with the f64 re-rank of the rounding band (a.packed()), or in f64
// throughout -- same results.  wst_io is always written.
hipError_t launch_nn_ring(const SearchArgs &a, int nblocks, hipStream_t stream);
// the persistent sweep: nprob problems of search_blocks(ns, kCoopLanes, max_blocks) workgroups, one query per lane
hipError_t launch_nn_wave_sweep(const SearchArgs &a, const SweepArgs &sa, hipStream_t stream);
// the visiting order of a grid with g.ring = rings (a new device buffer the caller owns: hipFree); *nrows = (2 rings + 1)^2
hipError_t build_ring_table(int rings, drv::DevBuf<RingRow> &d_tab);
// ... the same order on the host (empty for rings outside 1 .. kRingMaxRings)
std::vector<RingRow> ring_visiting_order(int rings);
// *out (device, zeroed by the caller) += the number of non-zero entries of count[0 .. n)
hipError_t launch_count_occupied(const unsigned *count, int64_t n, unsigned long long *out, hipStream_t stream);
int nn_wave_sweep_capacity();
// workgroups of the persistent kernel the current device holds at once (0: none -- do not launch it)
int coop_persist_capacity(int point_to_plane);
hipError_t launch_finalize_solve_batch(const double *partials, const ProbDesc *descs, DevIcpState *st,
                                       int nprob, hipStream_t stream, int plane = 0);

// ---- passes over the pairs of the last nn_pass (pair_pass.h; trim.hip, robust.hip, gicp.hip, colored.hip, information.hip) ----
// One grid, one row stride, one ticket word and one scratch (HipEngine::PairScratch) for all of them: they never overlap
// on the stream.
constexpr int kPairThreads = 256;
constexpr int kPairRow = 32;                           // doubles per partial row (a pass stores and folds its first kAcc columns)
constexpr int kPairMaxBlocks = 1024;                   // rows of the partials buffer: the cap of pair_reduce_blocks
constexpr int kPairMaxPublished = kNStats + 4;         // granules of the mapped host buffer: the robust pass publishes the most
inline int pair_reduce_blocks(int64_t ns)
{
    const int64_t want = (ns + kPairThreads - 1) / kPairThreads;
    return (int)(want < 1 ? 1 : (want > kPairMaxBlocks ? kPairMaxBlocks : want));
}
// the work words (PairScratch::work): the select's histograms, four tickets, then its state
constexpr int kTrimHistWords = 3 * 2048;               // three rounds of up to 2048 bins
constexpr int kSelectRounds = 3;                       // each round takes one ticket, then ...
constexpr int kPairTicketWord = kTrimHistWords + kSelectRounds;   // ... the reduction's
constexpr int kSelectStateWord = kPairTicketWord + 1;  // {cut d2 bits, need, ties, cut index}
constexpr int kTrimWorkWords = kSelectStateWord + 4;
// what every such reduction is given
struct PairPassArgs {
    const float4 *src = nullptr, *tgt = nullptr;       // fp32 clouds (caller's target order), or ...
    const Pt64 *src64 = nullptr, *tgt64 = nullptr;     // ... the f64 copies when the pass summed from them
    const int32_t *idx = nullptr;                      // the pass's winners per source position (< 0: no pair)
    int64_t ns = 0;
    Xform64 T64{};
    Offset64 off{};
    double *partials = nullptr;                        // one row of kPairRow doubles per workgroup
    unsigned *ticket = nullptr;                        // the word kPairTicketWord of the work words: zero before the first pass (self re-arming)
    double *host_out = nullptr;                        // mapped host memory: granules {value, seq}
    unsigned long long seq = 0;
};

// ---- trimmed ICP (trim.hip): the m pairs with the smallest key (d2, source index) of the last pass ----
constexpr int kTrimPublished = kNStats + 2;            // granules to the host: 38 statistics, cut d2, kept pairs
struct TrimReduceArgs : PairPassArgs {
    const float *d2 = nullptr;                         // the winners' fp32 squared distances: the ranking value
    const int32_t *order = nullptr;                    // source position -> caller's source index (NULL: identity)
    unsigned *work = nullptr;                          // the work words the select runs on: its state holds the cut
    unsigned char *mask = nullptr;                     // out: 1 per kept source position
};
int trim_select_blocks(int64_t ns);
// the three rounds of the select; m in [1, K]: the rank of the cut among the pairs; work: kTrimWorkWords words, zero
// before the first pass (self re-arming)
hipError_t launch_trim_select(const float *d2, const int32_t *idx, const int32_t *order, int64_t ns, unsigned m, unsigned *work,
                              hipStream_t stream);
hipError_t launch_trim_reduce(const TrimReduceArgs &a, hipStream_t stream);

// ---- robust ICP (robust.hip): every pair of the last pass weighted by a function of its own residual ----
constexpr int kRobustL2 = 0, kRobustHuber = 1, kRobustTukey = 2, kRobustCauchy = 3;   // = VISMA_ICP_ROBUST_*
constexpr int kRobustPublished = kNStats + 4;          // granules to the host: 38 statistics, c, v, pairs with w == 0, sum w r^2
struct RobustArgs : PairPassArgs {
    const float4 *nrm = nullptr;                       // target normals by original index (point-to-plane), and ...
    const Pt64 *nrm64 = nullptr;                       // ... in f64 where the f64 passes read them
    int kernel = kRobustHuber;                         // kRobustHuber / Tukey / Cauchy
    int auto_scale = 0;                                // 0: c = scale; 1: c = max(tune_k * sqrt(v), min_scale), v from the select
    double scale = 0.0, tune_k = 0.0, min_scale = 0.0; // tune_k = tune * 1.4826
    const unsigned *select_work = nullptr;             // the select's work words: its state holds v's bits
    float *r2_out = nullptr;                           // residual kernel: (float)(r^2) per source position
    double *w_out = nullptr;                           // out: the weight per source position (0: no pair)
};
hipError_t launch_robust_residual(const RobustArgs &a, hipStream_t stream);
hipError_t launch_robust_reduce(const RobustArgs &a, int plane, hipStream_t stream);

// ---- generalized ICP (gicp.hip): every pair of the last pass weighted by the inverse of the sum of both points' surface covariances ----
constexpr int kGicpPublished = kNStats + 1;            // granules to the host: 38 statistics, sum d^T M d
struct GicpArgs : PairPassArgs {
    const float4 *nrm = nullptr, *snrm = nullptr;      // target normals by original index, source normals by source position, and ...
    const Pt64 *nrm64 = nullptr, *snrm64 = nullptr;    // ... in f64 where the f64 passes read them (each on its own: NULL = the fp32 copy)
    double epsilon = 1.0;                              // the covariance along the normal, in (0, 1]
};
hipError_t launch_gicp_reduce(const GicpArgs &a, hipStream_t stream);

// ---- colored ICP (colored.hip): a photometric row next to the point-to-plane row of every pair ----
constexpr int kColoredPublished = kNStats + 2;         // granules to the host: 38 statistics, sum r_g^2, sum r_c^2
struct ColoredArgs : PairPassArgs {
    const float4 *nrm = nullptr;                       // target normals by original index, and ...
    const Pt64 *nrm64 = nullptr;                       // ... in f64 where the f64 passes read them
    const double *grad = nullptr;                      // the target's colour gradient, 3 doubles per point by original index
    const double *src_int = nullptr, *tgt_int = nullptr;   // intensities: by source position, by original target index
    double sqrt_lambda = 1.0, sqrt_one_minus_lambda = 0.0;
};
hipError_t launch_colored_reduce(const ColoredArgs &a, hipStream_t stream);

// ---- information matrix (information.hip): the ten sums over the target points of the last pass's pairs ----
constexpr int kInfoAcc = 10;                           // K, sum x, y, z, sum xx, yy, zz, xy, xz, yz: what is published, too
struct InformationArgs : PairPassArgs {};
hipError_t launch_information_reduce(const InformationArgs &a, hipStream_t stream);

// ---- RGB-D odometry (odometry_image.hip, odometry.hip): single-channel fp32 images, row-major ----
constexpr int kOdoMaxLevels = 8;
// the images of a pyramid level (visma_icp_odometry_get_image's `which`); kOdoSrcXyz has three floats per pixel
enum { kOdoSrcGray = 0, kOdoSrcDepth, kOdoTgtGray, kOdoTgtDepth, kOdoTgtGrayDx, kOdoTgtGrayDy, kOdoTgtDepthDx, kOdoTgtDepthDy,
       kOdoSrcXyz, kOdoImages };
constexpr int kOdoColor = 0, kOdoHybrid = 1;           // = VISMA_ICP_ODOMETRY_COLOR / HYBRID
// d < min_depth || d > max_depth || d <= 0 -> NaN (in place is allowed)
hipError_t launch_odo_preprocess_depth(const float *in, float *out, int64_t n, double min_depth, double max_depth, hipStream_t stream);
// one 3-tap pass along the rows (vertical == 0) or down the columns, indices clamped at the borders
hipError_t launch_odo_filter3(const float *in, float *out, int w, int h, float k0, float k1, float k2, int vertical, hipStream_t stream);
// out = floor(w / 2) x floor(h / 2)
hipError_t launch_odo_downsample(const float *in, int w, int h, float *out, hipStream_t stream);
// img = (float)(scale * img + 0.0)
hipError_t launch_odo_scale(float *img, int64_t n, double scale, hipStream_t stream);
// out[y * w + x] = {(float)((x - ox) * z * inv_fx), (float)((y - oy) * z * inv_fy), z, 0}
hipError_t launch_odo_xyz(const float *depth, int w, int h, double ox, double oy, double inv_fx, double inv_fy, float4 *out,
                          hipStream_t stream);
struct OdoProjection { double m[9]; double kt[3]; };   // K R K^-1 (row-major) and K t, formed on the host in f64
// idx[v_s * w + u_s] = v_t * w + u_t or -1
hipError_t launch_odo_correspondences(const float *depth_s, const float *depth_t, int w, int h, const OdoProjection &P,
                                      double max_depth_diff, int32_t *idx, hipStream_t stream);
// the sums NormalizeIntensity divides: publishes {K, sum gray_s over the pairs' source pixels, sum gray_t over their target pixels}
constexpr int kOdoMeanAcc = 3;
struct OdoMeanArgs : PairPassArgs { const float *gray_s = nullptr, *gray_t = nullptr; };
hipError_t launch_odo_mean_reduce(const OdoMeanArgs &a, hipStream_t stream);
// one Gauss-Newton step's sums over the pairs idx: publishes the 38 statistics {K, sum r^2, 21 of J^T J, 6 of J^T r, zeros}
struct OdometryArgs : PairPassArgs {
    const float *gray_s = nullptr, *gray_t = nullptr, *depth_t = nullptr;
    const float *gray_dx = nullptr, *gray_dy = nullptr, *depth_dx = nullptr, *depth_dy = nullptr;   // the target's Sobel images
    const float4 *xyz_s = nullptr;
    double fx = 0.0, fy = 0.0;                         // of the level
    double w_photo = 1.0, w_depth = 0.0;               // hybrid: sqrt(1 - 0.968), sqrt(0.968), formed on the host; colour: 1 (unused)
    int method = kOdoHybrid;
};
hipError_t launch_odometry_reduce(const OdometryArgs &a, hipStream_t stream);

// ---- TSDF integration (tsdf.hip): a uniform volume, or the units of a scalable one, resident on the device ----
constexpr int kTsdfColorNone = 0, kTsdfColorRgb8 = 1, kTsdfColorGray32 = 2;   // = VISMA_ICP_TSDF_COLOR_*
struct TsdfConfig {
    int resolution = 0;
    double length = 0.0, sdf_trunc = 0.0;
    int color_type = kTsdfColorNone;
    double origin[3] = {0.0, 0.0, 0.0};
    // a scalable volume (ScalableTSDFVolume): resolution and length are a UNIT's (length = voxel_length * resolution, so
    // that a unit's own voxel length is length / resolution as the reference's OpenVolumeUnit makes it); origin is unused
    int scalable = 0;
    double voxel_length = 0.0;
    int stride = 4;                                    // depth_sampling_stride
    int initial_units = 0;                             // the pool's first capacity (it doubles when it is full)
};
// one frame (host arrays): depth w x h fp32; color w x h x 3 uint8 (RGB8), w x h fp32 (Gray32) or NULL; extrinsic row-major
struct TsdfFrame {
    int w = 0, h = 0;
    const float *depth = nullptr;
    const void *color = nullptr;
    double fx = 0.0, fy = 0.0, cx = 0.0, cy = 0.0;
    double extrinsic[16] = {};
    bool on_device = false;                            // depth and color lie on this device (a resident Image's pixels)
};
// out[y * w + x] = sqrtf(xx^2 + yy^2 + 1), xx = ((float)x - (float)cx) * (1.0f / (float)fx): the multiplier image of a frame
hipError_t launch_tsdf_multiplier(float *out, int w, int h, double fx, double fy, double cx, double cy, hipStream_t stream);
struct TsdfDevice;                                     // the volume, the last frame and the last extraction on the device
// allocates the zero-filled volume; nothing is left allocated where it fails
hipError_t tsdf_device_create(const TsdfConfig &cfg, hipStream_t stream, TsdfDevice **out);
void tsdf_device_destroy(TsdfDevice *D);
hipError_t tsdf_device_reset(TsdfDevice *D);
// Integrate; pose = extrinsic^-1 (row-major, inverted by the caller in f64; read by a scalable volume only).  Returns with
// the stream idle (the frame is the caller's pageable memory).  A scalable volume opens every touched unit first; where the
// pool cannot grow it returns the error with the volume as it was.
hipError_t tsdf_device_integrate(TsdfDevice *D, const TsdfFrame &f, const double pose[16]);
// ExtractPointCloud (voxel_cloud == 0) or ExtractVoxelPointCloud into the device's output buffers: *n rows
hipError_t tsdf_device_extract(TsdfDevice *D, int voxel_cloud, int64_t *n);
// the rows of the last extraction of that kind (n x 3 doubles each; normals / colors may be NULL)
hipError_t tsdf_device_get_extract(TsdfDevice *D, int voxel_cloud, double *points, double *normals, double *colors);
// ExtractTriangleMesh (marching cubes; the case rule: mc_table.h) into the device's mesh buffers: *nv vertices, *nt triangles.
// hipErrorInvalidValue: more than 2^31 - 1 of either (vertex indices are int32).  Nothing is launched over a volume of
// R < 2, or over a scalable volume without units.
hipError_t tsdf_device_extract_mesh(TsdfDevice *D, int64_t *nv, int64_t *nt);
// the rows of the last mesh (vertices, colors nv x 3 doubles, triangles nt x 3 int32; each may be NULL)
hipError_t tsdf_device_get_mesh(TsdfDevice *D, double *vertices, double *colors, int32_t *triangles);
// the last mesh where it lies ON THE DEVICE (colors NULL for a volume without colour); false: no mesh since the last change
struct TsdfMeshView {
    const double *vertices = nullptr, *colors = nullptr;
    const int32_t *triangles = nullptr;
    int64_t nv = 0, nt = 0;
};
bool tsdf_device_mesh_view(const TsdfDevice *D, TsdfMeshView *view);
// the last ExtractPointCloud (voxel_cloud == 0) or ExtractVoxelPointCloud likewise (normals NULL for the voxel cloud, colors
// NULL for a surface cloud of a volume without colour); false: no such extraction since the last change
struct TsdfCloudView {
    const double *points = nullptr, *normals = nullptr, *colors = nullptr;
    int64_t n = 0;
};
bool tsdf_device_cloud_view(const TsdfDevice *D, int voxel_cloud, TsdfCloudView *view);
// the indices of a scalable volume's units, 3 per unit, in lexicographic order (the order of its extractions)
void tsdf_device_get_units(const TsdfDevice *D, std::vector<int32_t> *keys);
// tsdf, weight (R^3) and color (R^3 x 3, interleaved as the reference keeps it) of a uniform volume (unit == NULL) or of
// the unit with that index (hipErrorInvalidValue: no such unit); each output may be NULL
hipError_t tsdf_device_get_volume(TsdfDevice *D, const int32_t *unit, float *tsdf, float *weight, float *color);
// CreatePointCloudFromDepthImage / FromRGBDImage: pose = extrinsic^-1 (row-major, inverted by the caller in f64);
// color_type as above.  points / colors: room for ceil(w / stride) * ceil(h / stride) rows, or NULL (count only).
// cloud != NULL: the rows stay on the device as a new resident cloud (points, colours), nothing is downloaded.
// f.on_device: depth and color lie on this device
struct CloudDevice;
hipError_t point_cloud_from_depth_device(const TsdfFrame &f, const double pose[16], int color_type, int stride, double *points,
                                         double *colors, int64_t *n, hipStream_t stream, CloudDevice **cloud = nullptr);

// ---- TriangleMesh (trimesh.hip): a mesh resident on the device: normals, Purge, select, crop, Transform ----
// Every result is the reference's bit for bit (TriangleMesh.cpp, DownSample.cpp); the rules: visma_icp.h.  Each call returns
// with the stream idle.  The arguments are checked by the caller (aux_api.cpp) but for the indices: a triangle index outside
// [0, nv) (create) or a selected index outside it (select) is hipErrorInvalidValue, and nothing is made.
constexpr int kTriMeshVertexNormals = 1, kTriMeshVertexColors = 2, kTriMeshTriangleNormals = 4;
struct TriMeshDevice;
// vn, vc, tn may be NULL.  on_device: the arrays lie on this device and are copied there (the mesh of a TSDF volume)
hipError_t trimesh_device_create(const double *v, int64_t nv, const double *vn, const double *vc, const int32_t *tri, int64_t nt,
                                 const double *tn, bool on_device, hipStream_t stream, TriMeshDevice **out);
void trimesh_device_destroy(TriMeshDevice *M);
void trimesh_device_size(const TriMeshDevice *M, int64_t *nv, int64_t *nt, int *flags);
// each output may be NULL; an attribute the mesh does not have is not written
hipError_t trimesh_device_get(TriMeshDevice *M, double *v, double *vn, double *vc, int32_t *tri, double *tn, hipStream_t stream);
hipError_t trimesh_device_normalize_normals(TriMeshDevice *M, hipStream_t stream);
hipError_t trimesh_device_compute_triangle_normals(TriMeshDevice *M, bool normalized, hipStream_t stream);
hipError_t trimesh_device_compute_vertex_normals(TriMeshDevice *M, bool normalized, hipStream_t stream);
// step 0 .. 3: RemoveDuplicatedVertices, RemoveDuplicatedTriangles, RemoveNonManifoldTriangles, RemoveNonManifoldVertices
hipError_t trimesh_device_remove(TriMeshDevice *M, int step, int64_t *removed, hipStream_t stream);
hipError_t trimesh_device_purge(TriMeshDevice *M, int64_t removed[4], hipStream_t stream);
// a new mesh, purged (the source's scratch buffers are used: it is not const)
hipError_t trimesh_device_select(TriMeshDevice *S, const int64_t *indices, int64_t n, hipStream_t stream, TriMeshDevice **out);
hipError_t trimesh_device_crop(TriMeshDevice *S, const double lo[3], const double hi[3], hipStream_t stream, TriMeshDevice **out);
hipError_t trimesh_device_transform(TriMeshDevice *M, const double T[16], hipStream_t stream);
// the vertices and triangles on the device, for a reader on the same stream (render.hip)
void trimesh_device_arrays(const TriMeshDevice *M, int64_t *nv, int64_t *nt, const double **v, const int **tri);

// ---- PointCloud (cloud.hip): a cloud resident on the device: points and, optionally, normals and colours, n x 3 f64 ----
// Every result is the reference's bit for bit but for the stated deviations (PointCloud.cpp, DownSample.cpp,
// EstimateNormals.cpp); the rules: visma_icp.h.  Each call returns with the stream idle.  The arguments are checked by the
// caller (aux_api.cpp) but for the selected indices: one outside [0, n) is hipErrorInvalidValue, and nothing is made.
constexpr int kCloudNormals = 1, kCloudColors = 2;
struct CloudDevice;
// normals, colors may be NULL.  on_device: the arrays lie on this device and are copied there (the cloud of a TSDF volume)
hipError_t cloud_device_create(const double *points, int64_t n, const double *normals, const double *colors, bool on_device,
                               hipStream_t stream, CloudDevice **out);
void cloud_device_destroy(CloudDevice *P);
void cloud_device_size(const CloudDevice *P, int64_t *n, int *flags);
// each output may be NULL; an attribute the cloud does not have is not written
hipError_t cloud_device_get(CloudDevice *P, double *points, double *normals, double *colors, hipStream_t stream);
hipError_t cloud_device_transform(CloudDevice *P, const double T[16], hipStream_t stream);
hipError_t cloud_device_normalize_normals(CloudDevice *P, hipStream_t stream);
hipError_t cloud_device_paint_uniform_color(CloudDevice *P, const double rgb[3], hipStream_t stream);
hipError_t cloud_device_append(CloudDevice *P, const CloudDevice *other, hipStream_t stream);       // other may be P
hipError_t cloud_device_bounds(CloudDevice *P, double lo[3], double hi[3], hipStream_t stream);
// a new cloud (the source's scratch buffers are used: it is not const)
hipError_t cloud_device_select(CloudDevice *S, const int64_t *indices, int64_t n, hipStream_t stream, CloudDevice **out);
hipError_t cloud_device_uniform_down_sample(CloudDevice *S, int64_t every_k, hipStream_t stream, CloudDevice **out);
hipError_t cloud_device_crop(CloudDevice *S, const double lo[3], const double hi[3], hipStream_t stream, CloudDevice **out);
hipError_t cloud_device_voxel_down_sample(CloudDevice *S, double voxel, hipStream_t stream, CloudDevice **out);
hipError_t cloud_device_estimate_normals(CloudDevice *P, int search_type, int knn, double radius, hipStream_t stream);
// camera == false: OrientNormalsToAlignWithDirection(ref); true: OrientNormalsTowardsCameraLocation(ref).  The cloud has normals
hipError_t cloud_device_orient_normals(CloudDevice *P, bool camera, const double ref[3], hipStream_t stream);
// chunk: the points a serial sum runs over (the chunk sums are added in chunk order)
hipError_t cloud_device_mean_and_covariance(CloudDevice *P, int64_t chunk, double mean[3], double cov[9], hipStream_t stream);
// inv: the inverse covariance, row-major; out: n doubles on the host
hipError_t cloud_device_mahalanobis(CloudDevice *P, const double mean[3], const double inv[9], double *out, hipStream_t stream);

// ---- Image (image.hip): an image resident on the device: w x h pixels of ch channels of bpc bytes, row-major ----
// Every result is the reference's bit for bit but for the stated deviations (Image.cpp, ImageFactory.cpp,
// RGBDImageFactory.cpp); the rules: visma_icp.h.  Each call returns with the stream idle.  The arguments are checked by the
// caller (aux_api.cpp).  "The empty image" is the reference's Image(): 0 x 0, no channels.
struct ImageDevice;
// on_device: `data` lies on this device and is copied there
hipError_t image_device_create(int w, int h, int ch, int bpc, const void *data, bool on_device, hipStream_t stream, ImageDevice **out);
void image_device_destroy(ImageDevice *I);
void image_device_info(const ImageDevice *I, int *w, int *h, int *ch, int *bpc);
const void *image_device_pixels(const ImageDevice *I);  // on the device
hipError_t image_device_get(const ImageDevice *I, void *bytes, hipStream_t stream);
// a new image with uninitialised pixels for a kernel of another file to fill (render.hip).  integer: 1 x 4 bytes that hold
// int32, which no operation on float images accepts
hipError_t image_device_alloc(int w, int h, int ch, int bpc, bool integer, ImageDevice **out);
void *image_device_pixels_rw(ImageDevice *I);
bool image_device_is_integer(const ImageDevice *I);
// new images.  ImageScratch: what the two-pass operations work in, one per context (grow-only)
struct ImageScratch;
ImageScratch *image_scratch_create();
void image_scratch_destroy(ImageScratch *W);
hipError_t image_device_copy(const ImageDevice *S, hipStream_t stream, ImageDevice **out);
hipError_t image_device_to_float(const ImageDevice *S, int weighted, hipStream_t stream, ImageDevice **out);
hipError_t image_device_depth_to_float(const ImageDevice *S, double depth_scale, double depth_trunc, hipStream_t stream, ImageDevice **out);
hipError_t image_device_from_float(const ImageDevice *S, int bytes, hipStream_t stream, ImageDevice **out);
hipError_t image_device_filter_horizontal(const ImageDevice *S, ImageScratch *W, const double *kernel, int n, hipStream_t stream, ImageDevice **out);
hipError_t image_device_filter_separable(const ImageDevice *S, ImageScratch *W, const double *dx, int n_dx, const double *dy, int n_dy, hipStream_t stream,
                                         ImageDevice **out);
hipError_t image_device_flip(const ImageDevice *S, hipStream_t stream, ImageDevice **out);
hipError_t image_device_downsample(const ImageDevice *S, hipStream_t stream, ImageDevice **out);
hipError_t image_device_dilate(const ImageDevice *S, ImageScratch *W, int half_kernel_size, hipStream_t stream, ImageDevice **out);
// the SUN (nyu == false) or NYU decoding of a 1 x uint16 depth image
hipError_t image_device_decode_depth(const ImageDevice *S, bool nyu, hipStream_t stream, ImageDevice **out);
hipError_t image_device_distance_multiplier(int w, int h, const double intrinsic[4], hipStream_t stream, ImageDevice **out);
// in place; an unsupported format is left as it is
hipError_t image_device_linear_transform(ImageDevice *I, double scale, double offset, hipStream_t stream);
hipError_t image_device_clip_intensity(ImageDevice *I, double lo, double hi, hipStream_t stream);
// uv: n x 2 doubles on the host; ok, value: n each on the host
hipError_t image_device_float_value_at(const ImageDevice *I, const double *uv, int64_t n, uint8_t *ok, double *value, hipStream_t stream);

// ---- the mesh renderer (render.hip): a resident TriangleMesh into resident depth, index, mask and edge Images ----
// The rule is render_math.hpp's (visma_icp.h states it); visma_icp_render_host runs the same functions on the host.
struct RenderCamera;
struct RenderScratch;                                  // what a render works in, one per context (grow-only)
RenderScratch *render_scratch_create();
void render_scratch_destroy(RenderScratch *W);
// E: world -> camera, row-major 4 x 4 (the fourth row is not read).  depth, index, mask: each may be NULL
hipError_t render_device_render(RenderScratch *W, const TriMeshDevice *M, const RenderCamera &c, const double E[16], int encoding,
                                hipStream_t stream, ImageDevice **depth, ImageDevice **index, ImageDevice **mask);
// depth: 1 x float
hipError_t render_device_edges(const ImageDevice *depth, hipStream_t stream, ImageDevice **out);

// ---- color map optimization (colormap.hip): frames, vertices, visibility and poses resident on the device ----
constexpr int kColorMapSums = 29;                      // per camera: 21 upper entries of JJ (row by row), 6 of Jb, rr, count
constexpr int kColorMapMaxBlocks = 512;                // workgroups per camera of the iteration launch: beyond 512 * 256 visible
                                                       // vertices a camera's list is walked in strides (measured:
                                                       // profiles/colormap_blocks_ab.txt)
struct ColorMapConfig {
    int w = 0, h = 0, n_images = 0;
    double fx = 0.0, fy = 0.0, cx = 0.0, cy = 0.0;
    double max_depth = 2.5, visibility_threshold = 0.03, discontinuity_threshold = 0.1;
    int half_dilation = 3;
    int anchors = 0;                                   // > 0: a NON-RIGID map (colormap_warp.hip) with that many vertical anchors
    double anchor_weight = 0.316;                      // ... and its non_rigid_anchor_point_weight
};
struct ColorMapDevice;
// allocates the frames' buffers; nothing is left allocated where it fails
hipError_t color_map_device_create(const ColorMapConfig &cfg, hipStream_t stream, ColorMapDevice **out);
void color_map_device_destroy(ColorMapDevice *D);
// frame i: depth w x h fp32 (metres), rgb w x h x 3 uint8, extrinsic row-major (host arrays; copied before the return)
hipError_t color_map_device_set_image(ColorMapDevice *D, int i, const float *depth, const unsigned char *rgb, const double extrinsic[16]);
hipError_t color_map_device_set_vertices(ColorMapDevice *D, const double *vertices, int64_t n);
// gradient images, masks and the visibility of the poses as they are now; counts[n_images]: the cameras' visible vertices
hipError_t color_map_device_prepare(ColorMapDevice *D, int64_t *counts);
// which: 0 gray, 1 dx, 2 dy (w x h fp32), 3 mask (w x h uint8)
hipError_t color_map_device_get_image(ColorMapDevice *D, int i, int which, void *out);
int64_t color_map_device_visible_count(const ColorMapDevice *D, int i);
hipError_t color_map_device_get_visible(ColorMapDevice *D, int i, int32_t *out);      // ascending vertex ids
void color_map_device_get_extrinsics(const ColorMapDevice *D, double *out);           // n_images x 16
hipError_t color_map_device_set_extrinsics(ColorMapDevice *D, const double *in);
hipError_t color_map_device_get_proxy(ColorMapDevice *D, double *out);                // n_vertices, of the current poses
// rows[n_images x kColorMapSums] at the current poses; nothing moves
hipError_t color_map_device_sums(ColorMapDevice *D, double *rows);
// one Gauss-Newton iteration of every camera; rr[n_images], count[n_images] (a camera with count < 6 or a singular system
// keeps its pose)
hipError_t color_map_device_step(ColorMapDevice *D, double *rr, int64_t *count);
hipError_t color_map_device_get_colors(ColorMapDevice *D, double *out);               // n_vertices x 3, of the current poses
// -- a non-rigid map (cfg.anchors > 0; colormap_warp.hip); hipErrorInvalidValue on a rigid one --
hipError_t color_map_device_get_flow(const ColorMapDevice *D, double *out);           // n_images x 2 aw ah
hipError_t color_map_device_set_flow(ColorMapDevice *D, const double *in);
// rows[n_images x (aw - 1)(ah - 1) x 121] at the current poses and fields; nothing moves
hipError_t color_map_device_cell_sums(ColorMapDevice *D, double *rows);
// one iteration of every camera: pose and field; rr, rr_reg, count [n_images] of the state BEFORE the step
hipError_t color_map_device_step_non_rigid(ColorMapDevice *D, double *rr, double *rr_reg, int64_t *count);

// ---- the colour side of colored ICP (color_gradient.hip, colored.hip) ----
// I = (r + g + b) / 3.0 in f64, in that order (ColoredICP.cpp:94-95)
inline double color_intensity(const double *rgb) { return (rgb[0] + rgb[1] + rgb[2]) / 3.0; }
void color_intensities(const double *rgb, int64_t n, int stride, const int32_t *order, double *out);
// What the gradient kernel is given, all on the device: points and normals in exactly one of three forms each (n x 3
// doubles, Pt64, float4), one intensity per point.  origin: the point the fp32 binning copy is taken relative to.
struct ColorGradientInput {
    const double *xyz = nullptr; const Pt64 *xyz64 = nullptr; const float4 *xyz32 = nullptr;
    const double *nrm = nullptr; const Pt64 *nrm64 = nullptr; const float4 *nrm32 = nullptr;
    const double *intensity = nullptr;
    int64_t n = 0;
    double origin[3] = {0.0, 0.0, 0.0};
};
// ---- the grid of ONE cloud that normals.hip, color_gradient.hip and fpfh.hip search (nn_grid.hip; the search: nn_list.h) ----
// what each of their kernels is given first
struct NnGridView {
    const float4 *sorted;        // cell-sorted fp32 copy (cell binning only)
    const Pt64 *sorted64;        // cell-sorted points, w = original index
    const unsigned *start;       // cell table
    GridParams g;
    const Pt64 *pts;             // original order
};
// The first finite point of the cloud, the origin of the fp32 binning copy; `origin` stays as it is where there is none.
void nn_binning_origin(const double *h_xyz, int64_t n, double origin[3]);
// The grid and its buffers, freed with the object.  knn_cap == 0: cells of edge 1.001 `radius`, the 27 cells around a point
// cover the radius.  knn_cap > 0 (a KNN search of that many neighbours, `radius` unused): cells of about the distance to the
// knn_cap-th neighbour, sized from the measured population of the 27 cells -- any size is exact there.
struct NnGrid {
    NnGridView view{};
    // the buffers that depend on n alone (the cell table's are build's own)
    hipError_t alloc(int64_t n);
    // Points from whichever of the three forms `in` holds; d_nrm3 != NULL: its Pt64 or float4 normals repacked there as
    // n x 3 doubles.  The last grid build is still queued when it returns.
    hipError_t build(const ColorGradientInput &in, double *d_nrm3, double radius, int knn_cap, hipStream_t stream);

    // (build's own)
    DevBufs bufs;
    int64_t n = 0;
    float4 *f4 = nullptr, *sorted = nullptr;
    Pt64 *p8 = nullptr, *sorted64 = nullptr;
    unsigned *box = nullptr, *cell_of = nullptr;
    unsigned long long *n27 = nullptr;       // (KNN) sum of the sampled 27-cell populations, points sampled
};

// (tests: nn_selftest.hip) the lists themselves, host arrays in and out, in the points' order: idx / d2 n x cap padded with
// -1 / +inf behind the min(cap, n) entries a list can hold, cnt n.  search_type 0 KNN | 1 Radius as the normals' counting
// pass (cnt only) | 2 Hybrid; list_kind 0 NnList in LDS (cap <= kNormalsMaxList) | 1 NnHeap in global memory, sorted.
hipError_t nn_selftest_lists_device(const double *h_xyz, int64_t n, int search_type, int cap, double radius, int list_kind,
                                    int32_t *h_idx, double *h_d2, int32_t *h_cnt, hipStream_t stream);

// ---- KDTreeFlann (kdtree.hip): a cloud resident on the device, searched for ANY query points (host arrays in and out) ----
// The search is nn_list.h's; the grid is NnGrid's, built for the radius or the knn of a call and kept for the next call with
// the same parameter.  Lists in the queries' order, ascending (d2, index); idx / d2 nq x cap, -1 / +inf behind a list.
constexpr int64_t kKdTreeSlabEntries = 1ll << 22;        // list entries one KNN / Hybrid launch writes (its queries: a slab)
constexpr int64_t kKdTreeMaxRadiusEntries = 1ll << 28;   // entries of one uncapped Radius result (12 bytes each on the device)
struct KdTreeDevice;
hipError_t kdtree_device_create(const double *h_xyz, int64_t n, hipStream_t stream, KdTreeDevice **out);
void kdtree_device_destroy(KdTreeDevice *T);
// cap = knn (radius unused) or max_nn; the arguments are checked by the caller (aux_api.cpp)
hipError_t kdtree_device_search(KdTreeDevice *T, bool knn, const double *h_q, int64_t nq, double radius, int cap,
                                int32_t *h_idx, double *h_d2, int32_t *h_cnt, hipStream_t stream);
// count, scan, write: offsets[nq + 1], *total; the lists stay on the device for kdtree_device_radius_result.  More than
// kKdTreeMaxRadiusEntries: hipErrorOutOfMemory with *total set and nothing kept.
hipError_t kdtree_device_search_radius(KdTreeDevice *T, const double *h_q, int64_t nq, double radius, int64_t *h_offsets,
                                       int64_t *total, hipStream_t stream);
// hipErrorNotReady without a radius search before it, hipErrorInvalidValue for a NULL array where there are entries
hipError_t kdtree_device_radius_result(KdTreeDevice *T, int32_t *h_idx, double *h_d2, hipStream_t stream);

// the gradient per point (n x 3 doubles on the device, the points' order) by the Hybrid search (radius, max_nn);
// max_nn outside [3, kNormalsMaxList]: hipErrorInvalidValue.  Returns with the stream idle.
hipError_t color_gradient_on_device(const ColorGradientInput &in, double radius, int max_nn, double *d_grad, hipStream_t stream);
// ... host arrays in and out; h_rgb: n x 3 colours
hipError_t color_gradient_device(const double *h_xyz, int64_t n, const double *h_nrm, const double *h_rgb, double radius,
                                 int max_nn, double *h_out, hipStream_t stream);
// ---- FPFH features and their matching (fpfh.hip, feature_match.hip): host arrays in, host arrays out ----
// open3d::ComputeFPFHFeature: n x 33 doubles, point-major; search_type 0 KNN(knn) | 2 Hybrid(radius, max_nn = knn), knn in
// [2, kNormalsMaxList], else hipErrorInvalidValue.  second_pass 0: the first pass's lists kept in global memory where they
// fit, 1: kept, 2: rebuilt by the second pass.  ms (may be NULL): device time of the grid build and of the two passes.
hipError_t compute_fpfh_device(const double *h_xyz, int64_t n, const double *h_nrm, int search_type, int knn, double radius,
                               double *h_out, int second_pass, double ms[3], hipStream_t stream);
// for every row of fb (nb x dim) the row of fa (na x dim) at the smallest flann-L2 distance, lowest index on ties, -1 and
// +inf where no distance is finite; dim in [1, 64].  h_d2 and kernel_ms may be NULL.
hipError_t match_features_device(const double *h_fa, int64_t na, const double *h_fb, int64_t nb, int dim, int32_t *h_nn,
                                 double *h_d2, double *kernel_ms, hipStream_t stream);
// ---- RANSAC global registration (ransac.hip; the arithmetic of one trial: ransac.hpp) ----
struct RansacProblem {                                 // host arrays
    const double *src = nullptr; int64_t ns = 0;       // ns x 3
    const double *tgt = nullptr; int64_t nt = 0;
    const double *src_n = nullptr, *tgt_n = nullptr;   // normals (both or none are used)
    const int32_t *pair_src = nullptr;                 // pair k = (pair_src[k], pair_tgt[k]); NULL: (k, pair_tgt[k])
    const int32_t *pair_tgt = nullptr;                 // in [-1, nt): -1 = no partner
    int64_t n_pairs = 0;
    const int32_t *draws = nullptr; int64_t n_draw_trials = 0;   // ransac_n draws per trial, or NULL: seeded
    uint64_t seed = 0;
    int ransac_n = 4;
    double edge = 0.0, dist = 0.0, cos_normal = 0.0;
    int use_edge = 0, use_dist = 0, use_normal = 0;
};
struct RansacDevice;                                   // the problem resident on the device + the buffers of one chunk
hipError_t ransac_device_create(const RansacProblem &p, int64_t chunk_cap, hipStream_t stream, RansacDevice **out);
void ransac_device_destroy(RansacDevice *D);
// trials [t0, t0 + n), n <= chunk_cap: h_verdict[n]
// (kRansacPass / Before / After), h_T_all (may be NULL) n x 16 with zeros where nothing was solved; the trials that passed
// are appended in trial order to pass_trial / pass_T (16 doubles each; both may be NULL); *ms (may be NULL) += device time
hipError_t ransac_device_chunk(RansacDevice *D, int64_t t0, int64_t n, int8_t *h_verdict, double *h_T_all,
                               std::vector<int64_t> *pass_trial, std::vector<double> *pass_T, double *ms);
// the whole pair list scored under n transforms (h_T: n x 16): pairs with dis2 < max_dist^2 and the sum of their dis2
hipError_t ransac_score_device(RansacDevice *D, const double *h_T, int64_t n, double max_dist, int64_t *h_good, double *h_err2);

// fill n float4 with +inf (target padding)
hipError_t launch_fill_inf(float4 *dst, int64_t n, hipStream_t stream);
// AoS stride-s floats -> float4 (w = 0)
hipError_t launch_pack_float4(const float *src, int stride, float4 *dst, int64_t n,
                              hipStream_t stream);

// SO(3) self-test kernel: R = rodrigues(w), w2 = invrodrigues(R), v2 = g*v
hipError_t launch_so3_selftest(const double *w, double *R, double *w2, int n,
                               hipStream_t stream);
hipError_t launch_se3_selftest(const double *g, const double *h, const double *v, int n, double *gh, double *gv,
                               double *gi, hipStream_t stream);
hipError_t launch_so3_selftest_jac(const double *w, int n, double *R, double *dR, double *w2, double *dw, double *proj,
                                   hipStream_t stream);

}  // namespace visma

// kbhip_walk.hip — read-outs of the allocate walk on gfx950: which nodes a
// pop's walks visited (kbhip_walk_visits) and the per-node FitDelta records of
// a task that found no node (kbhip_fit_deltas).
//
// Both are an ordered stream compaction over the node columns: the records
// leave the device in ascending node order and the host copies only as many
// as there are.  Three launches, no atomics and no counter shared by blocks:
//   mark     one thread per node decides whether the node is a record; each
//            wave stores its 64-bit ballot (coalesced: 4 words per block) and
//            the block stores its count;
//   scan     one block turns the block counts into exclusive offsets (wave
//            shuffles + LDS, kBlock counts per round) and stores the total;
//   scatter  one thread per node; a record's index = its block's offset + the
//            counts of the waves before its own + the ballot bits below its
//            lane; only records load their columns and write.
// The mark of kbhip_fit_deltas is the pass over the node columns: the walk's
// own eval_node / eval_node_aff per node (rows loaded before the predicates'
// early exits, every load of a wave coalesced along the node index); the
// scatter reads the three Idle columns of the records alone.
#include <hip/hip_runtime.h>

#include "kbhip_eval.h"
#include "kbhip_internal.h"

namespace kbhip {

constexpr int kWaves = kBlock / 64;

int compact_blocks(int n_nodes) { return n_nodes > 0 ? (n_nodes + kBlock - 1) / kBlock : 1; }

// The block's ballot words and count from each thread's verdict.
__device__ __forceinline__ void mark_store(bool rec, uint64_t* mask, uint32_t* blk) {
    __shared__ uint32_t s_w[kWaves];
    const uint64_t b = __ballot(rec);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        mask[(int64_t)blockIdx.x * kWaves + w] = b;
        s_w[w] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (int q = 0; q < kWaves; ++q) c += s_w[q];
        blk[blockIdx.x] = c;
    }
}

// PLAIN: a class without pod (anti-)affinity or inter-pod terms (k_score_sweep's split).
template <bool PLAIN>
__global__ __launch_bounds__(kBlock) void k_fit_mark(Conf cf, NodeCols nc, DevTables t, TaskClass c,
                                                     const PopCtrl* ctrl, uint64_t* mask, uint32_t* blk) {
    const int n = blockIdx.x * kBlock + threadIdx.x;
    bool passed = false;
    if (n < nc.n) {
        int32_t s = 0;
        if constexpr (PLAIN) (void)eval_node(cf, c, t, nc, n, &s, &passed);
        else (void)eval_node_aff(cf, c, t, nc, n, ctrl->ipa_lo[0], ctrl->ipa_hi[0], ctrl->fallback, &s, &passed);
    }
    mark_store(passed, mask, blk);
}

__global__ __launch_bounds__(kBlock) void k_visit_mark(NodeCols nc, uint64_t* mask, uint32_t* blk) {
    const int n = blockIdx.x * kBlock + threadIdx.x;
    mark_store(n < nc.n && nc.visits[n] != 0, mask, blk);
}

// blk[0 .. nb) -> exclusive prefix sums, blk[nb] = total.  One block.
__global__ __launch_bounds__(kBlock) void k_compact_scan(uint32_t* blk, int nb) {
    __shared__ uint32_t s_w[kWaves];
    __shared__ uint32_t s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int base = 0; base < nb; base += kBlock) {
        const int i = base + threadIdx.x;
        const uint32_t v = i < nb ? blk[i] : 0;
        uint32_t x = v;  // inclusive scan within the wave
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) s_w[w] = x;
        __syncthreads();
        uint32_t pre = s_carry;
        for (int q = 0; q < w; ++q) pre += s_w[q];
        if (i < nb) blk[i] = pre + x - v;
        __syncthreads();  // every thread has read s_carry and s_w
        if (threadIdx.x == kBlock - 1) s_carry = pre + x;
        __syncthreads();
    }
    if (threadIdx.x == 0) blk[nb] = s_carry;
}

// This thread's record index, or -1 when its node is not a record.
__device__ __forceinline__ int64_t record_index(const uint64_t* mask, const uint32_t* blk) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t pos = blk[blockIdx.x];
    uint64_t mine = 0;
    for (int q = 0; q < kWaves; ++q) {  // (uniform per wave: scalar loads)
        const uint64_t b = mask[(int64_t)blockIdx.x * kWaves + q];
        if (q < w) pos += (uint32_t)__popcll(b);
        if (q == w) mine = b;
    }
    if (!((mine >> lane) & 1ull)) return -1;
    return (int64_t)pos + __popcll(mine & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(kBlock) void k_fit_scatter(NodeCols nc, TaskClass c, const uint64_t* mask,
                                                        const uint32_t* blk, int32_t* out_node, int64_t* out_delta) {
    const int n = blockIdx.x * kBlock + threadIdx.x;
    const int64_t i = record_index(mask, blk);
    if (i < 0 || n >= nc.n) return;
    // Idle.Clone().FitDelta(task.Resreq) (allocate.go:164-167, resource_info.go:134-147); Idle already
    // holds the walk's visit (Idle += Backfilled: commit_task applied it to every node of the walk)
    const int64_t ic = nc.idle_cpu[n], im = nc.idle_mem[n], ig = nc.idle_gpu[n];
    out_node[i] = n + nc.base;
    out_delta[3 * i + 0] = c.req_cpu > 0 ? ic - (c.req_cpu + kMinCPU) : ic;
    out_delta[3 * i + 1] = c.req_mem > 0 ? im - (c.req_mem + kMinMem) : im;
    out_delta[3 * i + 2] = c.req_gpu > 0 ? ig - (c.req_gpu + kMinGPU) : ig;
}

__global__ __launch_bounds__(kBlock) void k_visit_scatter(NodeCols nc, const uint64_t* mask, const uint32_t* blk,
                                                          int32_t* out_node, uint32_t* out_count, int clear) {
    const int n = blockIdx.x * kBlock + threadIdx.x;
    const int64_t i = record_index(mask, blk);
    if (i < 0 || n >= nc.n) return;
    out_node[i] = n + nc.base;
    out_count[i] = nc.visits[n];
    if (clear) nc.visits[n] = 0;
}

hipError_t launch_fit_mark(const Conf& cf, const NodeCols& nc, const DevTables& t, const TaskClass& c,
                           const PopCtrl* ctrl, uint64_t* mask, uint32_t* blk, hipStream_t st) {
    const int nb = compact_blocks(nc.n);
    if (!c.aff && c.ipa_n == 0)
        hipLaunchKernelGGL((k_fit_mark<true>), dim3(nb), dim3(kBlock), 0, st, cf, nc, t, c, ctrl, mask, blk);
    else
        hipLaunchKernelGGL((k_fit_mark<false>), dim3(nb), dim3(kBlock), 0, st, cf, nc, t, c, ctrl, mask, blk);
    return hipGetLastError();
}
hipError_t launch_visit_mark(const NodeCols& nc, uint64_t* mask, uint32_t* blk, hipStream_t st) {
    hipLaunchKernelGGL(k_visit_mark, dim3(compact_blocks(nc.n)), dim3(kBlock), 0, st, nc, mask, blk);
    return hipGetLastError();
}
hipError_t launch_compact_scan(uint32_t* blk, int nb, hipStream_t st) {
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(kBlock), 0, st, blk, nb);
    return hipGetLastError();
}
hipError_t launch_fit_scatter(const NodeCols& nc, const TaskClass& c, const uint64_t* mask, const uint32_t* blk,
                              int32_t* out_node, int64_t* out_delta, hipStream_t st) {
    hipLaunchKernelGGL(k_fit_scatter, dim3(compact_blocks(nc.n)), dim3(kBlock), 0, st, nc, c, mask, blk, out_node,
                       out_delta);
    return hipGetLastError();
}
hipError_t launch_visit_scatter(const NodeCols& nc, const uint64_t* mask, const uint32_t* blk, int32_t* out_node,
                                uint32_t* out_count, int clear, hipStream_t st) {
    hipLaunchKernelGGL(k_visit_scatter, dim3(compact_blocks(nc.n)), dim3(kBlock), 0, st, nc, mask, blk, out_node,
                       out_count, clear);
    return hipGetLastError();
}

}  // namespace kbhip

// Per-node rejection reasons of pending tasks on gfx950 (kbhip_explain_tasks).
//
// The reference tells why a node is lost to a task node by node: the error of
// the first predicate that failed (allocate.go:128-137 logging what
// predicates.go:123-203 returned), a NodeOrderFn error (allocate.go:139-146),
// or the resource fit (allocate.go:153-184).  The sweep below gives every
// (task, node) pair of a batch that verdict (node_verdict, kbhip_eval.h: one
// byte) and every task the histogram of its verdicts:
//   k_explain<WRITE>  grid (bx, requests), 256 threads.  blockIdx.y is the
//                     request; its class is read from the uploaded descriptor
//                     array.  A wave takes 64 consecutive nodes per step (lane =
//                     node, every column load coalesced), the steps beyond the
//                     grid strided by bx * 256 with the next step's flags, row
//                     and port words loaded before the current one is evaluated
//                     (as k_score_sweep_gs).  WRITE: the lane stores its node's
//                     byte into row blockIdx.y — a wave's 64 bytes are
//                     consecutive, one 64-B segment per store instruction;
//                     without WRITE the kernel has no per-node store at all.
//                     The histogram's bins are counted by one wave ballot and
//                     one population count each into wave-uniform counters; the
//                     four waves add theirs through LDS and the block writes
//                     its 16 counts to part[request][block][16].
//   k_explain_reduce  grid requests: the request's block counts summed in fixed
//                     order into out[request][0 .. 15] (64-bit).
// The launch boundary orders the two: no atomics, no block waits for another.
// Traffic per node and request: 81 B of columns (flags, Idle / Releasing /
// Backfilled, pods, maxtasks) + 8 B per taint word + the class's port words
// and label columns; 1 B written with WRITE.
#include <hip/hip_runtime.h>

#include "kbhip_eval.h"
#include "kbhip_internal.h"

namespace kbhip {

constexpr int kExplainWaves = kBlock / 64;

template <bool WRITE>
__global__ __launch_bounds__(kBlock) void k_explain(Conf cf, NodeCols nc, DevTables t, const TaskClass* d,
                                                    uint8_t* verdict, uint32_t* part) {
    __shared__ uint32_t s_bin[kExplainWaves][kWhyBins];
    const TaskClass& c = d[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int stride = gridDim.x * kBlock;
    uint8_t* const row = WRITE ? verdict + (size_t)blockIdx.y * (size_t)nc.n : nullptr;
    uint32_t cnt[kWhyBins];  // uniform over the wave
#pragma unroll
    for (int k = 0; k < kWhyBins; ++k) cnt[k] = 0;
    int n = blockIdx.x * kBlock + threadIdx.x;
    VerdictIn cur{};
    if (n < nc.n) cur = verdict_in(c, nc, n);
    // the wave's first node of the step is uniform: every lane reaches the ballots
    for (int b = blockIdx.x * kBlock + wave * 64; b < nc.n; b += stride, n += stride) {
        VerdictIn nxt{};
        if (n + stride < nc.n) nxt = verdict_in(c, nc, n + stride);
        uint32_t bins = 0;  // lanes past the last node are in no bin
        if (n < nc.n) {
            const uint8_t v = node_verdict_of(cf, c, t, nc, n, cur);
            if constexpr (WRITE) row[n] = v;
            bins = verdict_bins(v);
        }
#pragma unroll
        for (int k = 0; k < kWhyBins; ++k)
            if (k != kWhyCodes) cnt[k] += (uint32_t)__popcll(__ballot((bins >> k) & 1u));
        cur = nxt;
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kWhyBins; ++k) s_bin[wave][k] = cnt[k];
    }
    __syncthreads();
    if (threadIdx.x < kWhyBins) {
        uint32_t tot = 0;
        for (int w = 0; w < kExplainWaves; ++w) tot += s_bin[w][threadIdx.x];
        part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kWhyBins + threadIdx.x] = tot;
    }
}

// Thread (g, k) = (threadIdx.x / 16, threadIdx.x % 16) sums bin k of blocks g,
// g + 16, ...; the 16 groups' sums are added in group order.
__global__ __launch_bounds__(kBlock) void k_explain_reduce(const uint32_t* part, int nblk, int64_t* out) {
    __shared__ int64_t s_sum[kBlock / kWhyBins][kWhyBins];
    const int k = threadIdx.x % kWhyBins, g = threadIdx.x / kWhyBins;
    const uint32_t* p = part + (size_t)blockIdx.x * nblk * kWhyBins;
    int64_t sum = 0;
    for (int b = g; b < nblk; b += kBlock / kWhyBins) sum += p[(size_t)b * kWhyBins + k];
    s_sum[g][k] = sum;
    __syncthreads();
    if (threadIdx.x < kWhyBins) {
        int64_t tot = 0;
        for (int q = 0; q < kBlock / kWhyBins; ++q) tot += s_sum[q][threadIdx.x];
        out[(size_t)blockIdx.x * kWhyBins + threadIdx.x] = tot;
    }
}

// The sweep's grid x.  One request: a block per 256 nodes, at most one per CU.
// More requests share kExplainPerCU blocks per CU — what is resident at once
// at the kernel's register count, so the whole grid is one wave of blocks —
// each request getting an equal part of them, at least one block.  cap > 0
// (option "explain_blocks"): at most that many.
constexpr int kExplainPerCU = 4;
int explain_bx(int n_nodes, int n_req, int cap) {
    const int need = n_nodes > 0 ? (n_nodes + kBlock - 1) / kBlock : 1;
    const int cus = device_cu_count();
    const int part = n_req > 1 ? kExplainPerCU * cus / n_req : cus;
    int bx = need < part ? need : part;
    if (cap > 0 && bx > cap) bx = cap;
    return bx < 1 ? 1 : bx;
}

hipError_t launch_explain(const Conf& cf, const NodeCols& nc, const DevTables& t, const TaskClass* d_cls, int n_req,
                          int bx, uint8_t* verdict, uint32_t* part, int64_t* out, hipStream_t st) {
    if (n_req < 1 || n_req > kMaxChunk || bx < 1) return hipErrorInvalidValue;
    if (verdict)
        hipLaunchKernelGGL((k_explain<true>), dim3(bx, n_req), dim3(kBlock), 0, st, cf, nc, t, d_cls, verdict, part);
    else
        hipLaunchKernelGGL((k_explain<false>), dim3(bx, n_req), dim3(kBlock), 0, st, cf, nc, t, d_cls, verdict, part);
    hipLaunchKernelGGL(k_explain_reduce, dim3(n_req), dim3(kBlock), 0, st, (const uint32_t*)part, bx, out);
    return hipGetLastError();
}

}  // namespace kbhip

// The task queries' walk kernels on gfx950: the head of one task's walk
// (kbhip_rank_nodes, kbhip_rank_victim_nodes), the heads of several tasks in
// one launch pair (kbhip_rank_heads), the victim-candidate test and the
// compaction of a full walk by it.  The order they produce is the one of the
// reclaim / preempt ranking (kbhip_evict.hip), whose sorted keys the
// compaction reads and whose scan kernel it borrows.
#include <hip/hip_runtime.h>

#include "kbhip_batch.h"
#include "kbhip_eval.h"
#include "kbhip_internal.h"

namespace kbhip {

// ---------------------------------------------------------------------------
// The head of a walk (kbhip_rank_nodes with first + cap <= kTopK): the best
// kTopK keys of the order above and the passing count, with no per-node array
// written.  The walks of preempt and reclaim usually stop within their first
// few nodes; the head is what such a host asks for first.
//   k_rank_head        the sweep.  A wave takes 64 consecutive nodes per step
//                      (lane = node, loads coalesced), evaluates PredicateFn +
//                      NodeOrderFn into pack_key(score, index) (by_score 0:
//                      the predicates alone, score 0 — the order is the index),
//                      sorts the 64 keys in registers (wave_sort_desc) and
//                      merges them into its running top 64 (wave_merge_desc); a
//                      step none of whose keys beats the wave's 64th is not
//                      merged.  The block's waves merge through LDS; one sorted
//                      list of 64 keys and the block's passing count go out.
//                      Grid: at most one block per CU (rank_head_blocks), the
//                      steps beyond it grid-strided, a plain class's columns
//                      of the next step loaded before the current one is
//                      evaluated (as k_score_sweep_gs).
//   k_rank_head_merge  one block: wave w merges block lists w, w + 4, ...,
//                      the four results merge through LDS; out[0 .. 63] = the
//                      keys (descending, 0 beyond the passing count), out[64] =
//                      the passing count.
// The launch boundary orders the two kernels: no block waits for another.
// Traffic per node: the 41 B of columns of the sweep above (eval_node_aff's
// classes: the whole row), nothing written; per block 516 B out.
// ---------------------------------------------------------------------------
constexpr int kHeadWaves = kBlock / 64;
constexpr int kHeadMaxBlocks = 1024;  // scratch size (rank_head_words); the grid is capped at the CU count below it

// The waves' sorted lists merged into s_top[0] (every wave of the block calls).
__device__ __forceinline__ void head_block_merge(uint64_t (*s_top)[64], uint64_t top, int wave, int lane) {
    s_top[wave][lane] = top;
    __syncthreads();
#pragma unroll
    for (int s = kHeadWaves / 2; s >= 1; s >>= 1) {
        if (wave < s) s_top[wave][lane] = wave_merge_desc(s_top[wave][lane], s_top[wave + s][lane]);
        __syncthreads();
    }
}

// The victim-candidate test of kbhip_rank_victim_nodes (VictArgs,
// kbhip_internal.h) for node n: the candidate count and Resreq sums of the
// call's mode, from at most two table rows of column n (coalesced over the
// lanes of a wave) and the job's own list.
struct Vict4 {
    int64_t n, c, m, g;
};
__device__ __forceinline__ Vict4 vict_row(const VictArgs& v, int row, int n) {
    const size_t np = (size_t)v.npad;
    const int64_t* p = v.tab + (size_t)row * 4 * np + n;
    return Vict4{p[0], p[np], p[2 * np], p[3 * np]};
}
__device__ __forceinline__ Vict4 vict_own(const VictArgs& v, int n) {
    int lo = 0, hi = v.own_n;  // the first entry >= n
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v.own_node[mid] < n) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= v.own_n || v.own_node[lo] != n) return Vict4{0, 0, 0, 0};
    const int64_t* p = v.own_sum + 4 * (size_t)lo;
    return Vict4{p[0], p[1], p[2], p[3]};
}
__device__ __forceinline__ Vict4 vict_cand(const VictArgs& v, int n) {
    if (v.mode == 3) return vict_own(v, n);
    Vict4 a, b;
    if (v.mode == 1) { a = vict_row(v, v.nq, n); b = vict_row(v, v.q, n); }
    else { a = vict_row(v, v.q, n); b = vict_own(v, n); }
    return Vict4{a.n - b.n, a.c - b.c, a.m - b.m, a.g - b.g};
}
__device__ __forceinline__ bool vict_keep(const VictArgs& v, const Vict4& a) {
    return a.n > 0 && !(a.c < v.rc && a.m < v.rm && a.g < v.rg);
}

// FILT: the lane that evaluates a node also loads the node's candidate sums
// (before the evaluation: the loads run under it) and zeroes its key when the
// node fails the test; without FILT v is never read.
// lists / bcnt: the request's block lists and block counts (block blockIdx.x
// writes list blockIdx.x); slot: the PopCtrl task slot that holds the
// request's inter-pod min / max; stride: the nodes one step of the grid
// covers (gridDim.x * kBlock).  s_top / s_cnt: the block's LDS (the caller's,
// so that a kernel with two instantiations of the body declares it once).
// BOUND (kbhip_walk_victims_from): a key at or above `bound` — a node the
// caller's loop has left behind — becomes 0 before the count and the top-64
// test, so the count is the count below the bound and such a node enters no
// list; without BOUND bound is never read.
template <bool PLAIN, bool FILT, bool BOUND = false>
__device__ __forceinline__ void rank_head(const Conf& cf, const NodeCols& nc, const DevTables& t, const TaskClass& c,
                                          const PopCtrl* ctrl, int by_score, int slot, int stride, uint64_t* lists,
                                          uint32_t* bcnt, const VictArgs& v, uint64_t (*s_top)[64],
                                          uint32_t* s_cnt, uint64_t bound = 0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t top = 0;  // lane i: the wave's i-th best key so far
    uint32_t cnt = 0;  // passing nodes of the wave (uniform)
    // b is the wave's first node of the step: uniform, so every lane runs the
    // sort and merge networks (lanes past the last node hold key 0)
    int b = blockIdx.x * kBlock + wave * 64;
    SweepIn cur{};
    if (PLAIN && b + lane < nc.n) cur = sweep_in(nc, b + lane);
    for (; b < nc.n; b += stride) {
        const int n = b + lane;
        uint64_t k = 0;
        Vict4 va{};
        if constexpr (FILT) {
            if (n < nc.n) va = vict_cand(v, n);
        }
        if constexpr (PLAIN) {
            SweepIn nxt{};
            if (n + stride < nc.n) nxt = sweep_in(nc, n + stride);
            if (n < nc.n) {
                uint64_t pw[4] = {0, 0, 0, 0};
                if (c.has_ports)
                    for (int w = 0; w < 4; ++w) if (w < port_win(c, nc)) pw[w] = nc.ports[port_at(c, nc, w, n)];
                Row r{};
                r.acpu = cur.acpu; r.amem = cur.amem; r.nzc = cur.nzc; r.nzm = cur.nzm;
                r.pods = cur.pods; r.maxtasks = cur.maxtasks;
                const bool st = static_pred_f(cf, c, t, nc, n, cur.fl);
                const int32_t na = (st && cf.score_mult) ? na_weight(c, t, nc, n) : 0;
                int32_t s = 0;
                bool passed = false;
                (void)dyn_key(cf, c, t, nc, r, pw, n, st, na, &s, &passed);  // passed and s read no fit column
                k = passed ? pack_key(s, n + nc.base, 0) : 0;
            }
            cur = nxt;
        } else if (n < nc.n) {
            if (by_score) {
                int32_t s = 0;
                bool passed = false;
                (void)eval_node_aff(cf, c, t, nc, n, ctrl->ipa_lo[slot], ctrl->ipa_hi[slot], ctrl->fallback, &s,
                                    &passed);
                k = passed ? pack_key(s, n + nc.base, 0) : 0;
            } else {
                k = eval_first_fit(cf, c, t, nc, n);
            }
        }
        if constexpr (FILT) {
            if (!vict_keep(v, va)) k = 0;  // (lanes past the last node: va is zero, k already is)
        }
        if constexpr (BOUND) {
            if (k >= bound) k = 0;
        }
        cnt += (uint32_t)__popcll(__ballot(k != 0));
        if (__ballot(k > readlane64(top, 63)) == 0) continue;  // uniform: nothing enters the top 64
        top = wave_merge_desc(top, wave_sort_desc(k));
    }
    if (lane == 0) s_cnt[wave] = cnt;
    head_block_merge(s_top, top, wave, lane);
    if (wave == 0) lists[(size_t)blockIdx.x * 64 + lane] = s_top[0][lane];
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int w = 0; w < kHeadWaves; ++w) tot += s_cnt[w];
        bcnt[blockIdx.x] = tot;
    }
}

template <bool PLAIN>
__global__ __launch_bounds__(kBlock) void k_rank_head(Conf cf, NodeCols nc, DevTables t, TaskClass c,
                                                      const PopCtrl* ctrl, int by_score, uint64_t* lists,
                                                      uint32_t* bcnt) {
    __shared__ uint64_t s_top[kHeadWaves][64];
    __shared__ uint32_t s_cnt[kHeadWaves];
    rank_head<PLAIN, false>(cf, nc, t, c, ctrl, by_score, 0, gridDim.x * kBlock, lists, bcnt, VictArgs{}, s_top,
                            s_cnt);
}
template <bool PLAIN>
__global__ __launch_bounds__(kBlock) void k_rank_head_vict(Conf cf, NodeCols nc, DevTables t, TaskClass c,
                                                           const PopCtrl* ctrl, int by_score, uint64_t* lists,
                                                           uint32_t* bcnt, VictArgs v) {
    __shared__ uint64_t s_top[kHeadWaves][64];
    __shared__ uint32_t s_cnt[kHeadWaves];
    rank_head<PLAIN, true>(cf, nc, t, c, ctrl, by_score, 0, gridDim.x * kBlock, lists, bcnt, v, s_top, s_cnt);
}
// kbhip_walk_victims_from's sweep: k_rank_head_vict over the nodes whose key is below `bound` (> 0)
template <bool PLAIN>
__global__ __launch_bounds__(kBlock) void k_rank_head_vict_from(Conf cf, NodeCols nc, DevTables t, TaskClass c,
                                                                const PopCtrl* ctrl, int by_score, uint64_t* lists,
                                                                uint32_t* bcnt, VictArgs v, uint64_t bound) {
    __shared__ uint64_t s_top[kHeadWaves][64];
    __shared__ uint32_t s_cnt[kHeadWaves];
    rank_head<PLAIN, true, true>(cf, nc, t, c, ctrl, by_score, 0, gridDim.x * kBlock, lists, bcnt, v, s_top, s_cnt,
                                 bound);
}

__device__ __forceinline__ void rank_head_merge(const uint64_t* lists, const uint32_t* bcnt, int nblk,
                                                uint64_t* out) {
    __shared__ uint64_t s_top[kHeadWaves][64];
    __shared__ uint32_t s_cnt[kHeadWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t top = 0;
    for (int b = wave; b < nblk; b += kHeadWaves) top = wave_merge_desc(top, lists[(size_t)b * 64 + lane]);
    uint32_t cnt = 0;
    for (int b = threadIdx.x; b < nblk; b += kBlock) cnt += bcnt[b];
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) s_cnt[wave] = cnt;
    head_block_merge(s_top, top, wave, lane);
    if (wave == 0) out[lane] = s_top[0][lane];
    if (threadIdx.x == 0) {
        uint64_t tot = 0;
        for (int w = 0; w < kHeadWaves; ++w) tot += s_cnt[w];
        out[kTopK] = tot;
    }
}
__global__ __launch_bounds__(kBlock) void k_rank_head_merge(const uint64_t* lists, const uint32_t* bcnt, int nblk,
                                                            uint64_t* out) {
    rank_head_merge(lists, bcnt, nblk, out);
}

// ---------------------------------------------------------------------------
// The heads of several tasks of one session (kbhip_rank_heads): the two
// kernels above with blockIdx.y as the request.  Request r's descriptor
// (HeadDesc: its class, its victim test, its PopCtrl slot) is read from device
// memory; its blocks write lists [r gridDim.x, (r + 1) gridDim.x) of the
// scratch and k_rank_heads_merge's block r merges those into out[r][0 .. 64].
// Whether a request's class takes the PLAIN body is uniform per block.
// ---------------------------------------------------------------------------
template <bool FILT>
__global__ __launch_bounds__(kBlock) void k_rank_heads(Conf cf, NodeCols nc, DevTables t, const HeadDesc* d,
                                                       const PopCtrl* ctrl, int by_score, uint64_t* lists,
                                                       uint32_t* bcnt) {
    __shared__ uint64_t s_top[kHeadWaves][64];
    __shared__ uint32_t s_cnt[kHeadWaves];
    const HeadDesc& q = d[blockIdx.y];
    const size_t r = (size_t)blockIdx.y * gridDim.x;
    const int stride = gridDim.x * kBlock;
    if (by_score && !q.c.aff && q.c.ipa_n == 0)
        rank_head<true, FILT>(cf, nc, t, q.c, ctrl, by_score, q.slot, stride, lists + r * 64, bcnt + r, q.v, s_top,
                              s_cnt);
    else
        rank_head<false, FILT>(cf, nc, t, q.c, ctrl, by_score, q.slot, stride, lists + r * 64, bcnt + r, q.v, s_top,
                               s_cnt);
}
__global__ __launch_bounds__(kBlock) void k_rank_heads_merge(const uint64_t* lists, const uint32_t* bcnt, int nblk,
                                                             uint64_t* out) {
    const size_t r = (size_t)blockIdx.x * nblk;
    rank_head_merge(lists + r * 64, bcnt + r, nblk, out + (size_t)blockIdx.x * (kTopK + 1));
}

// The sweep's grid x for n_req requests.  A request alone takes the
// single-task grid (rank_head_blocks: one block per CU at most).  More
// requests share kHeadsPerCU blocks per CU — what is resident at once at the
// kernel's register count, so the whole grid is one wave of blocks — each
// request getting an equal part of them, at least one block.
constexpr int kHeadsPerCU = 4;
constexpr int kHeadsMaxLists = kHeadsPerCU * kHeadMaxBlocks;  // >= n_req * rank_heads_bx(n, n_req)
int rank_heads_bx(int n_nodes, int n_req) {
    const int one = rank_head_blocks(n_nodes);
    const int cus = device_cu_count() < kHeadMaxBlocks ? device_cu_count() : kHeadMaxBlocks;
    const int part = n_req > 0 ? kHeadsPerCU * cus / n_req : one;
    return part < 1 ? 1 : part < one ? part : one;
}
// scratch, in 8-byte words: kMaxChunk results (kTopK keys + the count each), the block lists, the block counts
size_t rank_heads_words() {
    return (size_t)kMaxChunk * (kTopK + 1) + (size_t)kHeadsMaxLists * 64 + kHeadsMaxLists / 2;
}

hipError_t launch_rank_heads(const Conf& cf, const NodeCols& nc, const DevTables& t, const HeadDesc* d_desc, int n_req,
                             bool filt, const PopCtrl* ctrl, int by_score, uint64_t* scratch, int* bx_out,
                             hipStream_t st) {
    static_assert(kMaxChunk <= kHeadsMaxLists, "one list per request at least");
    if (n_req < 1 || n_req > kMaxChunk) return hipErrorInvalidValue;
    uint64_t* out = scratch;
    uint64_t* lists = scratch + (size_t)kMaxChunk * (kTopK + 1);
    uint32_t* bcnt = reinterpret_cast<uint32_t*>(lists + (size_t)kHeadsMaxLists * 64);
    const int bx = rank_heads_bx(nc.n, n_req);
    if ((size_t)bx * n_req > (size_t)kHeadsMaxLists) return hipErrorInvalidValue;
    if (filt)
        hipLaunchKernelGGL((k_rank_heads<true>), dim3(bx, n_req), dim3(kBlock), 0, st, cf, nc, t, d_desc, ctrl,
                           by_score, lists, bcnt);
    else
        hipLaunchKernelGGL((k_rank_heads<false>), dim3(bx, n_req), dim3(kBlock), 0, st, cf, nc, t, d_desc, ctrl,
                           by_score, lists, bcnt);
    hipLaunchKernelGGL(k_rank_heads_merge, dim3(n_req), dim3(kBlock), 0, st, (const uint64_t*)lists,
                       (const uint32_t*)bcnt, bx, out);
    if (bx_out) *bx_out = bx;
    return hipGetLastError();
}

int rank_head_blocks(int n_nodes) {
    const int need = n_nodes > 0 ? (n_nodes + kBlock - 1) / kBlock : 1;
    const int cap = device_cu_count() < kHeadMaxBlocks ? device_cu_count() : kHeadMaxBlocks;
    return need < cap ? need : cap;
}
// scratch, in 8-byte words: the result (kTopK keys + the count), the block lists, the block counts
size_t rank_head_words() { return (size_t)(kTopK + 1) + (size_t)kHeadMaxBlocks * 64 + kHeadMaxBlocks / 2; }

hipError_t launch_rank_head(const Conf& cf, const NodeCols& nc, const DevTables& t, const TaskClass& c,
                            const PopCtrl* ctrl, int by_score, const VictArgs* v, uint64_t* scratch, hipStream_t st,
                            uint64_t bound) {
    static_assert(kTopK == 64, "one key per lane");
    uint64_t* out = scratch;
    uint64_t* lists = scratch + kTopK + 1;
    uint32_t* bcnt = reinterpret_cast<uint32_t*>(lists + (size_t)kHeadMaxBlocks * 64);
    const int grid = rank_head_blocks(nc.n);
    const bool plain = by_score && !c.aff && c.ipa_n == 0;
    if (bound != 0 && !v) return hipErrorInvalidValue;  // (the bounded sweep exists for the pruned walk only)
    if (bound != 0 && plain)
        hipLaunchKernelGGL((k_rank_head_vict_from<true>), dim3(grid), dim3(kBlock), 0, st, cf, nc, t, c, ctrl,
                           by_score, lists, bcnt, *v, bound);
    else if (bound != 0)
        hipLaunchKernelGGL((k_rank_head_vict_from<false>), dim3(grid), dim3(kBlock), 0, st, cf, nc, t, c, ctrl,
                           by_score, lists, bcnt, *v, bound);
    else if (v && plain)
        hipLaunchKernelGGL((k_rank_head_vict<true>), dim3(grid), dim3(kBlock), 0, st, cf, nc, t, c, ctrl, by_score,
                           lists, bcnt, *v);
    else if (v)
        hipLaunchKernelGGL((k_rank_head_vict<false>), dim3(grid), dim3(kBlock), 0, st, cf, nc, t, c, ctrl, by_score,
                           lists, bcnt, *v);
    else if (plain)
        hipLaunchKernelGGL((k_rank_head<true>), dim3(grid), dim3(kBlock), 0, st, cf, nc, t, c, ctrl, by_score, lists,
                           bcnt);
    else
        hipLaunchKernelGGL((k_rank_head<false>), dim3(grid), dim3(kBlock), 0, st, cf, nc, t, c, ctrl, by_score, lists,
                           bcnt);
    hipLaunchKernelGGL(k_rank_head_merge, dim3(1), dim3(kBlock), 0, st, (const uint64_t*)lists,
                       (const uint32_t*)bcnt, grid, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The full walk of kbhip_rank_victim_nodes: the sorted keys of the ranking
// above (count[0] of them, best first) without the nodes that fail the victim
// test, order kept.  Block b takes keys [b kBlock, (b + 1) kBlock):
//   k_vict_count    its survivors -> blk[b] (block 0 also zeroes blk[nblk])
//   k_rank_scan     exclusive scan of blk[0 .. nblk]: blk[nblk] = the total
//                   (kbhip_evict.hip's, through launch_rank_scan)
//   k_vict_scatter  survivor i of the block (wave ballots, earlier waves'
//                   counts) -> out_keys / out_cands[blk[b] + i]
// The launch boundaries order them: no block waits for another.  The test is
// evaluated in both passes (per key at most two table rows of its node,
// gathered in walk order, and the own list) instead of a flag array written
// and read back.
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool vict_key_keep(const uint64_t* sorted, const uint32_t* count, int n_nodes,
                                              const VictArgs& v, int i, uint64_t* k_out, Vict4* a_out) {
    const int cnt = (int)count[0] < n_nodes ? (int)count[0] : n_nodes;
    if (i >= cnt) return false;
    const uint64_t k = sorted[i];
    const int n = key_idx(k);
    if (!k || n < 0 || n >= n_nodes) return false;
    const Vict4 a = vict_cand(v, n);
    *k_out = k;
    *a_out = a;
    return vict_keep(v, a);
}
__global__ __launch_bounds__(kBlock) void k_vict_count(const uint64_t* sorted, const uint32_t* count, int n_nodes,
                                                       VictArgs v, uint32_t* blk) {
    __shared__ uint32_t s_cnt[kBlock / 64];
    uint64_t k;
    Vict4 a;
    const bool keep = vict_key_keep(sorted, count, n_nodes, v, blockIdx.x * kBlock + threadIdx.x, &k, &a);
    const uint32_t c = (uint32_t)__popcll(__ballot(keep));
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int w = 0; w < kBlock / 64; ++w) tot += s_cnt[w];
        blk[blockIdx.x] = tot;
        if (blockIdx.x == 0) blk[gridDim.x] = 0;
    }
}
__global__ __launch_bounds__(kBlock) void k_vict_scatter(const uint64_t* sorted, const uint32_t* count, int n_nodes,
                                                         VictArgs v, const uint32_t* blk, uint64_t* out_keys,
                                                         int32_t* out_cands) {
    __shared__ uint32_t s_cnt[kBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t k = 0;
    Vict4 a{};
    const bool keep = vict_key_keep(sorted, count, n_nodes, v, blockIdx.x * kBlock + threadIdx.x, &k, &a);
    const uint64_t m = __ballot(keep);
    if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!keep) return;
    uint32_t pos = blk[blockIdx.x] + (uint32_t)__popcll(m & (lane ? (~0ull >> (64 - lane)) : 0ull));
    for (int w = 0; w < wave; ++w) pos += s_cnt[w];
    if (pos >= (uint32_t)n_nodes) return;  // (the survivors are a subset of the n_nodes keys)
    out_keys[pos] = k;
    out_cands[pos] = (int32_t)a.n;
}

int vict_blocks(int n_nodes) { return n_nodes > 0 ? (n_nodes + kBlock - 1) / kBlock : 1; }

hipError_t launch_vict_compact(const uint64_t* sorted, const uint32_t* count, int n_nodes, const VictArgs& v,
                               uint32_t* blk, uint64_t* out_keys, int32_t* out_cands, hipStream_t st) {
    const int nblk = vict_blocks(n_nodes);
    hipLaunchKernelGGL(k_vict_count, dim3(nblk), dim3(kBlock), 0, st, sorted, count, n_nodes, v, blk);
    const hipError_t e = launch_rank_scan(blk, nblk + 1, st);  // (k_rank_scan lives in kbhip_evict.hip)
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_vict_scatter, dim3(nblk), dim3(kBlock), 0, st, sorted, count, n_nodes, v,
                       (const uint32_t*)blk, out_keys, out_cands);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The marks of kbhip_walk_begin_live: reclaim's order is the node index, so a
// ranking without the pod-affinity predicate needs no sort — one node per
// thread, keys[n] = eval_first_fit's key on a class whose affinity program is
// off (the static predicates, pod count and host ports; 0 where one fails),
// and the compaction above reads the array as a sorted ranking of nc.n keys
// (vict_key_keep drops the zeros).  Plain stores; no counter is accumulated.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_live_keys(Conf cf, NodeCols nc, DevTables t, TaskClass c, uint64_t* keys,
                                                      uint32_t* count) {
    const int n = blockIdx.x * kBlock + threadIdx.x;
    if (n < nc.n) keys[n] = eval_first_fit(cf, c, t, nc, n);
    if (n == 0) {
        count[0] = (uint32_t)(nc.n > 0 ? nc.n : 0);
        count[1] = 0;
    }
}

hipError_t launch_live_keys(const Conf& cf, const NodeCols& nc, const DevTables& t, const TaskClass& c, uint64_t* keys,
                            uint32_t* count, hipStream_t st) {
    if (!keys || !count) return hipErrorInvalidValue;
    TaskClass plain = c;
    plain.aff = 0;  // eval_first_fit leaves aff_pred out
    hipLaunchKernelGGL(k_live_keys, dim3(vict_blocks(nc.n)), dim3(kBlock), 0, st, cf, nc, t, plain, keys, count);
    return hipGetLastError();
}

}  // namespace kbhip

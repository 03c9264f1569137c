// The victim sets of a walk's head nodes on gfx950 (kbhip_head_victims).
//
// The head sweep and merge of kbhip_heads.hip leave the best kTopK keys of a
// task's pruned walk and their count in device memory.  k_head_victims reads
// them there — the node list makes no host round trip — and answers, for each
// of the first `cap` head nodes, what ssn.Reclaimable / ssn.Preemptable,
// validateVictims and the eviction loop would decide on it, from the victim
// state (kbhip_internal.h: the nodes' candidate tasks as a CSR of 48-byte
// records in node order, per-job and per-queue plugin records):
//   k_head_victims   grid cap, one wave per block, block i = head entry i.
//                    The node's task records are consecutive: lane l loads
//                    record l, l + 64, ... (vict_stage: the record, then its
//                    job's and queue's records, 32 and 48 bytes gathered per
//                    candidate) into LDS — or, for a node of more than
//                    kVictLds tasks, into the block's spill row in device
//                    memory — and finds the first task of its job and queue on
//                    the node (vict_link).  Lane 0 then runs vict_decide
//                    (kbhip_eval.h) over the staged records: the plugin chains
//                    of drf and proportion are sequential in task order by
//                    their definition (proportion skips an evictee without
//                    subtracting), and the host test entry runs the same
//                    function.  The lanes fill the victim row's tail with -1.
//                    Block 0 also copies the head's keys and count, so that
//                    one copy back returns everything.
//   k_heads_victims  kbhip_heads_victims: the same rows (one shared device
//                    function) for up to kMaxChunk tasks in one launch, grid
//                    (cap, requests): block (i, r) reads request r's head where
//                    k_rank_heads_merge left it and its header from a device
//                    array; the staged records take dynamic LDS sized by the
//                    state's longest node.
//   k_walk_victims   kbhip_walk_victims: one block walks the head entries in
//                    order, staging each node as above under an overlay of
//                    the evictions of the entries before it (walk_loop over
//                    walk_entry, described there).
//   k_walk_flags, k_walk_victims_from
//                    kbhip_walk_victims_from: the entries of a window behind
//                    the caller's resume point decided side by side (flags
//                    only), then the same walk_loop from the first entry that
//                    can act.
//   k_walk_scan, k_walk_cursor
//                    kbhip_walk_next: every entry of a kept order at or behind
//                    a position decided side by side, one wave per entry, into one
//                    word (the lowest position that can act), then walk_loop
//                    from that position.
//   k_walk_scan_live, k_walk_cursor_live
//                    the same two for a cursor of kbhip_walk_begin_live, whose
//                    kept order left the pod-affinity predicate out: both test
//                    it per entry on the count tables as they stand, and the
//                    walk ends behind the first node it acts on.
//   k_victims_patch  the records kbhip_apply_ops left dirty, one thread each.
// Stores are plain vector stores; the only atomics are k_walk_scan's two (a vector atomicMin and a vector
// atomicAdd per block, by lane 0); no block waits for another.
#include <hip/hip_runtime.h>

#include "kbhip_eval.h"
#include "kbhip_internal.h"

namespace kbhip {

// The task records of a head key's node: off, n.  False: the key names no node of the state, or records
// outside the state, or more than lds_cap staged records or a spill row of spill_stride (null: none) hold.
// What false means is the caller's: "no node" to head_victims_row, a visit that stages nothing to the walk.
__device__ __forceinline__ bool head_node_range(const VictState& st, uint64_t key, int node_base, int lds_cap,
                                                const VictRec* spill, int spill_stride, int& off, int& n) {
    const int node = key_idx(key) - node_base;
    if (key == 0 || node < 0 || node >= st.n_nodes) return false;
    off = st.node_off[node];
    n = st.node_off[node + 1] - off;
    return off >= 0 && n >= 0 && off + n <= st.n_tasks && (n <= lds_cap || (spill && n <= spill_stride));
}

// The node of `key` decided into `row` (count, evict, flags, then stride victims), by one wave.  lds: room
// for lds_cap staged records; a longer node stages into spill_row (spill_stride records, or null).  in false,
// or a key without a node: 0 / -1 written, nothing of the state read.
__device__ __forceinline__ void victims_row(const VictState& st, const VictHdr& h, uint64_t key, bool in, int stride,
                                            int node_base, VictRec* lds, int lds_cap, VictRec* spill_row,
                                            int spill_stride, int32_t* row) {
    const int lane = threadIdx.x;
    int off = 0, n;
    if (!in || !head_node_range(st, key, node_base, lds_cap, spill_row, spill_stride, off, n)) n = -1;  // no node
    int count = 0;
    if (n > 0) {  // (uniform over the block)
        VictRec* const rec = n <= lds_cap ? lds : spill_row;
        for (int k = lane; k < n; k += 64) vict_stage(st, h, off + k, rec[k]);
        __syncthreads();
        for (int k = lane; k < n; k += 64) vict_link(rec, k);
        __syncthreads();
        if (lane == 0) {
            int32_t evict = 0, flags = 0;
            count = vict_decide(h, rec, n, stride, row + 3, &evict, &flags);
            row[0] = count;
            row[1] = evict;
            row[2] = flags;
        }
        count = __shfl(count, 0, 64);
    } else if (lane == 0) {
        row[0] = row[1] = row[2] = 0;
    }
    for (int k = (count < stride ? count : stride) + lane; k < stride; k += 64) row[3 + k] = -1;
}

// Head entry i of `head` (the keys, then the count) decided into `row` by one wave: what k_head_victims and
// k_heads_victims run per block.  An entry at or beyond the head's count, or without a node, writes 0 / -1
// and reads nothing of the state.
__device__ __forceinline__ void head_victims_row(const VictState& st, const VictHdr& h, const uint64_t* head, int i,
                                                 int stride, int node_base, VictRec* lds, int lds_cap,
                                                 VictRec* spill_row, int spill_stride, int32_t* row) {
    const uint64_t key = head[i], total = head[kTopK];
    const bool in = ((uint64_t)i < total) & (key != 0);  // (&: the key's and the count's loads are in flight together)
    victims_row(st, h, key, in, stride, node_base, lds, lds_cap, spill_row, spill_stride, row);
}

__global__ __launch_bounds__(64) void k_head_victims(VictState st, VictHdr h, const uint64_t* head, int cap, int stride,
                                                     int node_base, VictRec* spill, int spill_stride,
                                                     uint64_t* out_keys, int32_t* out) {
    __shared__ VictRec s_rec[kVictLds];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= cap) return;
    if (i == 0) {
        out_keys[lane] = head[lane];
        if (lane == 0) out_keys[kTopK] = head[kTopK];
    }
    head_victims_row(st, h, head, i, stride, node_base, s_rec, kVictLds,
                     spill ? spill + (size_t)i * spill_stride : nullptr, spill_stride,
                     out + (size_t)i * (3 + stride));
}

// kbhip_heads_victims: the same rows for n_req requests, grid (cap, n_req), blockIdx.y = the request.  Block
// (i, r) reads request r's head where k_rank_heads_merge left it and its header from hdr[r]; the staged
// records live in lds_recs records of dynamic LDS — min(kVictLds, the state's longest node), so that
// sessions of small nodes keep a CU's 32 one-wave blocks resident where the static 43 KB allow three.
extern __shared__ VictRec s_dyn_rec[];
__global__ __launch_bounds__(64) void k_heads_victims(VictState st, const VictHdr* __restrict__ hdr,
                                                      const uint64_t* __restrict__ heads, int cap, int stride,
                                                      int node_base, int lds_recs, VictRec* spill, int spill_stride,
                                                      uint64_t* out_keys, int32_t* out) {
    const int i = blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    if (i >= cap) return;
    const uint64_t* const head = heads + (size_t)r * (kTopK + 1);
    if (i == 0) {
        uint64_t* const keys = out_keys + (size_t)r * (kTopK + 1);
        keys[lane] = head[lane];
        if (lane == 0) keys[kTopK] = head[kTopK];
    }
    const size_t at = (size_t)r * cap + i;
    head_victims_row(st, hdr[r], head, i, stride, node_base, s_dyn_rec, lds_recs,
                     spill ? spill + at * spill_stride : nullptr, spill_stride, out + at * (3 + stride));
}

__global__ __launch_bounds__(256) void k_victims_patch(VictTask* task, VictJob* job, VictQueue* queue, int n_tasks,
                                                       int n_jobs, int n_queues, VictPatch p) {
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i < p.n_t) {
        const int at = p.t_pos[i];
        if (at >= 0 && at < n_tasks) task[at].flags = p.t_flags[i];
        return;
    }
    i -= p.n_t;
    if (i < p.n_j) {
        const int j = p.j_id[i];
        if (j >= 0 && j < n_jobs) job[j] = p.j_rec[i];
        return;
    }
    i -= p.n_j;
    if (i < p.n_q) {
        const int q = p.q_id[i];
        if (q >= 0 && q < n_queues) queue[q] = p.q_rec[i];
    }
}

// The eviction walk of one task, one block of kWalkBlock threads: what k_walk_victims and
// k_walk_victims_from share.  The loop over the entries is sequential by its definition (entry i + 1 reads
// what entry i evicted); inside an entry the threads stage and link the node's records under the overlay,
// thread 0 runs walk_step (the decision, the ops, the fold: the evicted prefix is a few tasks, and the fold
// keeps the job's entries in victim order), and a barrier hands the overlay to the next entry.  Records,
// overlay, header and progress live in LDS (43 KB + 9 KB); nothing is prefetched for the next entry while
// thread 0 decides.
constexpr int kWalkBlock = 256;
struct WalkLds { VictRec rec[kVictLds]; WalkOverlay ov; VictHdr h; WalkCtl c; };
struct WalkArgs { int node_base; VictRec* spill; int spill_stride; int32_t *out_pod, *out_node; };  // as the kernels'

// Entry i, by the whole block.  A key without a node, or whose node can be staged nowhere, stages nothing
// and is still visited.  res (k_walk_victims_from; else null): *res = i unless the entry was refused with
// kWalkCapacity.  Every thread reads walk_step's result behind the last barrier.
__device__ __forceinline__ void walk_entry(const VictState& st, WalkLds& s, const WalkArgs& a, uint64_t key, int i,
                                           int* res) {
    const int tid = threadIdx.x;
    int off = 0, n;
    if (!head_node_range(st, key, a.node_base, kVictLds, a.spill, a.spill_stride, off, n)) n = 0;
    VictRec* const rec = n <= kVictLds ? s.rec : a.spill;
    for (int k = tid; k < n; k += kWalkBlock) vict_stage_walk(st, s.h, s.ov, off + k, rec[k]);
    __syncthreads();
    for (int k = tid; k < n; k += kWalkBlock) vict_link(rec, k);
    __syncthreads();
    if (tid == 0) {
        const int acted = s.c.acted;
        walk_step(s.h, s.ov, s.c, rec, n, key_idx(key), key_score(key), a.out_pod, a.out_node);
        if (res && (s.c.stop != kWalkCapacity || s.c.acted != acted)) *res = i;  // passed over or acted on
    }
    __syncthreads();
}

// Entries [i, lim) of `head` in order until one stops the walk, then out_info[0 .. 3] and [6]: the stop reason,
// `total` (the count of the order `head` is part of: entries at and beyond it do not exist), the visits, the
// nodes acted on, the ops.  kHead (k_walk_victims): at most `cap` visits, and an entry whose key is not below
// after_key (0: none) is left out.  (Every condition is uniform over the block.)
template <bool kHead>
__device__ __forceinline__ void walk_loop(const VictState& st, WalkLds& s, const WalkArgs& a, const uint64_t* head,
                                          int i, int lim, int cap, uint64_t after_key, uint64_t total, int* res,
                                          int64_t* out_info) {
    for (; i < lim; ++i) {
        if (kHead && s.c.visited >= cap) break;
        const uint64_t key = head[i];
        if (kHead && after_key != 0 && key >= after_key) continue;
        walk_entry(st, s, a, key, i, res);
        if (s.c.stop != 0) break;
    }
    if (threadIdx.x != 0) return;
    out_info[0] = s.c.stop != 0 ? s.c.stop : (uint64_t)i < total ? kWalkHeadEnd : kWalkExhausted;
    out_info[1] = (int64_t)total;
    out_info[2] = s.c.visited;
    out_info[3] = s.c.acted;
    out_info[6] = s.c.n_ops;
}

// kbhip_walk_victims: the walk over the head from its top.
__global__ __launch_bounds__(kWalkBlock) void k_walk_victims(VictState st, VictHdr h0, const uint64_t* head, int cap,
                                                             uint64_t after_key, int task, int node_base,
                                                             VictRec* spill, int spill_stride, int ov_cap_j,
                                                             int ov_cap_q, int64_t cap_ops, int64_t* out_info,
                                                             int32_t* out_pod, int32_t* out_node) {
    __shared__ WalkLds s;
    const int tid = threadIdx.x;
    if (tid == 0) {
        s.h = h0;
        walk_ov_init(s.ov, ov_cap_j, ov_cap_q);
        s.c = WalkCtl{0, cap_ops, 0, 0, 0, -1, 0, task};
    }
    __syncthreads();
    const uint64_t total = head[kTopK];
    const int in_head = total < (uint64_t)kTopK ? (int)total : kTopK;
    walk_loop<true>(st, s, WalkArgs{node_base, spill, spill_stride, out_pod, out_node}, head, 0, in_head, cap,
                    after_key, total, nullptr, out_info);
    if (tid == 0) {
        out_info[4] = s.c.last_node;
        out_info[5] = s.c.last_score;
        out_info[7] = 0;
    }
}

// kbhip_walk_victims_from, the stateless pre-pass: window entry blockIdx.x decided against the state as it
// stands by one wave — head_victims_row with no victim row (stride 0: vict_decide stores no victim), so
// flags[3 i ..] = entry i's count, evict, flags and nothing else is written.  Dynamic LDS as k_heads_victims.
__global__ __launch_bounds__(64) void k_walk_flags(VictState st, VictHdr h, const uint64_t* __restrict__ head, int cap,
                                                   int node_base, int lds_recs, VictRec* spill, int spill_stride,
                                                   int32_t* flags) {
    const int i = blockIdx.x;
    if (i >= cap || i >= kTopK) return;
    head_victims_row(st, h, head, i, 0, node_base, s_dyn_rec, lds_recs,
                     spill ? spill + (size_t)i * spill_stride : nullptr, spill_stride, flags + 3 * i);
}

// kbhip_walk_victims_from, the walk: the same loop over a window every entry of which is behind the
// caller's resume point (the bounded sweep left the others out), so no entry is skipped by its key and an
// entry's window index is the number of entries decided before it: `lim` bounds the visits.  The entries
// before the first one the pre-pass found VALID (a ballot over the flag words) are passed over without
// staging: no eviction precedes them, so the overlay is empty and the stateless flag is the walk's answer.
// The loop starts at that entry — it too is decided by walk_step, and the entries after it never by their
// flag: carried state can turn an invalid node valid.  s_res: the window index of the resume point, the
// last entry passed over or acted on (an entry refused with kWalkCapacity is met again by the next call).
__global__ __launch_bounds__(kWalkBlock) void k_walk_victims_from(VictState st, VictHdr h0, const uint64_t* head,
                                                                  int cap, const int32_t* flags, int task,
                                                                  int node_base, VictRec* spill, int spill_stride,
                                                                  int ov_cap_j, int ov_cap_q, int64_t cap_ops,
                                                                  int64_t* out_info, int32_t* out_pod,
                                                                  int32_t* out_node) {
    __shared__ WalkLds s;
    __shared__ int s_first, s_res;
    const int tid = threadIdx.x;
    const uint64_t total = head[kTopK];
    const int in_win = total < (uint64_t)kTopK ? (int)total : kTopK;
    const int lim = cap < in_win ? cap : in_win;  // the entries this call decides
    if (tid < 64) {                               // (wave 0: one lane per window entry)
        const uint64_t valid = __ballot(tid < lim && (flags[3 * tid + 2] & 1) != 0);
        if (tid == 0) {
            const int first = valid ? __ffsll((unsigned long long)valid) - 1 : -1;
            const int passed = first < 0 ? lim : first;
            s_first = first;
            s_res = passed - 1;
            s.h = h0;
            walk_ov_init(s.ov, ov_cap_j, ov_cap_q);
            s.c = WalkCtl{0, cap_ops, 0, passed, 0, -1, 0, task};
        }
    }
    __syncthreads();
    walk_loop<false>(st, s, WalkArgs{node_base, spill, spill_stride, out_pod, out_node}, head,
                     s_first < 0 ? lim : s_first, lim, cap, 0, total, &s_res, out_info);
    if (tid == 0) {
        const int res = s_res;
        out_info[4] = res >= 0 ? key_idx(head[res]) : -1;
        out_info[5] = res >= 0 ? key_score(head[res]) : 0;
        out_info[7] = res;
        out_info[8] = s.c.last_node;
        out_info[9] = s_first;
    }
}

// kbhip_walk_next, the scan: entry i of the kept order `keys` (total entries), pos <= i < total, is decided
// against the state as it stands by one wave — victims_row with no victim row, its three words in LDS — and
// the lowest position whose decision is VALID is formed in scan[0] by lane 0's atomicMin (a vector atomic;
// the word is ~0 when the launch starts — kbhip_walk_begin sets it, k_walk_cursor puts it back — so "none" is
// any value >= total).  The grid is at
// most kWalkScanBlocks one-wave blocks; block b takes entries pos + b, pos + b + grid, ..: the entries in
// flight at any moment are a stretch of about one grid's length, so few entries behind the result are
// decided in vain, and a short remainder takes a short grid.  scan[1] += the entries a block decided, once
// per block.
// The early exit: before each entry the block reads the word, and an entry behind its present value cannot
// lower it — nor can any later entry of the block — so the block ends.  That is a hint and nothing rests on
// it: the load is relaxed, may be stale and may be missed altogether; the word only ever falls, so an entry
// left out was behind the final value too, and every entry at or before the final value is decided — the
// atomicMin alone forms the result.  (One load by the wave, made uniform: the branch is taken by the whole
// block or not at all, before any barrier.)
// The spill rule: the scan has no spill rows (one per entry in flight would be grid x longest node records),
// so an entry whose node holds more records than the lds_recs staged in LDS is not decided here — it reports
// itself as if VALID, and k_walk_cursor's serial loop, which owns the one spill row, decides it exactly.
// The live cursor (kbhip_walk_begin_live; L = WalkLive, else WalkFixed and nothing of this is compiled):
// the kept order holds every node that passes the class's other predicates, and an entry is VALID only where
// walk_live_pred — eval_first_fit's pod-affinity test, on the count tables as they stand — holds for its node
// too.  The test comes before the staging: a few loads, the same for every lane (made uniform: the branch is
// taken by the whole block or not at all, before any barrier), and an entry that fails stages nothing and
// counts as decided.  The spill rule comes before the test: a node longer than the LDS rows reports itself
// undecided, predicate included.  The early exit and the atomicMin's argument are untouched: an entry that
// fails the predicate lowers nothing, as an entry that is not VALID.
struct WalkFixed { static constexpr bool kLive = false; };
__device__ __forceinline__ bool walk_live_pred(const WalkFixed&, uint64_t) { return true; }
__device__ __forceinline__ bool walk_live_pred(const WalkLive& lv, uint64_t key) {
    const int n = key_idx(key) - lv.nc.base;
    if (key == 0 || n < 0 || n >= lv.nc.n) return true;  // no node of the session: what head_node_range makes of it
    const bool ok = !(lv.cf.pred_on && lv.c.aff) || aff_pred(lv.c, lv.t, lv.nc, n);
    return __builtin_amdgcn_readfirstlane((int)ok) != 0;
}
constexpr int kWalkScanBlocks = 2048;
template <class L>
__device__ __forceinline__ void walk_scan(const VictState& st, const VictHdr& h, const uint64_t* __restrict__ keys,
                                          int pos, int total, int node_base, int lds_recs, uint32_t* scan,
                                          const L& lv) {
    __shared__ int32_t s_row[3];
    const int lane = threadIdx.x;
    if (pos < 0) return;
    uint32_t decided = 0;
    for (int64_t at = (int64_t)pos + blockIdx.x; at < total; at += gridDim.x) {
        const int i = (int)at;
        const uint32_t seen = __builtin_amdgcn_readfirstlane(
            __hip_atomic_load(&scan[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (seen < (uint32_t)i) break;
        const uint64_t key = keys[i];
        int off = 0, n = 0;
        const bool fits = head_node_range(st, key, node_base, lds_recs, nullptr, 0, off, n);
        bool cand = !fits && n > lds_recs;  // a node of the state longer than the LDS rows: the serial loop's
        if constexpr (L::kLive) {
            if (!cand && !walk_live_pred(lv, key)) {  // (uniform) decided: it cannot act, and nothing was staged
                decided += 1;
                continue;
            }
        }
        if (!cand) {
            victims_row(st, h, key, fits, 0, node_base, s_dyn_rec, lds_recs, nullptr, 0, s_row);
            cand = lane == 0 && (s_row[2] & 1) != 0;  // (lane 0 wrote the words it reads)
        }
        decided += 1;
        if (lane == 0 && cand) atomicMin(&scan[0], (uint32_t)i);
        __syncthreads();  // (one wave: the next entry's staging follows lane 0's reads of this one's)
    }
    if (lane == 0 && decided) atomicAdd(&scan[1], decided);
}
__global__ __launch_bounds__(64) void k_walk_scan(VictState st, VictHdr h, const uint64_t* __restrict__ keys, int pos,
                                                  int total, int node_base, int lds_recs, uint32_t* scan) {
    walk_scan(st, h, keys, pos, total, node_base, lds_recs, scan, WalkFixed{});
}
__global__ __launch_bounds__(64) void k_walk_scan_live(VictState st, VictHdr h, const uint64_t* __restrict__ keys,
                                                       int pos, int total, int node_base, int lds_recs,
                                                       uint32_t* scan, WalkLive lv) {
    walk_scan(st, h, keys, pos, total, node_base, lds_recs, scan, lv);
}

// kbhip_walk_next, the walk: one block.  first = min(scan[0], total).  Entries [pos, first) are passed over
// and counted: no eviction of this call precedes them, so the overlay is empty and the scan's stateless
// answer is the walk's.  From `first` the loop k_walk_victims_from runs, over at most `cap` entries of the
// kept order: that entry too is decided by walk_step, and no entry after it by a flag.  s_res: the position
// of the last entry passed over or acted on (an entry refused with kWalkCapacity is met again by the next call).
// The live cursor's loop: the predicate is tested in front of walk_entry, on the tables the scan read — an
// entry that fails is passed over, counted and gives no op (a spill-rule candidate among them) — and the
// loop ends behind the first node acted on: that node's evictions change the count tables only through
// kbhip_apply_ops, which the carried overlay cannot stand in for, so the entries behind it are the next
// call's.  The stop reason then follows the position behind that node.  (Every branch is uniform over the
// block and in front of walk_entry's barriers; thread 0 alone writes s.c and *res.)
__device__ __forceinline__ void walk_loop_live(const VictState& st, WalkLds& s, const WalkArgs& a, const uint64_t* keys,
                                               int i, int lim, uint64_t total, int* res, int64_t* out_info,
                                               const WalkLive& lv) {
    for (; i < lim; ++i) {
        const uint64_t key = keys[i];
        if (!walk_live_pred(lv, key)) {
            if (threadIdx.x == 0) {
                s.c.visited += 1;
                *res = i;
            }
            continue;
        }
        walk_entry(st, s, a, key, i, res);
        if (s.c.stop != 0 || s.c.acted != 0) break;
    }
    if (threadIdx.x != 0) return;
    out_info[0] = s.c.stop != 0 ? s.c.stop : (uint64_t)(*res + 1) < total ? kWalkHeadEnd : kWalkExhausted;
    out_info[1] = (int64_t)total;
    out_info[2] = s.c.visited;
    out_info[3] = s.c.acted;
    out_info[6] = s.c.n_ops;
}

template <class L>
__device__ __forceinline__ void walk_cursor(const VictState& st, const VictHdr& h0, const uint64_t* keys, int pos,
                                            int total, int cap, uint32_t* scan, int task, int node_base,
                                            VictRec* spill, int spill_stride, int ov_cap_j, int ov_cap_q,
                                            int64_t cap_ops, int64_t* out_info, int32_t* out_pod, int32_t* out_node,
                                            const L& lv) {
    __shared__ WalkLds s;
    __shared__ int s_res;
    const int tid = threadIdx.x;
    const uint32_t seen = scan[0];
    const int first = seen < (uint32_t)total ? ((int)seen < pos ? pos : (int)seen) : total;
    const int lim = total - first < cap ? total : first + cap;
    if (tid == 0) {
        s_res = first - 1;
        s.h = h0;
        walk_ov_init(s.ov, ov_cap_j, ov_cap_q);
        s.c = WalkCtl{0, cap_ops, 0, first - pos, 0, -1, 0, task};
    }
    __syncthreads();
    if constexpr (L::kLive)
        walk_loop_live(st, s, WalkArgs{node_base, spill, spill_stride, out_pod, out_node}, keys, first, lim,
                       (uint64_t)total, &s_res, out_info, lv);
    else
        walk_loop<false>(st, s, WalkArgs{node_base, spill, spill_stride, out_pod, out_node}, keys, first, lim, cap, 0,
                         (uint64_t)total, &s_res, out_info);
    if (tid == 0) {
        out_info[4] = s_res + 1;
        out_info[5] = first < total ? first : -1;
        out_info[7] = 0;
        out_info[8] = s.c.last_node;
        out_info[9] = scan[1];
        scan[0] = ~0u;  // the two words as the next call's scan expects them (every thread read scan[0] before
        scan[1] = 0;    // the first barrier)
    }
}
__global__ __launch_bounds__(kWalkBlock) void k_walk_cursor(VictState st, VictHdr h0, const uint64_t* keys, int pos,
                                                            int total, int cap, uint32_t* scan, int task,
                                                            int node_base, VictRec* spill, int spill_stride,
                                                            int ov_cap_j, int ov_cap_q, int64_t cap_ops,
                                                            int64_t* out_info, int32_t* out_pod, int32_t* out_node) {
    walk_cursor(st, h0, keys, pos, total, cap, scan, task, node_base, spill, spill_stride, ov_cap_j, ov_cap_q, cap_ops,
                out_info, out_pod, out_node, WalkFixed{});
}
__global__ __launch_bounds__(kWalkBlock) void k_walk_cursor_live(VictState st, VictHdr h0, const uint64_t* keys,
                                                                 int pos, int total, int cap, uint32_t* scan, int task,
                                                                 int node_base, VictRec* spill, int spill_stride,
                                                                 int ov_cap_j, int ov_cap_q, int64_t cap_ops,
                                                                 int64_t* out_info, int32_t* out_pod,
                                                                 int32_t* out_node, WalkLive lv) {
    walk_cursor(st, h0, keys, pos, total, cap, scan, task, node_base, spill, spill_stride, ov_cap_j, ov_cap_q, cap_ops,
                out_info, out_pod, out_node, lv);
}

// The scan's two words as k_walk_scan expects them: ~0 and 0 (kbhip_walk_begin; k_walk_cursor restores them).
hipError_t launch_walk_scan_init(uint32_t* scan, hipStream_t stm) {
    const hipError_t e = hipMemsetAsync(scan, 0xff, sizeof(uint32_t), stm);
    return e != hipSuccess ? e : hipMemsetAsync(scan + 1, 0, sizeof(uint32_t), stm);
}

hipError_t launch_walk_cursor(const VictState& st, const VictHdr& h, const uint64_t* keys, int64_t pos, int64_t total,
                              int cap, int task, int node_base, int lds_recs, VictRec* spill, int spill_stride,
                              int ov_cap_j, int ov_cap_q, int64_t cap_ops, uint32_t* scan, int64_t* out_info,
                              int32_t* out_pod, int32_t* out_node, hipStream_t stm, const WalkLive* live) {
    static_assert(sizeof(WalkLive) + sizeof(VictState) + sizeof(VictHdr) + 128 <= 4096, "the kernels' arguments");
    if (cap < 1 || cap > kTopK || cap_ops < 1 || lds_recs < 1 || lds_recs > kVictLds || pos < 0 || pos > total ||
        total > INT32_MAX || !keys || !scan)
        return hipErrorInvalidValue;
    // (an empty remainder still takes both launches: the call's launch count does not depend on its position)
    const int64_t left = total - pos;
    const dim3 grid(left < 1 ? 1u : left < kWalkScanBlocks ? (unsigned)left : (unsigned)kWalkScanBlocks);
    const size_t lds = (size_t)lds_recs * sizeof(VictRec);
    if (live) {
        hipLaunchKernelGGL(k_walk_scan_live, grid, dim3(64), lds, stm, st, h, keys, (int)pos, (int)total, node_base,
                           lds_recs, scan, *live);
        hipLaunchKernelGGL(k_walk_cursor_live, dim3(1), dim3(kWalkBlock), 0, stm, st, h, keys, (int)pos, (int)total,
                           cap, scan, task, node_base, spill, spill_stride, ov_cap_j, ov_cap_q, cap_ops, out_info,
                           out_pod, out_node, *live);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_walk_scan, grid, dim3(64), lds, stm, st, h, keys, (int)pos, (int)total, node_base, lds_recs,
                       scan);
    hipLaunchKernelGGL(k_walk_cursor, dim3(1), dim3(kWalkBlock), 0, stm, st, h, keys, (int)pos, (int)total, cap,
                       scan, task, node_base, spill, spill_stride, ov_cap_j, ov_cap_q, cap_ops,
                       out_info, out_pod, out_node);
    return hipGetLastError();
}

hipError_t launch_walk_victims_from(const VictState& st, const VictHdr& h, const uint64_t* head, int cap, int task,
                                    int node_base, int lds_recs, VictRec* spill, int spill_stride, int ov_cap_j,
                                    int ov_cap_q, int64_t cap_ops, int32_t* flags, int64_t* out_info,
                                    int32_t* out_pod, int32_t* out_node, hipStream_t stm) {
    if (cap < 1 || cap > kTopK || cap_ops < 1 || lds_recs < 1 || lds_recs > kVictLds) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_walk_flags, dim3(cap), dim3(64), (size_t)lds_recs * sizeof(VictRec), stm, st, h, head, cap,
                       node_base, lds_recs, spill, spill_stride, flags);
    hipLaunchKernelGGL(k_walk_victims_from, dim3(1), dim3(kWalkBlock), 0, stm, st, h, head, cap,
                       (const int32_t*)flags, task, node_base, spill, spill_stride, ov_cap_j, ov_cap_q, cap_ops,
                       out_info, out_pod, out_node);
    return hipGetLastError();
}

hipError_t launch_walk_victims(const VictState& st, const VictHdr& h, const uint64_t* head, int cap, uint64_t after_key,
                               int task, int node_base, VictRec* spill, int spill_stride, int ov_cap_j, int ov_cap_q,
                               int64_t cap_ops, int64_t* out_info, int32_t* out_pod, int32_t* out_node,
                               hipStream_t stm) {
    if (cap < 1 || cap > kTopK || cap_ops < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_walk_victims, dim3(1), dim3(kWalkBlock), 0, stm, st, h, head, cap, after_key, task, node_base,
                       spill, spill_stride, ov_cap_j, ov_cap_q, cap_ops, out_info, out_pod, out_node);
    return hipGetLastError();
}

hipError_t launch_head_victims(const VictState& st, const VictHdr& h, const uint64_t* head, int cap, int stride,
                               int node_base, VictRec* spill, int spill_stride, uint64_t* out_keys, int32_t* out,
                               hipStream_t stm) {
    if (cap < 1 || cap > kTopK || stride < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_head_victims, dim3(cap), dim3(64), 0, stm, st, h, head, cap, stride, node_base, spill,
                       spill_stride, out_keys, out);
    return hipGetLastError();
}

hipError_t launch_heads_victims(const VictState& st, const VictHdr* hdr, const uint64_t* heads, int n_req, int cap,
                                int stride, int node_base, int lds_recs, VictRec* spill, int spill_stride,
                                uint64_t* out_keys, int32_t* out, hipStream_t stm) {
    if (n_req < 1 || n_req > kMaxChunk || cap < 1 || cap > kTopK || stride < 1 || lds_recs < 1 || lds_recs > kVictLds)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_heads_victims, dim3(cap, n_req), dim3(64), (size_t)lds_recs * sizeof(VictRec), stm, st, hdr,
                       heads, cap, stride, node_base, lds_recs, spill, spill_stride, out_keys, out);
    return hipGetLastError();
}

hipError_t launch_victims_patch(const VictState& st, const VictPatch& p, hipStream_t stm) {
    const int n = p.n_t + p.n_j + p.n_q;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_victims_patch, dim3((n + 255) / 256), dim3(256), 0, stm, const_cast<VictTask*>(st.task),
                       const_cast<VictJob*>(st.job), const_cast<VictQueue*>(st.queue), st.n_tasks, st.n_jobs,
                       st.n_queues, p);
    return hipGetLastError();
}

}  // namespace kbhip

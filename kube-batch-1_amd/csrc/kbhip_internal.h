// kbhip_internal.h — declarations shared by the host encoder/driver and the
// kernel translation unit (not part of the public ABI).
#pragma once
#include <hip/hip_runtime.h>

#include "kbhip_types.h"

namespace kbhip {

// Read-only per-session tables (device pointers).
struct DevTables {
    const TaskClass* classes;
    const Term* terms;
    const Req* reqs;
    const int32_t* vals;
    const int64_t* valint;  // per global value id: parsed int64 (Gt/Lt)
    const uint8_t* valok;   // per global value id: strconv.ParseInt succeeded
    const uint64_t* masks;  // tolerated-taint / port-conflict / own-port words
    // pod (anti-)affinity (kbhip_affinity.h)
    const int32_t* aff_items;  // programs: ea pairs, ipa quads, upd triples
    int32_t* aff_cnt;          // count tables, indexed cnt_off + domain
    int32_t* aff_scalar;       // PA target totals, session counters
    // placement 7 with per-domain candidates: the best key of every domain of the
    // class's dd_space over all blocks (kDedupMax entries; zero between launches)
    uint64_t* dd_max;
};

// The per-task path's control block set up on the device (CtrlInit, kbhip_types.h).
hipError_t launch_ctrl_init(PopCtrl* ctrl, const CtrlInit& ci, hipStream_t st);
// Per-task sweep; dbg (debug only): per-node keys, raw inter-pod counts,
// [lo, hi, F, max key]: rows of 2 npad + 4 words per task of the chunk; commit_here = the last block commits (one GPU).  Sharded
// sessions reduce ctrl->slot[task_i] across shards and then launch_commit_task.
hipError_t launch_sweep_argmax(const Conf& cf, const NodeCols& nc, const DevTables& t, PopCtrl* ctrl, int task_i,
                               uint64_t* walk, hipStream_t st, bool commit_here = true, uint64_t* dbg = nullptr,
                               bool defer_visits = false, const int64_t* ipa_pre = nullptr);
// defer_visits (one GPU): the GetAccessibleResource mutation of the walk runs as a
// second, grid-wide kernel (k_visit_mutate) instead of in the committing block.
hipError_t launch_commit_task(const NodeCols& nc, const DevTables& t, PopCtrl* ctrl, int task_i, const uint64_t* walk,
                              hipStream_t st);
// Inter-pod affinity priority prepass: min / max of the raw count over all
// nodes for task task_i (interpod_affinity.go:214-226) -> ctrl->ipa_lo/hi;
// counts (optional, npad entries): each node's raw count, which the sweep that
// follows on the same state then reads (launch_sweep_argmax's ipa_pre).
hipError_t launch_ipa_minmax(const NodeCols& nc, const DevTables& t, PopCtrl* ctrl, int task_i, hipStream_t st,
                             int64_t* counts = nullptr);

// Reclaim / preempt (kbhip_evict.hip): per-node order keys of the task of
// ctrl->cls[0] (by_score 1: predicates + score, preempt; 0: predicates only,
// reclaim), *count += passing nodes; one node-row update (op 0 evict, 1
// pipeline, 2 unpipeline).
// kbhip_sweep_scores' standalone sweep: keys per node, the passing count in
// 8 counters (counts[32 g], g = 0..7; the caller zeroes and sums them).
hipError_t launch_evict_read(const void* buf, size_t bytes, hipStream_t st);  // time_sweeps_cold = 2
void set_sweep_variant(int v);  // option "sweep_variant" (process-wide tuning knob)
hipError_t launch_score_sweep(const Conf& cf, const NodeCols& nc, const DevTables& t, const TaskClass& c,
                              const PopCtrl* ctrl, uint64_t* keys, uint32_t* counts, hipStream_t st);
// Walk read-outs (kbhip_walk.hip): ordered stream compaction over the node
// columns in three launches.  mark: one ballot word per wave (mask, 4 per
// block of kBlock nodes) and the block's count (blk[b]); scan: blk[0 .. nb)
// becomes the exclusive prefix sum and blk[nb] the total; scatter: record i of
// the ascending node order lands at index i.  compact_blocks(n) = nb.
int compact_blocks(int n_nodes);
// mark of kbhip_fit_deltas: the nodes the walk of the task of class c visits
// (PredicateFn passes and NodeOrderFn scores: the walk's own eval_node /
// eval_node_aff, ctrl task 0 holding the inter-pod prepass and fallback node)
hipError_t launch_fit_mark(const Conf& cf, const NodeCols& nc, const DevTables& t, const TaskClass& c,
                           const PopCtrl* ctrl, uint64_t* mask, uint32_t* blk, hipStream_t st);
// mark of kbhip_walk_visits: nodes with a non-zero visit counter
hipError_t launch_visit_mark(const NodeCols& nc, uint64_t* mask, uint32_t* blk, hipStream_t st);
hipError_t launch_compact_scan(uint32_t* blk, int nb, hipStream_t st);
// out_delta[3 i ..]: Idle.FitDelta(Resreq) of record i's node (resource_info.go:134-147)
hipError_t launch_fit_scatter(const NodeCols& nc, const TaskClass& c, const uint64_t* mask, const uint32_t* blk,
                              int32_t* out_node, int64_t* out_delta, hipStream_t st);
// out_count[i]: the node's counter, cleared when clear != 0
hipError_t launch_visit_scatter(const NodeCols& nc, const uint64_t* mask, const uint32_t* blk, int32_t* out_node,
                                uint32_t* out_count, int clear, hipStream_t st);
hipError_t launch_rank_nodes(const Conf& cf, const NodeCols& nc, const DevTables& t, const PopCtrl* ctrl,
                             int by_score, uint64_t* keys, uint32_t* count, hipStream_t st);
// Wide score ranges: the passing keys of launch_rank_nodes (n keys, zeros
// dropped; *count = passing nodes) sorted descending by four stable 8-bit
// counting passes over the score (hist: rank_hist_words(n) words; tmp: n keys).
hipError_t launch_rank_radix(const uint64_t* keys, int n, const uint32_t* count, uint32_t* hist, uint64_t* tmp,
                             uint64_t* sorted, hipStream_t st);
// The walk order by a hand-written stable counting sort over the score (class
// score range [slo, shi] of at most 256 values; hipErrorInvalidValue beyond):
// keys, sorted (descending key order), *count += passing nodes; hist holds
// rank_hist_words(n) words of scratch.
hipError_t launch_rank_sorted(const Conf& cf, const NodeCols& nc, const DevTables& t, const TaskClass& c,
                              const PopCtrl* ctrl, int by_score, int slo, int shi, uint64_t* keys, uint32_t* hist,
                              uint64_t* sorted, uint32_t* count, hipStream_t st);
size_t rank_hist_words(int n_nodes);
// The sort's scan kernel for another translation unit (kbhip_heads.hip): v[0 .. n) becomes its exclusive
// prefix sum, in one block.
hipError_t launch_rank_scan(uint32_t* v, int n, hipStream_t st);
// The current device's compute units (256 when the runtime does not say): what the sweeps size their grids by.
int device_cu_count();
// The head of that order without a per-node array (kbhip_heads.hip, kbhip_rank_nodes): a fused
// predicate + score + top-kTopK sweep, then a one-block merge of the blocks'
// lists.  Afterwards scratch[0 .. kTopK) = the best keys, descending (0 beyond
// the passing count), scratch[kTopK] = the passing count; scratch holds
// rank_head_words() 8-byte words.  ctrl task 0: the class, the fallback node
// and the inter-pod prepass, as for launch_rank_nodes.
int rank_head_blocks(int n_nodes);  // the sweep's grid
size_t rank_head_words();
// kbhip_rank_victim_nodes: the walk without the nodes validateVictims
// (preempt.go:355-370) rejects whatever the plugins answer.  The candidate
// table (device pointers) holds per queue q and node n the Running tasks with
// a Running node copy and a job: tab[(q * 4 + k) * npad + n], k = 0 their
// count, 1..3 the sum of their Resreq (cpu, memory, gpu); row nq is the total
// over the queues.  A lane that owns a node reads at most two rows of it.
// mode (KBHIP_VICTIMS_*): 1 total - row q, 2 row q - the job's own, 3 the
// job's own; the job's own candidates per node come as a list of distinct
// nodes in ascending order (own_node) with their four sums (own_sum[4 i ..]),
// found by binary search.  A node is kept when its candidate count is > 0 and
// the sum is not strictly below (rc, rm, rg) — the task's InitResreq — in all
// three resources.
struct VictArgs {
    const int64_t* tab;
    const int32_t* own_node;
    const int64_t* own_sum;
    int32_t npad, nq, q, mode, own_n;
    int64_t rc, rm, rg;
};
// The head's launch; v non-null (kbhip_rank_victim_nodes): the test above applied by the lane that
// evaluates the node (the count is the kept nodes').  bound != 0 (kbhip_walk_victims_from, v non-null):
// the sweep's bounded variant — only nodes whose key is below bound are counted or listed.
hipError_t launch_rank_head(const Conf& cf, const NodeCols& nc, const DevTables& t, const TaskClass& c,
                            const PopCtrl* ctrl, int by_score, const VictArgs* v, uint64_t* scratch, hipStream_t st,
                            uint64_t bound = 0);
// kbhip_rank_heads: the heads of n_req (1 .. kMaxChunk) tasks of one session in
// one sweep launch (grid (bx, n_req), blockIdx.y = the request) and one merge
// launch (grid n_req).  Request r is d_desc[r] in device memory: its class,
// its victim test (read with filt only; own_node / own_sum point into the
// call's concatenated own-job lists) and the PopCtrl task slot that holds its
// inter-pod min / max (launch_ipa_minmax(…, slot, …) before the sweep; several
// requests of one class share a slot).  Afterwards scratch[r (kTopK + 1) ..]
// is request r's result as launch_rank_head leaves one; scratch holds
// rank_heads_words() 8-byte words whatever the batch.  rank_heads_bx: the
// sweep's grid x for that many requests.
struct HeadDesc {
    TaskClass c;
    VictArgs v;
    int32_t slot, pad;
};
int rank_heads_bx(int n_nodes, int n_req);
size_t rank_heads_words();
hipError_t launch_rank_heads(const Conf& cf, const NodeCols& nc, const DevTables& t, const HeadDesc* d_desc, int n_req,
                             bool filt, const PopCtrl* ctrl, int by_score, uint64_t* scratch, int* bx_out,
                             hipStream_t st);
// kbhip_explain_tasks (kbhip_explain.hip): the verdict byte (node_verdict,
// kbhip_eval.h) of every node for n_req (1 .. kMaxChunk) tasks of one session
// and each task's histogram, in one sweep launch (grid (bx, n_req), blockIdx.y
// = the request, its class d_cls[request] in device memory) and one reduce
// launch (grid n_req).  verdict: n_req rows of nc.n bytes, or null (no
// per-node store); part: n_req * bx * 16 words of block counts; out: n_req
// rows of 16 64-bit bins.  explain_bx: the sweep's grid x for that many
// requests (cap > 0: at most cap).
int explain_bx(int n_nodes, int n_req, int cap);
hipError_t launch_explain(const Conf& cf, const NodeCols& nc, const DevTables& t, const TaskClass* d_cls, int n_req,
                          int bx, uint8_t* verdict, uint32_t* part, int64_t* out, hipStream_t st);
// The filtered full walk: a stable compaction of launch_rank_sorted's /
// launch_rank_radix's output (sorted, *count keys) in three launches — per
// block of kBlock keys the survivors' count (blk[b]), k_rank_scan over blk
// (blk[nblk] = the total afterwards), a scatter of the survivors and their
// candidate counts in order.  blk holds vict_blocks(n) + 1 words; out_keys /
// out_cands n_nodes entries.
int vict_blocks(int n_nodes);
hipError_t launch_vict_compact(const uint64_t* sorted, const uint32_t* count, int n_nodes, const VictArgs& v,
                               uint32_t* blk, uint64_t* out_keys, int32_t* out_cands, hipStream_t st);
// kbhip_walk_begin_live's marks (kbhip_heads.hip): keys[n] = the by_score 0 key of node n where it passes
// class c's predicates with the pod-affinity predicate left out (eval_first_fit on c with its affinity
// program switched off), else 0, for every node; count[0] = the nodes, count[1] = 0.  The node order is the
// walk order, so launch_vict_compact takes keys / count as it takes a sorted ranking's.  One launch.
hipError_t launch_live_keys(const Conf& cf, const NodeCols& nc, const DevTables& t, const TaskClass& c, uint64_t* keys,
                            uint32_t* count, hipStream_t st);
// One session's ranking request in a batched launch (what-if sessions).
struct RankDesc {
    Conf cf;
    NodeCols nc;
    DevTables t;
    TaskClass c;  // the request's class (ctrl->cls[0]), here so a block needs no load chain to it
    const PopCtrl* ctrl;
    int by_score, shi, nb, nblk;
    uint64_t* keys;
    uint32_t* hist;
    uint64_t* sorted;
    uint32_t* count;
};
hipError_t fill_rank_desc(RankDesc* q, const Conf& cf, const NodeCols& nc, const DevTables& t, const TaskClass& c,
                          const PopCtrl* ctrl, int by_score, int slo, int shi, uint64_t* keys, uint32_t* hist,
                          uint64_t* sorted, uint32_t* count);
hipError_t launch_rank_sorted_multi(const RankDesc* d_desc, int n_desc, int max_nblk, hipStream_t st);
// Count-table deltas (pod (anti-)affinity): idx >= 0 aff_cnt, < 0 aff_scalar[-1 - idx]; distinct indices.
hipError_t launch_tab_add(const DevTables& t, const int32_t* idx, const int32_t* delta, int n, hipStream_t st);
hipError_t launch_rel_add(const NodeCols& nc, const int32_t* node, const int64_t* d, int n, hipStream_t st);
// carry's node-row patch: entry i writes the low size bytes (8, 4 or 1) of val at device address addr
struct RowPatch {
    uint64_t addr, val;
    int32_t size, pad;
};
hipError_t launch_row_patch(const RowPatch* e, int n, hipStream_t st);
// op 0 Releasing += (rc, rm, rg), 1 a pipelined pod committed, 2 uncommitted, on this shard's row n of
// global node g (n = -1: another shard's node — the replicated count tables only)
hipError_t launch_node_op(const NodeCols& nc, const DevTables& t, int op, int n, int g, int cls, int64_t rc,
                          int64_t rm, int64_t rg, hipStream_t st);

// A batch of those updates grouped stably by node (kbhip_apply_ops; device pointers): segment i holds the
// operations [seg_off[i], seg_off[i + 1]) of local row seg_node[i] in batch order (the rows are distinct);
// operation j is kind_cls[j] & 3 (the op above) on class kind_cls[j] >> 2, an eviction's Resreq in req[3 j ..].
struct ApplyOps {
    const int32_t* seg_node;
    const int32_t* seg_off;  // n_seg + 1 entries
    const int32_t* kind_cls;
    const int64_t* req;
    int n_seg;
    // the victim-candidate table (VictArgs above) while the session holds a current one, else null: an
    // eviction takes the pod's Resreq and 1 off its queue's row (queue[j], evictions only) and off the total row
    const int32_t* queue;
    int64_t* vict;
    int32_t vict_npad, vict_nq;
};
// One lane per segment, as many blocks as the segments need (one launch whatever the batch holds).
hipError_t launch_apply_ops(const NodeCols& nc, const DevTables& t, const ApplyOps& a, hipStream_t st);

// kbhip_head_victims (kbhip_victims.hip): the victim state — what ssn.Reclaimable / ssn.Preemptable read
// on a node, as flat records (device pointers; an encode-only session's host vectors for
// kbhip_debug_victims).  task[node_off[n] .. node_off[n + 1]): the tasks of node n that were candidates
// when the state was built (Running, a Running node copy, a job), in pod-index order — the CSR never
// changes between rebuilds, an eviction or unevict only clears kVictRunCopy.
constexpr int32_t kVictRunCopy = 1, kVictCritical = 2;  // VictTask::flags
struct VictTask {
    int32_t pod, job, queue, min_avail;
    int64_t req[3];  // Resreq: cpu, memory, gpu
    int32_t flags, pad;
};
struct VictJob {
    double alloc[3];  // drf's allocated (HJob::drf_alloc)
    int32_t ready, pad;  // gang's readyTaskNum
};
struct VictQueue {
    double alloc[3], des[3];  // proportion's allocated / deserved
};
struct VictState {
    const int32_t* node_off;  // n_nodes + 1
    const VictTask* task;
    const VictJob* job;
    const VictQueue* queue;
    int32_t n_nodes, n_jobs, n_queues, n_tasks;
};
// One call's constants: the task, the candidates' mode and the victim functions of the action in tier
// order (EvictAction::compile_victims' codes: 1 gang, 2 conformance, 3 drf, 4 proportion; 0 ends a tier).
constexpr int kVictMaxCodes = 40;
struct VictHdr {
    double total[3];  // drf's cluster total
    double la[3];     // the task's job's drf allocation plus the task's Resreq (drf.go:88-90)
    int64_t ireq[3];  // the task's InitResreq
    int32_t mode, queue, job, n_codes;
    int8_t codes[kVictMaxCodes];
};
// A node task staged for vict_decide (kbhip_eval.h): its record, its job's and queue's records, the first
// task of the node with the same job / queue (where the running sums of one plugin call live), and the
// decision's marks.
struct VictRec {
    VictTask t;
    double jalloc[3], qalloc[3], qdes[3], run[3];
    int32_t ready, jfirst, qfirst, stamp;
    uint8_t cand, alive, pad[6];
};
constexpr int kVictLds = 256;  // node tasks a block stages in LDS; larger nodes use the spill rows
// out_keys[0 .. kTopK] = head[0 .. kTopK] (launch_rank_head's result: the keys, then the count); row i of
// out (3 + stride int32: count, evict, flags, then stride victims) for head entry i < cap, defined for
// every i (entries beyond min(cap, head[kTopK]): 0 / -1).  spill: cap rows of spill_stride records, read
// only by nodes of more than kVictLds tasks (spill_stride >= the largest node of the state).
hipError_t launch_head_victims(const VictState& st, const VictHdr& h, const uint64_t* head, int cap, int stride,
                               int node_base, VictRec* spill, int spill_stride, uint64_t* out_keys, int32_t* out,
                               hipStream_t stm);
// kbhip_heads_victims: the same rows for n_req (1 .. kMaxChunk) requests in one launch, grid (cap, n_req).
// Request r's head is heads[r (kTopK + 1) ..] (launch_rank_heads' result), its header hdr[r] (device
// memory).  out_keys: n_req results of kTopK + 1 words; out: n_req * cap rows as above, request-major.
// lds_recs (1 .. kVictLds): the records a block stages in dynamic LDS, at least min(kVictLds, the largest
// node of the state).  spill: n_req * cap rows of spill_stride records, or null when no node is longer.
hipError_t launch_heads_victims(const VictState& st, const VictHdr* hdr, const uint64_t* heads, int n_req, int cap,
                                int stride, int node_base, int lds_recs, VictRec* spill, int spill_stride,
                                uint64_t* out_keys, int32_t* out, hipStream_t stm);
// The records kbhip_apply_ops left dirty, scattered into the state: task[t_pos[i]].flags = t_flags[i],
// job[j_id[i]] = j_rec[i], queue[q_id[i]] = q_rec[i] (device pointers; indices distinct within each list).
struct VictPatch {
    const int32_t* t_pos;
    const int32_t* t_flags;
    const int32_t* j_id;
    const VictJob* j_rec;
    const int32_t* q_id;
    const VictQueue* q_rec;
    int32_t n_t, n_j, n_q;
};
hipError_t launch_victims_patch(const VictState& st, const VictPatch& p, hipStream_t stm);

// kbhip_walk_victims (k_walk_victims, kbhip_victims.hip): one task's eviction walk over the head.  The
// evictions of a node that is valid but does not cover InitResreq change what the victim functions read on
// the nodes after it; the walk carries those changes in an overlay over the victim state instead of
// writing them: per touched job the evicted Resreq sum (off drf's allocation) and the evicted count (off
// gang's readyTaskNum), per touched queue the evicted Resreq sum (off proportion's allocation).  Short
// lists keyed by id, searched linearly; Resreq sums are integers, so the sums are exact and the order of
// the subtractions does not matter.  cap_j / cap_q: the capacities in force (option "walk_overlay_max").
constexpr int kWalkOvJobs = 256, kWalkOvQueues = 64;
struct WalkOverlay {
    int32_t n_j, n_q, cap_j, cap_q;
    int32_t j_id[kWalkOvJobs], j_gone[kWalkOvJobs];
    int64_t j_sub[kWalkOvJobs][3];
    int32_t q_id[kWalkOvQueues];
    int64_t q_sub[kWalkOvQueues][3];
};
// The walk's progress and result words (kbhip.h: out_info[0 .. 5], the op count).  stop: 0 while the walk
// goes on, else the KBHIP_WALK_* reason.
constexpr int32_t kWalkAssigned = 1, kWalkExhausted = 2, kWalkHeadEnd = 3, kWalkCapacity = 4;
struct WalkCtl {
    int64_t n_ops, cap_ops;
    int32_t stop, visited, acted, last_node, last_score, task;
};
// One block.  head: launch_rank_head's result (keys, then the count).  Visits up to `cap` head entries
// whose key is below after_key (0: from the top), stages each node against st under the overlay and runs
// walk_step (kbhip_eval.h).  out_info (8 int64): stop, total, visited, acted, last node, last score, ops,
// 0; out_pod / out_node: cap_ops entries each — every op is an eviction of out_pod on out_node but the last
// one of a walk that stopped KBHIP_WALK_ASSIGNED, which pipelines `task` there.  spill: one row of
// spill_stride records for nodes of more than kVictLds tasks.
hipError_t launch_walk_victims(const VictState& st, const VictHdr& h, const uint64_t* head, int cap, uint64_t after_key,
                               int task, int node_base, VictRec* spill, int spill_stride, int ov_cap_j, int ov_cap_q,
                               int64_t cap_ops, int64_t* out_info, int32_t* out_pod, int32_t* out_node,
                               hipStream_t stm);
// kbhip_walk_victims_from (kbhip_victims.hip): the walk over a window — `head` is the bounded sweep's
// result, every entry of it behind the caller's resume point — in two launches.  k_walk_flags: the
// window's first `cap` entries decided side by side against the state as it stands, one wave each
// (head_victims_row with no victim row), flags[3 i ..] = entry i's count, evict, flags; lds_recs and spill
// (cap rows) as launch_heads_victims.  k_walk_victims_from: one block; the entries before the first VALID
// one are passed over by their flag (no eviction precedes them, so the flag is the walk's answer), from it
// on the loop k_walk_victims runs.  out_info (10 int64): stop, total, visited, acted, the resume point's node and
// score (-1, 0: no entry was passed over or acted on), ops, the resume point's window index (-1), the last
// acted-on node (-1), the first VALID entry's window index (-1).
hipError_t launch_walk_victims_from(const VictState& st, const VictHdr& h, const uint64_t* head, int cap, int task,
                                    int node_base, int lds_recs, VictRec* spill, int spill_stride, int ov_cap_j,
                                    int ov_cap_q, int64_t cap_ops, int32_t* flags, int64_t* out_info,
                                    int32_t* out_pod, int32_t* out_node, hipStream_t stm);
// kbhip_walk_next (kbhip_victims.hip): the walk over entries [pos, total) of a kept order — `keys` is
// launch_vict_compact's output, `total` its count — in two launches.  k_walk_scan: one wave per entry (a
// bounded grid of one-wave blocks, each taking every grid-th entry until it meets one behind the result so
// far), each decided against the state as it stands; scan[0] = the lowest position whose decision
// is VALID (an atomicMin by lane 0; any value >= total: none), scan[1] = the entries it decided; both words
// are as launch_walk_scan_init leaves them when the launch starts, and k_walk_cursor puts them back, so a
// call that fails between the two launches ends the cursor.  An entry whose node holds more than lds_recs records is not
// decided by the scan and counts as VALID for it.  k_walk_cursor: one block; the entries before scan[0] are
// passed over, from it on the loop k_walk_victims runs over at most `cap` entries, with the one spill row.
// out_info (10 int64): stop, total, entries decided (passed over and visited), acted, the next position,
// scan[0]'s position (-1: none), ops, 0, the last acted-on node (-1), scan[1].
// live (kbhip_walk_begin_live's cursor; null: kbhip_walk_begin's): `keys` left the class's pod-affinity
// predicate out, and both kernels (their live instantiations) test it per entry on the count tables as they
// stand — the scan before it stages an entry (a node longer than lds_recs is not decided in this either), the
// walk before walk_entry; an entry that fails is counted as decided and gives no op.  The walk then ends
// behind the first node it acts on: HEAD_END while entries remain, EXHAUSTED at total, ASSIGNED / CAPACITY as
// walk_step sets them.
struct WalkLive {
    static constexpr bool kLive = true;
    Conf cf;
    NodeCols nc;
    DevTables t;
    TaskClass c;
};
hipError_t launch_walk_scan_init(uint32_t* scan, hipStream_t stm);
hipError_t launch_walk_cursor(const VictState& st, const VictHdr& h, const uint64_t* keys, int64_t pos, int64_t total,
                              int cap, int task, int node_base, int lds_recs, VictRec* spill, int spill_stride,
                              int ov_cap_j, int ov_cap_q, int64_t cap_ops, uint32_t* scan, int64_t* out_info,
                              int32_t* out_pod, int32_t* out_node, hipStream_t stm, const WalkLive* live = nullptr);

// Selection-key format of a batched launch: 32-bit keys when the class's
// score range and the node count fit (kbhip_kernels.hip, PopArgs).
struct KeyFormat {
    bool use32 = false;
    bool ent32 = false;  // parallel-levels placement entries fit 32 bits too
    int32_t base = 0, shift = 0, idxmax = 0;
};
struct ShardMsg;  // kbhip_eval.h
struct MboxArgs;  // kbhip_eval.h
// Batched path v2: one launch per pop chunk; results land in `out_dev`
// (device pointer of a pinned host PopOut, pop_out_bytes() long).
// placement 2: parallel levels; 6: sessions with Backfilled nodes; 7:
// pod-affinity classes; 3 (node-array shards): no placement — the shard's
// top-64 with rows goes to shard_out for the all-gather, then
// launch_shard_place places.
hipError_t launch_pop_batch(const Conf& cf, const NodeCols& nc, const DevTables& t, int cls, int n_tasks,
                            int gang_mode, int min_avail, int ready_count, uint32_t epoch, uint64_t* cand,
                            uint32_t* arrive, void* out_dev, hipStream_t st, int placement, const KeyFormat& kf,
                            int fit_set, ShardMsg* shard_out = nullptr, const struct MboxArgs* mbox = nullptr);
// The placement of a sharded batched pop on the gathered ShardMsgs (world of
// them, rank order): identical on every shard; each writes back its own rows.
// flags (mailbox exchange): this rank's mailbox flags of the pop's slot —
// the kernel waits until rank r's flag (flags[16 r]) reads seq.
hipError_t launch_shard_place(const Conf& cf, const NodeCols& nc, const DevTables& t, int cls, int n_tasks,
                              int gang_mode, int min_avail, int ready_count, uint32_t epoch, const KeyFormat& kf,
                              const ShardMsg* msgs, int world, void* out_dev, hipStream_t st,
                              const uint64_t* flags = nullptr, uint32_t seq = 0, struct PopLink* link = nullptr);
// Chain state of overlapped batched pops (kbhip_kernels.hip, k_pop_batch_ov):
// done = sequence number of the last pop whose node write-back is visible;
// touched[e % kLinkSlots][i] = {e << 32 | node}, candidate i of pop e (node
// -1: none).  At session open: done 0, every slot tagged 0 with no nodes.
constexpr int kMaxGroups = 32;  // >= kGroups of kbhip_kernels.hip
// Overlapped pops' lists as self-tagged granules: 64 keys + 4 FitDelta counts
// per block and per group, 80 words (5 lines) apart.
constexpr int kCandStride = 80;
constexpr int kMaxDep = 2;     // previous pops an overlapped pop runs beside (streams - 1)
constexpr int kMaxSpeculate = 6;  // predicted batched pops queued behind the running one (option "speculate")
constexpr int kLinkSlots = 4;  // > kMaxDep: a slot is rewritten only after its readers finished
// rows[e % kLinkSlots][f][i] = {e << 32 | half f of candidate i's row after
// pop e} — kRowWords 32-bit halves of Row's dynamic and static fields (not
// Backfilled: overlapped pops run only in sessions without it), written after
// pop e's write-back drained: the next pops read their previous pops'
// candidates' rows from here (contiguous, self-tagged) instead of polling
// `done` and gathering the node columns.
constexpr int kRowWords = 22;
struct PopLink {
    uint32_t done;
    uint32_t pad0[31];
    uint64_t touched[kLinkSlots][64];
    uint64_t rows[kLinkSlots][kRowWords][64];
};
// Overlapped shard pops (mailbox exchange): this shard's sweep of pop mb.seq
// beside pop mb.seq-1's k_shard_place (launch_shard_place with `link`), whose
// candidates it leaves out and then re-evaluates once that pop's write-back on
// this device is done (prev_chained: pop mb.seq-1 ran as such a pop and
// published its candidates in `link`).  Sends the shard's message like
// placement 3.
hipError_t launch_shard_sweep_ov(const Conf& cf, const NodeCols& nc, const DevTables& t, int cls, const TaskClass& cl,
                                 int n_tasks, int gang_mode, int min_avail, int ready_count, uint32_t epoch,
                                 uint64_t* cand, uint32_t* arrive, const KeyFormat& kf, int fit_set, PopLink* link,
                                 int prev_chained, const MboxArgs& mb, hipStream_t st);
// Overlapped batched pop number `seq` (>= 1) on stream st; pop seq-1 may
// still run on the other stream: it leaves that pop's candidates out of its
// sweep and re-evaluates them once pop seq-1's write-back is done.  cand
// holds (blocks + kMaxGroups) * 64 keys, arrive (3 * kMaxGroups + 1) * 32
// counters, both private to the launch's stream; fit_set alternates per
// launch on a stream (FitDelta counter sets).
hipError_t launch_pop_batch_ov(const Conf& cf, const NodeCols& nc, const DevTables& t, int cls, const TaskClass& cl,
                               int n_tasks, int gang_mode, int min_avail, int ready_count, uint32_t epoch,
                               uint64_t* cand, uint32_t* arrive, void* out_dev, hipStream_t st, const KeyFormat& kf,
                               PopLink* link, uint32_t seq, int fit_set, int dep, uint32_t msg_from);
// Node updates of given placements again (after launch_undo_pop).
hipError_t launch_redo_pop(const NodeCols& nc, const DevTables& t, int cls, int n, const int32_t* node,
                           const int32_t* kind, hipStream_t st);
// One task's walk FitDelta histogram on the current state (kbhip_kernels.hip):
// the task is ctrl's task 0 (class, fallback node, inter-pod affinity min /
// max); chosen >= 0: the node its walk stopped at (ctrl->slot[0] <- its walk
// key on this shard, 0 elsewhere: all-reduce MAX before the histogram on
// shards — launch_fit_key, then launch_fit_count).
hipError_t launch_fit_key(const Conf& cf, const NodeCols& nc, const DevTables& t, PopCtrl* ctrl, int chosen,
                          hipStream_t st);
hipError_t launch_fit_count(const Conf& cf, const NodeCols& nc, const DevTables& t, PopCtrl* ctrl, int chosen,
                            int chosen_kind, int32_t* out4, hipStream_t st);
// Inverse node updates of a batched pop's placements (a retracted prediction).
hipError_t launch_undo_pop(const NodeCols& nc, const DevTables& t, int cls, int n, const int32_t* node,
                           const int32_t* kind, hipStream_t st);
int pop_blocks(int n_nodes, int* R_out);
// A batched pop of one session in a multi-session launch (what-if sessions,
// placement 6 or 7): the arguments of launch_pop_batch.
constexpr int kPopMulti = 8;  // sessions per launch (kernel argument space)
struct PopReq {
    Conf cf;
    NodeCols nc;
    DevTables t;
    int cls, n_tasks, gang_mode, min_avail, ready_count;
    uint32_t epoch;
    KeyFormat kf;
    uint64_t* cand;
    uint32_t* arrive;
    void* out;
    int placement, fit_set;
};
// Launches every request (grouped by nodes per lane, key type and placement,
// kPopMulti per launch; *launches = launches made).
hipError_t launch_pop_batch_multi(const PopReq* reqs, int n, hipStream_t st, int* launches);
// A what-if session's per-task chunk (k_sweep_argmax_multi): m tasks of the
// control block `ctrl`, committed on the device (defer: the visited nodes'
// GetAccessibleResource mutation by k_visit_mutate_multi).
struct SweepReq {
    Conf cf;
    NodeCols nc;
    DevTables t;
    PopCtrl* ctrl;
    uint64_t* walk;
    int m;
    int defer;
};
hipError_t launch_sweep_multi(const SweepReq* reqs, int n, int k, hipStream_t st, int* launches);
size_t pop_out_bytes();
// The persistent pop engine (kbhip_engine.hip, kbhip_engine.h): one resident
// grid of engine_grid(A) blocks serving batched pops from a descriptor ring.
struct EngArgs;
hipError_t launch_engine(const Conf& cf, const NodeCols& nc, const DevTables& t, const EngArgs& A, hipStream_t st);
hipError_t engine_occupancy(int* blocks_per_cu, bool lists = false);  // lists: the list-mode kernel
int engine_grid(const EngArgs& A);
#ifdef KBHIP_STAMPS
hipError_t set_stamp_buffer(uint64_t* p);
#endif
#ifdef KBHIP_TIMELINE
hipError_t set_timeline_buffer(uint64_t* p);
#endif
struct PopOutHost {  // host view of the device PopOut: self-tagged granules
    uint64_t g[kMaxChunk];
    uint64_t fit[2];
};

}  // namespace kbhip

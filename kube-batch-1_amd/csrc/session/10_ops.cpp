// kbhip session, part 10: host-decided evictions and pipelines (kbhip_apply_ops)
#include "framework.h"

namespace kbhip {

namespace {

constexpr int kMarkEvicted = 1, kMarkPipelined = 2, kMarkNodeRel = 4;  // ops_sim's bits above the status
constexpr int kSimShift = 12;                                         // (St values stay below 1 << 12)

// The batch checked operation by operation against each pod's status as the
// operations before it leave it (S.ops_sim holds the pods the batch touched;
// reset before returning or throwing).  Nothing of the session changes: the
// marks are set by commit_marks once the batch is on the device.
void validate_ops(Session& S, const uint8_t* op, const int32_t* pod, const int32_t* node, int64_t n) {
    const int P = (int)S.pods.size();
    if (S.op_mark_gen != S.model_gen || (int)S.op_mark.size() != P) {  // a carry-over ended the earlier operations
        S.op_mark.assign(P, 0);
        S.op_mark_gen = S.model_gen;
    }
    if ((int)S.ops_sim.size() != P) S.ops_sim.assign(P, -1);
    vector<int32_t> touched;
    const char* bad = nullptr;
    for (int64_t i = 0; i < n && !bad; ++i) {
        const int pi = pod[i];
        if (pi < 0 || pi >= P) { bad = "kbhip_apply_ops: pod index out of range"; break; }
        const HPod& p = S.pods[pi];
        int32_t& sim = S.ops_sim[pi];
        if (sim < 0) {
            sim = p.status | ((int)S.op_mark[pi] | (p.node_rel ? kMarkNodeRel : 0)) << kSimShift;
            touched.push_back(pi);
        }
        const int st = sim & ((1 << kSimShift) - 1), mk = sim >> kSimShift;
        switch (op[i]) {
            case KBHIP_OP_EVICT:
                if (st != Running || (mk & kMarkNodeRel) || !on_node_of(p) || p.node >= S.n_total || p.job < 0)
                    bad = "kbhip_apply_ops: KBHIP_OP_EVICT of a pod that is not Running on its node";
                else sim = Releasing | (mk | kMarkEvicted) << kSimShift;
                break;
            case KBHIP_OP_PIPELINE:
                if (st != Pending || p.cls < 0 || p.job < 0)
                    bad = "kbhip_apply_ops: KBHIP_OP_PIPELINE of a pod that is not a Pending task with a task class";
                else if (node[i] < 0 || node[i] >= S.n_total)
                    bad = "kbhip_apply_ops: KBHIP_OP_PIPELINE node index out of range";
                else sim = Pipelined | (mk | kMarkPipelined) << kSimShift;
                break;
            case KBHIP_OP_UNPIPELINE:
                if (st != Pipelined || !(mk & kMarkPipelined))
                    bad = "kbhip_apply_ops: KBHIP_OP_UNPIPELINE of a pod no earlier KBHIP_OP_PIPELINE pipelined";
                else sim = Pending | (mk & ~kMarkPipelined) << kSimShift;
                break;
            case KBHIP_OP_UNEVICT:
                if (st != Releasing || !(mk & kMarkEvicted))
                    bad = "kbhip_apply_ops: KBHIP_OP_UNEVICT of a pod no earlier KBHIP_OP_EVICT evicted";
                else sim = Running | ((mk & ~kMarkEvicted) | kMarkNodeRel) << kSimShift;
                break;
            default: bad = "kbhip_apply_ops: unknown operation";
        }
    }
    for (int32_t pi : touched) S.ops_sim[pi] = -1;
    if (bad) throw Error(KBHIP_EINVAL, bad);
}

// The "evicted / pipelined by an earlier operation" marks of a batch that reached the host model and
// the device (a batch that failed on the way leaves the marks of the operations before it).
void commit_marks(Session& S, const uint8_t* op, const int32_t* pod, int64_t n) {
    for (int64_t i = 0; i < n; ++i) {
        uint8_t& m = S.op_mark[pod[i]];
        switch (op[i]) {
            case KBHIP_OP_EVICT: m |= kMarkEvicted; break;
            case KBHIP_OP_PIPELINE: m |= kMarkPipelined; break;
            case KBHIP_OP_UNPIPELINE: m &= (uint8_t)~kMarkPipelined; break;
            default: m &= (uint8_t)~kMarkEvicted; break;
        }
    }
}

// The host-model half of a validated batch: the eviction actions' own statement operations
// (framework.h), in order; out = the batch's node operations in order, none of them launched.
// drf / proportion open first (on the statuses before the batch, as OnSessionOpen sees them), so
// the event handlers change what a later action reads.
void apply_ops_model(Session& S, const uint8_t* op, const int32_t* pod, const int32_t* node, int64_t n,
                     vector<NodeOp>& out) {
    S.fit_task = -1;
    Framework F(S);
    F.open_plugins();
    F.ops_out = &out;
    for (int64_t i = 0; i < n; ++i) {
        switch (op[i]) {
            case KBHIP_OP_EVICT: F.evict_in_session(pod[i]); break;
            case KBHIP_OP_PIPELINE: F.pipeline(pod[i], node[i]); break;
            case KBHIP_OP_UNPIPELINE: F.unpipeline(pod[i]); break;
            default: F.unevict(pod[i]); break;
        }
    }
}

size_t align8(size_t x) { return (x + 7) & ~(size_t)7; }

}  // namespace

// The node operations of a batch on the device: grouped stably by node in
// pinned staging (distinct nodes in first-touch order, segment offsets, then
// per operation its kind and class and an eviction's Resreq), one copy, one
// launch_apply_ops.  Nothing waits: ev_ops marks the end of the copy, and the
// next call waits for it before it writes the staging again.
static int launch_node_ops(Session& S, const vector<NodeOp>& ops) {
    const size_t M = ops.size();
    if (!M) return 0;
    if (S.ops_seg.size() != (size_t)S.n_total) S.ops_seg.assign(S.n_total, -1);
    vector<int32_t> seg_node, seg_cnt;  // first-touch order
    struct SegReset {  // ops_seg is -1 everywhere between calls, whichever way this one ends
        vector<int32_t>& seg;
        const vector<int32_t>& nodes;
        ~SegReset() { for (int32_t g : nodes) seg[g] = -1; }
    } seg_reset{S.ops_seg, seg_node};
    for (const NodeOp& o : ops) {
        int32_t& sg = S.ops_seg[o.node];
        if (sg < 0) { sg = (int32_t)seg_node.size(); seg_node.push_back(o.node); seg_cnt.push_back(0); }
        seg_cnt[sg]++;
    }
    const size_t D = seg_node.size();
    const bool vict = S.vict_live && S.b_vict.p;  // the victim-candidate table follows the evictions
    // staging layout (8-byte aligned parts): req[3 M] | seg_node[D] | seg_off[D + 1] | kind_cls[M] | queue[M]
    // (queue: only with a live victim-candidate table)
    const size_t o_req = 0, o_node = o_req + 3 * M * sizeof(int64_t), o_off = o_node + align8(D * sizeof(int32_t)),
                 o_kc = o_off + align8((D + 1) * sizeof(int32_t)), o_q = o_kc + align8(M * sizeof(int32_t)),
                 bytes = o_q + (vict ? align8(M * sizeof(int32_t)) : 0);
    if (!S.ev_ops) HIPCHK(hipEventCreateWithFlags(&S.ev_ops, hipEventDisableTiming));
    else HIPCHK(hipEventSynchronize(S.ev_ops));  // the previous call's copy has read the staging
    S.h_ops.fit(bytes, std::max<size_t>(bytes + bytes / 2, 4096));
    S.b_ops.grow(S.stream, bytes, std::max<size_t>(bytes + bytes / 2, 4096));
    uint8_t* const h = S.h_ops.as<uint8_t>();
    int64_t* h_req = (int64_t*)(h + o_req);
    int32_t* h_node = (int32_t*)(h + o_node);
    int32_t* h_off = (int32_t*)(h + o_off);
    int32_t* h_kc = (int32_t*)(h + o_kc);
    int32_t* h_q = vict ? (int32_t*)(h + o_q) : nullptr;
    int32_t run = 0;
    for (size_t d = 0; d < D; ++d) {
        h_node[d] = seg_node[d] - S.nc.base;  // (one-GPU sessions: base 0)
        h_off[d] = run;
        run += seg_cnt[d];
        seg_cnt[d] = h_off[d];  // the segment's write cursor
    }
    h_off[D] = run;
    for (const NodeOp& o : ops) {
        const int32_t j = seg_cnt[S.ops_seg[o.node]]++;
        h_kc[j] = o.kind | (o.cls << 2);
        h_req[3 * (size_t)j] = o.req.c; h_req[3 * (size_t)j + 1] = o.req.m; h_req[3 * (size_t)j + 2] = o.req.g;
        if (h_q) h_q[j] = o.queue;
    }
    uint8_t* d = (uint8_t*)S.b_ops.p;
    HIPCHK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, S.stream));
    HIPCHK(hipEventRecord(S.ev_ops, S.stream));
    ApplyOps a{(const int32_t*)(d + o_node), (const int32_t*)(d + o_off), (const int32_t*)(d + o_kc),
               (const int64_t*)(d + o_req), (int)D, vict ? (const int32_t*)(d + o_q) : nullptr,
               vict ? (int64_t*)S.b_vict.p : nullptr, S.nc.npad, (int32_t)S.queues.size()};
    HIPCHK(launch_apply_ops(S.nc, S.tab, a, S.stream));
    return 1;
}

int64_t apply_ops(Session& S, const uint8_t* op, const int32_t* pod, const int32_t* node, int64_t n,
                  int64_t* out_launches) {
    if (S.world != 1) throw Error(KBHIP_EUNSUPPORTED, "kbhip_apply_ops on a node-sharded session");
    if (out_launches) *out_launches = 0;
    if (n == 0) return 0;
    if (n > (int64_t)INT32_MAX)  // (the segment offsets on the device are 32-bit)
        throw Error(KBHIP_EINVAL, "kbhip_apply_ops: n exceeds 2^31 - 1 operations");
    validate_ops(S, op, pod, node, n);
    struct VictGuard {  // a batch that fails part way leaves the victim-candidate table to be rebuilt
        Session& S;
        bool done = false;
        ~VictGuard() { if (!done) vict_stale(S); }
    } vict_guard{S};
    ov_quiesce(S);  // device work outside the batched pops' chain follows
    vector<NodeOp> ops;
    ops.reserve((size_t)n);
    apply_ops_model(S, op, pod, node, n, ops);
    int launches = launch_node_ops(S, ops);  // (a live victim-candidate table: its evictions in the same launch)
    if (S.vict_live) vict_apply_evictions(S, ops);
    vs_mark_dirty(S, pod, n);  // (host lists only: the next kbhip_head_victims patches the victim state)
    vict_guard.done = true;
    launches += flush_tables(S);  // the evictions' / unevicts' predicate-target changes
    commit_marks(S, op, pod, n);
    if (out_launches) *out_launches = launches;
    return n;
}

}  // namespace kbhip

using namespace kbhip;

extern "C" {

int64_t kbhip_apply_ops(kb_session* s, const uint8_t* op, const int32_t* pod, const int32_t* node, int64_t n,
                        int64_t* out_launches) {
    ABI_GUARD_S(s, {
        if (n < 0 || (n > 0 && (!op || !pod || !node)))
            throw kbhip::Error(KBHIP_EINVAL, "kbhip_apply_ops: negative n, or a null op / pod / node array with n > 0");
        return kbhip::apply_ops(kbhip::device_session(s), op, pod, node, n, out_launches);
    })
}

}  // extern "C"

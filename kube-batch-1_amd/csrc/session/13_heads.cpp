// kbhip session, part 13: the walk heads of several tasks in one launch pair (kbhip_rank_heads), and the batch
// staging it shares with kbhip_heads_victims
#include "session.h"

namespace kbhip {

namespace {

static_assert(KBHIP_RANK_HEADS_MAX == kMaxChunk, "one PopCtrl task slot per request");

constexpr size_t align8(size_t x) { return (x + 7) & ~(size_t)7; }

}  // namespace

// A batch's upload staged in h_heads_in (session.h: HeadsBatch).  Request i takes slot i of a PopCtrl image
// that belongs to the call (the session's own control block is not touched): its class there, and —
// by_score and a class with inter-pod priority terms — the class's min / max from one launch_ipa_minmax per
// distinct such class, whose slot the later requests of the class share.  The image, the descriptors, the
// own-job lists (one per distinct job of the batch) and `extra_bytes` of the caller's behind them (B.h_extra,
// filled before heads_enqueue) go up in one copy.  The candidate table is current when this is called.
void heads_stage(Session& S, const int32_t* task_ids, int n, bool by_score, int mode, size_t extra_bytes,
                 HeadsBatch& B) {
    B.n = n;
    B.by_score = by_score;
    B.mode = mode;
    B.n_ipa = 0;
    B.owns.clear();
    vector<HeadsBatch::Own>& owns = B.owns;
    int* const job_of = B.job_of;
    size_t own_total = 0;
    for (int i = 0; i < n; ++i) {
        job_of[i] = -1;
        if (mode == 0 || mode == KBHIP_VICTIMS_OTHER_QUEUES) continue;
        const int jb = S.pods[task_ids[i]].job;
        for (size_t k = 0; k < owns.size() && job_of[i] < 0; ++k)
            if (owns[k].jb == jb) job_of[i] = (int)k;
        if (job_of[i] >= 0) continue;
        owns.push_back(HeadsBatch::Own{jb, own_total, {}, {}});
        vict_own_list(S, jb, owns.back().node, owns.back().sum);
        own_total += owns.back().node.size();
        job_of[i] = (int)owns.size() - 1;
    }

    const size_t off_desc = align8(sizeof(PopCtrl)), off_sum = align8(off_desc + (size_t)n * sizeof(HeadDesc)),
                 off_node = off_sum + own_total * 4 * sizeof(int64_t),
                 off_extra = align8(off_node + own_total * sizeof(int32_t)),
                 in_bytes = align8(off_extra + extra_bytes);
    S.h_heads_in.fit(in_bytes, std::max<size_t>(2 * in_bytes, 1 << 16));
    S.b_heads_in.grow(S.stream, in_bytes, std::max<size_t>(2 * in_bytes, 1 << 16));
    if (!S.b_heads.p) S.b_heads.alloc<uint64_t>(rank_heads_words());
    B.off_desc = off_desc;
    B.in_bytes = in_bytes;

    uint8_t* const h_in = S.h_heads_in.as<uint8_t>();
    uint8_t* const d_in = (uint8_t*)S.b_heads_in.p;
    B.h_extra = h_in + off_extra;
    B.d_extra = d_in + off_extra;
    PopCtrl* const h_ctrl = (PopCtrl*)h_in;
    HeadDesc* const h_desc = (HeadDesc*)(h_in + off_desc);
    std::memset(h_in, 0, off_sum);
    h_ctrl->stop = -1;
    h_ctrl->n_tasks = n;
    h_ctrl->any_bf = S.any_bf;
    h_ctrl->fallback = S.fallback;
    for (const HeadsBatch::Own& o : owns) {
        if (o.node.empty()) continue;
        std::memcpy(h_in + off_sum + o.off * 4 * sizeof(int64_t), o.sum.data(),
                    o.node.size() * 4 * sizeof(int64_t));
        std::memcpy(h_in + off_node + o.off * sizeof(int32_t), o.node.data(), o.node.size() * sizeof(int32_t));
    }
    int* const ipa_slots = B.ipa_slots;
    int& n_ipa = B.n_ipa;
    for (int i = 0; i < n; ++i) {
        const HPod& p = S.pods[task_ids[i]];
        const TaskClass& c = S.classes[p.cls];
        h_ctrl->cls[i] = p.cls;
        HeadDesc& q = h_desc[i];
        q.c = c;
        q.slot = i;
        if (by_score && c.ipa_n > 0) {
            for (int k = 0; k < n_ipa && q.slot == i; ++k)
                if (h_ctrl->cls[ipa_slots[k]] == p.cls) q.slot = ipa_slots[k];
            if (q.slot == i) ipa_slots[n_ipa++] = i;
        }
        if (mode != 0) {
            const HeadsBatch::Own* o = job_of[i] >= 0 ? &owns[job_of[i]] : nullptr;
            const size_t own_n = o ? o->node.size() : 0;
            q.v = VictArgs{(const int64_t*)S.b_vict.p,
                           own_n ? (const int32_t*)(d_in + off_node) + o->off : nullptr,
                           own_n ? (const int64_t*)(d_in + off_sum) + 4 * o->off : nullptr,
                           S.nc.npad, (int32_t)S.queues.size(), S.jobs[p.job].queue, mode, (int32_t)own_n,
                           p.ireq.c, p.ireq.m, p.ireq.g};
        }
    }
}

// The staged batch uploaded and its heads enqueued: the inter-pod prepasses, the sweep and the merge.
// Afterwards (in stream order) b_heads holds request r's keys and count at word r (kTopK + 1).  Nothing is
// copied back or waited for.  Returns the launches made; *bx: the sweep grid's x size.
int heads_enqueue(Session& S, const HeadsBatch& B, int* bx) {
    uint8_t* const d_in = (uint8_t*)S.b_heads_in.p;
    PopCtrl* const d_ctrl = (PopCtrl*)d_in;
    HIPCHK(hipMemcpyAsync(d_in, S.h_heads_in.p, B.in_bytes, hipMemcpyHostToDevice, S.stream));
    for (int k = 0; k < B.n_ipa; ++k) HIPCHK(launch_ipa_minmax(S.nc, S.tab, d_ctrl, B.ipa_slots[k], S.stream));
    HIPCHK(launch_rank_heads(S.conf, S.nc, S.tab, (const HeadDesc*)(d_in + B.off_desc), B.n, B.mode != 0, d_ctrl,
                             B.by_score ? 1 : 0, (uint64_t*)S.b_heads.p, bx, S.stream));
    return B.n_ipa + 2;
}

// The heads (entries [0, cap) of the walk order and the order's length) of
// n tasks of the session as it stands: what kbhip_rank_nodes (mode 0) or
// kbhip_rank_victim_nodes (mode 1..3) answers for (task, by_score, first 0,
// cap), from one sweep launch, one merge launch and one copy back for the
// whole batch (heads_stage, heads_enqueue).  The candidate counts of the
// returned nodes come from the host copy of the table, as in
// rank_victim_nodes_abi.  Reads the session state, changes nothing but the
// victim-candidate table's liveness (vict_ensure).
int64_t rank_heads_abi(Session& S, const int32_t* task_ids, int n, bool by_score, int mode, int cap,
                       int64_t* out_total, int32_t* out_node, int32_t* out_score, int32_t* out_cands,
                       int64_t* out_info) {
    for (int i = 0; i < n; ++i)
        query_task(S, task_ids[i], "kbhip_rank_heads: task_ids[" + std::to_string(i) + "] ", mode != 0);
    query_begin(S, "kbhip_rank_heads");
    const bool rebuilt = mode != 0 && vict_ensure(S);

    HeadsBatch B;
    heads_stage(S, task_ids, n, by_score, mode, 0, B);
    S.h_heads_out.fit((size_t)kMaxChunk * (kTopK + 1) * sizeof(uint64_t));
    const vector<HeadsBatch::Own>& owns = B.owns;
    const int* const job_of = B.job_of;

    int64_t launches = flush_tables(S);  // evictions / unevicts so far change pod-affinity predicates
    int bx = 0;
    launches += heads_enqueue(S, B, &bx);
    HIPCHK(hipMemcpyAsync(S.h_heads_out.p, S.b_heads.p, (size_t)n * (kTopK + 1) * sizeof(uint64_t),
                          hipMemcpyDeviceToHost, S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));

    for (int i = 0; i < n; ++i) {
        const uint64_t* keys = S.h_heads_out.as<uint64_t>() + (size_t)i * (kTopK + 1);
        const int64_t total = (int64_t)keys[kTopK], n_keys = std::min<int64_t>(cap, total);
        const size_t row = (size_t)i * cap;
        const HeadsBatch::Own* o = job_of[i] >= 0 ? &owns[job_of[i]] : nullptr;
        static const vector<int32_t> no_node;
        static const vector<int64_t> no_sum;
        for (int64_t j = 0; j < cap; ++j) {
            const bool in = j < n_keys;
            out_node[row + j] = in ? key_idx(keys[j]) : -1;
            if (out_score) out_score[row + j] = in && by_score ? key_score(keys[j]) : 0;
            if (out_cands)
                out_cands[row + j] = in && mode != 0
                                         ? (int32_t)vict_count_host(S, mode, S.jobs[S.pods[task_ids[i]].job].queue,
                                                                    o ? o->node : no_node, o ? o->sum : no_sum,
                                                                    key_idx(keys[j]))
                                         : 0;
        }
        out_total[i] = total;
    }
    if (out_info) {
        out_info[0] = rebuilt ? 1 : 0;
        out_info[1] = launches;
        out_info[2] = bx;
    }
    S.stats.rank_heads += n;
    S.stats.sweeps += n;
    return n;
}

}  // namespace kbhip

using namespace kbhip;

extern "C" {

int64_t kbhip_rank_heads(kb_session* s, const int32_t* task_ids, int32_t n_tasks, int32_t by_score, int32_t victims,
                         int32_t cap, int64_t* out_total, int32_t* out_node, int32_t* out_score, int32_t* out_cands,
                         int64_t* out_info) {
    ABI_GUARD_S(s, {
        if (n_tasks < 0 || n_tasks > KBHIP_RANK_HEADS_MAX)
            throw kbhip::Error(KBHIP_EINVAL, "kbhip_rank_heads: n_tasks is 0 .. KBHIP_RANK_HEADS_MAX (64)");
        check_cap("kbhip_rank_heads", cap);
        check_by_score("kbhip_rank_heads", by_score);
        check_victims("kbhip_rank_heads", victims, true);
        if (!task_ids || !out_total || !out_node)
            throw kbhip::Error(KBHIP_EINVAL, "kbhip_rank_heads: null task_ids, out_total or out_node");
        kbhip::Session& S = kbhip::device_session(s);
        if (n_tasks == 0) return 0;
        return kbhip::rank_heads_abi(S, task_ids, n_tasks, by_score != 0, victims, cap, out_total, out_node,
                                     out_score, out_cands, out_info);
    })
}

}  // extern "C"

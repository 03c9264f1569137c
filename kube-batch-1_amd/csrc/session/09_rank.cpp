// kbhip session, part 09: the ranked node walk of one task (kbhip_rank_nodes)
#include "session.h"

namespace kbhip {

// Entries [first, first + cap) of the walk order of task `pod` (by_score:
// preempt's SelectBestNode order, else reclaim's index order) and the number
// of nodes in it.  The head of the walk (first + cap <= kTopK) comes from the
// fused top-kTopK sweep (launch_rank_head: nothing of size N written, kTopK
// keys and the count copied back); anything else from the full device sort of
// the reclaim / preempt actions (rank_launch), of which the count and then
// only the entries asked for are copied.  Reads the session state, changes
// nothing; nothing is kept for a later call.
int64_t rank_nodes_abi(Session& S, int pod, bool by_score, int64_t first, int32_t* out_node, int32_t* out_score,
                       int64_t cap) {
    if (pod < 0 || pod >= (int)S.pods.size() || S.pods[pod].cls < 0)
        throw Error(KBHIP_EINVAL, "task id has no task class (not a pending task of the session)");
    if (S.pods[pod].status != Pending)
        throw Error(KBHIP_EINVAL, "kbhip_rank_nodes: the task is not Pending (the session placed it)");
    if (S.world != 1) throw Error(KBHIP_EUNSUPPORTED, "kbhip_rank_nodes on a node-sharded session");
    ov_quiesce(S);
    const int cls = S.pods[pod].cls;
    const uint64_t* keys = nullptr;  // entries [first, first + n_keys) of the order, on the host
    int64_t total = 0, n_keys = 0;
    if (cap > 0 && first <= kTopK && cap <= kTopK - first) {
        if (!S.b_rank_head.p) S.b_rank_head.alloc<uint64_t>(rank_head_words());
        if (!S.h_rank_head)
            S.h_rank_head = (uint64_t*)MemPool::get().take(MemPool::kPinned, (size_t)(kTopK + 1) * sizeof(uint64_t),
                                                           &S.h_rank_head_cap);
        flush_tables(S);  // evictions / unevicts so far change pod-affinity predicates
        ctrl_setup(S, 1, &cls, 0, 0, 0, 0, -1, 0);
        const TaskClass& c = S.classes[cls];
        if (by_score && c.ipa_n > 0) HIPCHK(launch_ipa_minmax(S.nc, S.tab, S.d_ctrl, 0, S.stream));
        HIPCHK(launch_rank_head(S.conf, S.nc, S.tab, c, S.d_ctrl, by_score ? 1 : 0, (uint64_t*)S.b_rank_head.p,
                                S.stream));
        HIPCHK(hipMemcpyAsync(S.h_rank_head, S.b_rank_head.p, (size_t)(kTopK + 1) * sizeof(uint64_t),
                              hipMemcpyDeviceToHost, S.stream));
        HIPCHK(hipStreamSynchronize(S.stream));
        total = (int64_t)S.h_rank_head[kTopK];
        n_keys = first < total ? std::min(cap, total - first) : 0;
        keys = S.h_rank_head + first;
        S.stats.rank_heads++;
    } else {
        rank_launch(S, cls, by_score);
        HIPCHK(hipMemcpyAsync(S.h_rank, S.b_rank_cnt.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, S.stream));
        HIPCHK(hipStreamSynchronize(S.stream));
        if (S.h_rank[0] >> 32) throw Error(KBHIP_EDEVICE, "rank_nodes: node score outside the class score range");
        total = (int64_t)(uint32_t)S.h_rank[0];
        n_keys = first < total ? std::min(cap, total - first) : 0;
        if (n_keys > 0) {
            HIPCHK(hipMemcpyAsync(S.h_rank + 1, (const uint64_t*)S.b_rank_sorted.p + first,
                                  (size_t)n_keys * sizeof(uint64_t), hipMemcpyDeviceToHost, S.stream));
            HIPCHK(hipStreamSynchronize(S.stream));
        }
        keys = S.h_rank + 1;
        S.stats.rank_fulls++;
    }
    for (int64_t i = 0; i < n_keys; ++i) {
        out_node[i] = key_idx(keys[i]);
        if (out_score) out_score[i] = by_score ? key_score(keys[i]) : 0;
    }
    S.stats.sweeps++;
    return total;
}

}  // namespace kbhip

using namespace kbhip;

extern "C" {

int64_t kbhip_rank_nodes(kb_session* s, int32_t task_id, int32_t by_score, int64_t first, int32_t* out_node,
                         int32_t* out_score, int64_t cap) {
    ABI_GUARD_S(s, {
        if (!s) throw kbhip::Error(KBHIP_EINVAL, "null session");
        if (first < 0 || cap < 0 || (cap > 0 && !out_node))
            throw kbhip::Error(KBHIP_EINVAL, "kbhip_rank_nodes: negative first or cap, or null out_node with cap > 0");
        if (by_score != 0 && by_score != 1) throw kbhip::Error(KBHIP_EINVAL, "kbhip_rank_nodes: by_score is 0 or 1");
        if (s->s.encode_only) throw kbhip::Error(KBHIP_EINVAL, "encode-only session has no device state");
        kbhip::require_no_tickets(s->s);
        HIPCHK(hipSetDevice(s->s.device));
        return kbhip::rank_nodes_abi(s->s, task_id, by_score != 0, first, out_node, out_score, cap);
    })
}

}  // extern "C"

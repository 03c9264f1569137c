// kbhip session, part 15: the victim sets of a walk's head nodes (kbhip_head_victims), the preparation the
// victim queries share, and the same decision on the host tables (kbhip_debug_victims)
#include "framework.h"

namespace kbhip {

static_assert(KBHIP_HEAD_VICTIMS_VALID == 1 && KBHIP_HEAD_VICTIMS_COVERS == 2, "vict_decide's flag bits");

// One call's constants: the task, the mode, and the victim functions of the mode's action (preempt for the
// two preempt modes, reclaim for OTHER_QUEUES) tier by tier.
VictHdr make_hdr(const Session& S, const HPod& p, int mode) {
    VictHdr h{};
    h.total[0] = S.total.c; h.total[1] = S.total.m; h.total[2] = S.total.g;
    F3 la = S.jobs[p.job].drf_alloc;
    la.add(p.req);
    h.la[0] = la.c; h.la[1] = la.m; h.la[2] = la.g;
    h.ireq[0] = p.ireq.c; h.ireq[1] = p.ireq.m; h.ireq[2] = p.ireq.g;
    h.mode = mode;
    h.queue = S.jobs[p.job].queue;
    h.job = p.job;
    for (const auto& tier : victim_tier_codes(S, mode != KBHIP_VICTIMS_OTHER_QUEUES)) {
        if (h.n_codes + (int)tier.size() + 1 > kVictMaxCodes)
            throw Error(KBHIP_EUNSUPPORTED, "kbhip_head_victims: more than " + std::to_string(kVictMaxCodes) +
                                                " victim functions and tiers");
        for (int c : tier) h.codes[h.n_codes++] = (int8_t)c;
        h.codes[h.n_codes++] = 0;
    }
    return h;
}

// Both tables made current (built, or the dirty records patched in one launch) and the pending count-table
// changes flushed, for a call that opened the plugins.
VictPrep vict_prepare(Session& S, int batch_rows) {
    const bool vs_rebuilt = !S.vs_live;
    if (!S.vict_live) vict_check_size(S);     // both tables' limits are checked before either is uploaded
    if (vs_rebuilt) vs_build(S, batch_rows);  // (its own limit: after the host build, before the upload)
    const bool rebuilt = vict_ensure(S);
    int64_t launches = flush_tables(S);  // evictions / unevicts so far change pod-affinity predicates
    const int64_t patched = vs_rebuilt ? 0 : vs_patch(S);
    launches += patched ? 1 : 0;
    return VictPrep{rebuilt, vs_rebuilt, patched, launches};
}

// What every victim query does before it ranks or walks: the plugins opened, the call's header, both tables
// made current (kbhip_walk_next stops here: it walks a kept order).
HeadPrep state_prepare(Session& S, const HPod& p, int mode) {
    Framework F(S);
    F.open_plugins();  // drf / proportion as OnSessionOpen leaves them (kbhip_apply_ops opens them the same way)
    const VictHdr h = make_hdr(S, p, mode);
    const VictPrep vp = vict_prepare(S, 0);
    return HeadPrep{h, vp, vp.launches};
}

// What kbhip_head_victims, kbhip_walk_victims and kbhip_walk_victims_from do before their own kernel:
// state_prepare, then the head sweep and merge of kbhip_rank_victim_nodes enqueued — b_rank_head holds the
// head in stream order (bound != 0: the head among the nodes whose key is below it).
HeadPrep head_prepare(Session& S, const HPod& p, bool by_score, int mode, uint64_t bound) {
    const HeadPrep sp = state_prepare(S, p, mode);
    const VictHdr& h = sp.h;
    const VictPrep& vp = sp.vp;
    int64_t launches = sp.launches;
    vector<int32_t> own_node;
    vector<int64_t> own_sum;
    const VictArgs v = vict_args(S, p, mode, own_node, own_sum);
    launches += rank_head_enqueue(S, p.cls, by_score, &v, bound);
    return HeadPrep{h, vp, launches};
}

int64_t head_rows_unpack(const uint64_t* keys, const int32_t* rows, int cap, int stride, int dstride, bool by_score,
                         int32_t* out_node, int32_t* out_score, int32_t* out_count, int32_t* out_evict,
                         uint8_t* out_flags, int32_t* out_victim) {
    const int64_t total = (int64_t)keys[kTopK];
    int64_t max_count = 0;
    for (int i = 0; i < cap; ++i) {
        const bool in = i < total;
        const int32_t* row = rows + (size_t)i * (3 + dstride);
        out_node[i] = in ? key_idx(keys[i]) : -1;
        if (out_score) out_score[i] = in && by_score ? key_score(keys[i]) : 0;
        out_count[i] = row[0];
        out_evict[i] = row[1];
        out_flags[i] = (uint8_t)row[2];
        int32_t* vrow = out_victim + (size_t)i * stride;
        std::memcpy(vrow, row + 3, (size_t)dstride * sizeof(int32_t));
        std::fill(vrow + dstride, vrow + stride, -1);
        max_count = std::max<int64_t>(max_count, row[0]);
    }
    return max_count;
}

void head_info_fill(int64_t* out_info, const VictPrep& vp, int64_t launches, int64_t max_count) {
    const int64_t v[5] = {vp.rebuilt ? 1 : 0, vp.vs_rebuilt ? 1 : 0, vp.patched, launches, max_count};
    if (out_info) std::copy(v, v + 5, out_info);
}

// The head of the task's pruned walk and the victim decision on each of its first `cap` nodes: the state
// made current (built, or the dirty records patched in one launch), the head sweep and merge of
// kbhip_rank_victim_nodes, k_head_victims on the merged keys, one copy back, one wait.  Reads the session
// state and changes nothing but the currency of the two tables and the plugins' open state.
int64_t head_victims_abi(Session& S, int pod, bool by_score, int mode, int cap, int stride, int32_t* out_node,
                         int32_t* out_score, int32_t* out_count, int32_t* out_evict, uint8_t* out_flags,
                         int32_t* out_victim, int64_t* out_info) {
    const HPod& p = query_task(S, pod, "kbhip_head_victims: the task ", true, "task id ");
    query_begin(S, "kbhip_head_victims");
    const HeadPrep hp = head_prepare(S, p, by_score, mode);
    // the rows hold at most the longest node's tasks; a larger stride is filled with -1 here
    const int dstride = std::max(1, std::min(stride, S.vs_max_tasks));
    const size_t key_bytes = (size_t)(kTopK + 1) * sizeof(uint64_t),
                 out_bytes = key_bytes + (size_t)cap * (3 + (size_t)dstride) * sizeof(int32_t);
    S.h_vs_out.fit(out_bytes, std::max<size_t>(out_bytes, 4096));
    S.b_vs_out.grow(S.stream, out_bytes, std::max<size_t>(out_bytes, 4096));
    uint8_t* const d_out = (uint8_t*)S.b_vs_out.p;
    HIPCHK(launch_head_victims(vs_device_view(S), hp.h, (const uint64_t*)S.b_rank_head.p, cap, dstride, S.nc.base,
                               vs_spill_rows(S), vs_spill_stride(S), (uint64_t*)d_out, (int32_t*)(d_out + key_bytes),
                               S.stream));
    HIPCHK(hipMemcpyAsync(S.h_vs_out.p, d_out, out_bytes, hipMemcpyDeviceToHost, S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));
    const uint64_t* keys = S.h_vs_out.as<uint64_t>();
    const int32_t* rows = (const int32_t*)(S.h_vs_out.as<uint8_t>() + key_bytes);
    const int64_t total = (int64_t)keys[kTopK];
    const int64_t max_count = head_rows_unpack(keys, rows, cap, stride, dstride, by_score, out_node, out_score,
                                               out_count, out_evict, out_flags, out_victim);
    head_info_fill(out_info, hp.vp, hp.launches + 1, max_count);
    S.stats.sweeps++;
    return total;
}

// The same decision for one node from the host tables of an encode-only session: the state built on the
// host, then vict_stage / vict_link / vict_decide, the functions the kernel runs.
void debug_victims(Session& S, int pod, int mode, int node, int stride, int32_t* out_count, int32_t* out_evict,
                   uint8_t* out_flags, int32_t* out_victim) {
    const HPod& p = query_task(S, pod, "kbhip_debug_victims: the task ", true, "task id ");
    if (node < 0 || node >= S.n_total) throw Error(KBHIP_EINVAL, "kbhip_debug_victims: node index out of range");
    Framework F(S);
    F.open_plugins();
    Session::VictHost H;  // built per call: kbhip_debug_replay changes the host tables between calls
    vs_build_host(S, H);
    const VictHdr h = make_hdr(S, p, mode);
    const VictState st = H.view(S);
    const int off = st.node_off[node], n = st.node_off[node + 1] - off;
    vector<VictRec> rec(std::max(n, 1));
    for (int k = 0; k < n; ++k) vict_stage(st, h, off + k, rec[k]);
    for (int k = 0; k < n; ++k) vict_link(rec.data(), k);
    std::fill(out_victim, out_victim + stride, -1);
    int32_t evict = 0, flags = 0;
    *out_count = vict_decide(h, rec.data(), n, stride, out_victim, &evict, &flags);
    *out_evict = evict;
    *out_flags = (uint8_t)flags;
}

}  // namespace kbhip

using namespace kbhip;

extern "C" {

int64_t kbhip_head_victims(kb_session* s, int32_t task_id, int32_t by_score, int32_t victims, int32_t cap,
                           int32_t stride, int32_t* out_node, int32_t* out_score, int32_t* out_count,
                           int32_t* out_evict, uint8_t* out_flags, int32_t* out_victim, int64_t* out_info) {
    ABI_GUARD_S(s, {
        check_cap("kbhip_head_victims", cap);
        check_stride("kbhip_head_victims", stride);
        if (!out_node || !out_count || !out_evict || !out_flags || !out_victim)
            throw kbhip::Error(KBHIP_EINVAL,
                               "kbhip_head_victims: null out_node, out_count, out_evict, out_flags or out_victim");
        check_by_score("kbhip_head_victims", by_score);
        check_victims("kbhip_head_victims", victims);
        return kbhip::head_victims_abi(kbhip::device_session(s), task_id, by_score != 0, victims, cap, stride,
                                       out_node, out_score, out_count, out_evict, out_flags, out_victim, out_info);
    })
}

int kbhip_debug_victims(kb_session* s, int32_t task_id, int32_t victims, int32_t node, int32_t stride,
                        int32_t* out_count, int32_t* out_evict, uint8_t* out_flags, int32_t* out_victim) {
    ABI_GUARD({
        if (!s || !out_count || !out_evict || !out_flags || !out_victim)
            throw kbhip::Error(KBHIP_EINVAL, "null argument");
        if (!s->s.encode_only) throw kbhip::Error(KBHIP_EINVAL, "kbhip_debug_victims needs an encode-only session");
        check_stride("kbhip_debug_victims", stride);
        check_victims("kbhip_debug_victims", victims);
        kbhip::debug_victims(s->s, task_id, victims, node, stride, out_count, out_evict, out_flags, out_victim);
        return KBHIP_OK;
    })
}

}  // extern "C"

// kbhip session, part 19: a task's eviction walk over an order ranked once and kept on the device
// (kbhip_walk_begin: kbhip_rank_victim_nodes' full sort and compaction, the keys left in a buffer the
// cursor owns; kbhip_walk_begin_live: for reclaim's order and a class whose predicates read pod-affinity
// targets, the order without that predicate, which kbhip_walk_next then tests per call; kbhip_walk_next: every remaining entry decided side by side in one launch, the serial walk
// from the first one that can act; kbhip_walk_order: the kept order read back; kbhip_walk_end)
#include "framework.h"

namespace kbhip {

namespace {

// The open cursor of a call that reads it; node-sharded sessions never hold one and are refused as such.
void cursor_check(const Session& S, const char* call) {
    if (S.world != 1) throw Error(KBHIP_EUNSUPPORTED, string(call) + " on a node-sharded session");
    if (!S.wc_open)
        throw Error(KBHIP_EINVAL, string(call) + ": no cursor is open (kbhip_walk_begin opens one; a call that "
                                                 "changes pod statuses outside kbhip_apply_ops drops it)");
}

// The class's predicates read pod-affinity targets (existing anti-affinity pairs, the pod's own affinity or
// anti-affinity terms): what an applied eviction can change for a node the cursor has already ranked.
bool reads_affinity_targets(const TaskClass& c) { return c.ea_n > 0 || c.pa_space >= 0 || c.paa_space >= 0; }

}  // namespace

// The ranking of rank_victim_nodes_abi's full path — rank_launch, then launch_vict_compact — with the
// compaction's keys written straight into b_wc_keys (the candidate counts go to the shared scratch and are
// not kept); the count and the sort's two counters come back in one wait.
// live_call (kbhip_walk_begin_live, by_score false): a class that reads affinity targets gets a live cursor —
// launch_live_keys' marks in place of the ranking (node order is the walk order: one launch, no sort), the
// same compaction, and wc_live tells kbhip_walk_next to test the predicate left out; any other class takes
// the path above unchanged.
int64_t walk_begin_abi(Session& S, int pod, bool by_score, int mode, bool live_call, int64_t* out_info) {
    const string api = live_call ? "kbhip_walk_begin_live" : "kbhip_walk_begin";
    const HPod& p = query_task(S, pod, api + ": the task ", true, "task id ");
    query_begin(S, api.c_str());
    const bool reads = reads_affinity_targets(S.classes[p.cls]), live = live_call && reads;
    const int N = S.nc.n;
    const bool rebuilt = vict_ensure(S);
    vector<int32_t> own_node;
    vector<int64_t> own_sum;
    const VictArgs v = vict_args(S, p, mode, own_node, own_sum);
    S.h_vict_out.fit(((size_t)N + 2) * sizeof(int32_t));
    int64_t launches = flush_tables(S);  // evictions / unevicts so far change pod-affinity predicates
    if (live) {
        rank_buffers(S);
        HIPCHK(launch_live_keys(S.conf, S.nc, S.tab, S.classes[p.cls], (uint64_t*)S.b_rank_keys.p,
                                (uint32_t*)S.b_rank_cnt.p, S.stream));
        launches += 1;
    } else {
        launches += rank_launch(S, p.cls, by_score);
    }
    const uint64_t* const ranked = (const uint64_t*)(live ? S.b_rank_keys.p : S.b_rank_sorted.p);
    vict_compact_buffers(S);
    const size_t key_bytes = (size_t)std::max(N, 1) * sizeof(uint64_t);
    S.wc_open = false;  // from here on the kept keys are overwritten: a failure leaves no cursor
    S.b_wc_keys.grow(S.stream, key_bytes, key_bytes);
    S.b_wc_scan.grow(S.stream, 2 * sizeof(uint32_t), 2 * sizeof(uint32_t));
    HIPCHK(launch_vict_compact(ranked, (const uint32_t*)S.b_rank_cnt.p, N, v,
                               (uint32_t*)S.b_vict_blk.p, (uint64_t*)S.b_wc_keys.p, (int32_t*)S.b_vict_cands.p,
                               S.stream));
    HIPCHK(launch_walk_scan_init((uint32_t*)S.b_wc_scan.p, S.stream));
    launches += 3;
    int32_t* const h_out = S.h_vict_out.as<int32_t>();
    uint64_t* const h_rank = S.h_rank.as<uint64_t>();
    HIPCHK(hipMemcpyAsync(h_out, (const uint32_t*)S.b_vict_blk.p + vict_blocks(N), sizeof(uint32_t),
                          hipMemcpyDeviceToHost, S.stream));
    HIPCHK(hipMemcpyAsync(h_rank, S.b_rank_cnt.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));
    if (h_rank[0] >> 32) throw Error(KBHIP_EDEVICE, "walk_begin: node score outside the class score range");
    S.wc_live = live;
    S.wc_total = (int64_t)(uint32_t)h_out[0];
    S.wc_task = pod;
    S.wc_by_score = by_score;
    S.wc_mode = mode;
    S.wc_open = true;
    if (out_info) {
        out_info[0] = launches;
        out_info[1] = rebuilt ? 1 : 0;
        out_info[2] = (int64_t)(S.b_wc_keys.req + S.b_wc_scan.req);
        out_info[3] = live ? 2 : reads ? 1 : 0;
    }
    S.stats.sweeps++;
    return S.wc_total;
}

// Entries [pos, total) of the kept order: the state made current as the other walk calls make it (no
// ranking), k_walk_scan and k_walk_cursor, one copy back, one wait.  Read-only as kbhip_walk_victims is.
int64_t walk_next_abi(Session& S, int64_t pos, int cap, uint8_t* out_op, int32_t* out_pod, int32_t* out_node,
                      int64_t cap_ops, int64_t* out_info) {
    cursor_check(S, "kbhip_walk_next");
    const HPod& p = query_task(S, S.wc_task, "kbhip_walk_next: the cursor's task ", true);
    if (pos < 0 || pos > S.wc_total)
        throw Error(KBHIP_EINVAL, "kbhip_walk_next: pos is 0 .. the total kbhip_walk_begin returned");
    query_begin(S, "kbhip_walk_next");
    const HeadPrep hp = state_prepare(S, p, S.wc_mode);
    const WalkOut o = walk_layout(S, cap_ops, 10, 0);
    struct ScanGuard {  // a call that fails between its launches leaves the scan's words unknown: no cursor
        Session& S;
        bool done = false;
        ~ScanGuard() { if (!done) S.wc_open = false; }
    } scan_guard{S};
    // a live cursor: the class's pod-affinity predicate on the count tables state_prepare just made current
    const WalkLive live{S.conf, S.nc, S.tab, S.classes[p.cls]};
    HIPCHK(launch_walk_cursor(vs_device_view(S), hp.h, (const uint64_t*)S.b_wc_keys.p, pos, S.wc_total, cap,
                              S.wc_task, S.nc.base, vs_lds_recs(S), vs_spill_rows(S), vs_spill_stride(S),
                              walk_ov_jobs(S), walk_ov_queues(S), o.dcap, (uint32_t*)S.b_wc_scan.p, o.info(),
                              o.pods(), o.nodes(), S.stream, S.wc_live ? &live : nullptr));
    int64_t n;
    const int64_t* info = walk_finish(S, o, hp, out_op, out_pod, out_node, out_info, &n);
    scan_guard.done = true;
    if (out_info) {
        for (int k = 0; k < 6; ++k) out_info[k] = info[k];
        out_info[6] = hp.launches + 2;  // the scan and the walk
        out_info[8] = info[8];
        out_info[9] = info[9];
    }
    return n;
}

int64_t walk_order_abi(Session& S, int64_t first, int32_t* out_node, int32_t* out_score, int64_t cap) {
    cursor_check(S, "kbhip_walk_order");
    const int64_t n = first < S.wc_total ? std::min(cap, S.wc_total - first) : 0;
    if (n > 0) {
        uint64_t* const h_keys = S.h_rank.as<uint64_t>() + 1;  // (rank_buffers: room for every node's key)
        HIPCHK(hipMemcpyAsync(h_keys, (const uint64_t*)S.b_wc_keys.p + first, (size_t)n * sizeof(uint64_t),
                              hipMemcpyDeviceToHost, S.stream));
        HIPCHK(hipStreamSynchronize(S.stream));
        for (int64_t i = 0; i < n; ++i) {
            out_node[i] = key_idx(h_keys[i]);
            if (out_score) out_score[i] = S.wc_by_score ? key_score(h_keys[i]) : 0;
        }
    }
    return S.wc_total;
}

}  // namespace kbhip

using namespace kbhip;

extern "C" {

int64_t kbhip_walk_begin(kb_session* s, int32_t task_id, int32_t by_score, int32_t victims, int64_t* out_info) {
    ABI_GUARD_S(s, {
        check_by_score("kbhip_walk_begin", by_score);
        check_victims("kbhip_walk_begin", victims);
        return kbhip::walk_begin_abi(kbhip::device_session(s), task_id, by_score != 0, victims, false, out_info);
    })
}

int64_t kbhip_walk_begin_live(kb_session* s, int32_t task_id, int32_t victims, int64_t* out_info) {
    ABI_GUARD_S(s, {
        check_victims("kbhip_walk_begin_live", victims);
        return kbhip::walk_begin_abi(kbhip::device_session(s), task_id, false, victims, true, out_info);
    })
}

int64_t kbhip_walk_next(kb_session* s, int64_t pos, int32_t cap, uint8_t* out_op, int32_t* out_pod, int32_t* out_node,
                        int64_t cap_ops, int64_t* out_info) {
    ABI_GUARD_S(s, {
        check_cap("kbhip_walk_next", cap);
        check_cap_ops("kbhip_walk_next", cap_ops);
        if (!out_op || !out_pod || !out_node)
            throw kbhip::Error(KBHIP_EINVAL, "kbhip_walk_next: null out_op, out_pod or out_node");
        refuse_unless(pos >= 0, "kbhip_walk_next", ": pos is 0 .. the total kbhip_walk_begin returned");
        return kbhip::walk_next_abi(kbhip::device_session(s), pos, cap, out_op, out_pod, out_node, cap_ops, out_info);
    })
}

int64_t kbhip_walk_order(kb_session* s, int64_t first, int32_t* out_node, int32_t* out_score, int64_t cap) {
    ABI_GUARD_S(s, {
        if (first < 0 || cap < 0 || (cap > 0 && !out_node))
            throw kbhip::Error(KBHIP_EINVAL, "kbhip_walk_order: negative first or cap, or null out_node with cap > 0");
        return kbhip::walk_order_abi(kbhip::device_session(s), first, out_node, out_score, cap);
    })
}

int kbhip_walk_end(kb_session* s) {
    ABI_GUARD_S(s, {
        if (!s) throw kbhip::Error(KBHIP_EINVAL, "null session");
        const bool was = s->s.wc_open;
        s->s.wc_open = false;
        return was ? 1 : 0;
    })
}

}  // extern "C"

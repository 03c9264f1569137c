// kbhip session, part 17: a task's eviction walk — over the head of its pruned walk (kbhip_walk_victims),
// over one window behind a resume point (kbhip_walk_victims_from: the head sweep leaves out the nodes the
// caller's loop has left behind, a pre-pass decides the window's entries side by side, the serial walk starts
// at the first entry that can act), and over a caller's node list on the host (kbhip_debug_walk_victims)
#include "framework.h"

namespace kbhip {

static_assert(KBHIP_WALK_ASSIGNED == kWalkAssigned && KBHIP_WALK_EXHAUSTED == kWalkExhausted &&
                  KBHIP_WALK_HEAD_END == kWalkHeadEnd && KBHIP_WALK_CAPACITY == kWalkCapacity,
              "walk_step's stop reasons");

namespace {

// The key the sweep forms for the resume point (by_score 0: score 0), never 0 for a node index; 0: from the top.
uint64_t resume_key(const Session& S, const char* call, int after_node, int after_score, bool by_score) {
    if (after_node < -1 || after_node >= S.n_total)
        throw Error(KBHIP_EINVAL, string(call) + ": after_node is -1 or a node index");
    return after_node < 0 ? 0 : pack_key(by_score ? after_score : 0, after_node, 0);
}

}  // namespace

// (session.h: what the walk calls share around their kernel)
WalkOut walk_layout(Session& S, int64_t cap_ops, int info_words, size_t extra_bytes) {
    const int64_t most = std::min<int64_t>((int64_t)kTopK * S.vs_max_tasks, S.vs_tasks) + 1,
                  dcap = std::min(cap_ops, most);
    const size_t info_bytes = info_words * sizeof(int64_t), out_bytes = info_bytes + (size_t)dcap * 2 * sizeof(int32_t),
                 all_bytes = out_bytes + extra_bytes;
    S.h_vs_out.fit(out_bytes, std::max<size_t>(out_bytes, 4096));
    S.b_vs_out.grow(S.stream, all_bytes, std::max<size_t>(all_bytes, 4096));
    return WalkOut{dcap, info_bytes, out_bytes, (uint8_t*)S.b_vs_out.p};
}

const int64_t* walk_finish(Session& S, const WalkOut& o, const HeadPrep& hp, uint8_t* out_op, int32_t* out_pod,
                           int32_t* out_node, int64_t* out_info, int64_t* n) {
    HIPCHK(hipMemcpyAsync(S.h_vs_out.p, o.d, o.out_bytes, hipMemcpyDeviceToHost, S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));
    const int64_t* info = S.h_vs_out.as<int64_t>();
    const int32_t* pods = (const int32_t*)(S.h_vs_out.as<uint8_t>() + o.info_bytes);
    *n = std::min(std::max<int64_t>(info[6], 0), o.dcap);
    std::memcpy(out_pod, pods, (size_t)*n * sizeof(int32_t));
    std::memcpy(out_node, pods + o.dcap, (size_t)*n * sizeof(int32_t));
    std::fill(out_op, out_op + *n, (uint8_t)KBHIP_OP_EVICT);
    if (info[0] == KBHIP_WALK_ASSIGNED && *n > 0) out_op[*n - 1] = KBHIP_OP_PIPELINE;
    if (out_info) out_info[7] = (hp.vp.rebuilt ? 1 : 0) | (hp.vp.vs_rebuilt ? 2 : 0) | (hp.vp.patched << 8);
    S.stats.sweeps++;
    return info;
}

// One task's eviction walk over the head (kbhip_walk_victims): kbhip_head_victims' preparation, then
// k_walk_victims on the merged keys — the node loop with the evictions of the earlier nodes carried in an
// overlay inside the launch — one copy back, one wait.  Read-only as kbhip_head_victims is.
int64_t walk_victims_abi(Session& S, int pod, bool by_score, int mode, int cap, int after_node, int after_score,
                         uint8_t* out_op, int32_t* out_pod, int32_t* out_node, int64_t cap_ops, int64_t* out_info) {
    const HPod& p = query_task(S, pod, "kbhip_walk_victims: the task ", true, "task id ");
    const uint64_t after_key = resume_key(S, "kbhip_walk_victims", after_node, after_score, by_score);
    query_begin(S, "kbhip_walk_victims");
    const HeadPrep hp = head_prepare(S, p, by_score, mode);
    const WalkOut o = walk_layout(S, cap_ops, 8, 0);
    HIPCHK(launch_walk_victims(vs_device_view(S), hp.h, (const uint64_t*)S.b_rank_head.p, cap, after_key, pod,
                               S.nc.base, vs_spill_rows(S), vs_spill_stride(S), walk_ov_jobs(S), walk_ov_queues(S),
                               o.dcap, o.info(), o.pods(), o.nodes(), S.stream));
    int64_t n;
    const int64_t* info = walk_finish(S, o, hp, out_op, out_pod, out_node, out_info, &n);
    if (out_info) {
        for (int k = 0; k < 6; ++k) out_info[k] = info[k];
        if (!by_score) out_info[5] = 0;
        out_info[6] = hp.launches + 1;
    }
    return n;
}

// One window behind a resume point (kbhip_walk_victims_from): kbhip_head_victims' preparation with the sweep
// bounded by the resume key, then k_walk_flags and k_walk_victims_from on the merged keys (the pre-pass rows,
// kTopK x 3 int32, behind the output), one copy back, one wait.  Read-only as kbhip_walk_victims is.
int64_t walk_victims_from_abi(Session& S, int pod, bool by_score, int mode, int cap, int after_node, int after_score,
                              uint8_t* out_op, int32_t* out_pod, int32_t* out_node, int64_t cap_ops,
                              int64_t* out_info) {
    const HPod& p = query_task(S, pod, "kbhip_walk_victims_from: the task ", true, "task id ");
    const uint64_t bound = resume_key(S, "kbhip_walk_victims_from", after_node, after_score, by_score);
    query_begin(S, "kbhip_walk_victims_from");
    const HeadPrep hp = head_prepare(S, p, by_score, mode, bound);
    const WalkOut o = walk_layout(S, cap_ops, 10, (size_t)kTopK * 3 * sizeof(int32_t));
    HIPCHK(launch_walk_victims_from(vs_device_view(S), hp.h, (const uint64_t*)S.b_rank_head.p, cap, pod, S.nc.base,
                                    vs_lds_recs(S), vs_spill_rows(S), vs_spill_stride(S), walk_ov_jobs(S),
                                    walk_ov_queues(S), o.dcap, (int32_t*)(o.d + o.out_bytes), o.info(), o.pods(),
                                    o.nodes(), S.stream));
    int64_t n;
    const int64_t* info = walk_finish(S, o, hp, out_op, out_pod, out_node, out_info, &n);
    if (out_info) {
        for (int k = 0; k < 4; ++k) out_info[k] = info[k];
        const bool moved = info[7] >= 0;  // an entry was passed over or acted on: the resume point moves to it
        out_info[4] = moved ? info[4] : after_node;
        out_info[5] = !by_score ? 0 : moved ? info[5] : after_score;
        out_info[6] = hp.launches + 2;  // the pre-pass and the walk
        out_info[8] = info[8];
        out_info[9] = info[9];
    }
    return n;
}

// The same walk over a caller's node list from the host tables of an encode-only session: the state built
// on the host, then per node vict_stage_walk / vict_link / walk_step, the functions the kernel runs.
int64_t debug_walk_victims(Session& S, int pod, int mode, const int32_t* nodes, int n_nodes, int64_t cap_ops,
                           uint8_t* out_op, int32_t* out_pod, int32_t* out_node, int64_t* out_info) {
    const HPod& p = query_task(S, pod, "kbhip_debug_walk_victims: the task ", true, "task id ");
    for (int i = 0; i < n_nodes; ++i)
        if (nodes[i] < 0 || nodes[i] >= S.n_total)
            throw Error(KBHIP_EINVAL, "kbhip_debug_walk_victims: node index out of range");
    Framework F(S);
    F.open_plugins();
    Session::VictHost H;
    vs_build_host(S, H);
    VictHdr h = make_hdr(S, p, mode);
    const VictState st = H.view(S);
    const int64_t dcap = std::min<int64_t>(cap_ops, (int64_t)H.task.size() + 1);
    vector<int32_t> pods((size_t)dcap), onto((size_t)dcap);
    vector<VictRec> rec(std::max(H.max_tasks, 1));
    WalkOverlay ov;
    walk_ov_init(ov, walk_ov_jobs(S), walk_ov_queues(S));
    WalkCtl c{0, dcap, 0, 0, 0, -1, 0, pod};
    for (int i = 0; i < n_nodes && c.stop == 0; ++i) {
        const int off = st.node_off[nodes[i]], n = st.node_off[nodes[i] + 1] - off;
        for (int k = 0; k < n; ++k) vict_stage_walk(st, h, ov, off + k, rec[k]);
        for (int k = 0; k < n; ++k) vict_link(rec.data(), k);
        walk_step(h, ov, c, rec.data(), n, nodes[i], 0, pods.data(), onto.data());
    }
    const int64_t n = c.n_ops;
    std::copy(pods.begin(), pods.begin() + n, out_pod);
    std::copy(onto.begin(), onto.begin() + n, out_node);
    std::fill(out_op, out_op + n, (uint8_t)KBHIP_OP_EVICT);
    if (c.stop == kWalkAssigned) out_op[n - 1] = KBHIP_OP_PIPELINE;
    if (out_info) {
        const int64_t v[8] = {c.stop ? c.stop : kWalkExhausted, n_nodes, c.visited, c.acted, c.last_node, 0, 0, 0};
        std::copy(v, v + 8, out_info);
    }
    return n;
}

}  // namespace kbhip

using namespace kbhip;

extern "C" {

int64_t kbhip_walk_victims(kb_session* s, int32_t task_id, int32_t by_score, int32_t victims, int32_t cap,
                           int32_t after_node, int32_t after_score, uint8_t* out_op, int32_t* out_pod,
                           int32_t* out_node, int64_t cap_ops, int64_t* out_info) {
    ABI_GUARD_S(s, {
        check_cap("kbhip_walk_victims", cap);
        check_cap_ops("kbhip_walk_victims", cap_ops);
        if (!out_op || !out_pod || !out_node)
            throw kbhip::Error(KBHIP_EINVAL, "kbhip_walk_victims: null out_op, out_pod or out_node");
        check_by_score("kbhip_walk_victims", by_score);
        check_victims("kbhip_walk_victims", victims);
        return kbhip::walk_victims_abi(kbhip::device_session(s), task_id, by_score != 0, victims, cap, after_node,
                                       after_score, out_op, out_pod, out_node, cap_ops, out_info);
    })
}

int64_t kbhip_walk_victims_from(kb_session* s, int32_t task_id, int32_t by_score, int32_t victims, int32_t cap,
                                int32_t after_node, int32_t after_score, uint8_t* out_op, int32_t* out_pod,
                                int32_t* out_node, int64_t cap_ops, int64_t* out_info) {
    ABI_GUARD_S(s, {
        check_cap("kbhip_walk_victims_from", cap);
        check_cap_ops("kbhip_walk_victims_from", cap_ops);
        if (!out_op || !out_pod || !out_node)
            throw kbhip::Error(KBHIP_EINVAL, "kbhip_walk_victims_from: null out_op, out_pod or out_node");
        check_by_score("kbhip_walk_victims_from", by_score);
        check_victims("kbhip_walk_victims_from", victims);
        return kbhip::walk_victims_from_abi(kbhip::device_session(s), task_id, by_score != 0, victims, cap,
                                            after_node, after_score, out_op, out_pod, out_node, cap_ops, out_info);
    })
}

int64_t kbhip_debug_walk_victims(kb_session* s, int32_t task_id, int32_t victims, const int32_t* nodes,
                                 int32_t n_nodes, int64_t cap_ops, uint8_t* out_op, int32_t* out_pod,
                                 int32_t* out_node, int64_t* out_info) {
    ABI_GUARD({
        if (!s || !out_op || !out_pod || !out_node || (n_nodes > 0 && !nodes))
            throw kbhip::Error(KBHIP_EINVAL, "null argument");
        if (!s->s.encode_only)
            throw kbhip::Error(KBHIP_EINVAL, "kbhip_debug_walk_victims needs an encode-only session");
        if (n_nodes < 0) throw kbhip::Error(KBHIP_EINVAL, "kbhip_debug_walk_victims: negative n_nodes");
        check_cap_ops("kbhip_debug_walk_victims", cap_ops);
        check_victims("kbhip_debug_walk_victims", victims);
        return kbhip::debug_walk_victims(s->s, task_id, victims, nodes, n_nodes, cap_ops, out_op, out_pod, out_node,
                                         out_info);
    })
}

}  // extern "C"

// kbhip session, part 17: one window of a task's eviction walk behind a resume point
// (kbhip_walk_victims_from) — the walk of kbhip_walk_victims (15_victims.cpp) without the 64-entry head as
// its end: the head sweep leaves out the nodes the caller's loop has left behind, a pre-pass decides the
// window's entries side by side, and the serial walk starts at the first entry that can act.
#include "session.h"

namespace kbhip {

// kbhip_head_victims' preparation with the sweep bounded by the resume key, then k_walk_flags and
// k_walk_victims_from on the merged keys, one copy back, one wait.  Read-only as kbhip_walk_victims is.
int64_t walk_victims_from_abi(Session& S, int pod, bool by_score, int mode, int cap, int after_node, int after_score,
                              uint8_t* out_op, int32_t* out_pod, int32_t* out_node, int64_t cap_ops,
                              int64_t* out_info) {
    const HPod& p = query_task(S, pod, "kbhip_walk_victims_from: the task ", true, "task id ");
    if (after_node < -1 || after_node >= S.n_total)
        throw Error(KBHIP_EINVAL, "kbhip_walk_victims_from: after_node is -1 or a node index");
    query_begin(S, "kbhip_walk_victims_from");
    // the key the sweep forms for the resume point (by_score 0: score 0); never 0 for a node index
    const uint64_t bound = after_node < 0 ? 0 : pack_key(by_score ? after_score : 0, after_node, 0);
    const HeadPrep hp = head_prepare(S, p, by_score, mode, bound);
    // no window writes more ops than the tasks of kTopK nodes (or of the state) and one pipeline
    const int64_t most = std::min<int64_t>((int64_t)kTopK * S.vs_max_tasks, S.vs_tasks) + 1,
                  dcap = std::min(cap_ops, most);
    // device layout: info (10 int64) | pods[dcap] | nodes[dcap] | the pre-pass rows (kTopK x 3 int32, not copied back)
    const size_t info_bytes = 10 * sizeof(int64_t), out_bytes = info_bytes + (size_t)dcap * 2 * sizeof(int32_t),
                 all_bytes = out_bytes + (size_t)kTopK * 3 * sizeof(int32_t);
    S.h_vs_out.fit(out_bytes, std::max<size_t>(out_bytes, 4096));
    S.b_vs_out.grow(S.stream, all_bytes, std::max<size_t>(all_bytes, 4096));
    uint8_t* const d_out = (uint8_t*)S.b_vs_out.p;
    const bool spill = S.vs_max_tasks > kVictLds;
    const int ov = S.walk_ov_max;
    HIPCHK(launch_walk_victims_from(vs_device_view(S), hp.h, (const uint64_t*)S.b_rank_head.p, cap, pod, S.nc.base,
                                    std::min(kVictLds, std::max(S.vs_max_tasks, 1)),
                                    spill ? (VictRec*)S.b_vs_spill.p : nullptr, spill ? S.vs_max_tasks : 0,
                                    ov > 0 ? ov : kWalkOvJobs, ov > 0 ? ov : kWalkOvQueues, dcap,
                                    (int32_t*)(d_out + out_bytes), (int64_t*)d_out, (int32_t*)(d_out + info_bytes),
                                    (int32_t*)(d_out + info_bytes) + dcap, S.stream));
    HIPCHK(hipMemcpyAsync(S.h_vs_out.p, d_out, out_bytes, hipMemcpyDeviceToHost, S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));
    const int64_t* info = S.h_vs_out.as<int64_t>();
    const int32_t* pods = (const int32_t*)(S.h_vs_out.as<uint8_t>() + info_bytes);
    const int64_t n = std::min(std::max<int64_t>(info[6], 0), dcap);
    std::memcpy(out_pod, pods, (size_t)n * sizeof(int32_t));
    std::memcpy(out_node, pods + dcap, (size_t)n * sizeof(int32_t));
    std::fill(out_op, out_op + n, (uint8_t)KBHIP_OP_EVICT);
    if (info[0] == KBHIP_WALK_ASSIGNED && n > 0) out_op[n - 1] = KBHIP_OP_PIPELINE;
    if (out_info) {
        for (int k = 0; k < 4; ++k) out_info[k] = info[k];
        const bool moved = info[7] >= 0;  // an entry was passed over or acted on: the resume point moves to it
        out_info[4] = moved ? info[4] : after_node;
        out_info[5] = !by_score ? 0 : moved ? info[5] : after_score;
        out_info[6] = hp.launches + 2;  // the pre-pass and the walk
        out_info[7] = (hp.rebuilt ? 1 : 0) | (hp.vs_rebuilt ? 2 : 0) | (hp.patched << 8);
        out_info[8] = info[8];
        out_info[9] = info[9];
    }
    S.stats.sweeps++;
    return n;
}

}  // namespace kbhip

using namespace kbhip;

extern "C" {

int64_t kbhip_walk_victims_from(kb_session* s, int32_t task_id, int32_t by_score, int32_t victims, int32_t cap,
                                int32_t after_node, int32_t after_score, uint8_t* out_op, int32_t* out_pod,
                                int32_t* out_node, int64_t cap_ops, int64_t* out_info) {
    ABI_GUARD_S(s, {
        if (cap < 1 || cap > 64) throw kbhip::Error(KBHIP_EINVAL, "kbhip_walk_victims_from: cap is 1 .. 64");
        if (cap_ops < 1) throw kbhip::Error(KBHIP_EINVAL, "kbhip_walk_victims_from: cap_ops is at least 1");
        if (!out_op || !out_pod || !out_node)
            throw kbhip::Error(KBHIP_EINVAL, "kbhip_walk_victims_from: null out_op, out_pod or out_node");
        if (by_score != 0 && by_score != 1)
            throw kbhip::Error(KBHIP_EINVAL, "kbhip_walk_victims_from: by_score is 0 or 1");
        if (victims < KBHIP_VICTIMS_OTHER_QUEUES || victims > KBHIP_VICTIMS_SAME_JOB)
            throw kbhip::Error(KBHIP_EINVAL, "kbhip_walk_victims_from: victims is one of KBHIP_VICTIMS_* (1..3)");
        return kbhip::walk_victims_from_abi(kbhip::device_session(s), task_id, by_score != 0, victims, cap,
                                            after_node, after_score, out_op, out_pod, out_node, cap_ops, out_info);
    })
}

}  // extern "C"

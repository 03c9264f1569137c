// kbhip session, part 18: the victim state the victim queries read (VictState, kbhip_internal.h) — built
// from the host model, uploaded, patched from the dirty lists kbhip_apply_ops leaves — and kbhip_debug_table's
// views of the plugin state behind it
#include "framework.h"

namespace kbhip {

namespace {

constexpr size_t kVsMaxBytes = (size_t)512 << 20;  // the state's design limit (include/kbhip.h)

int32_t task_flags(const Session& S, const HPod& p) {
    return (vict_candidate(S, p) ? kVictRunCopy : 0) | (p.critical ? kVictCritical : 0);
}
VictJob job_record(const Session& S, int jb) {  // readyTaskNum (gang.go:212-222) and drf's allocation
    const HJob& j = S.jobs[jb];
    int c = 0;
    for (int t : j.tasks) c += Framework::gang_ready_status(S.pods[t].status);
    return VictJob{{j.drf_alloc.c, j.drf_alloc.m, j.drf_alloc.g}, c, 0};
}
VictQueue queue_record(const Session& S, int q) {
    const HQueue& Q = S.queues[q];
    return VictQueue{{Q.allocated.c, Q.allocated.m, Q.allocated.g}, {Q.deserved.c, Q.deserved.m, Q.deserved.g}};
}
size_t vs_bytes_of(const Session::VictHost& H) {
    return H.node_off.size() * sizeof(int32_t) + H.task.size() * sizeof(VictTask) + H.job.size() * sizeof(VictJob) +
           H.queue.size() * sizeof(VictQueue);
}
size_t align8(size_t x) { return (x + 7) & ~(size_t)7; }
void sort_unique(vector<int32_t>& v) {
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
}

}  // namespace

// The state from the host model (plugins opened): two passes over the pods by pod ranges in parallel, as
// EvictAction::build_node_tasks — per range the candidates per node, then each node's row sized and the
// ranges' records written at their offsets (pod order within a node kept) — and the jobs by job ranges.
void vs_build_host(const Session& S, Session::VictHost& H) {
    const int N = S.n_total, P = (int)S.pods.size(), J = (int)S.jobs.size(), Q = (int)S.queues.size();
    const int nth = P < (1 << 16) ? 1 : host_threads();
    vector<vector<int32_t>> cnt(nth, vector<int32_t>(N, 0));
    run_ranges(nth, [&](int r) {
        const auto [b, e] = range_of(P, r, nth);
        int32_t* c = cnt[r].data();
        for (int i = b; i < e; ++i)
            if (vict_candidate(S, S.pods[i])) c[S.pods[i].node]++;
    });
    H.node_off.assign((size_t)N + 1, 0);
    int64_t run = 0;
    H.max_tasks = 0;
    for (int n = 0; n < N; ++n) {
        const int64_t at = run;
        for (int r = 0; r < nth; ++r) { const int32_t k = cnt[r][n]; cnt[r][n] = (int32_t)run; run += k; }
        if (run > INT32_MAX) throw Error(KBHIP_EUNSUPPORTED, "kbhip_head_victims: more than 2^31 - 1 candidate tasks");
        H.node_off[n + 1] = (int32_t)run;
        H.max_tasks = std::max<int32_t>(H.max_tasks, (int32_t)(run - at));
    }
    H.task.assign((size_t)run, VictTask{});
    H.pos.assign(P, -1);
    run_ranges(nth, [&](int r) {
        const auto [b, e] = range_of(P, r, nth);
        int32_t* c = cnt[r].data();
        for (int i = b; i < e; ++i) {
            const HPod& p = S.pods[i];
            if (!vict_candidate(S, p)) continue;
            const HJob& j = S.jobs[p.job];
            const int32_t at = c[p.node]++;
            H.task[at] = VictTask{i, p.job, j.queue, j.min_avail, {p.req.c, p.req.m, p.req.g}, task_flags(S, p), 0};
            H.pos[i] = at;
        }
    });
    H.job.resize(J);
    const int jth = P < (1 << 16) ? 1 : host_threads();
    run_ranges(jth, [&](int r) {
        const auto [b, e] = range_of(J, r, jth);
        for (int jb = b; jb < e; ++jb) H.job[jb] = job_record(S, jb);
    });
    H.queue.resize(Q);
    for (int q = 0; q < Q; ++q) H.queue[q] = queue_record(S, q);
}

VictState vs_device_view(const Session& S) {
    return VictState{(const int32_t*)S.b_vs_off.p, (const VictTask*)S.b_vs_task.p, (const VictJob*)S.b_vs_job.p,
                     (const VictQueue*)S.b_vs_queue.p, S.n_total, (int32_t)S.jobs.size(), (int32_t)S.queues.size(),
                     S.vs_tasks};
}

void vs_spill_check(const Session& S, int32_t max_tasks, int rows) {
    if (max_tasks <= kVictLds) return;
    const size_t bytes = (size_t)rows * max_tasks * sizeof(VictRec);
    if (bytes > (size_t)S.vs_spill_max)
        throw Error(KBHIP_EUNSUPPORTED, "kbhip_heads_victims: the " + std::to_string(rows) +
                                            " staging rows of one task for nodes of up to " +
                                            std::to_string(max_tasks) + " tasks take " + std::to_string(bytes) +
                                            " bytes, above victims_spill_max (" + std::to_string(S.vs_spill_max) +
                                            " bytes)");
}

// The state built and uploaded (the pageable sources are read when this returns).  batch_rows > 0:
// vs_spill_check before the upload.
void vs_build(Session& S, int batch_rows) {
    const auto t0 = Clock::now();
    Session::VictHost H;
    vs_build_host(S, H);
    const size_t bytes = vs_bytes_of(H);
    if (bytes > kVsMaxBytes)
        throw Error(KBHIP_EUNSUPPORTED, "kbhip_head_victims: the victim state of " + std::to_string(H.task.size()) +
                                            " candidate tasks, " + std::to_string(H.job.size()) + " jobs and " +
                                            std::to_string(H.queue.size()) + " queues takes " +
                                            std::to_string(bytes >> 20) + " MB, above the 512 MB limit");
    if (batch_rows > 0) vs_spill_check(S, H.max_tasks, batch_rows);
    // (every earlier call that read these buffers ended with a wait; a buffer that has to grow drains the stream)
    auto up = [&](DevBuf& b, const void* src, size_t n) {
        b.grow(S.stream, std::max<size_t>(n, 16), std::max<size_t>(n + n / 8, 4096));
        if (n) HIPCHK(hipMemcpyAsync(b.p, src, n, hipMemcpyHostToDevice, S.stream));
    };
    up(S.b_vs_off, H.node_off.data(), H.node_off.size() * sizeof(int32_t));
    up(S.b_vs_task, H.task.data(), H.task.size() * sizeof(VictTask));
    up(S.b_vs_job, H.job.data(), H.job.size() * sizeof(VictJob));
    up(S.b_vs_queue, H.queue.data(), H.queue.size() * sizeof(VictQueue));
    if (H.max_tasks > kVictLds)
        S.b_vs_spill.grow(S.stream, (size_t)kTopK * H.max_tasks * sizeof(VictRec),
                          (size_t)kTopK * H.max_tasks * sizeof(VictRec));
    HIPCHK(hipStreamSynchronize(S.stream));
    S.vs_pos = std::move(H.pos);
    S.vs_tasks = (int32_t)H.task.size();
    S.vs_max_tasks = H.max_tasks;
    S.vs_bytes = (int64_t)bytes;
    S.vs_dirty_pod.clear();
    S.vs_dirty_job.clear();
    S.vs_dirty_queue.clear();
    S.vs_live = true;
    S.vs_build_s = seconds_since(t0);
}

// The dirty records of the kbhip_apply_ops batches since the last call, uploaded compactly (pinned
// staging: the previous call ended with a wait) and scattered by one launch.  Returns the records patched.
int64_t vs_patch(Session& S) {
    sort_unique(S.vs_dirty_pod);
    sort_unique(S.vs_dirty_job);
    sort_unique(S.vs_dirty_queue);
    vector<int32_t> pos, flags;
    for (int32_t pi : S.vs_dirty_pod) {
        const int32_t at = pi >= 0 && pi < (int32_t)S.vs_pos.size() ? S.vs_pos[pi] : -1;
        if (at < 0) continue;  // (a pipelined task: never a candidate)
        pos.push_back(at);
        flags.push_back(task_flags(S, S.pods[pi]));
    }
    const size_t nt = pos.size(), nj = S.vs_dirty_job.size(), nq = S.vs_dirty_queue.size();
    S.vs_dirty_pod.clear();
    if (nt + nj + nq == 0) return 0;
    // staging layout (8-byte aligned parts): t_pos[nt] | t_flags[nt] | j_id[nj] | q_id[nq] | j_rec[nj] | q_rec[nq]
    const size_t o_pos = 0, o_fl = o_pos + align8(nt * 4), o_jid = o_fl + align8(nt * 4), o_qid = o_jid + align8(nj * 4),
                 o_jrec = o_qid + align8(nq * 4), o_qrec = o_jrec + nj * sizeof(VictJob),
                 bytes = o_qrec + nq * sizeof(VictQueue);
    S.h_vs_patch.fit(bytes, std::max<size_t>(2 * bytes, 4096));
    S.b_vs_patch.grow(S.stream, bytes, std::max<size_t>(2 * bytes, 4096));
    uint8_t* const h = S.h_vs_patch.as<uint8_t>();
    if (nt) { std::memcpy(h + o_pos, pos.data(), nt * 4); std::memcpy(h + o_fl, flags.data(), nt * 4); }
    for (size_t i = 0; i < nj; ++i) {
        ((int32_t*)(h + o_jid))[i] = S.vs_dirty_job[i];
        ((VictJob*)(h + o_jrec))[i] = job_record(S, S.vs_dirty_job[i]);
    }
    for (size_t i = 0; i < nq; ++i) {
        ((int32_t*)(h + o_qid))[i] = S.vs_dirty_queue[i];
        ((VictQueue*)(h + o_qrec))[i] = queue_record(S, S.vs_dirty_queue[i]);
    }
    S.vs_dirty_job.clear();
    S.vs_dirty_queue.clear();
    const uint8_t* d = (const uint8_t*)S.b_vs_patch.p;
    HIPCHK(hipMemcpyAsync(S.b_vs_patch.p, h, bytes, hipMemcpyHostToDevice, S.stream));
    const VictPatch p{(const int32_t*)(d + o_pos), (const int32_t*)(d + o_fl), (const int32_t*)(d + o_jid),
                      (const VictJob*)(d + o_jrec), (const int32_t*)(d + o_qid), (const VictQueue*)(d + o_qrec),
                      (int32_t)nt, (int32_t)nj, (int32_t)nq};
    HIPCHK(launch_victims_patch(vs_device_view(S), p, S.stream));
    return (int64_t)(nt + nj + nq);
}

void vs_mark_dirty(Session& S, const int32_t* pod, int64_t n) {
    if (!S.vs_live) return;
    if ((int64_t)S.vs_dirty_pod.size() + n > S.vs_dirty_max) {  // cheaper rebuilt than patched
        S.vs_live = false;
        S.vs_dirty_pod.clear();
        S.vs_dirty_job.clear();
        S.vs_dirty_queue.clear();
        return;
    }
    for (int64_t i = 0; i < n; ++i) {
        const HPod& p = S.pods[pod[i]];
        S.vs_dirty_pod.push_back(pod[i]);
        if (p.job < 0) continue;
        S.vs_dirty_job.push_back(p.job);
        if (S.jobs[p.job].queue >= 0) S.vs_dirty_queue.push_back(S.jobs[p.job].queue);
    }
}

// kbhip_debug_table's views of the plugin state the victim functions read (drf / proportion opened first)
bool debug_victim_table(Session& S, const string& name, vector<uint8_t>& out) {
    auto put = [&out](const auto* src, size_t n) {
        out.resize(n * sizeof(*src));
        if (n) std::memcpy(out.data(), src, out.size());
    };
    if (name == "pod_job" || name == "pod_queue") {
        vector<int32_t> v(S.pods.size(), -1);
        for (size_t i = 0; i < v.size(); ++i) {
            const int jb = S.pods[i].job;
            v[i] = name == "pod_job" ? jb : (jb >= 0 ? S.jobs[jb].queue : -1);
        }
        put(v.data(), v.size());
        return true;
    }
    if (name == "victim_state") {  // the last build: bytes uploaded, host microseconds, CSR length, longest node
        const int64_t v[4] = {S.vs_bytes, (int64_t)(S.vs_build_s * 1e6), S.vs_tasks, S.vs_max_tasks};
        put(v, 4);
        return true;
    }
    if (name != "job_ready" && name != "job_drf_alloc" && name != "queue_allocated" && name != "queue_deserved")
        return false;
    Framework F(S);
    F.open_plugins();
    if (name == "job_ready") {
        vector<int32_t> v(S.jobs.size());
        for (size_t j = 0; j < v.size(); ++j) v[j] = job_record(S, (int)j).ready;
        put(v.data(), v.size());
        return true;
    }
    vector<double> v;
    if (name == "job_drf_alloc")
        for (const HJob& j : S.jobs) v.insert(v.end(), {j.drf_alloc.c, j.drf_alloc.m, j.drf_alloc.g});
    else
        for (const HQueue& q : S.queues) {
            const F3& f = name == "queue_allocated" ? q.allocated : q.deserved;
            v.insert(v.end(), {f.c, f.m, f.g});
        }
    put(v.data(), v.size());
    return true;
}

}  // namespace kbhip

// kbhip session, part 15: the victim sets of a walk's head nodes (kbhip_head_victims), the victim state they
// are read from, one task's whole eviction walk over that head (kbhip_walk_victims), and the same decisions
// on the host tables (kbhip_debug_victims, kbhip_debug_walk_victims)
#include "framework.h"

namespace kbhip {

static_assert(KBHIP_HEAD_VICTIMS_VALID == 1 && KBHIP_HEAD_VICTIMS_COVERS == 2, "vict_decide's flag bits");
static_assert(KBHIP_WALK_ASSIGNED == kWalkAssigned && KBHIP_WALK_EXHAUSTED == kWalkExhausted &&
                  KBHIP_WALK_HEAD_END == kWalkHeadEnd && KBHIP_WALK_CAPACITY == kWalkCapacity,
              "walk_step's stop reasons");

struct Session::VictHost {  // the victim state on the host (VictState, kbhip_internal.h)
    vector<int32_t> node_off, pos;
    vector<VictTask> task;
    vector<VictJob> job;
    vector<VictQueue> queue;
    int32_t max_tasks = 0;
    VictState view(const Session& S) const {
        return VictState{node_off.data(), task.data(), job.data(), queue.data(), S.n_total, (int32_t)job.size(),
                         (int32_t)queue.size(), (int32_t)task.size()};
    }
};

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

size_t vs_bytes_of(const Session::VictHost& H) {
    return H.node_off.size() * sizeof(int32_t) + H.task.size() * sizeof(VictTask) + H.job.size() * sizeof(VictJob) +
           H.queue.size() * sizeof(VictQueue);
}

}  // namespace

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

namespace {

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

size_t align8(size_t x) { return (x + 7) & ~(size_t)7; }

void sort_unique(vector<int32_t>& v) {
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
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

}  // namespace

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

// What kbhip_head_victims, kbhip_walk_victims and kbhip_walk_victims_from do before their own kernel: the
// plugins opened, the call's header, both tables made current and the head sweep and merge of
// kbhip_rank_victim_nodes enqueued — b_rank_head holds the head in stream order (bound != 0: the head
// among the nodes whose key is below it).
HeadPrep head_prepare(Session& S, const HPod& p, bool by_score, int mode, uint64_t bound) {
    Framework F(S);
    F.open_plugins();  // drf / proportion as OnSessionOpen leaves them (kbhip_apply_ops opens them the same way)
    const VictHdr h = make_hdr(S, p, mode);
    const VictPrep vp = vict_prepare(S, 0);
    int64_t launches = vp.launches;
    vector<int32_t> own_node;
    vector<int64_t> own_sum;
    const VictArgs v = vict_args(S, p, mode, own_node, own_sum);
    launches += rank_head_enqueue(S, p.cls, by_score, &v, bound);
    return HeadPrep{h, vp.rebuilt, vp.vs_rebuilt, vp.patched, launches};
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
    const VictHdr& h = hp.h;
    const bool rebuilt = hp.rebuilt, vs_rebuilt = hp.vs_rebuilt;
    const int64_t patched = hp.patched;
    int64_t launches = hp.launches;
    // the rows hold at most the longest node's tasks; a larger stride is filled with -1 here
    const int dstride = std::max(1, std::min(stride, S.vs_max_tasks));
    const size_t key_bytes = (size_t)(kTopK + 1) * sizeof(uint64_t),
                 out_bytes = key_bytes + (size_t)cap * (3 + (size_t)dstride) * sizeof(int32_t);
    S.h_vs_out.fit(out_bytes, std::max<size_t>(out_bytes, 4096));
    S.b_vs_out.grow(S.stream, out_bytes, std::max<size_t>(out_bytes, 4096));
    uint8_t* const d_out = (uint8_t*)S.b_vs_out.p;
    HIPCHK(launch_head_victims(vs_device_view(S), h, (const uint64_t*)S.b_rank_head.p, cap, dstride, S.nc.base,
                               S.vs_max_tasks > kVictLds ? (VictRec*)S.b_vs_spill.p : nullptr,
                               S.vs_max_tasks > kVictLds ? S.vs_max_tasks : 0, (uint64_t*)d_out,
                               (int32_t*)(d_out + key_bytes), S.stream));
    launches += 1;
    HIPCHK(hipMemcpyAsync(S.h_vs_out.p, d_out, out_bytes, hipMemcpyDeviceToHost, S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));
    const uint64_t* keys = S.h_vs_out.as<uint64_t>();
    const int32_t* rows = (const int32_t*)(S.h_vs_out.as<uint8_t>() + key_bytes);
    const int64_t total = (int64_t)keys[kTopK];
    const int64_t max_count = head_rows_unpack(keys, rows, cap, stride, dstride, by_score, out_node, out_score,
                                               out_count, out_evict, out_flags, out_victim);
    if (out_info) {
        out_info[0] = rebuilt ? 1 : 0;
        out_info[1] = vs_rebuilt ? 1 : 0;
        out_info[2] = patched;
        out_info[3] = launches;
        out_info[4] = max_count;
    }
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

// One task's eviction walk over the head (kbhip_walk_victims): kbhip_head_victims' preparation, then
// k_walk_victims on the merged keys — the node loop with the evictions of the earlier nodes carried in an
// overlay inside the launch — one copy back, one wait.  Read-only as kbhip_head_victims is.
int64_t walk_victims_abi(Session& S, int pod, bool by_score, int mode, int cap, int after_node, int after_score,
                         uint8_t* out_op, int32_t* out_pod, int32_t* out_node, int64_t cap_ops, int64_t* out_info) {
    const HPod& p = query_task(S, pod, "kbhip_walk_victims: the task ", true, "task id ");
    if (after_node < -1 || after_node >= S.n_total)
        throw Error(KBHIP_EINVAL, "kbhip_walk_victims: after_node is -1 or a node index");
    query_begin(S, "kbhip_walk_victims");
    const HeadPrep hp = head_prepare(S, p, by_score, mode);
    // no walk writes more ops than the tasks of kTopK nodes (or of the state) and one pipeline
    const int64_t most = std::min<int64_t>((int64_t)kTopK * S.vs_max_tasks, S.vs_tasks) + 1,
                  dcap = std::min(cap_ops, most);
    const size_t info_bytes = 8 * sizeof(int64_t), out_bytes = info_bytes + (size_t)dcap * 2 * sizeof(int32_t);
    S.h_vs_out.fit(out_bytes, std::max<size_t>(out_bytes, 4096));
    S.b_vs_out.grow(S.stream, out_bytes, std::max<size_t>(out_bytes, 4096));
    uint8_t* const d_out = (uint8_t*)S.b_vs_out.p;
    const uint64_t after_key = after_node < 0 ? 0 : pack_key(by_score ? after_score : 0, after_node, 0);
    const bool spill = S.vs_max_tasks > kVictLds;
    const int ov = S.walk_ov_max;
    HIPCHK(launch_walk_victims(vs_device_view(S), hp.h, (const uint64_t*)S.b_rank_head.p, cap, after_key, pod,
                               S.nc.base, spill ? (VictRec*)S.b_vs_spill.p : nullptr, spill ? S.vs_max_tasks : 0,
                               ov > 0 ? ov : kWalkOvJobs, ov > 0 ? ov : kWalkOvQueues, dcap, (int64_t*)d_out,
                               (int32_t*)(d_out + info_bytes), (int32_t*)(d_out + info_bytes) + dcap, S.stream));
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
        for (int k = 0; k < 6; ++k) out_info[k] = info[k];
        if (!by_score) out_info[5] = 0;
        out_info[6] = hp.launches + 1;
        out_info[7] = (hp.rebuilt ? 1 : 0) | (hp.vs_rebuilt ? 2 : 0) | (hp.patched << 8);
    }
    S.stats.sweeps++;
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
    const int ovm = S.walk_ov_max;
    walk_ov_init(ov, ovm > 0 ? ovm : kWalkOvJobs, ovm > 0 ? ovm : kWalkOvQueues);
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

using namespace kbhip;

extern "C" {

int64_t kbhip_head_victims(kb_session* s, int32_t task_id, int32_t by_score, int32_t victims, int32_t cap,
                           int32_t stride, int32_t* out_node, int32_t* out_score, int32_t* out_count,
                           int32_t* out_evict, uint8_t* out_flags, int32_t* out_victim, int64_t* out_info) {
    ABI_GUARD_S(s, {
        if (cap < 1 || cap > 64) throw kbhip::Error(KBHIP_EINVAL, "kbhip_head_victims: cap is 1 .. 64");
        if (stride < 1) throw kbhip::Error(KBHIP_EINVAL, "kbhip_head_victims: stride is at least 1");
        if (!out_node || !out_count || !out_evict || !out_flags || !out_victim)
            throw kbhip::Error(KBHIP_EINVAL,
                               "kbhip_head_victims: null out_node, out_count, out_evict, out_flags or out_victim");
        if (by_score != 0 && by_score != 1) throw kbhip::Error(KBHIP_EINVAL, "kbhip_head_victims: by_score is 0 or 1");
        if (victims < KBHIP_VICTIMS_OTHER_QUEUES || victims > KBHIP_VICTIMS_SAME_JOB)
            throw kbhip::Error(KBHIP_EINVAL, "kbhip_head_victims: victims is one of KBHIP_VICTIMS_* (1..3)");
        return kbhip::head_victims_abi(kbhip::device_session(s), task_id, by_score != 0, victims, cap, stride,
                                       out_node, out_score, out_count, out_evict, out_flags, out_victim, out_info);
    })
}

int64_t kbhip_walk_victims(kb_session* s, int32_t task_id, int32_t by_score, int32_t victims, int32_t cap,
                           int32_t after_node, int32_t after_score, uint8_t* out_op, int32_t* out_pod,
                           int32_t* out_node, int64_t cap_ops, int64_t* out_info) {
    ABI_GUARD_S(s, {
        if (cap < 1 || cap > 64) throw kbhip::Error(KBHIP_EINVAL, "kbhip_walk_victims: cap is 1 .. 64");
        if (cap_ops < 1) throw kbhip::Error(KBHIP_EINVAL, "kbhip_walk_victims: cap_ops is at least 1");
        if (!out_op || !out_pod || !out_node)
            throw kbhip::Error(KBHIP_EINVAL, "kbhip_walk_victims: null out_op, out_pod or out_node");
        if (by_score != 0 && by_score != 1) throw kbhip::Error(KBHIP_EINVAL, "kbhip_walk_victims: by_score is 0 or 1");
        if (victims < KBHIP_VICTIMS_OTHER_QUEUES || victims > KBHIP_VICTIMS_SAME_JOB)
            throw kbhip::Error(KBHIP_EINVAL, "kbhip_walk_victims: victims is one of KBHIP_VICTIMS_* (1..3)");
        return kbhip::walk_victims_abi(kbhip::device_session(s), task_id, by_score != 0, victims, cap, after_node,
                                       after_score, out_op, out_pod, out_node, cap_ops, out_info);
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
        if (cap_ops < 1) throw kbhip::Error(KBHIP_EINVAL, "kbhip_debug_walk_victims: cap_ops is at least 1");
        if (victims < KBHIP_VICTIMS_OTHER_QUEUES || victims > KBHIP_VICTIMS_SAME_JOB)
            throw kbhip::Error(KBHIP_EINVAL, "kbhip_debug_walk_victims: victims is one of KBHIP_VICTIMS_* (1..3)");
        return kbhip::debug_walk_victims(s->s, task_id, victims, nodes, n_nodes, cap_ops, out_op, out_pod, out_node,
                                         out_info);
    })
}

int kbhip_debug_victims(kb_session* s, int32_t task_id, int32_t victims, int32_t node, int32_t stride,
                        int32_t* out_count, int32_t* out_evict, uint8_t* out_flags, int32_t* out_victim) {
    ABI_GUARD({
        if (!s || !out_count || !out_evict || !out_flags || !out_victim)
            throw kbhip::Error(KBHIP_EINVAL, "null argument");
        if (!s->s.encode_only) throw kbhip::Error(KBHIP_EINVAL, "kbhip_debug_victims needs an encode-only session");
        if (stride < 1) throw kbhip::Error(KBHIP_EINVAL, "kbhip_debug_victims: stride is at least 1");
        if (victims < KBHIP_VICTIMS_OTHER_QUEUES || victims > KBHIP_VICTIMS_SAME_JOB)
            throw kbhip::Error(KBHIP_EINVAL, "kbhip_debug_victims: victims is one of KBHIP_VICTIMS_* (1..3)");
        kbhip::debug_victims(s->s, task_id, victims, node, stride, out_count, out_evict, out_flags, out_victim);
        return KBHIP_OK;
    })
}

}  // extern "C"

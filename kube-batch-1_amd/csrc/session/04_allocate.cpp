// kbhip session, part 04: the allocate action on the framework model (framework.h), and first_fit
#include "framework.h"

namespace kbhip {

using QueueHeap = GoHeap<QueueLess>;
using JobQueues = std::map<int, JobQueue<JobLess>>;  // per queue, in queue order

// A job's pending tasks as allocate.go:91-104 queues them (BestEffort ones left out), in
// TaskOrderFn order (a strict total order), built on the job's first pop.
static void build_pending(const Framework& F, HJob& job) {
    if (job.pending_built) return;
    Session& S = F.S;
    for (int t : job.tasks) {
        const HPod& p = S.pods[t];
        if (p.status != Pending) continue;
        if (p.req.c < kMinCPU && p.req.m < kMinMem && p.req.g < kMinGPU) continue;  // BestEffort
        job.pending.push_back(t);
    }
    std::sort(job.pending.begin(), job.pending.end(), [&F](int a, int b) { return F.task_less(a, b); });
    job.pending_built = true;
}

// Speculation: while a batched pop runs, the host predicts
// the next pops — assuming each places its tasks as Allocated up to the gang
// stop — by running the allocate loop on its own state with every change
// undone afterwards (heap operations through a journal, job / queue fields
// saved), and queues those pops' launches behind the running one.  The next
// real pop uses the oldest queued launch only if it is exactly that pop (job,
// first task, ready count, class, chunk), in which case the launch ran on
// exactly the device state the real pop sees; otherwise every queued launch is
// retracted (k_undo_pop) before anything else runs.
struct Speculation {
    Session& S;
    Framework& F;
    QueueHeap& queues;
    JobQueues& jobs_map;
    Speculation(Framework& f, QueueHeap& q, JobQueues& j) : S(f.S), F(f), queues(q), jobs_map(j) {}

    struct Pop {  // what tells one batched pop from another
        int jb = -1, cls = -1, m = 0, ready = 0;
        size_t cur = 0;
        bool operator==(const Pop& o) const {
            return jb == o.jb && cur == o.cur && ready == o.ready && cls == o.cls && m == o.m;
        }
    };
    struct Spec {  // a launched prediction
        BatchLaunch L;
        Pop pop;
    };
    struct Pred {  // a predicted pop: its queue and the job's remaining tasks with it
        Pop pop;
        int q = -1, n = 0;
    };
    struct JobSave {
        int jb, cnt;
        size_t cur;
        F3 drf;
        double share;
    };
    struct QueueSave {
        int q;
        F3 alloc;
        double share;
    };
    std::deque<Spec> specs;  // launched predictions, oldest first
    HeapJournal journal;
    vector<JobSave> job_saves;
    vector<QueueSave> queue_saves;
    static constexpr int kPredictSkip = 64;

    // the heaps are built: from here their operations can be journalled
    void attach() {
        queues.jr = &journal;
        for (auto& kv : jobs_map) kv.second.set_journal(&journal);
    }
    // The oldest queued launch if it is exactly this pop; any other queued launch means the
    // predictions failed, and all are retracted.
    bool take(const Pop& pop, BatchLaunch* L) {
        if (specs.empty()) return false;
        if (!(specs.front().pop == pop)) {
            discard_all();
            return false;
        }
        *L = specs.front().L;
        specs.pop_front();
        S.stats.spec_hits++;
        return true;
    }
    void discard_all() {
        if (specs.empty()) return;
        vector<int32_t> node(specs.size() * kMaxChunk), kind(specs.size() * kMaxChunk);
        vector<int> nd(specs.size());
        for (size_t i = 0; i < specs.size(); ++i) {
            int st = 0;
            collect_batched(S, specs[i].L, &nd[i], &st, node.data() + i * kMaxChunk, kind.data() + i * kMaxChunk);
        }
        ov_quiesce(S);
        for (size_t i = 0; i < specs.size(); ++i) {  // inverse updates commute
            HIPCHK(launch_undo_pop(S.nc, S.tab, specs[i].L.cls, nd[i], node.data() + i * kMaxChunk,
                                   kind.data() + i * kMaxChunk, S.stream));
            S.stats.spec_missed++;
        }
        if (S.overlap > 0) HIPCHK(hipStreamSynchronize(S.stream));  // overlapped pops are not ordered after it
        specs.clear();
    }
    // The predicted outcome of pop (q, jb) whose first chunk of m of its n
    // remaining tasks runs: k tasks Allocated, then the stop; -1 if the pop
    // would continue past this chunk.  Saves what it changes.
    int apply_outcome(int q, int jb, int m, int n) {
        HJob& job = S.jobs[jb];
        int k, pstop;
        if (S.gang_ready) {  // gang.go:63-66: stop once #AllocatedStatuses >= MinAvailable
            const int need = job.min_avail - job.cnt_alloc;
            k = need <= 1 ? 1 : need;
            if (k <= m) pstop = KBHIP_STOP_READY;
            else if (m == n) { k = m; pstop = KBHIP_STOP_ALL; }
            else return -1;
        } else {
            k = 1;  // no JobReadyFn: always ready, one task per pop
            pstop = KBHIP_STOP_READY;
        }
        HQueue& Q = S.queues[q];
        job_saves.push_back({jb, job.cnt_alloc, job.cursor, job.drf_alloc, job.drf_share});
        queue_saves.push_back({q, Q.allocated, Q.share});
        for (int i = 0; i < k; ++i) {
            const HPod& p = S.pods[job.pending[job.cursor + i]];
            if (S.drf_on) job.drf_alloc.add(p.req);
            if (S.prop_on) Q.allocated.add(p.req);
        }
        job.cnt_alloc += k;
        job.cursor += k;
        if (S.drf_on) F.drf_update(job);
        if (S.prop_on) F.prop_update(Q);
        return pstop;
    }
    void restore_saves() {
        for (auto it = job_saves.rbegin(); it != job_saves.rend(); ++it) {
            HJob& j = S.jobs[it->jb];
            j.cnt_alloc = it->cnt;
            j.cursor = it->cur;
            j.drf_alloc = it->drf;
            j.drf_share = it->share;
        }
        for (auto it = queue_saves.rbegin(); it != queue_saves.rend(); ++it) {
            HQueue& Q = S.queues[it->q];
            Q.allocated = it->alloc;
            Q.share = it->share;
        }
        job_saves.clear();
        queue_saves.clear();
    }
    // The loop's next pop after pop (q, jb) stopped with pstop (heaps
    // changed through the journal); false when it is not a batched pop.
    // The loop's steps that place nothing (an overused queue or one without
    // jobs is dropped, a job without pending tasks is dropped and its queue
    // pushed back) are followed, up to kPredictSkip of them.
    bool next_pop(int q, int jb, int pstop, Pred* P) {
        if (pstop == KBHIP_STOP_READY) jobs_map.at(q).push(jb);
        queues.push(q);
        for (int skip = 0; skip <= kPredictSkip && !queues.empty(); ++skip) {
            const int q2 = queues.pop();
            if (F.overused(q2)) continue;
            auto jit2 = jobs_map.find(q2);
            if (jit2 == jobs_map.end() || jit2->second.empty()) continue;
            const int jb2 = jit2->second.pop();
            HJob& j2 = S.jobs[jb2];
            build_pending(F, j2);
            const size_t cur2 = j2.cursor;
            if (cur2 >= j2.pending.size()) {  // an empty pop
                queues.push(q2);
                continue;
            }
            const int cls2 = S.pods[j2.pending[cur2]].cls;
            const size_t rem = j2.pending.size() - cur2;
            int m2 = 0;
            while ((size_t)m2 < rem && m2 < kMaxChunk && S.pods[j2.pending[cur2 + m2]].cls == cls2) ++m2;
            if (!batchable(S, cls2)) return false;
            *P = Pred{Pop{jb2, cls2, m2, j2.cnt_alloc, cur2}, q2, (int)rem};
            return true;
        }
        return false;
    }
    // Keep up to S.speculate predicted pops queued behind pop (q, jb).
    void speculate(int q, int jb, int m, int n) {
        Pred p[kMaxSpeculate];
        int got = 0;
        journal.on = true;
        for (int cq = q, cjb = jb, cm = m, cn = n; got < S.speculate && got < kMaxSpeculate;) {
            const int ps = apply_outcome(cq, cjb, cm, cn);
            if (ps < 0 || !next_pop(cq, cjb, ps, &p[got])) break;
            cq = p[got].q;
            cjb = p[got].pop.jb;
            cm = p[got].pop.m;
            cn = p[got].n;
            ++got;
        }
        journal.on = false;
        journal.rollback();
        restore_saves();
        // queued predictions are the oldest ones: chain only behind agreeing ones
        for (size_t i = 0; i < specs.size(); ++i)
            if ((int)i >= got || !(specs[i].pop == p[i].pop)) return;
        for (int i = (int)specs.size(); i < got; ++i) {
            const Pop& pop = p[i].pop;
            specs.push_back({launch_batched(S, pop.cls, pop.m, S.gang_ready ? 1 : 0, S.jobs[pop.jb].min_avail, pop.ready),
                             pop});
        }
    }
};

// allocate.go:41-201 on the host model, its placements through the device pops (03_pop.cpp)
struct AllocateAction {
    Session& S;
    Framework F;
    QueueHeap queues;
    JobQueues jobs_map;
    Speculation spec;
    vector<int32_t> ids, onode;  // the running pop: its tasks, and per task the node and kind it got
    vector<uint8_t> okind;
    const int gm;
    explicit AllocateAction(Session& s)
        : S(s), F(s), queues(QueueLess{&F}), spec(F, queues, jobs_map), gm(s.gang_ready ? 1 : 0) {}

    // allocate.go:45-63: plugins open, one queue copy and one job-queue entry per job
    void setup() {
        // KBHIP_OPEN_PROFILE=1: the setup's phases on stderr (diagnostic)
        static const bool prof = std::getenv("KBHIP_OPEN_PROFILE") != nullptr;
        auto tp = Clock::now();
        auto mark = [&](const char* what) {
            if (!prof) return;
            std::fprintf(stderr, "[alloc] %-10s %8.2f ms\n", what, seconds_since(tp) * 1e3);
            tp = Clock::now();
        };
        F.compile_orders();
        F.open_plugins();
        mark("plugins");
        // allocate.go:91-104: a job has work if it holds a pending task that is not BestEffort
        // (its task lists scanned over job ranges in parallel; the pushes below stay in order)
        const int NJ = (int)S.jobs.size();
        vector<uint8_t> has_work(NJ, 0);
        const int nth = NJ < (1 << 14) ? 1 : host_threads();
        run_ranges(nth, [&](int r) {
            const auto [b, e] = range_of(NJ, r, nth);
            for (int j = b; j < e; ++j) {
                const HJob& job = S.jobs[j];
                bool work = false;
                if (job.pending_built) work = job.cursor < job.pending.size();
                else if (job.maybe_pending)
                    for (int t : job.tasks) {
                        const HPod& p = S.pods[t];
                        if (p.status == Pending && !(p.req.c < kMinCPU && p.req.m < kMinMem && p.req.g < kMinGPU)) {
                            work = true;
                            break;
                        }
                    }
                has_work[j] = work;
            }
        });
        for (size_t j = 0; j < S.jobs.size(); ++j) {
            const int q = S.jobs[j].queue;
            // one queue copy per job, as allocate.go pushes them: a queue's share changes while
            // its other copies sit in the heap, so the Go heap's layout — which the copies of
            // jobs without pending tasks shape too — decides later pops (exactness needs them)
            queues.push(q);
            auto it = jobs_map.find(q);
            if (it == jobs_map.end()) it = jobs_map.emplace(q, JobQueue<JobLess>(JobLess{&F})).first;
            if (has_work[j]) {
                it->second.push((int)j);
            } else {
                it->second.idle.push_back((int)j);
                S.jobs[j].pending_built = true;  // what build_pending would find: nothing
            }
        }
        mark("heaps");
        for (auto& kv : jobs_map) F.sort_jobs(kv.second.idle);
        mark("idle");
        if (!S.ev_run[0]) { HIPCHK(hipEventCreate(&S.ev_run[0])); HIPCHK(hipEventCreate(&S.ev_run[1])); }
        ov_quiesce(S);
        mark("quiesce");
    }

    // The walk FitDelta histogram of a pop's last task when the kernels did
    // not report it (a pop that placed every pending task and left its job
    // not Ready): recomputed on the device state that task saw — queued
    // predictions retracted, its own commit undone and redone around the
    // recount (k_fit_key / k_fit_delta), the fallback node as it was before
    // that commit, and for a class with inter-pod priority terms the
    // score's min / max prepass on that state.  Shards: the chosen node's
    // walk key (its owner computes it) and the counts are all-reduced.
    void fit_sync(int cls, int node, int kind, HJob& job) {
        S.stats.fit_syncs++;
        spec.discard_all();
        ov_quiesce(S);
        const int32_t nd[1] = {node}, kd[1] = {kind};
        if (node >= 0) {
            HIPCHK(launch_undo_pop(S.nc, S.tab, cls, 1, nd, kd, S.stream));
            sess_placed(S, node, -1);  // the fallback node the task saw
        }
        ctrl_setup(S, 1, &cls, 0, 0, 0, 0, -1, 0);
        if (node >= 0) sess_placed(S, node, +1);
        if (S.classes[cls].ipa_n > 0) {
            HIPCHK(launch_ipa_minmax(S.nc, S.tab, S.d_ctrl, 0, S.stream));
            exchange(S, &S.d_ctrl->ipa_lo[0], KBHIP_RED_MIN_I64);
            exchange(S, &S.d_ctrl->ipa_hi[0], KBHIP_RED_MAX_I64);
        }
        if (node >= 0) {
            HIPCHK(launch_fit_key(S.conf, S.nc, S.tab, S.d_ctrl, node, S.stream));
            exchange(S, &S.d_ctrl->slot[0], KBHIP_RED_MAX_U64);
        }
        HIPCHK(hipMemsetAsync(S.d_fit4, 0, 4 * sizeof(int32_t), S.stream));
        HIPCHK(launch_fit_count(S.conf, S.nc, S.tab, S.d_ctrl, node, kind, S.d_fit4, S.stream));
        if (node >= 0) HIPCHK(launch_redo_pop(S.nc, S.tab, cls, 1, nd, kd, S.stream));
        HIPCHK(hipMemcpyAsync(job.fit, S.d_fit4, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, S.stream));
        HIPCHK(hipStreamSynchronize(S.stream));
        fit_allreduce(S, job.fit);
    }

    // One job pop through the device (allocate.go:106-181, the tasks in ids): the first
    // chunk batched (possibly already queued by speculation), the rest through place_job.
    void exec_pop(int q, int jb, int n, int32_t* n_done, int32_t* stop) {
        HJob& job = S.jobs[jb];
        const int cls0 = S.pods[ids[0]].cls;
        int m = 1;
        while (m < n && m < kMaxChunk && S.pods[ids[m]].cls == cls0) ++m;
        bool batch = batchable(S, cls0);
        if (batch && S.any_bf && cls0 < (int)S.bf_backoff.size() && S.bf_backoff[cls0] > 0) {
            S.bf_backoff[cls0]--;  // placement 6 missed for this class recently (place_job)
            batch = false;
        }
        if (!batch) {
            spec.discard_all();
            place_job(S, ids.data(), n, gm, job.min_avail, job.cnt_alloc, onode.data(), okind.data(), n_done, stop);
            return;
        }
        BatchLaunch L;
        if (!spec.take({jb, cls0, m, job.cnt_alloc, job.cursor}, &L))
            L = launch_batched(S, cls0, m, gm, job.min_avail, job.cnt_alloc);
        if (S.speculate > 0 && !S.any_bf) spec.speculate(q, jb, m, n);  // the undo of a pop has no visit rule
        int nd = 0, st = 0;
        collect_batched(S, L, &nd, &st, S.res_node_buf, S.res_kind_buf);
        if (st < 0) throw Error(KBHIP_EDEVICE, "device pop did not complete");
        if (nd == 0 && L.bf) {  // placed nothing: the rest of this pop and the class's next pops take
            if (S.bf_backoff.size() < S.classes.size()) S.bf_backoff.resize(S.classes.size(), 0);
            S.bf_backoff[cls0] = kBfBackoff + 1;  // the general path (place_job below consumes one)
        }
        int alloc = 0;
        for (int j = 0; j < nd; ++j) alloc += S.res_kind_buf[j] == 1;
        apply_results(S, ids.data(), nd, S.res_node_buf, S.res_kind_buf, onode.data(), okind.data());
        if (st == KBHIP_STOP_ALL && nd < n) {  // more chunks: the prediction assumed the pop ended here
            spec.discard_all();
            int32_t nd2 = 0, st2 = 0;
            place_job(S, ids.data() + nd, n - nd, gm, job.min_avail, job.cnt_alloc + alloc, onode.data() + nd,
                      okind.data() + nd, &nd2, &st2);
            nd += nd2;
            st = st2;
        }
        *n_done = nd;
        *stop = st;
    }

    // ssn.Allocate / ssn.Pipeline of the pop's first n_done tasks on the host model
    // (allocate.go:150-180, session.go:199-297)
    void record_pop(HJob& job, int n_done) {
        for (int i = 0; i < n_done; ++i) {
            const int pi = ids[i];
            if (onode[i] < 0) continue;
            HPod& p = S.pods[pi];
            p.node = onode[i];
            if (okind[i] == KBHIP_ALLOCATED) { p.status = Allocated; job.cnt_alloc++; }
            else p.status = Pipelined;
            job.priority = p.priority;  // UpdateTaskStatus -> AddTaskInfo (job_info.go:242)
            F.on_allocate(pi);
            S.log.emplace_back(pi, onode[i], okind[i]);
            S.stats.placed++;
            if (p.status == Allocated) F.dispatch_if_ready(job);
        }
        job.cursor += n_done;
    }

    void run() {  // allocate.go:41-201
        const auto t0 = Clock::now();
        setup();
        S.stats.alloc_setup_s += seconds_since(t0);
        HIPCHK(hipEventRecord(S.ev_run[0], S.stream));
        spec.attach();
        while (!queues.empty()) {
            int q = queues.pop();
            if (F.overused(q)) continue;
            auto jit = jobs_map.find(q);
            if (jit == jobs_map.end() || jit->second.empty()) continue;
            int jb = jit->second.pop();
            HJob& job = S.jobs[jb];
            S.stats.pops++;
            build_pending(F, job);
            if (job.cursor < job.pending.size()) {
                int n = (int)(job.pending.size() - job.cursor);
                ids.assign(job.pending.begin() + job.cursor, job.pending.end());
                onode.assign(n, -1);
                okind.assign(n, 0);
                int32_t n_done = 0, stop = 0;
                exec_pop(q, jb, n, &n_done, &stop);
                S.fit_task = (stop == KBHIP_STOP_UNASSIGNED && n_done >= 1) ? ids[n_done - 1] : -1;  // kbhip_fit_deltas
                S.stats.tasks += n_done;
                record_pop(job, n_done);
                // NodesFitDelta (allocate.go:124-126, 164-167): what the job keeps is the walk of
                // the task that ended its last pop; only a job left not Ready reports it
                if (stop == KBHIP_STOP_UNASSIGNED && S.last_fit_ok) {
                    for (int k = 0; k < 4; ++k) job.fit[k] = S.last_fit[k];
                } else if (S.gang_close && n_done >= 1 &&
                           (stop == KBHIP_STOP_UNASSIGNED || (stop == KBHIP_STOP_ALL && !F.job_ready(job)))) {
                    const int last = n_done - 1;
                    fit_sync(S.pods[ids[last]].cls, stop == KBHIP_STOP_UNASSIGNED ? -1 : onode[last], okind[last], job);
                }
                if (stop == KBHIP_STOP_READY) jit->second.push(jb);
                if (stop == KBHIP_STOP_UNASSIGNED) S.stats.unassigned_pops++;
            }
            queues.push(q);
        }
        spec.discard_all();  // predicted pops that never came
        ov_quiesce(S);
        ev_harvest_all(S);
        HIPCHK(hipEventRecord(S.ev_run[1], S.stream));
        HIPCHK(hipStreamSynchronize(S.stream));
        float dms = 0;
        HIPCHK(hipEventElapsedTime(&dms, S.ev_run[0], S.ev_run[1]));
        S.alloc_device_s += dms * 1e-3;
        S.stats.allocate_s += seconds_since(t0);
    }
};

void allocate_run(Session& S) {
    S.fit_task = -1;
    vict_stale(S);
    AllocateAction a(S);
    a.run();
}

// ---------------------------------------------------------------------------
// backfill action (actions/backfill/backfill.go:40-70): every Pending task of
// every job whose InitResreq is empty is allocated on the first node (lowest
// index) passing the predicates.  Pinned order:
// jobs by UID, tasks by UID, nodes by index.  Per-task first-fit sweeps of the
// general kernel (mode 1), 64 tasks per control-block round trip.
// ---------------------------------------------------------------------------
// first_fit: the inner loop of backfill.go:51-65 for the given tasks, in
// order: each goes to the lowest-index node passing PredicateFn and is
// committed with Session.Allocate (session.go:237-297); out_node[i] = that
// node or -1.  Tasks must be Pending tasks of the session (task class >= 0).
void first_fit(Session& S, const int32_t* ids, int n, int32_t* out_node) {
    vector<int> cand(ids, ids + n);
    for (int t : cand)
        if (t < 0 || t >= (int)S.pods.size() || S.pods[t].cls < 0 || S.pods[t].status != Pending)
            throw Error(KBHIP_EINVAL, "task id is not a pending task of the session");
    std::fill(out_node, out_node + n, -1);
    S.fit_task = -1;
    vict_stale(S);
    ov_quiesce(S);
    Framework F(S);
    F.compile_orders();
    F.open_plugins();
    for (size_t off = 0; off < cand.size(); off += kMaxChunk) {
        const int m = (int)std::min<size_t>(kMaxChunk, cand.size() - off);
        int cls[kMaxChunk];
        for (int i = 0; i < m; ++i) cls[i] = S.pods[cand[off + i]].cls;
        uint32_t epoch = 0;
        const int slot = take_slot(S, &epoch);
        ctrl_setup(S, m, cls, 0, 0, 0, 1, slot, epoch);
        sweep_chunk(S, m, cls, false);
        int n_done = 0, stop = -1;
        collect_tasks(S, slot, epoch, m, &n_done, &stop, S.res_node_buf, S.res_kind_buf, nullptr);
        S.stats.sweeps += m;
        S.stats.tasks += m;
        if (n_done != m || stop != 0) throw Error(KBHIP_EDEVICE, "backfill chunk did not complete");
        for (int i = 0; i < m; ++i) {
            const int node = S.res_node_buf[i];
            out_node[off + i] = node;
            if (node < 0) continue;
            const int pi = cand[off + i];
            HPod& p = S.pods[pi];
            HJob& job = S.jobs[p.job];
            p.status = Allocated;  // Session.Allocate(task, node, false) (session.go:237-297)
            p.node = node;
            job.cnt_alloc++;
            job.priority = p.priority;  // UpdateTaskStatus -> AddTaskInfo (job_info.go:242)
            S.used[node].c += p.req.c; S.used[node].m += p.req.m; S.used[node].g += p.req.g;
            sess_placed(S, node, +1);
            F.on_allocate(pi);  // drf / proportion AllocateFunc
            S.stats.placed++;
            S.log.emplace_back(pi, node, KBHIP_ALLOCATED);
            F.dispatch_if_ready(job);  // (session.go:286-321)
            if (S.classes[cls[i]].backfill) S.any_bf = 1;  // IsBackfill commit (commit_task)
        }
    }
}

}  // namespace kbhip

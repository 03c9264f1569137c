// framework.h — the Go framework's model on the host, shared by the parts that
// run actions on it (04_allocate, 10_ops, 11_evict): the Go heaps restated, the
// job / queue / task order functions, drf and proportion (open and event
// handlers), the task status index, and the statement operations.  Nothing
// here launches a placement; the statement operations update the device rows
// an eviction or a pipeline changes.
#pragma once
#include "session.h"

namespace kbhip {

// Range-parallel host loops: fn(0..nth-1), fn(0) on this thread
template <typename Fn>
void run_ranges(int nth, Fn fn) {
    vector<std::thread> th;
    for (int r = 1; r < nth; ++r) th.emplace_back(fn, r);
    fn(0);
    for (auto& x : th) x.join();
}
inline std::pair<int, int> range_of(int total, int r, int nth) {  // part r of nth of [0, total)
    return {(int)((int64_t)total * r / nth), (int)((int64_t)total * (r + 1) / nth)};
}
using Clock = std::chrono::steady_clock;
inline double seconds_since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

// Undo log of speculative heap operations: (heap items, position, old value);
// position -1 records the old size.
struct HeapJournal {
    bool on = false;
    struct Entry {
        vector<int>* v;
        int pos, val;
    };
    vector<Entry> e;
    void rollback() {
        for (auto it = e.rbegin(); it != e.rend(); ++it) {
            if (it->pos < 0) it->v->resize(it->val);
            else (*it->v)[it->pos] = it->val;
        }
        e.clear();
    }
};

template <typename L>
struct GoHeap {  // Go container/heap (up/down exactly as heap.go), with an optional undo log
    vector<int> items;
    L less;
    HeapJournal* jr = nullptr;
    explicit GoHeap(L l) : less(l) {}
    bool Less(int i, int j) { return less(items[i], items[j]); }
    void swap_at(int i, int j) {
        if (jr && jr->on) {
            jr->e.push_back({&items, i, items[i]});
            jr->e.push_back({&items, j, items[j]});
        }
        std::swap(items[i], items[j]);
    }
    void up(int j) {
        for (;;) {
            int i = (j - 1) / 2;
            if (i == j || !Less(j, i)) break;
            swap_at(i, j);
            j = i;
        }
    }
    void down(int i, int n) {
        for (;;) {
            int j1 = 2 * i + 1;
            if (j1 >= n || j1 < 0) break;
            int j = j1, j2 = j1 + 1;
            if (j2 < n && Less(j2, j1)) j = j2;
            if (!Less(j, i)) break;
            swap_at(i, j);
            i = j;
        }
    }
    void push(int x) {
        if (jr && jr->on) jr->e.push_back({&items, -1, (int)items.size()});
        items.push_back(x);
        up((int)items.size() - 1);
    }
    int pop() {
        int n = (int)items.size() - 1;
        swap_at(0, n);
        down(0, n);
        int x = items.back();
        if (jr && jr->on) {  // rolled back in reverse: size first, then the slot
            jr->e.push_back({&items, n, x});
            jr->e.push_back({&items, -1, n + 1});
        }
        items.pop_back();
        return x;
    }
    bool empty() const { return items.empty(); }
};

// A queue's job heap in allocate (allocate.go:48-63, 87): a job's order key
// (priority, gang readiness, DRF share, creation time, UID) changes only
// while the job is popped, so the heap never holds a stale key and pops in
// exact key order (a strict total order) whatever its layout.  Jobs with no
// pending task when the action starts are never pushed back and never change
// key: they wait in a list sorted by key, and a pop takes the smaller of its
// head and the heap's top.  Only the jobs with pending tasks pay heap work
// (C5: ~180k running jobs, a few hundred pending ones).
template <typename L>
struct JobQueue {
    GoHeap<L> heap;
    vector<int> idle;       // jobs without pending tasks, ascending key
    vector<int> head{0};    // next idle job (a vector: the speculation journal restores it)
    L less;
    explicit JobQueue(L l) : heap(l), less(l) {}
    void set_journal(HeapJournal* jr) { heap.jr = jr; }
    void push(int x) { heap.push(x); }
    bool empty() const { return head[0] >= (int)idle.size() && heap.empty(); }
    int pop() {
        const int h = head[0];
        if (h < (int)idle.size() && (heap.empty() || less(idle[h], heap.items[0]))) {
            if (heap.jr && heap.jr->on) heap.jr->e.push_back({&head, 0, h});
            head[0] = h + 1;
            return idle[h];
        }
        return heap.pop();
    }
};

// The session as the actions see it: order functions, drf / proportion, the
// status index, statements.  One per action (or per ABI call that changes the
// model); what outlives it is in the Session.
struct Framework {
    Session& S;
    explicit Framework(Session& s) : S(s) {}

    int readiness(const HJob& j) const {  // job_info.go:374-388
        if (j.cnt_alloc >= j.min_avail) return 1;
        if (j.cnt_alloc + j.cnt_aob >= j.min_avail) return 2;
        return 4;
    }
    bool job_ready(const HJob& j) const { return !S.gang_ready || readiness(j) == 1; }  // session_plugins.go:167-186
    // dispatch (session.go:286-294): once its job is Ready, every Allocated task goes to Binding
    void dispatch_if_ready(HJob& job) {
        if (!job_ready(job)) return;
        for (int t : job.tasks)
            if (S.pods[t].status == Allocated) { S.pods[t].status = Binding; job.priority = S.pods[t].priority; }
    }
    // tier dispatch compiled once: enabled order functions in tier order
    // (session_plugins.go:244-329); codes 1 priority, 2 gang, 3 drf
    vector<int> job_order;
    bool queue_prop = false, task_prio = false;
    void compile_orders() {
        for (auto& tier : S.tiers)
            for (auto& p : tier) {
                if (!(p.flags & KBS_DIS_JOBORDER)) {
                    if (p.name == "priority") job_order.push_back(1);
                    else if (p.name == "gang") job_order.push_back(2);
                    else if (p.name == "drf") job_order.push_back(3);
                }
                if (!(p.flags & KBS_DIS_QUEUEORDER) && p.name == "proportion") queue_prop = true;
                if (!(p.flags & KBS_DIS_TASKORDER) && p.name == "priority") task_prio = true;
            }
    }
    bool job_less(int l, int r) const {  // session_plugins.go:244-268
        if (l == r) return false;
        const HJob &L = S.jobs[l], &R = S.jobs[r];
        for (int code : job_order) {
            int c;
            if (code == 1) c = L.priority > R.priority ? -1 : L.priority < R.priority ? 1 : 0;  // priority.go:60-76
            else if (code == 2) {  // gang.go:136-160
                bool lr = readiness(L) == 1, rr = readiness(R) == 1;
                c = (lr && rr) ? 0 : lr ? 1 : rr ? -1 : 0;
            } else c = L.drf_share == R.drf_share ? 0 : L.drf_share < R.drf_share ? -1 : 1;  // drf.go:113-129
            if (c != 0) return c < 0;
        }
        if (L.ts == R.ts) return l < r;  // UID order: jobs are numbered in UID order at open
        return L.ts < R.ts;
    }
    // jobs in job_less order, sorted on compact keys: job_less's comparisons in
    // turn as unsigned digits (priority descending, gang-ready last, DRF share
    // ascending — non-negative doubles order as their bits — creation time),
    // then the job index (UID order)
    void sort_jobs(vector<int>& v) const {
        struct K {
            uint64_t d[3];
            int64_t ts;
            int j;
        };
        const int nd = (int)job_order.size();
        bool neg = false;  // (DRF shares are sums of requests over totals: never negative)
        for (int j : v) neg = neg || S.jobs[j].drf_share < 0;
        if (nd > 3 || neg) {  // more order codes than digits (repeated plugins): the comparator itself
            std::sort(v.begin(), v.end(), [this](int a, int b) { return job_less(a, b); });
            return;
        }
        vector<K> k(v.size());
        auto keys = [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; ++i) {
                const HJob& J = S.jobs[v[i]];
                K& x = k[i];
                for (int c = 0; c < nd; ++c) {
                    const int code = job_order[c];
                    if (code == 1) x.d[c] = (uint64_t)((int64_t)INT32_MAX - (int64_t)J.priority);
                    else if (code == 2) x.d[c] = readiness(J) == 1 ? 1 : 0;
                    else {
                        uint64_t b = 0;
                        if (J.drf_share != 0) std::memcpy(&b, &J.drf_share, 8);
                        x.d[c] = b;
                    }
                }
                x.ts = J.ts;
                x.j = v[i];
            }
        };
        auto lt = [nd](const K& a, const K& b) {
            for (int c = 0; c < nd; ++c)
                if (a.d[c] != b.d[c]) return a.d[c] < b.d[c];
            if (a.ts != b.ts) return a.ts < b.ts;
            return a.j < b.j;
        };
        const size_t n = k.size();
        if (n < (1u << 14)) {
            keys(0, n);
            std::sort(k.begin(), k.end(), lt);
        } else {  // C4 / C5: 10 k - 180 k jobs without pending tasks: 8 runs keyed and sorted in parallel,
                  // merged pairwise (each level's merges in parallel)
            constexpr int kRuns = 8;
            vector<size_t> cut(kRuns + 1);
            for (int r = 0; r <= kRuns; ++r) cut[r] = n * r / kRuns;
            run_ranges(kRuns, [&](int r) {
                keys(cut[r], cut[r + 1]);
                std::sort(k.begin() + cut[r], k.begin() + cut[r + 1], lt);
            });
            for (int w = 1; w < kRuns; w *= 2)  // the keys are distinct (job index last): a strict order
                run_ranges(kRuns / (2 * w), [&, w](int i) {
                    const int r = 2 * w * i;
                    std::inplace_merge(k.begin() + cut[r], k.begin() + cut[r + w],
                                       k.begin() + cut[std::min(r + 2 * w, kRuns)], lt);
                });
        }
        for (size_t i = 0; i < v.size(); ++i) v[i] = k[i].j;
    }
    bool queue_less(int l, int r) const {  // session_plugins.go:270-295, proportion.go:144-157
        if (l == r) return false;  // copies of one queue (one heap entry per job) are equal
        const HQueue &L = S.queues[l], &R = S.queues[r];
        if (queue_prop && L.share != R.share) return L.share < R.share;
        if (L.ts == R.ts) return L.rank < R.rank;
        return L.ts < R.ts;
    }
    bool task_less(int l, int r) const {  // session_plugins.go:297-329, priority.go:39-55
        const HPod &L = S.pods[l], &R = S.pods[r];
        if (task_prio && L.priority != R.priority) return L.priority > R.priority;
        if (L.ts == R.ts) return L.uid_rank < R.uid_rank;
        return L.ts < R.ts;
    }
    double drf_share_of(const F3& a) const {  // drf.go:160-170
        double res = 0;
        for (int k = 0; k < 3; ++k) { double x = share(a.get(k), S.total.get(k)); if (x > res) res = x; }
        return res;
    }
    void drf_update(HJob& j) { j.drf_share = drf_share_of(j.drf_alloc); }  // drf.go:156-170
    void prop_update(HQueue& q) {  // proportion.go:229-241
        double res = 0;
        for (int k = 0; k < 3; ++k) { double x = share(q.allocated.get(k), q.deserved.get(k)); if (x > res) res = x; }
        q.share = res;
    }
    void open_plugins() {
        if (S.plugins_opened) return;
        S.plugins_opened = true;
        if (S.drf_on) {  // drf.go:65-82 (each job's sum over its own tasks, in order: job ranges in parallel)
            const int J = (int)S.jobs.size();
            const int nth = J < (1 << 14) ? 1 : host_threads();
            run_ranges(nth, [&](int t) {
                const auto [b, e] = range_of(J, t, nth);
                for (int jb = b; jb < e; ++jb) {
                    HJob& j = S.jobs[jb];
                    for (int k : j.tasks) if (allocated_status(S.pods[k].status)) j.drf_alloc.add(S.pods[k].req);
                    drf_update(j);
                }
            });
        }
        if (S.prop_on) {  // proportion.go:65-142
            // each queue's sums in job and task order (floating point: the order is kept), queues
            // split over the threads — or, when prop_sums_exact finds every addend and every
            // total a non-negative integer below 2^53, job ranges in parallel
            const int NQ = (int)S.queues.size();
            const int nth = S.pods.size() < (1u << 16) ? 1 : std::min(NQ, host_threads());
            if (nth > 0 && !(S.pods.size() >= (1u << 16) && prop_sums_exact()))
                run_ranges(nth, [&](int t) {
                    for (auto& j : S.jobs) {
                        if (j.queue % nth != t) continue;
                        HQueue& q = S.queues[j.queue];
                        q.has_attr = true;
                        for (int k : j.tasks) {
                            const HPod& p = S.pods[k];
                            if (allocated_status(p.status)) { q.allocated.add(p.req); q.request.add(p.req); }
                            else if (p.status == Pending) q.request.add(p.req);
                        }
                    }
                });
            vector<int> order;
            for (size_t i = 0; i < S.queues.size(); ++i) if (S.queues[i].has_attr) order.push_back((int)i);
            F3 remaining = S.total;
            vector<char> meet(S.queues.size(), 0);
            for (;;) {
                int32_t tw = 0;
                for (int q : order) if (!meet[q]) tw += S.queues[q].weight;
                if (tw == 0) break;
                F3 deserved;
                for (int qi : order) {
                    if (meet[qi]) continue;
                    HQueue& q = S.queues[qi];
                    const double ratio = (double)q.weight / (double)tw;
                    F3 r = remaining;
                    r.c *= ratio; r.m *= ratio; r.g *= ratio;
                    q.deserved.addf(r);
                    if (!q.deserved.less_equal(q.request)) {  // helpers.Min
                        q.deserved.c = std::fmin(q.deserved.c, q.request.c);
                        q.deserved.g = std::fmin(q.deserved.g, q.request.g);
                        q.deserved.m = std::fmin(q.deserved.m, q.request.m);
                        meet[qi] = 1;
                    }
                    prop_update(q);
                    deserved.addf(q.deserved);
                }
                remaining.subf(deserved);
                if (remaining.empty()) break;
            }
        }
    }
    // proportion's queue sums (proportion.go:88-103) over job ranges in parallel. A float64 sum
    // of non-negative integers whose total stays below 2^53 is exact in any order (every
    // partial sum is an integer no larger than the total), so it equals the in-order sum; the
    // queues are written only when every addend, start value and total meets that.
    bool prop_sums_exact() {
        constexpr int64_t kLim = int64_t(1) << 53;
        const int NQ = (int)S.queues.size(), J = (int)S.jobs.size();
        const int nth = std::max(1, std::min(host_threads(), J / 256));
        vector<vector<int64_t>> acc(nth, vector<int64_t>(6 * (size_t)NQ, 0));
        vector<vector<uint8_t>> has(nth, vector<uint8_t>(NQ, 0));
        vector<uint8_t> ok(nth, 1);
        run_ranges(nth, [&](int t) {
            int64_t* a = acc[t].data();
            auto put = [&](int64_t* s, const R3& r) {
                if ((uint64_t)r.c >= (uint64_t)kLim || (uint64_t)r.m >= (uint64_t)kLim ||
                    (uint64_t)r.g >= (uint64_t)kLim)
                    return false;  // negative or too large
                s[0] += r.c; s[1] += r.m; s[2] += r.g;
                return s[0] < kLim && s[1] < kLim && s[2] < kLim;
            };
            const auto [b, e] = range_of(J, t, nth);
            for (int jb = b; jb < e; ++jb) {
                const HJob& j = S.jobs[jb];
                has[t][j.queue] = 1;
                int64_t* qa = a + 6 * (size_t)j.queue;
                for (int k : j.tasks) {
                    const HPod& p = S.pods[k];
                    bool good = true;
                    if (allocated_status(p.status)) good = put(qa, p.req) && put(qa + 3, p.req);
                    else if (p.status == Pending) good = put(qa + 3, p.req);
                    if (!good) { ok[t] = 0; return; }
                }
            }
        });
        for (int t = 0; t < nth; ++t) if (!ok[t]) return false;
        vector<double> out(6 * (size_t)NQ);
        for (int q = 0; q < NQ; ++q) {
            const HQueue& Q = S.queues[q];
            const double x0[6] = {Q.allocated.c, Q.allocated.m, Q.allocated.g, Q.request.c, Q.request.m, Q.request.g};
            for (int k = 0; k < 6; ++k) {
                if (!(x0[k] >= 0 && x0[k] < (double)kLim && x0[k] == std::floor(x0[k]))) return false;
                int64_t s = (int64_t)x0[k];
                for (int t = 0; t < nth; ++t) s += acc[t][6 * (size_t)q + k];  // each < 2^53: no overflow
                if (s >= kLim) return false;
                out[6 * (size_t)q + k] = (double)s;
            }
        }
        for (int q = 0; q < NQ; ++q) {
            HQueue& Q = S.queues[q];
            const double* o = &out[6 * (size_t)q];
            Q.allocated.c = o[0]; Q.allocated.m = o[1]; Q.allocated.g = o[2];
            Q.request.c = o[3]; Q.request.m = o[4]; Q.request.g = o[5];
            for (int t = 0; t < nth; ++t) if (has[t][q]) Q.has_attr = true;
        }
        return true;
    }
    bool overused(int qi) const {  // proportion.go:186-197
        if (!S.prop_on) return false;
        return S.queues[qi].deserved.less_equal(S.queues[qi].allocated);
    }
    void on_allocate(int pi) {  // event handlers drf.go:134-143, proportion.go:200-210
        const HPod& p = S.pods[pi];
        HJob& j = S.jobs[p.job];
        if (S.drf_on) { j.drf_alloc.add(p.req); drf_update(j); }
        if (S.prop_on) { HQueue& q = S.queues[j.queue]; q.allocated.add(p.req); prop_update(q); }
    }
    void on_deallocate(int pi) {  // event handlers drf.go:144-151, proportion.go:211-219
        const HPod& p = S.pods[pi];
        HJob& j = S.jobs[p.job];
        if (S.drf_on) { j.drf_alloc.sub(p.req); drf_update(j); }
        if (S.prop_on) { HQueue& q = S.queues[j.queue]; q.allocated.sub(p.req); prop_update(q); }
    }

    // Caches over the task statuses that set_status (and unevict) keep exact.  Each is
    // empty until an eviction action builds it, and empty means untracked: an index past a
    // cache's size is left alone, so a Framework that only applies operations
    // (kbhip_apply_ops) maintains nothing, and the next eviction action builds its own from
    // the pods (reset_ready_cache / scan_jobs, build_node_tasks, compile_victims).
    //   ready_val[job]  gang's readyTaskNum (gang.go:212-222), valid where ready_ok[job]
    //   run_copy[pod]   the pod is Running and its node holds that copy (not a Releasing one)
    vector<uint8_t> ready_ok;
    vector<int> ready_val;
    vector<uint8_t> run_copy;
    void reset_ready_cache() {
        ready_ok.assign(S.jobs.size(), 0);
        ready_val.assign(S.jobs.size(), 0);
    }
    // JobInfo.UpdateTaskStatus (job_info.go:251-264): the status index, and
    // AddTaskInfo's "job priority = this task's priority" (:242)
    static bool gang_ready_status(int st) { return allocated_status(st) || st == Succeeded || st == Pipelined; }
    void set_status(int pi, int st) {
        HPod& p = S.pods[pi];
        HJob& j = S.jobs[p.job];
        if (p.job < (int)ready_ok.size() && ready_ok[p.job])
            ready_val[p.job] += (int)gang_ready_status(st) - (int)gang_ready_status(p.status);
        if (pi < (int)run_copy.size()) run_copy[pi] = (st == Running && !p.node_rel) ? 1 : 0;
        if (allocated_status(p.status)) j.cnt_alloc--;
        if (p.status == AOB) j.cnt_aob--;
        p.status = st;
        if (allocated_status(st)) j.cnt_alloc++;
        if (st == AOB) j.cnt_aob++;
        j.priority = p.priority;
    }

    // Statement operations (framework/statement.go, session.go Evict / Pipeline): the host
    // model first, then the device rows they change (Releasing, pod count, nonzero requests,
    // ports) before the next sweep.  Node-sharded sessions: the row on the owning shard only,
    // the pod-affinity count tables on every shard.
    int local_node(int g) const {  // this shard's row of global node g, or -1
        const int l = g - S.nc.base;
        return l >= 0 && l < S.nc.n ? l : -1;
    }
    // kbhip_apply_ops: the four operations run on the host model as in the actions, their node-row
    // halves collected here in order instead of launched or summed (the caller applies them in one
    // launch, launch_apply_ops)
    vector<NodeOp>* ops_out = nullptr;
    void dev_op(int op, int pi) {
        const HPod& p = S.pods[pi];
        if (ops_out) { ops_out->push_back(NodeOp{op, p.node, p.cls, R3{}}); return; }
        HIPCHK(launch_node_op(S.nc, S.tab, op, local_node(p.node), p.node, p.cls, p.req.c, p.req.m, p.req.g,
                              S.stream));
    }
    // the session half of an eviction (session.go:331-356 / statement.go:35-67)
    void evict_in_session(int v) {
        if (allocated_status(S.pods[v].status)) queue_target(S, v, -1);  // no longer a predicate target
        set_status(v, Releasing);
        // node.UpdateTask: Releasing += Resreq.  No node ranking reads Releasing, so
        // evictions are summed per node and applied in one launch (flush_evictions)
        const HPod& p = S.pods[v];
        if (ops_out) {
            ops_out->push_back(NodeOp{0, p.node, 0, p.req, S.jobs[p.job].queue});
            on_deallocate(v);
            return;
        }
        if (S.rel_delta.empty()) { S.rel_delta.assign(S.n_total, R3{}); S.rel_flag.assign(S.n_total, 0); }
        if (!S.rel_flag[p.node]) { S.rel_flag[p.node] = 1; S.rel_touched.push_back(p.node); }
        R3& d = S.rel_delta[p.node];
        d.c += p.req.c; d.m += p.req.m; d.g += p.req.g;
        on_deallocate(v);
    }
    void flush_evictions() {
        const int nt = (int)S.rel_touched.size();
        if (!nt) return;
        vector<int32_t> nodes;
        vector<int64_t> d;
        nodes.reserve(nt);
        d.reserve(3 * (size_t)nt);
        for (int i = 0; i < nt; ++i) {
            const int v = S.rel_touched[i];
            const int l = local_node(v);  // (shards: the owning rank's rows only)
            if (l >= 0) {
                nodes.push_back(l);
                d.push_back(S.rel_delta[v].c); d.push_back(S.rel_delta[v].m); d.push_back(S.rel_delta[v].g);
            }
            S.rel_delta[v] = R3{};
            S.rel_flag[v] = 0;
        }
        S.rel_touched.clear();
        const int n = (int)nodes.size();
        if (!n) { flush_tables(S); return; }
        int32_t* dn = S.b_rel_nodes.alloc<int32_t>(n);
        int64_t* dd = S.b_rel_d.alloc<int64_t>(3 * (size_t)n);
        HIPCHK(hipMemcpyAsync(dn, nodes.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, S.stream));
        HIPCHK(hipMemcpyAsync(dd, d.data(), d.size() * sizeof(int64_t), hipMemcpyHostToDevice, S.stream));
        HIPCHK(launch_rel_add(S.nc, dn, dd, n, S.stream));
        HIPCHK(hipStreamSynchronize(S.stream));  // the pageable sources must outlive the copies
        flush_tables(S);
    }
    void unevict(int v) {  // statement.go:81-105: node.AddTask fails, the node keeps its Releasing copy
        set_status(v, Running);
        queue_target(S, v, +1);  // a predicate target again (the lister reads the job's status index)
        S.pods[v].node_rel = true;
        if (v < (int)run_copy.size()) run_copy[v] = 0;
        on_allocate(v);
    }
    void pipeline(int t, int n) {  // statement.go:96-136 / session.go:199-235
        HPod& p = S.pods[t];
        set_status(t, Pipelined);
        p.node = n;
        // NodeInfo.Tasks exists while an eviction action runs (build_node_tasks at its start; every such
        // action rebuilds it); between actions (kbhip_apply_ops) a list left by an earlier action takes
        // the operations' inserts and erases and nothing is built: the next eviction action reads the pods
        if (n < (int)S.node_tasks.size()) {
            auto& nt = S.node_tasks[n];
            nt.insert(std::lower_bound(nt.begin(), nt.end(), t), t);
        }
        dev_op(1, t);
        S.used[n].c += p.req.c; S.used[n].m += p.req.m; S.used[n].g += p.req.g;
        sess_placed(S, n, +1);
        if (S.classes[p.cls].backfill) S.any_bf = 1;
        on_allocate(t);
    }
    void unpipeline(int t) {  // statement.go:141-172 (task.NodeName stays set)
        HPod& p = S.pods[t];
        set_status(t, Pending);
        if (p.node < (int)S.node_tasks.size()) {
            auto& nt = S.node_tasks[p.node];
            nt.erase(std::lower_bound(nt.begin(), nt.end(), t));  // (a list that exists holds every Pipelined task)
        }
        dev_op(2, t);
        S.used[p.node].c -= p.req.c; S.used[p.node].m -= p.req.m; S.used[p.node].g -= p.req.g;
        sess_placed(S, p.node, -1);
        on_deallocate(t);
    }
    struct Stmt {  // framework.Statement: (0 evict | 1 pipeline, pod)
        vector<std::pair<int, int>> ops;
    };
    void commit(Stmt& st) {  // statement.go:188-198: evictions reach the cache (recorded), pipelines bind nothing
        for (auto& op : st.ops)
            S.log.emplace_back(op.second, S.pods[op.second].node, op.first == 0 ? KBHIP_EVICTED : KBHIP_PIPELINED);
        st.ops.clear();
    }
    void discard(Stmt& st) {  // statement.go:174-186
        for (auto it = st.ops.rbegin(); it != st.ops.rend(); ++it) {
            if (it->first == 0) unevict(it->second);
            else unpipeline(it->second);
        }
        st.ops.clear();
    }
};

// The victim functions of an action in tier order, as codes (1 gang, 2 conformance, 3 drf, 4 proportion;
// the tiers' plugin names compared once, not per node visited): Preemptable's for preempt, else Reclaimable's.
inline vector<vector<int>> victim_tier_codes(const Session& S, bool preempt) {
    vector<vector<int>> out;
    for (auto& tier : S.tiers) {
        vector<int> codes;
        for (auto& pl : tier) {
            if (pl.flags & (preempt ? KBS_DIS_PREEMPTABLE : KBS_DIS_RECLAIMABLE)) continue;
            if (pl.name == "gang") codes.push_back(1);
            else if (pl.name == "conformance") codes.push_back(2);
            else if (preempt && pl.name == "drf" && S.drf_on) codes.push_back(3);
            else if (!preempt && pl.name == "proportion" && S.prop_on) codes.push_back(4);
        }
        out.push_back(std::move(codes));
    }
    return out;
}

// The order functions as heap comparators (util/priority_queue.go over Job / QueueOrderFn)
struct JobLess {
    const Framework* F;
    bool operator()(int a, int b) const { return F->job_less(a, b); }
};
struct QueueLess {
    const Framework* F;
    bool operator()(int a, int b) const { return F->queue_less(a, b); }
};

}  // namespace kbhip

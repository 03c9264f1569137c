// kbhip session, part 11: the reclaim / preempt actions and the device ranking of a task's nodes
#include "framework.h"

namespace kbhip {

// The node-ranking buffers of a session (keys, sorted keys, histogram,
// counters, the host copy), allocated on its first ranking.
void rank_buffers(Session& S) {
    if (S.b_rank_sorted.p) return;
    const int N = S.nc.n;
    S.b_rank_keys.alloc<uint64_t>(N);
    S.b_rank_sorted.alloc<uint64_t>(N);
    S.b_rank_cnt.alloc<uint32_t>(4);
    S.rank_tmp_bytes = std::max<size_t>((size_t)16, rank_hist_words(N) * sizeof(uint32_t));
    S.b_rank_tmp.alloc<uint8_t>(S.rank_tmp_bytes);
    S.b_rank_radix.alloc<uint64_t>(std::max(N, 1));
    S.h_rank.fit((size_t)(N + 1) * sizeof(uint64_t));
}

// The device ranking of the task class cls on the session's stream: the keys
// of the walk order (rank_nodes below; by_score: preempt, else reclaim) sorted
// descending in b_rank_sorted, the passing count in b_rank_cnt[0] and the
// nodes whose score left the class's range in b_rank_cnt[1].  Nothing is
// copied back or waited for (the what-if batcher's shared launch aside).
// Returns the kernel launches it made (the batcher's shared launch counted as
// the session's own three).
int rank_launch(Session& S, int cls, bool by_score) {
    const int N = S.nc.n;
    rank_buffers(S);
    int launches = flush_tables(S);  // evictions / unevicts so far change pod-affinity predicates
    ctrl_setup(S, 1, &cls, 0, 0, 0, 0, -1, 0);
    launches += 1;
    HIPCHK(hipMemsetAsync(S.b_rank_cnt.p, 0, 2 * sizeof(uint32_t), S.stream));
    auto sr = S.class_srange[cls];
    if (by_score && S.classes[cls].ipa_n > 0) {  // inter-pod priority: normalisation prepass, wider range
        HIPCHK(launch_ipa_minmax(S.nc, S.tab, S.d_ctrl, 0, S.stream));
        launches += 1;
        exchange(S, &S.d_ctrl->ipa_lo[0], KBHIP_RED_MIN_I64);  // (shards: over every node)
        exchange(S, &S.d_ctrl->ipa_hi[0], KBHIP_RED_MAX_I64);
        const int64_t w = 10 * (int64_t)S.conf.w_pa * S.conf.score_mult;
        sr.first += std::min<int64_t>(0, w);
        sr.second += std::max<int64_t>(0, w);
    }
    const bool counting = !S.force_radix && sr.second - sr.first < 256 && sr.first >= INT32_MIN &&
                          sr.second <= INT32_MAX;
    if (counting && S.rank_group && S.world == 1) {  // one launch with the concurrent what-if sessions' rankings
        StepBatcher::Req r;
        r.kind = StepBatcher::kRank;
        HIPCHK(fill_rank_desc(&r.rank, S.conf, S.nc, S.tab, S.classes[cls], S.d_ctrl, by_score ? 1 : 0, (int)sr.first,
                              (int)sr.second, (uint64_t*)S.b_rank_keys.p, (uint32_t*)S.b_rank_tmp.p,
                              (uint64_t*)S.b_rank_sorted.p, (uint32_t*)S.b_rank_cnt.p));
        r.st = S.stream;
        r.device = S.device;
        HIPCHK(hipStreamSynchronize(S.stream));  // this request's control block and counters are in place
        StepBatcher::get().submit(r);
        HIPCHK(hipSetDevice(S.device));
        HIPCHK(r.err);
        S.stats.rank_requests++;
        S.stats.rank_batch_sum += r.batch;
        launches += 3;
    } else if (counting) {  // hand-written stable counting sort over the score
        HIPCHK(launch_rank_sorted(S.conf, S.nc, S.tab, S.classes[cls], S.d_ctrl, by_score ? 1 : 0, (int)sr.first,
                                  (int)sr.second,
                                  (uint64_t*)S.b_rank_keys.p, (uint32_t*)S.b_rank_tmp.p,
                                  (uint64_t*)S.b_rank_sorted.p, (uint32_t*)S.b_rank_cnt.p, S.stream));
        launches += 3;  // bucket, scan, scatter
    } else {  // wide score ranges (large nodeorder weights): 8-bit LSD radix passes over the score
        HIPCHK(launch_rank_nodes(S.conf, S.nc, S.tab, S.d_ctrl, by_score ? 1 : 0, (uint64_t*)S.b_rank_keys.p,
                                 (uint32_t*)S.b_rank_cnt.p, S.stream));
        HIPCHK(launch_rank_radix((const uint64_t*)S.b_rank_keys.p, N, (const uint32_t*)S.b_rank_cnt.p,
                                 (uint32_t*)S.b_rank_tmp.p, (uint64_t*)S.b_rank_radix.p,
                                 (uint64_t*)S.b_rank_sorted.p, S.stream));
        launches += 1 + 4 * 3;  // the key sweep, then four passes of bucket, scan, scatter
    }
    return launches;
}

// Node-sharded ranking: every shard's sorted passing keys (descending; global node index
// inside) all-gathered as fixed-size records [count, keys...], merged into the order one
// GPU's sort of every node gives (the keys are distinct).
static void merge_shard_ranks(Session& S, int cnt, vector<int>& out) {
    const uint64_t* const h_rank = S.h_rank.as<uint64_t>();
    const size_t rec = (size_t)(S.n_total + S.world - 1) / S.world + 1;  // >= every shard's rows + 1
    vector<uint64_t> send(rec, 0), recv(rec * S.world);
    send[0] = (uint64_t)cnt;
    std::memcpy(send.data() + 1, h_rank + 1, (size_t)cnt * sizeof(uint64_t));
    gather_host(S, send.data(), recv.data(), rec * sizeof(uint64_t));
    vector<size_t> at(S.world), end(S.world);
    size_t total = 0;
    for (int r = 0; r < S.world; ++r) {
        const uint64_t c = recv[rec * r];
        if (c >= rec) throw Error(KBHIP_EDEVICE, "shard ranking: a rank's count exceeds its record");
        at[r] = rec * r + 1;
        end[r] = at[r] + c;
        total += c;
    }
    out.resize(total);
    for (size_t i = 0; i < total; ++i) {
        int best = -1;
        for (int r = 0; r < S.world; ++r)
            if (at[r] < end[r] && (best < 0 || recv[at[r]] > recv[at[best]])) best = r;
        out[i] = key_idx(recv[at[best]++]);
    }
}
static void rank_nodes_inner(Session& S, int cls, bool by_score, vector<int>& out) {
    const int N = S.nc.n;
    rank_launch(S, cls, by_score);
    uint64_t* const h_rank = S.h_rank.as<uint64_t>();
    const int first = std::min(N, S.rank_first);
    HIPCHK(hipMemcpyAsync(h_rank, S.b_rank_cnt.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, S.stream));
    HIPCHK(hipMemcpyAsync(h_rank + 1, S.b_rank_sorted.p, first * sizeof(uint64_t), hipMemcpyDeviceToHost,
                          S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));
    const int cnt = (int)(uint32_t)h_rank[0];
    if (h_rank[0] >> 32) throw Error(KBHIP_EDEVICE, "rank_nodes: node score outside the class score range");
    if (cnt > first) {
        HIPCHK(hipMemcpyAsync(h_rank + 1 + first, (const uint64_t*)S.b_rank_sorted.p + first,
                              (size_t)(cnt - first) * sizeof(uint64_t), hipMemcpyDeviceToHost, S.stream));
        HIPCHK(hipStreamSynchronize(S.stream));
    }
    if (S.world > 1) {
        merge_shard_ranks(S, cnt, out);
    } else {
        out.resize(cnt);
        for (int i = 0; i < cnt; ++i) out[i] = key_idx(h_rank[1 + i]);
    }
    S.stats.sweeps++;
    S.stats.tasks++;
}
// The walk order of the task of class cls: preempt (by_score) = SelectBestNode order of
// the nodes passing PredicateFn with a NodeOrderFn score; reclaim = passing nodes in order.
static void rank_nodes(Session& S, int cls, bool by_score, vector<int>& out) {
    const auto tr0 = Clock::now();
    rank_nodes_inner(S, cls, by_score, out);
    S.stats.evict_rank_s += seconds_since(tr0);
}

#ifdef KBHIP_WALK_PROF  // diagnostic build: reclaim walk split (gather / victims / evictions), stderr
#define WP_MARK(ph) wp_mark(ph)
#define WP_REPORT(name) (fprintf(stderr, "walkprof %s gather %.3g victims %.3g evict %.3g Gcycles\n", name, \
                                 wp_acc[0] * 1e-9, wp_acc[1] * 1e-9, wp_acc[2] * 1e-9), wp_ph = -1)
#else
#define WP_MARK(ph) ((void)0)
#define WP_REPORT(name) ((void)0)
#endif

// ---------------------------------------------------------------------------
// reclaim / preempt (actions/reclaim/reclaim.go:41-196,
// actions/preempt/preempt.go:43-353).  The walk order of a preemptor's nodes
// comes from the device (kbhip_evict.hip); victims are chosen per node on the
// host model, in the pinned order of NodeInfo.Tasks (pod index); evictions and
// pipelines are the framework's statement operations (framework.h).
// Node-sharded sessions: the host model — victims, statements,
// records — is replicated on every rank; each rank ranks its own node range and
// the sorted lists are all-gathered and merged (the keys carry the global node
// index, so the merge is the one-GPU order).
// ---------------------------------------------------------------------------
struct EvictAction {
    Session& S;
    Framework F;
    using Stmt = Framework::Stmt;
    explicit EvictAction(Session& s) : S(s), F(s) {}

    static bool le_tol(const R3& a, const R3& b) {  // Resource.LessEqual on exact integers (Appendix A.2)
        return a.c - b.c < kMinCPU && a.m - b.m < kMinMem && a.g - b.g < kMinGPU;
    }
    static bool less_strict(const R3& a, const R3& b) { return a.c < b.c && a.m < b.m && a.g < b.g; }
    void check_evict_supported() {
        if (S.world != 1 && !S.xgfn && !S.comm)
            throw Error(KBHIP_EINVAL, "reclaim / preempt on a node-sharded session need an all-gather "
                                      "(kbhip_shard_connect_host with a gather, or kbhip_shard_connect_rccl)");
    }
    void build_node_tasks() {  // NodeInfo.Tasks of every node from the host model
        // two passes over the pod records (≈ 110 MB at C5) by pod ranges in parallel: each
        // pod's running-copy byte and per range the tasks per node; then each node's list
        // sized and the ranges' pods written at their offsets (pod order within a node kept)
        const int N = S.n_total, P = (int)S.pods.size();  // (every node: the host model is global on shards)
        const int nth = P < (1 << 16) ? 1 : host_threads();
        vector<vector<int32_t>> cnt(nth, vector<int32_t>(N, 0));
        F.run_copy.assign(P, 0);
        run_ranges(nth, [&](int r) {
            const auto [b, e] = range_of(P, r, nth);
            int32_t* c = cnt[r].data();
            for (int i = b; i < e; ++i) {
                const HPod& p = S.pods[i];
                F.run_copy[i] = (p.status == Running && !p.node_rel) ? 1 : 0;
                if (on_node_of(p) && p.status != Pending) c[p.node]++;
            }
        });
        S.node_tasks.resize(N);
        for (int n = 0; n < N; ++n) {
            int32_t base = 0;
            for (int r = 0; r < nth; ++r) { const int32_t k = cnt[r][n]; cnt[r][n] = base; base += k; }
            S.node_tasks[n].resize(base);
        }
        run_ranges(nth, [&](int r) {
            const auto [b, e] = range_of(P, r, nth);
            int32_t* c = cnt[r].data();
            for (int i = b; i < e; ++i) {
                const HPod& p = S.pods[i];
                if (on_node_of(p) && p.status != Pending) S.node_tasks[p.node][c[p.node]++] = i;
            }
        });
    }
    // The eviction actions' job scan (reclaim.go:60-90 / preempt.go:58-85 build their
    // preemptor lists from every job's Pending tasks): per job its Pending tasks in
    // TaskOrderFn order, and gang's readyTaskNum (gang.go:212-222) of every job, kept exact
    // from here on by set_status; job ranges in parallel
    void scan_jobs(vector<vector<int>>& pend) {
        const int J = (int)S.jobs.size();
        pend.assign(J, {});
        F.reset_ready_cache();
        const int nth = S.pods.size() < (1u << 16) ? 1 : host_threads();
        run_ranges(nth, [&](int r) {
            const auto [b, e] = range_of(J, r, nth);
            for (int jb = b; jb < e; ++jb) {
                int c = 0;
                for (int t : S.jobs[jb].tasks) {
                    const int st = S.pods[t].status;
                    c += Framework::gang_ready_status(st);
                    if (st == Pending) pend[jb].push_back(t);
                }
                F.ready_val[jb] = c;
                F.ready_ok[jb] = 1;
                if (pend[jb].size() > 1)
                    std::sort(pend[jb].begin(), pend[jb].end(), [this](int a, int b) { return F.task_less(a, b); });
            }
        });
    }

    // victims_of's per-call scratch keyed by job / queue slot, valid where stamp == the call's epoch
    vector<uint32_t> alloc_stamp;
    vector<F3> alloc_val;
    uint32_t epoch = 0;
    vector<int> cand, inter;
    vector<uint32_t> mark;  // pod -> epoch: membership in the plugin's answer (the tier intersection)
    // per action: the victim functions in tier order as codes (1 gang, 2 conformance, 3 drf,
    // 4 proportion; the tiers' plugin names compared once, not per node visited), and per pod
    // its job's queue and MinAvailable (read for every candidate of every visit)
    vector<vector<int>> vic_tiers;
    void compile_victims(bool preempt) {
        vic_tiers = victim_tier_codes(S, preempt);
        const int P = (int)S.pods.size();
        if ((int)S.pod_queue.size() != P || S.pod_queue_gen != S.model_gen) {  // once per session model
            S.pod_queue.assign(P, -1);
            S.pod_min.assign(P, 0);
            for (const HJob& J : S.jobs)  // job-major: a job's tasks are neighbouring pods
                for (int t : J.tasks) { S.pod_queue[t] = J.queue; S.pod_min[t] = J.min_avail; }
            S.pod_queue_gen = S.model_gen;
        }
    }
    // Session.Preemptable / Reclaimable (session_plugins.go:67-148): per tier the
    // intersection of the enabled plugins' victims; the first non-empty tier decides,
    // and once a plugin has answered later tiers only intersect further.
    // (setup below has run: vic_tiers, pod_queue / pod_min, run_copy and the ready cache are the action's)
    void victims_of(int evictor, const vector<int>& evictees, vector<int>& victims) {
        victims.clear();
        S.stats.evict_visits++;
        S.stats.evict_cands += (int64_t)evictees.size();
        if (evictees.empty()) return;  // every plugin returns nil for no candidates
        bool init = false;
        if (alloc_stamp.empty()) {
            const size_t J = S.jobs.size(), Q = S.queues.size();
            alloc_stamp.assign(std::max(J, Q), 0); alloc_val.assign(std::max(J, Q), F3{});
            mark.assign(S.pods.size(), 0);
        }
        for (auto& tier : vic_tiers) {
            for (int code : tier) {
                cand.clear();
                if (code == 1) {  // gang.go:107-129
                    for (int e : evictees) {
                        const int jb = S.pods[e].job;
                        if (!F.ready_ok[jb]) {  // readyTaskNum (gang.go:212-222)
                            int c = 0;
                            for (int t : S.jobs[jb].tasks) c += Framework::gang_ready_status(S.pods[t].status);
                            F.ready_ok[jb] = 1;
                            F.ready_val[jb] = c;
                        }
                        const int mn = S.pod_min[e];
                        if (mn <= F.ready_val[jb] - 1 || mn == 1) cand.push_back(e);
                    }
                } else if (code == 2) {  // conformance.go:37-56
                    for (int e : evictees) if (!S.pods[e].critical) cand.push_back(e);
                } else if (code == 3) {  // drf.go:84-109
                    const HPod& pr = S.pods[evictor];
                    F3 la = S.jobs[pr.job].drf_alloc;
                    la.add(pr.req);
                    const double ls = F.drf_share_of(la);
                    const uint32_t ea = ++epoch;
                    for (int e : evictees) {
                        const int jb = S.pods[e].job;
                        if (alloc_stamp[jb] != ea) { alloc_stamp[jb] = ea; alloc_val[jb] = S.jobs[jb].drf_alloc; }
                        alloc_val[jb].sub(S.pods[e].req);
                        const double rs = F.drf_share_of(alloc_val[jb]);
                        if (ls < rs || std::fabs(ls - rs) <= 0.000001) cand.push_back(e);  // shareDelta (drf.go:29)
                    }
                } else if (code == 4) {  // proportion.go:159-183
                    const uint32_t ea = ++epoch;
                    for (int e : evictees) {
                        const int qi = S.pod_queue[e];
                        const HQueue& q = S.queues[qi];
                        if (alloc_stamp[qi] != ea) { alloc_stamp[qi] = ea; alloc_val[qi] = q.allocated; }
                        F3 rq;
                        rq.add(S.pods[e].req);
                        if (alloc_val[qi].less(rq)) continue;
                        alloc_val[qi].sub(S.pods[e].req);
                        if (q.deserved.less_equal(alloc_val[qi])) cand.push_back(e);
                    }
                }
                if (!init) {
                    victims = cand;
                    init = true;
                } else {  // victims in their order, kept where the plugin also answered them
                    const uint32_t em = ++epoch;
                    for (int c : cand) mark[c] = em;
                    inter.clear();
                    for (int v : victims)
                        if (mark[v] == em) inter.push_back(v);
                    victims.swap(inter);
                }
            }
            if (!victims.empty()) return;
        }
    }

    // The walks read the records of every task on each visited node (run copy, queue,
    // MinAvailable, job, request) and evict most candidates (C5: ≈ 2.4 M candidates and
    // ≈ 720 k evictions per reclaim, pods scattered over 160 MB of records): the next
    // nodes' records are prefetched while one node is visited (the order is known), their
    // jobs one visit ahead (the job index is in the pod record fetched before).
    static constexpr int kPrefetchAhead = 3;
    void prefetch_pods(int n) {
        for (int t : S.node_tasks[n]) {
            const char* pp = reinterpret_cast<const char*>(&S.pods[t]);
            for (size_t o = 0; o < sizeof(HPod); o += 64) __builtin_prefetch(pp + o);
            __builtin_prefetch(pp + sizeof(HPod) - 1);
            __builtin_prefetch(&F.run_copy[t]);
            __builtin_prefetch(&S.pod_queue[t]);
            __builtin_prefetch(&S.pod_min[t]);
        }
    }
    void prefetch_jobs(int n) {
        for (int t : S.node_tasks[n]) {
            const int jb = S.pods[t].job;
            if (jb < 0) continue;
            const char* jp = reinterpret_cast<const char*>(&S.jobs[jb]);
            for (size_t o = 0; o < sizeof(HJob); o += 64) __builtin_prefetch(jp + o);
            __builtin_prefetch(jp + sizeof(HJob) - 1);
            __builtin_prefetch(&F.ready_val[jb]);
        }
    }
    // visit oi of a walk: the records the next visits read
    void prefetch_ahead(const vector<int>& order, int oi) {
        const int no = (int)order.size();
        if (oi == 0)
            for (int i = 0; i < std::min(no, kPrefetchAhead); ++i) prefetch_pods(order[i]);
        if (oi + kPrefetchAhead < no) prefetch_pods(order[oi + kPrefetchAhead]);
        if (oi + 1 < no) prefetch_jobs(order[oi + 1]);
    }
    // preempt() (preempt.go:259-353); filter over the node's task copies
    template <typename Filter>
    bool preempt_one(Stmt& st, int pi, Filter keep) {
        const HPod& pr = S.pods[pi];
        if (pr.cls < 0) throw Error(KBHIP_EUNSUPPORTED, "preemptor without a task class");
        vector<int> order, cands, victims;
        rank_nodes(S, pr.cls, true, order);
        const int no = (int)order.size();
        for (int oi = 0; oi < no; ++oi) {
            const int n = order[oi];
            prefetch_ahead(order, oi);
            cands.clear();
            for (int t : S.node_tasks[n]) if (keep(t)) cands.push_back(t);
            victims_of(pi, cands, victims);
            if (victims.empty()) continue;  // validateVictims (:355-370)
            R3 all, resreq = pr.ireq, got;
            for (int v : victims) { all.c += S.pods[v].req.c; all.m += S.pods[v].req.m; all.g += S.pods[v].req.g; }
            if (less_strict(all, resreq)) continue;
            for (int v : victims) {
                const R3 vr = S.pods[v].req;
                F.evict_in_session(v);
                st.ops.emplace_back(0, v);
                got.c += vr.c; got.m += vr.m; got.g += vr.g;
                if (le_tol(resreq, vr)) break;
                resreq.c -= vr.c; resreq.m -= vr.m; resreq.g -= vr.g;
            }
            if (le_tol(pr.ireq, got)) {
                F.pipeline(pi, n);
                st.ops.emplace_back(1, pi);
                return true;
            }
        }
        return false;
    }
#ifdef KBHIP_WALK_PROF
    uint64_t wp_acc[3] = {0, 0, 0}, wp_last = 0;
    int wp_ph = -1;
    void wp_mark(int ph) {
        const uint64_t t = __builtin_ia32_rdtsc();
        if (wp_ph >= 0) wp_acc[wp_ph] += t - wp_last;
        wp_last = t;
        wp_ph = ph;
    }
#endif
    // host wall time of an eviction action minus its node rankings (stats.evict_walk_s)
    struct WalkTimer {
        Session& S;
        Clock::time_point t0;
        double rank0;
        explicit WalkTimer(Session& s) : S(s), t0(Clock::now()), rank0(s.stats.evict_rank_s) {}
        void setup_done() { S.stats.evict_setup_s += seconds_since(t0); }
        ~WalkTimer() { S.stats.evict_walk_s += seconds_since(t0) - (S.stats.evict_rank_s - rank0); }
    };

    // What both actions start with (reclaim.go:44-90 / preempt.go:46-85): the plugins open,
    // NodeInfo.Tasks, the victim functions, and per queue the jobs with Pending tasks as a
    // JobOrderFn heap, each with its Pending tasks in TaskOrderFn order.  on_job(jb, pending)
    // runs for every job in order, before the job is queued.
    std::map<int, GoHeap<JobLess>> preemptors;
    std::unordered_map<int, std::pair<vector<int>, size_t>> ptasks;  // job -> (tasks, cursor)
    template <typename OnJob>
    void setup(bool preempt, OnJob on_job) {
        F.reset_ready_cache();
        F.compile_orders();
        F.open_plugins();
        check_evict_supported();
        build_node_tasks();
        compile_victims(preempt);
        vector<vector<int>> pends;
        scan_jobs(pends);
        for (int jb = 0; jb < (int)S.jobs.size(); ++jb) {
            const int q = S.jobs[jb].queue;
            vector<int>& pend = pends[jb];
            on_job(jb, !pend.empty());
            if (pend.empty()) continue;
            auto it = preemptors.find(q);
            if (it == preemptors.end()) it = preemptors.emplace(q, GoHeap<JobLess>(JobLess{&F})).first;
            it->second.push(jb);
            ptasks[jb] = {std::move(pend), 0};
        }
    }
    void preempt_action() {  // preempt.go:43-255
        WalkTimer wt(S);
        vector<int> under;
        vector<char> seen(S.queues.size(), 0);
        setup(true, [&](int jb, bool pending) {
            seen[S.jobs[jb].queue] = 1;
            if (pending) under.push_back(jb);
        });
        wt.setup_done();
        Stmt st;
        for (int qi = 0; qi < (int)S.queues.size(); ++qi) {  // map `queues`, pinned to queue order
            if (!seen[qi]) continue;
            for (;;) {  // between jobs of the queue (:87-149)
                auto pit = preemptors.find(qi);
                if (pit == preemptors.end() || pit->second.empty()) break;
                const int pj = pit->second.pop();
                bool assigned = false;
                auto& tq = ptasks[pj];
                for (;;) {
                    if (tq.second >= tq.first.size()) break;
                    const int pt = tq.first[tq.second++];
                    const int pq = S.jobs[pj].queue, ptj = S.pods[pt].job;
                    if (preempt_one(st, pt, [&](int t) {
                            const HPod& p = S.pods[t];
                            return F.run_copy[t] && p.job >= 0 && S.pod_queue[t] == pq && ptj != p.job;
                        }))
                        assigned = true;
                    if (F.job_ready(S.jobs[pj])) {
                        F.commit(st);
                        break;
                    }
                }
                if (!F.job_ready(S.jobs[pj])) {
                    F.discard(st);
                    continue;
                }
                st.ops.clear();  // neither committed nor discarded: the session keeps the operations
                if (assigned) pit->second.push(pj);
            }
            for (int jb : under) {  // between tasks of a job (:151-181)
                auto& tq = ptasks[jb];
                for (;;) {
                    if (tq.second >= tq.first.size()) break;
                    const int pt = tq.first[tq.second++];
                    Stmt s2;
                    const int ptj = S.pods[pt].job;
                    const bool assigned = preempt_one(s2, pt, [&](int t) {
                        return F.run_copy[t] && ptj == S.pods[t].job;
                    });
                    F.commit(s2);
                    if (!assigned) break;
                }
            }
        }
        F.flush_evictions();
    }
    void reclaim_action() {  // reclaim.go:41-196
        WalkTimer wt(S);
        GoHeap<QueueLess> queues(QueueLess{&F});
        vector<char> qseen(S.queues.size(), 0);
        setup(false, [&](int jb, bool) {
            const int q = S.jobs[jb].queue;
            if (!qseen[q]) { qseen[q] = 1; queues.push(q); }
        });
        wt.setup_done();
        vector<int> order, cands, victims;
        while (!queues.empty()) {
            const int qi = queues.pop();
            if (F.overused(qi)) continue;
            auto pit = preemptors.find(qi);
            if (pit == preemptors.end() || pit->second.empty()) continue;
            const int jb = pit->second.pop();
            auto& tq = ptasks[jb];
            if (tq.second >= tq.first.size()) continue;
            const int pt = tq.first[tq.second++];
            const HPod& pr = S.pods[pt];
            if (pr.cls < 0) throw Error(KBHIP_EUNSUPPORTED, "reclaimer without a task class");
            const int jq = S.jobs[jb].queue;
            bool assigned = false;
            rank_nodes(S, pr.cls, false, order);
            const int no = (int)order.size();
            for (int oi = 0; oi < no; ++oi) {
                const int n = order[oi];
                WP_MARK(0);
                prefetch_ahead(order, oi);
                cands.clear();
                for (int t : S.node_tasks[n])
                    if (F.run_copy[t] && S.pod_queue[t] >= 0 && S.pod_queue[t] != jq) cands.push_back(t);
                WP_MARK(1);
                victims_of(pt, cands, victims);
                WP_MARK(2);
                if (victims.empty()) continue;
                R3 all, resreq = pr.ireq, got;
                for (int v : victims) { all.c += S.pods[v].req.c; all.m += S.pods[v].req.m; all.g += S.pods[v].req.g; }
                if (less_strict(all, resreq)) continue;
                for (int v : victims) {
                    const R3 vr = S.pods[v].req;
                    S.log.emplace_back(v, S.pods[v].node, KBHIP_EVICTED);  // ssn.Evict: cache.Evict first
                    F.evict_in_session(v);
                    got.c += vr.c; got.m += vr.m; got.g += vr.g;
                    if (le_tol(resreq, vr)) break;
                    resreq.c -= vr.c; resreq.m -= vr.m; resreq.g -= vr.g;
                }
                if (le_tol(pr.ireq, got)) {
                    F.pipeline(pt, n);
                    S.log.emplace_back(pt, n, KBHIP_PIPELINED);
                    S.stats.placed++;
                    assigned = true;
                    break;
                }
            }
            if (assigned) queues.push(qi);
        }
        WP_MARK(0);
        WP_REPORT("reclaim");
        F.flush_evictions();
        HIPCHK(hipStreamSynchronize(S.stream));
    }
};

void evict_run(Session& S, bool preempt) {
    S.fit_task = -1;
    vict_stale(S);
    EvictAction a(S);
    if (preempt) a.preempt_action();
    else a.reclaim_action();
}

}  // namespace kbhip

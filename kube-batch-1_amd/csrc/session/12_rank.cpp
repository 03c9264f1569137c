// kbhip session, part 12: the ranked node walk of one task (kbhip_rank_nodes), the victim-candidate table and
// the walk pruned by it (kbhip_rank_victim_nodes)
#include "framework.h"

namespace kbhip {

namespace {

constexpr size_t kVictMaxBytes = (size_t)512 << 20;  // the table's design limit (include/kbhip.h)

size_t vict_tab_words(const Session& S) { return (S.queues.size() + 1) * 4 * (size_t)S.nc.npad; }

// The table from the host model and its upload: a parallel pass over the pods
// by pod ranges (as EvictAction::build_node_tasks), each range into a table of
// its own; the ranges' tables are then summed by node ranges, which also
// gives the total row.  The ranges are as many as keep the partial tables
// within the table's own size limit.
void vict_build(Session& S) {
    const size_t Q = S.queues.size(), np = (size_t)S.nc.npad, words = vict_tab_words(S), bytes = words * sizeof(int64_t);
    vict_check_size(S);
    const int P = (int)S.pods.size(), N = S.n_total;
    int nth = P < (1 << 16) ? 1 : host_threads();
    nth = (int)std::max<size_t>(1, std::min<size_t>((size_t)nth, kVictMaxBytes / std::max<size_t>(bytes, 1)));
    S.vict_tab.assign(words, 0);
    vector<vector<int64_t>> part(nth - 1);
    run_ranges(nth, [&](int r) {
        if (r > 0) part[r - 1].assign(words, 0);
        int64_t* tab = r > 0 ? part[r - 1].data() : S.vict_tab.data();
        const auto [b, e] = range_of(P, r, nth);
        for (int i = b; i < e; ++i) {
            const HPod& p = S.pods[i];
            if (!vict_candidate(S, p)) continue;
            const int q = S.jobs[p.job].queue;
            if (q < 0 || q >= (int)Q) continue;
            int64_t* row = tab + (size_t)q * 4 * np + p.node;
            row[0] += 1; row[np] += p.req.c; row[2 * np] += p.req.m; row[3 * np] += p.req.g;
        }
    });
    const int nsum = nth > 1 || N >= (1 << 16) ? std::min(host_threads(), std::max(1, N / 4096)) : 1;
    run_ranges(nsum, [&](int r) {
        const auto [b, e] = range_of(N, r, nsum);
        int64_t* tab = S.vict_tab.data();
        for (size_t qk = 0; qk < Q * 4; ++qk) {
            int64_t* row = tab + qk * np;
            for (const auto& pt : part) {
                const int64_t* src = pt.data() + qk * np;
                for (int n = b; n < e; ++n) row[n] += src[n];
            }
            int64_t* tot = tab + (Q * 4 + qk % 4) * np;
            for (int n = b; n < e; ++n) tot[n] += row[n];
        }
    });
    if (S.b_vict.cap < bytes || !S.b_vict.p) S.b_vict.alloc<int64_t>(words);
    HIPCHK(hipMemcpyAsync(S.b_vict.p, S.vict_tab.data(), bytes, hipMemcpyHostToDevice, S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));  // the pageable source is read by then
    S.vict_live = true;
}

}  // namespace

void vict_check_size(const Session& S) {
    const size_t Q = S.queues.size(), np = (size_t)S.nc.npad, bytes = vict_tab_words(S) * sizeof(int64_t);
    if (bytes > kVictMaxBytes)
        throw Error(KBHIP_EUNSUPPORTED, "kbhip_rank_victim_nodes: the victim-candidate table of " + std::to_string(Q) +
                                            " queues x " + std::to_string(np) + " nodes takes " +
                                            std::to_string(bytes >> 20) + " MB, above the 512 MB limit");
}

void vict_compact_buffers(Session& S) {
    if (S.b_vict_keys.p) return;
    const int N = S.nc.n;
    S.b_vict_keys.alloc<uint64_t>(std::max(N, 1));
    S.b_vict_cands.alloc<int32_t>(std::max(N, 1));
    S.b_vict_blk.alloc<uint32_t>((size_t)vict_blocks(N) + 1);
}

bool vict_ensure(Session& S) {
    if (S.vict_live) return false;
    vict_build(S);
    return true;
}

// The candidate tasks of job jb per node: distinct nodes ascending, four sums each.
void vict_own_list(const Session& S, int jb, vector<int32_t>& node, vector<int64_t>& sum) {
    node.clear();
    sum.clear();
    vector<std::pair<int32_t, int32_t>> on;  // (node, pod)
    for (int t : S.jobs[jb].tasks)
        if (vict_candidate(S, S.pods[t])) on.emplace_back(S.pods[t].node, t);
    std::sort(on.begin(), on.end());
    for (const auto& [n, t] : on) {
        if (node.empty() || node.back() != n) {
            node.push_back(n);
            sum.insert(sum.end(), 4, 0);
        }
        int64_t* s = &sum[sum.size() - 4];
        const R3& r = S.pods[t].req;
        s[0] += 1; s[1] += r.c; s[2] += r.m; s[3] += r.g;
    }
}

// vict_cand of kbhip_heads.hip on the host copy: the candidate count of node n
int64_t vict_count_host(const Session& S, int mode, int q, const vector<int32_t>& own_node,
                        const vector<int64_t>& own_sum, int n) {
    const size_t np = (size_t)S.nc.npad, Q = S.queues.size();
    int64_t own = 0;
    if (mode != 1) {
        const auto it = std::lower_bound(own_node.begin(), own_node.end(), n);
        if (it != own_node.end() && *it == n) own = own_sum[4 * (size_t)(it - own_node.begin())];
    }
    if (mode == 3) return own;
    if (mode == 1) return S.vict_tab[Q * 4 * np + n] - S.vict_tab[(size_t)q * 4 * np + n];
    return S.vict_tab[(size_t)q * 4 * np + n] - own;
}

void vict_apply_evictions(Session& S, const vector<NodeOp>& ops) {
    const size_t np = (size_t)S.nc.npad, Q = S.queues.size();
    for (const NodeOp& o : ops) {
        if (o.kind != 0) continue;
        if (o.queue < 0 || o.queue >= (int)Q || o.node < 0 || o.node >= S.nc.npad) { S.vict_live = false; return; }
        for (size_t row : {(size_t)o.queue, Q}) {
            int64_t* p = S.vict_tab.data() + row * 4 * np + o.node;
            p[0] -= 1; p[np] -= o.req.c; p[2 * np] -= o.req.m; p[3 * np] -= o.req.g;
        }
    }
}

// The job's own list of a call in a victim mode other than OTHER_QUEUES, uploaded (sums, then nodes, in
// one copy: the previous call's copy ended with that call), and the call's VictArgs.
VictArgs vict_args(Session& S, const HPod& p, int mode, vector<int32_t>& own_node, vector<int64_t>& own_sum) {
    if (mode != KBHIP_VICTIMS_OTHER_QUEUES) vict_own_list(S, p.job, own_node, own_sum);
    const size_t own_n = own_node.size(), own_bytes = own_n * (4 * sizeof(int64_t) + sizeof(int32_t));
    if (own_n) {
        S.h_vict_own.fit(own_bytes, std::max<size_t>(2 * own_bytes, 4096));
        S.b_vict_own.grow(S.stream, own_bytes, std::max<size_t>(2 * own_bytes, 4096));
        uint8_t* const h_own = S.h_vict_own.as<uint8_t>();
        std::memcpy(h_own, own_sum.data(), own_n * 4 * sizeof(int64_t));
        std::memcpy(h_own + own_n * 4 * sizeof(int64_t), own_node.data(), own_n * sizeof(int32_t));
        HIPCHK(hipMemcpyAsync(S.b_vict_own.p, h_own, own_bytes, hipMemcpyHostToDevice, S.stream));
    }
    const uint8_t* d_own = (const uint8_t*)S.b_vict_own.p;
    return VictArgs{(const int64_t*)S.b_vict.p,
                    own_n ? (const int32_t*)(d_own + own_n * 4 * sizeof(int64_t)) : nullptr,
                    own_n ? (const int64_t*)d_own : nullptr,
                    S.nc.npad, (int32_t)S.queues.size(), S.jobs[p.job].queue, mode, (int32_t)own_n,
                    p.ireq.c, p.ireq.m, p.ireq.g};
}

// The head of the walk of class cls, enqueued: afterwards (in stream order) b_rank_head holds the kTopK
// best keys and the count.  Nothing is copied back or waited for.  bound != 0 (with v): the bounded sweep.
int rank_head_enqueue(Session& S, int cls, bool by_score, const VictArgs* v, uint64_t bound) {
    const TaskClass& c = S.classes[cls];
    int launches = 0;
    if (!S.b_rank_head.p) S.b_rank_head.alloc<uint64_t>(rank_head_words());
    ctrl_setup(S, 1, &cls, 0, 0, 0, 0, -1, 0);
    launches += 1;
    if (by_score && c.ipa_n > 0) {
        HIPCHK(launch_ipa_minmax(S.nc, S.tab, S.d_ctrl, 0, S.stream));
        launches += 1;
    }
    HIPCHK(launch_rank_head(S.conf, S.nc, S.tab, c, S.d_ctrl, by_score ? 1 : 0, v, (uint64_t*)S.b_rank_head.p,
                            S.stream, bound));
    return launches + 2;  // sweep + merge
}

// Entries [first, first + cap) of the walk order of task `pod` (by_score:
// preempt's SelectBestNode order, else reclaim's index order) and the number
// of nodes in it.  mode 0 (kbhip_rank_nodes): every node of the order.  mode
// KBHIP_VICTIMS_* (kbhip_rank_victim_nodes): without the nodes whose victim
// candidates of that mode are none, or together strictly short of the task's
// InitResreq in all three resources; the victim-candidate table is built
// unless it is live, the job's own list goes up, and the window's candidate
// counts come back.  The head of the walk (first + cap <= kTopK) is one fused
// top-kTopK sweep (launch_rank_head, filtered by the lane that evaluates the
// node: nothing of size N written, kTopK keys and the count copied back, the
// candidate counts of the returned nodes taken from the host copy of the
// table); anything else is the full device sort of the reclaim / preempt
// actions (rank_launch), followed in a victim mode by a stable compaction
// (launch_vict_compact), of which the count and then only the window asked
// for are copied.  Reads the session state and changes nothing but the
// table's liveness; nothing is kept for a later call.
int64_t rank_victim_nodes_abi(Session& S, int pod, bool by_score, int mode, int64_t first, int32_t* out_node,
                              int32_t* out_score, int32_t* out_cands, int64_t cap, int64_t* out_info) {
    const char* const api = mode ? "kbhip_rank_victim_nodes" : "kbhip_rank_nodes";
    const HPod& p = query_task(S, pod, string(api) + ": the task ", mode != 0, "task id ");
    query_begin(S, api);
    const int cls = p.cls, N = S.nc.n;
    const bool rebuilt = mode != 0 && vict_ensure(S);
    vector<int32_t> own_node;
    vector<int64_t> own_sum;
    VictArgs v{};
    if (mode != 0) {
        v = vict_args(S, p, mode, own_node, own_sum);
        S.h_vict_out.fit(((size_t)N + 2) * sizeof(int32_t));
    }
    int32_t* const h_out = S.h_vict_out.as<int32_t>();  // victim modes: [0] the kept count, then the window's counts
    const uint64_t* keys = nullptr;  // entries [first, first + n_keys) of the order, on the host
    int64_t total = 0, n_keys = 0, launches = flush_tables(S);  // evictions / unevicts so far change pod-affinity predicates
    const bool head = cap > 0 && first <= kTopK && cap <= kTopK - first;
    if (head) {
        S.h_rank_head.fit((size_t)(kTopK + 1) * sizeof(uint64_t));
        uint64_t* const h_head = S.h_rank_head.as<uint64_t>();
        launches += rank_head_enqueue(S, cls, by_score, mode ? &v : nullptr);
        HIPCHK(hipMemcpyAsync(h_head, S.b_rank_head.p, (size_t)(kTopK + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost,
                              S.stream));
        HIPCHK(hipStreamSynchronize(S.stream));
        total = (int64_t)h_head[kTopK];
        n_keys = first < total ? std::min(cap, total - first) : 0;
        keys = h_head + first;
        for (int64_t i = 0; mode != 0 && i < n_keys; ++i)
            h_out[1 + i] = (int32_t)vict_count_host(S, mode, v.q, own_node, own_sum, key_idx(keys[i]));
        if (mode == 0) S.stats.rank_heads++;
    } else {
        launches += rank_launch(S, cls, by_score);
        const uint64_t* d_keys = (const uint64_t*)S.b_rank_sorted.p;  // the order the window is read from
        uint64_t* const h_rank = S.h_rank.as<uint64_t>();
        if (mode != 0) {
            vict_compact_buffers(S);
            HIPCHK(launch_vict_compact(d_keys, (const uint32_t*)S.b_rank_cnt.p, N, v, (uint32_t*)S.b_vict_blk.p,
                                       (uint64_t*)S.b_vict_keys.p, (int32_t*)S.b_vict_cands.p, S.stream));
            launches += 3;
            d_keys = (const uint64_t*)S.b_vict_keys.p;
            HIPCHK(hipMemcpyAsync(h_out, (const uint32_t*)S.b_vict_blk.p + vict_blocks(N), sizeof(uint32_t),
                                  hipMemcpyDeviceToHost, S.stream));
        }
        HIPCHK(hipMemcpyAsync(h_rank, S.b_rank_cnt.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, S.stream));
        HIPCHK(hipStreamSynchronize(S.stream));
        if (h_rank[0] >> 32)  // (the text names the call without its "kbhip_")
            throw Error(KBHIP_EDEVICE, string(api + 6) + ": node score outside the class score range");
        total = mode != 0 ? (int64_t)(uint32_t)h_out[0] : (int64_t)(uint32_t)h_rank[0];
        n_keys = first < total ? std::min(cap, total - first) : 0;
        if (n_keys > 0) {
            HIPCHK(hipMemcpyAsync(h_rank + 1, d_keys + first, (size_t)n_keys * sizeof(uint64_t), hipMemcpyDeviceToHost,
                                  S.stream));
            if (mode != 0)
                HIPCHK(hipMemcpyAsync(h_out + 1, (const int32_t*)S.b_vict_cands.p + first,
                                      (size_t)n_keys * sizeof(int32_t), hipMemcpyDeviceToHost, S.stream));
            HIPCHK(hipStreamSynchronize(S.stream));
        }
        keys = h_rank + 1;
        if (mode == 0) S.stats.rank_fulls++;
    }
    for (int64_t i = 0; i < n_keys; ++i) {
        out_node[i] = key_idx(keys[i]);
        if (out_score) out_score[i] = by_score ? key_score(keys[i]) : 0;
        if (out_cands) out_cands[i] = h_out[1 + i];
    }
    if (out_info) {
        out_info[0] = head ? 1 : 0;
        out_info[1] = rebuilt ? 1 : 0;
        out_info[2] = launches;
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
        if (first < 0 || cap < 0 || (cap > 0 && !out_node))
            throw kbhip::Error(KBHIP_EINVAL, "kbhip_rank_nodes: negative first or cap, or null out_node with cap > 0");
        check_by_score("kbhip_rank_nodes", by_score);
        return kbhip::rank_victim_nodes_abi(kbhip::device_session(s), task_id, by_score != 0, 0, first, out_node,
                                            out_score, nullptr, cap, nullptr);
    })
}

int64_t kbhip_rank_victim_nodes(kb_session* s, int32_t task_id, int32_t by_score, int32_t victims, int64_t first,
                                int32_t* out_node, int32_t* out_score, int32_t* out_cands, int64_t cap,
                                int64_t* out_info) {
    ABI_GUARD_S(s, {
        if (first < 0 || cap < 0 || (cap > 0 && !out_node))
            throw kbhip::Error(KBHIP_EINVAL,
                               "kbhip_rank_victim_nodes: negative first or cap, or null out_node with cap > 0");
        check_by_score("kbhip_rank_victim_nodes", by_score);
        check_victims("kbhip_rank_victim_nodes", victims);
        return kbhip::rank_victim_nodes_abi(kbhip::device_session(s), task_id, by_score != 0, victims, first, out_node,
                                            out_score, out_cands, cap, out_info);
    })
}

}  // extern "C"

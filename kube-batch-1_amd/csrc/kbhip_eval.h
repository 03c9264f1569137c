// kbhip_eval.h — the per-node evaluation and commit arithmetic of the
// placement kernels: predicates, scores, fit, selection key, node-row and
// pod-affinity commits.  __host__ __device__ so that the same functions the
// kernels run can also be replayed on the host by the test-only entry point
// kbhip_debug_replay (checked against the CPU oracle without a GPU); the
// placement path itself runs them on the device only.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "kbhip_internal.h"

#define KBHIP_HD __host__ __device__ __forceinline__

namespace kbhip {

// ---------------------------------------------------------------------------
// node row + evaluation
// ---------------------------------------------------------------------------
struct Row {  // the dynamic part of a node's state
    int64_t idle_cpu, idle_mem, idle_gpu, rel_cpu, rel_mem, rel_gpu, bf_cpu, bf_mem, bf_gpu;
    int64_t acpu, amem, nzc, nzm;
    int32_t pods, maxtasks;
};

// Node-array shards, batched pops: what each shard contributes
// to a pop — its top-64 keys with the rows the placement needs — exchanged by
// one all-gather; every shard then places the chunk on the merged list.
struct ShardCand {
    uint64_t key;    // 64-bit selection key (global node index), 0 = none
    int32_t node;    // global node index, -1 = none
    int32_t na;      // static node-affinity weight of the node for the class
    Row row;
    uint64_t pw[4];  // host-port words
};
struct ShardMsg {
    uint32_t fit[4];  // the shard's sweep FitDelta counts (walk nodes, cpu, memory, GPU)
    uint32_t pad[2];
    ShardCand c[kTopK];
};
static_assert(sizeof(ShardCand) % 8 == 0 && sizeof(ShardMsg) % 8 == 0, "mailbox copies move 8-byte words");

// Peer mailboxes (kbhip_shard_connect_mailbox): every rank's device holds one;
// for each batched pop every shard writes its ShardMsg straight into every
// rank's mailbox (its own included) — over xGMI when the ranks are on
// different GPUs — and then a self-tagged flag word {pop sequence number}
// per destination; the placement kernel of each rank waits for the W flags of
// its own mailbox.  Two slots (sequence parity): a shard can run at most one
// pop ahead of the slowest, whose reads of the other slot are then done.
constexpr int kMaxWorld = 16;
constexpr int kMboxSlots = 2;
struct Mailbox {
    uint64_t flag[kMboxSlots][kMaxWorld][16];  // [slot][source][0]: sequence number (a 128-B line each)
    ShardMsg msg[kMboxSlots][kMaxWorld];
};
struct MboxArgs {                 // kernel argument of a shard's sweep (world 0: no mailbox)
    Mailbox* dst[kMaxWorld];      // every rank's mailbox as mapped in this process
    int32_t rank, world;
    uint32_t seq;
    int32_t pad;
};

// Host-port words of a class: its window of the port columns (TaskClass::pw_lo).
KBHIP_HD int port_win(const TaskClass& c, const NodeCols& nc) {
    const int k = nc.port_words - c.pw_lo;
    return k < kPortWin ? k : kPortWin;
}
KBHIP_HD int64_t port_at(const TaskClass& c, const NodeCols& nc, int w, int n) {
    return (int64_t)(c.pw_lo + w) * nc.npad + n;
}

KBHIP_HD Row load_row(const NodeCols& nc, int n) {
    Row r;
    r.idle_cpu = nc.idle_cpu[n]; r.idle_mem = nc.idle_mem[n]; r.idle_gpu = nc.idle_gpu[n];
    r.rel_cpu = nc.rel_cpu[n]; r.rel_mem = nc.rel_mem[n]; r.rel_gpu = nc.rel_gpu[n];
    r.bf_cpu = nc.bf_cpu[n]; r.bf_mem = nc.bf_mem[n]; r.bf_gpu = nc.bf_gpu[n];
    r.acpu = nc.acpu[n]; r.amem = nc.amem[n]; r.nzc = nc.nzc[n]; r.nzm = nc.nzm[n];
    r.pods = nc.pods[n]; r.maxtasks = nc.maxtasks[n];
    return r;
}

// The columns PredicateFn + NodeOrderFn read of a node (41 B: no Idle /
// Releasing / Backfilled column), loaded a step ahead by the sweeps that
// prefetch (k_score_sweep_gs, rank_bucket, rank_head).
struct SweepIn {
    int64_t acpu, amem, nzc, nzm;
    int32_t pods, maxtasks;
    uint8_t fl;
};
__device__ __forceinline__ SweepIn sweep_in(const NodeCols& nc, int n) {
    SweepIn v;
    v.acpu = nc.acpu[n]; v.amem = nc.amem[n]; v.nzc = nc.nzc[n]; v.nzm = nc.nzm[n];
    v.pods = nc.pods[n]; v.maxtasks = nc.maxtasks[n]; v.fl = nc.flags[n];
    return v;
}

KBHIP_HD bool req_match(const DevTables& t, const NodeCols& nc, const Req& r, int n) {
    // labels.Requirement.Matches (apimachinery/pkg/labels/selector.go:192-236)
    switch (r.op) {
        case OP_NAME_IN: return n + nc.base == r.val_off;      // field selector metadata.name
        case OP_NAME_NOTIN: return n + nc.base != r.val_off;
        case OP_FALSE: return false;
        default: break;
    }
    const int v = nc.labels[(int64_t)r.key * nc.npad + n];
    switch (r.op) {
        case OP_IN:
        case OP_NOTIN: {
            bool hit = false;
            for (int i = 0; i < r.nvals; ++i) hit |= t.vals[r.val_off + i] == v;
            if (r.op == OP_IN) return v >= 0 && hit;
            return v < 0 || !hit;
        }
        case OP_EXISTS: return v >= 0;
        case OP_DNE: return v < 0;
        case OP_GT: return v >= 0 && t.valok[v] && t.valint[v] > r.rhs;
        case OP_LT: return v >= 0 && t.valok[v] && t.valint[v] < r.rhs;
    }
    return false;
}

KBHIP_HD bool term_match(const DevTables& t, const NodeCols& nc, const Term& tm, int n) {
    bool ok = true;
    for (int i = 0; i < tm.req_n; ++i) ok = ok && req_match(t, nc, t.reqs[tm.req_off + i], n);
    return ok;
}

// The static part of the predicates: selector / node affinity, unschedulable,
// taints.  Does not change while a session runs.
KBHIP_HD bool static_pred_f(const Conf& cf, const TaskClass& c, const DevTables& t, const NodeCols& nc, int n,
                            uint8_t flags) {  // flags = nc.flags[n], loaded by the caller with the row
    if (!cf.pred_on) return true;
    if (c.pred_err) return false;
    if (flags & 1) return false;                                         // predicates.go:107-112
    for (int w = 0; w < nc.taint_words; ++w)                             // helper/helpers.go:425-440
        if (nc.taints[(int64_t)w * nc.npad + n] & ~t.masks[c.tol_off + w]) return false;
    if (c.nsel_term >= 0 && !term_match(t, nc, t.terms[c.nsel_term], n)) return false;  // predicates.go:809-814
    if (c.req_term_n >= 0) {                                             // predicates.go:826-846
        bool any = false;
        for (int i = 0; i < c.req_term_n; ++i) any = any || term_match(t, nc, t.terms[c.req_term_off + i], n);
        if (!any) return false;
    }
    return true;
}
KBHIP_HD bool static_pred(const Conf& cf, const TaskClass& c, const DevTables& t, const NodeCols& nc, int n) {
    return static_pred_f(cf, c, t, nc, n, cf.pred_on ? nc.flags[n] : (uint8_t)0);
}

// Static part of the node-affinity priority: the summed weights of the
// preferred terms the node matches (node_affinity.go:34-74).  Node labels do
// not change in a session, so callers compute it once per node.
KBHIP_HD int32_t na_weight(const TaskClass& c, const DevTables& t, const NodeCols& nc, int n) {
    int32_t na = 0;
    for (int i = 0; i < c.pref_term_n; ++i) {
        const Term& tm = t.terms[c.pref_term_off + i];
        if (term_match(t, nc, tm, n)) na += tm.weight;
    }
    return na;
}

// least_requested.go:44-53: ((cap - req) * 10) / cap for 0 <= req <= cap,
// cap > 0 (a quotient in [0, 10]), given f = the correctly rounded req / cap
// (BRA's fraction, computed anyway): 10 - 10 f is within 1e-14 of the exact
// quotient, so its truncation is off by at most one and the two exact
// integer steps fix it — one IEEE division per resource instead of two.
KBHIP_HD int64_t lr_score_f(int64_t req, int64_t cap, double f) {
    if (cap == 0 || req > cap) return 0;
    const int64_t num = (cap - req) * 10;
    int64_t q = (int64_t)(10.0 - 10.0 * f);
    q = q < 0 ? 0 : (q > 10 ? 10 : q);
    if (q * cap > num) --q;
    if ((q + 1) * cap <= num) ++q;
    return q;
}

// Score of a feasible node (nodeorder.go:281-313): LR and BRA from the row,
// na = na_weight(), ipa = the normalised inter-pod affinity score (0 for
// classes without inter-pod terms).
KBHIP_HD int32_t node_score(const Conf& cf, const TaskClass& c, const Row& r, int32_t na, int32_t ipa) {
    if (!cf.score_mult) return 0;
    const int64_t rc = c.nz_cpu + r.nzc, rm = c.nz_mem + r.nzm;
    // balanced_resource_allocation.go:41-77, IEEE double, no contraction
    const double cpuF = r.acpu == 0 ? 1.0 : (double)rc / (double)r.acpu;
    const double memF = r.amem == 0 ? 1.0 : (double)rm / (double)r.amem;
    const int64_t lr = (lr_score_f(rc, r.acpu, cpuF) + lr_score_f(rm, r.amem, memF)) / 2;
    int64_t bra = 0;
    if (!(cpuF >= 1.0 || memF >= 1.0)) {
        const double d = fabs(cpuF - memF);
        const double one_minus = 1.0 - d;
        bra = (int64_t)(one_minus * 10.0);
    }
    return ((int32_t)lr * cf.w_lr + (int32_t)bra * cf.w_bra + na * cf.w_na + ipa * cf.w_pa) * cf.score_mult;
}

// allocate.go:153 (InitResreq <= Idle + Backfilled) and :173 (<= Releasing),
// Resource.LessEqual's epsilon form (resource_info.go:164-168).
KBHIP_HD bool fit_idle(const TaskClass& c, const Row& r) {
    return c.ireq_cpu - (r.idle_cpu + r.bf_cpu) < kMinCPU && c.ireq_mem - (r.idle_mem + r.bf_mem) < kMinMem &&
           c.ireq_gpu - (r.idle_gpu + r.bf_gpu) < kMinGPU;
}
KBHIP_HD bool fit_releasing(const TaskClass& c, const Row& r) {
    return c.ireq_cpu - r.rel_cpu < kMinCPU && c.ireq_mem - r.rel_mem < kMinMem && c.ireq_gpu - r.rel_gpu < kMinGPU;
}

// Dynamic predicates (pod count, host ports) + fit + key, given the row.
// passed: predicate pass and score computed (the node is in the walk).
KBHIP_HD uint64_t dyn_key(const Conf& cf, const TaskClass& c, const DevTables& t,
                                            const NodeCols& nc, const Row& r, const uint64_t* portw,
                                            int n, bool stat_ok, int32_t na, int32_t* score_out, bool* passed,
                                            int32_t ipa = 0) {
    bool ok = stat_ok;
    if (cf.pred_on) {
        if (r.maxtasks <= r.pods) ok = false;                            // predicates.go:127
        if (c.has_ports)                                                 // host_ports.go:96-125
            for (int w = 0; w < 4; ++w) if (w < port_win(c, nc))
                if (portw[w] & t.masks[c.pconf_off + w]) ok = false;
    }
    if (ok && c.score_err) ok = false;  // NodeOrderFn error drops the node (allocate.go:141-145)
    *passed = ok;
    if (!ok) return 0;
    const int32_t s = node_score(cf, c, r, na, ipa);
    *score_out = s;
    const bool fit_acc = fit_idle(c, r), fit_rel = fit_releasing(c, r);
    if (!fit_acc && !fit_rel) return 0;
    return pack_key(s, n + nc.base, fit_acc ? 0 : 1);
}

// NodesFitDelta of a task that found no node (allocate.go:164-167: every node
// of the walk gets Idle.FitDelta(Resreq), resource_info.go:134-147), counted
// the way JobInfo.FitError reads it (job_info.go:343-372): bit 0 = the node is
// in the walk (predicates pass, no NodeOrderFn error), bits 1..3 = its delta
// is negative for cpu / memory / GPU.  The walk visits every such node, so
// Idle is taken after GetAccessibleResource's visit (Idle += Backfilled).
KBHIP_HD uint32_t fit_bits(const TaskClass& c, const Row& r, bool passed) {
    if (!passed) return 0;
    const int64_t ic = r.idle_cpu + r.bf_cpu, im = r.idle_mem + r.bf_mem, ig = r.idle_gpu + r.bf_gpu;
    const int64_t dc = c.req_cpu > 0 ? ic - (c.req_cpu + kMinCPU) : ic;
    const int64_t dm = c.req_mem > 0 ? im - (c.req_mem + kMinMem) : im;
    const int64_t dg = c.req_gpu > 0 ? ig - (c.req_gpu + kMinGPU) : ig;
    return 1u | (dc < 0 ? 2u : 0u) | (dm < 0 ? 4u : 0u) | (dg < 0 ? 8u : 0u);
}

KBHIP_HD uint64_t eval_node(const Conf& cf, const TaskClass& c, const DevTables& t,
                                              const NodeCols& nc, int n, int32_t* score_out, bool* passed,
                                              uint32_t* fit = nullptr) {
    // the flags, row and port words first: their loads do not depend on the
    // predicates' early exits, so they share one memory round trip instead of
    // following each other
    const uint8_t fl = nc.flags[n];
    const Row r = load_row(nc, n);
    uint64_t pw[4] = {0, 0, 0, 0};
    if (c.has_ports)
        for (int w = 0; w < 4; ++w) if (w < port_win(c, nc)) pw[w] = nc.ports[port_at(c, nc, w, n)];
    const bool st = static_pred_f(cf, c, t, nc, n, fl);
    const int32_t na = (st && cf.score_mult) ? na_weight(c, t, nc, n) : 0;
    const uint64_t k = dyn_key(cf, c, t, nc, r, pw, n, st, na, score_out, passed);
    if (fit) *fit = fit_bits(c, r, *passed);
    return k;
}

// The batched sweep of a session with Backfilled nodes (placement 6): a node
// in the walk that cannot fit yet stays a candidate when it carries Backfilled
// resources — each visit of a walk adds them to its Idle (GetAccessibleResource,
// node_info.go:209-211), so it may fit a later task of the pop — keyed by its
// walk position (score, index; kind bit 0).
KBHIP_HD uint64_t eval_node_walk(const Conf& cf, const TaskClass& c, const DevTables& t,
                                 const NodeCols& nc, int n, uint32_t* fit) {
    const Row r = load_row(nc, n);  // before the predicates' early exits (eval_node)
    uint64_t pw[4] = {0, 0, 0, 0};
    if (c.has_ports)
        for (int w = 0; w < 4; ++w) if (w < port_win(c, nc)) pw[w] = nc.ports[port_at(c, nc, w, n)];
    const bool st = static_pred(cf, c, t, nc, n);
    const int32_t na = (st && cf.score_mult) ? na_weight(c, t, nc, n) : 0;
    int32_t s = 0;
    bool passed = false;
    uint64_t k = dyn_key(cf, c, t, nc, r, pw, n, st, na, &s, &passed);
    if (!k && passed && (r.bf_cpu | r.bf_mem | r.bf_gpu)) k = pack_key(s, n + nc.base, 0);
    *fit = fit_bits(c, r, passed);
    return k;
}

// ---------------------------------------------------------------------------
// pod (anti-)affinity (kbhip_affinity.h): count tables per term class,
// indexed by the node's topology domain.
// ---------------------------------------------------------------------------
// Domain columns are replicated over the whole node array (every shard holds
// them): dom_g takes a global node index, dom_of a local row of this shard.
KBHIP_HD int32_t dom_g(const NodeCols& nc, int space, int g) {
    return nc.dom[(int64_t)space * nc.dom_stride + g];
}
KBHIP_HD int32_t dom_of(const NodeCols& nc, int space, int n) { return dom_g(nc, space, n + nc.base); }

// predicates.go:1293-1458 for one node.
KBHIP_HD bool aff_pred(const TaskClass& c, const DevTables& t, const NodeCols& nc, int n) {
    // existing pods' required anti-affinity: a matching target in n's domain
    for (int i = 0; i < c.ea_n; ++i) {
        const int d = dom_of(nc, t.aff_items[c.ea_off + 2 * i], n);
        if (d >= 0 && t.aff_cnt[t.aff_items[c.ea_off + 2 * i + 1] + d] > 0) return false;
    }
    // own required affinity: a target matching every term in n's domain tuple,
    // or no target matches the terms anywhere and the pod matches them itself
    if (c.pa_space >= 0) {
        const int d = dom_of(nc, c.pa_space, n);
        const bool match = d >= 0 && t.aff_cnt[c.pa_cnt + d] > 0;
        if (!match && !(c.pa_self && t.aff_scalar[c.pa_total] == 0)) return false;
    }
    // own required anti-affinity: a target matching every term in n's domain tuple
    if (c.paa_space >= 0) {
        const int d = dom_of(nc, c.paa_space, n);
        if (d >= 0 && t.aff_cnt[c.paa_cnt + d] > 0) return false;
    }
    return true;
}

// Raw inter-pod affinity count of node n (interpod_affinity.go:119-212):
// sum over the task's term classes of weight x pods of the class in n's
// domain; session-placed pods count at the fallback node F's domain.
KBHIP_HD int64_t ipa_count(const TaskClass& c, const DevTables& t, const NodeCols& nc, int n,
                                             int F) {
    int64_t sum = 0;
    for (int i = 0; i < c.ipa_n; ++i) {
        const int32_t* it = t.aff_items + c.ipa_off + 4 * i;
        const int d = dom_of(nc, it[0], n);
        if (d < 0) continue;
        int64_t x = t.aff_cnt[it[1] + d];
        if (F >= 0 && dom_g(nc, it[0], F) == d) x += t.aff_scalar[it[2]];
        sum += (int64_t)it[3] * x;
    }
    return sum;
}

// Full evaluation for the per-task path: static + affinity predicates, the
// inter-pod score normalised by the prepass's [lo, hi] (interpod_affinity.go:228-237).
KBHIP_HD uint64_t eval_node_aff(const Conf& cf, const TaskClass& c, const DevTables& t,
                                                  const NodeCols& nc, int n, int64_t lo, int64_t hi, int F,
                                                  int32_t* score_out, bool* passed, uint32_t* fit = nullptr,
                                                  const int64_t* ipa_pre = nullptr) {
    bool st = static_pred(cf, c, t, nc, n);
    if (st && c.aff && cf.pred_on) st = aff_pred(c, t, nc, n);
    int32_t ipa = 0;
    if (st && c.ipa_n && hi - lo > 0)  // ipa_pre: the raw counts k_ipa_minmax just computed on this state
        ipa = (int32_t)(10.0 * ((double)((ipa_pre ? ipa_pre[n] : ipa_count(c, t, nc, n, F)) - lo) / (double)(hi - lo)));
    const int32_t na = (st && cf.score_mult) ? na_weight(c, t, nc, n) : 0;
    const Row r = load_row(nc, n);
    uint64_t pw[4] = {0, 0, 0, 0};
    if (c.has_ports)
        for (int w = 0; w < 4; ++w) if (w < port_win(c, nc)) pw[w] = nc.ports[port_at(c, nc, w, n)];
    const uint64_t k = dyn_key(cf, c, t, nc, r, pw, n, st, na, score_out, passed, ipa);
    if (fit) *fit = fit_bits(c, r, *passed);
    return k;
}

// Why node n is, or is not, a node of the task's allocate walk
// (kbhip_explain_tasks; the KBHIP_WHY_* codes of include/kbhip.h): the first
// step that rejects it in the reference's order — predicates.go:123-203 (pod
// count, node selector / required node affinity, host ports, unschedulable,
// taints, pod (anti-)affinity), then NodeOrderFn's error (allocate.go:140-145)
// — which is not the order static_pred_f and dyn_key test in: they only need
// the conjunction.  A node no step rejects is in the walk: 0 where allocate.go:153
// holds, 1 where only :173 does, 2 where neither, with fit_bits' cpu / memory /
// GPU bits in bits 4..6.  Flags, row, port words and the taint test are loaded
// before the steps' early exits, as in eval_node.  No score is needed, hence no
// inter-pod prepass for any class.
constexpr int kWhyFitsIdle = 0, kWhyFitsReleasing = 1, kWhyResources = 2, kWhyPodCount = 3, kWhyNodeSelector = 4,
              kWhyHostPorts = 5, kWhyUnschedulable = 6, kWhyTaints = 7, kWhyPodAffinity = 8, kWhyScoreError = 9;
constexpr int kWhyCodes = 10, kWhyShortShift = 3;  // fit_bits' bits 1..3 << 3 = 0x10, 0x20, 0x40
constexpr int kWhyBins = 16;  // the histogram of a request (kbhip.h): 10 codes, a gap, 3 short bits, walk, nodes
struct VerdictIn {  // what node_verdict reads of a node whatever its steps decide (the sweep prefetches it)
    Row r;          // (the steps use the fit columns, pods and maxtasks: the other loads are dropped)
    uint64_t pw[4];
    uint8_t fl;
};
KBHIP_HD VerdictIn verdict_in(const TaskClass& c, const NodeCols& nc, int n) {
    VerdictIn v;
    v.fl = nc.flags[n];
    v.r = load_row(nc, n);
    for (int w = 0; w < 4; ++w) v.pw[w] = 0;
    if (c.has_ports)
        for (int w = 0; w < 4; ++w) if (w < port_win(c, nc)) v.pw[w] = nc.ports[port_at(c, nc, w, n)];
    return v;
}
KBHIP_HD uint8_t node_verdict_of(const Conf& cf, const TaskClass& c, const DevTables& t, const NodeCols& nc, int n,
                                 const VerdictIn& in) {
    const uint8_t fl = in.fl;
    const Row& r = in.r;
    bool port_hit = false, taint_hit = false;
    if (c.has_ports)                                                     // host_ports.go:96-125
        for (int w = 0; w < 4; ++w) if (w < port_win(c, nc))
            if (in.pw[w] & t.masks[c.pconf_off + w]) port_hit = true;
    for (int w = 0; w < nc.taint_words; ++w)                             // helper/helpers.go:425-440
        if (nc.taints[(int64_t)w * nc.npad + n] & ~t.masks[c.tol_off + w]) taint_hit = true;
    if (cf.pred_on) {
        if (r.maxtasks <= r.pods) return kWhyPodCount;                   // predicates.go:127
        if (c.nsel_term >= 0 && !term_match(t, nc, t.terms[c.nsel_term], n)) return kWhyNodeSelector;
        if (c.req_term_n >= 0) {                                         // predicates.go:132-143
            bool any = false;
            for (int i = 0; i < c.req_term_n; ++i) any = any || term_match(t, nc, t.terms[c.req_term_off + i], n);
            if (!any) return kWhyNodeSelector;
        }
        if (port_hit) return kWhyHostPorts;                              // predicates.go:146-157
        if (fl & 1) return kWhyUnschedulable;                            // predicates.go:160-171
        if (taint_hit) return kWhyTaints;                                // predicates.go:174-185
        if (c.pred_err || (c.aff && !aff_pred(c, t, nc, n))) return kWhyPodAffinity;  // predicates.go:188-200
    }
    if (c.score_err) return kWhyScoreError;                              // allocate.go:140-145
    const int code = fit_idle(c, r) ? kWhyFitsIdle : fit_releasing(c, r) ? kWhyFitsReleasing : kWhyResources;
    return (uint8_t)(code | ((fit_bits(c, r, true) & 0xeu) << kWhyShortShift));
}
KBHIP_HD uint8_t node_verdict(const Conf& cf, const TaskClass& c, const DevTables& t, const NodeCols& nc, int n) {
    return node_verdict_of(cf, c, t, nc, n, verdict_in(c, nc, n));
}
// A verdict's bins of the request's histogram, as bits: its code's bin, and for
// a node of the walk bin 14 and the bins 11..13 of its short bits.  Bin 15 (the
// node count) is every node's.
KBHIP_HD uint32_t verdict_bins(uint8_t v) {
    const uint32_t code = v & 15u;
    uint32_t b = (1u << code) | (1u << 15);
    if (code <= (uint32_t)kWhyResources) b |= (1u << 14) | ((uint32_t)(v >> 4) & 7u) << 11;
    return b;
}

// Backfill's node test (backfill.go:51-56): the predicates only — no score,
// no fit — keyed so that the max key is the lowest passing index.
KBHIP_HD uint64_t eval_first_fit(const Conf& cf, const TaskClass& c, const DevTables& t,
                                                   const NodeCols& nc, int n) {
    bool ok = static_pred(cf, c, t, nc, n);
    if (ok && cf.pred_on) {
        if (c.aff) ok = aff_pred(c, t, nc, n);
        if (nc.maxtasks[n] <= nc.pods[n]) ok = false;                    // predicates.go:127
        if (c.has_ports)                                                 // host_ports.go:96-125
            for (int w = 0; w < 4; ++w) if (w < port_win(c, nc))
                if (nc.ports[port_at(c, nc, w, n)] & t.masks[c.pconf_off + w]) ok = false;
    }
    return ok ? pack_key(0, n + nc.base, 0) : 0;
}

// Count-table updates of a committed task (kind 1 Allocated, 2 Pipelined) on
// global node g (every shard applies them).
//   UPD_CNT_ALLOC (0):    Allocated only: a new predicate target in g's domain
//   UPD_SCALAR_ALLOC (1): Allocated only: target total of a PA class
//   UPD_SCALAR_ANY (2):   any commit: a session-placed pod (inter-pod priority)
// Written branch-free on purpose: the if / else-if / else form (one increment
// per branch, two tables) is miscompiled by the ROCm 7.2 gfx950 backend when
// it runs in a single lane — the UPD_SCALAR_ANY branch reused a stale table
// pointer register ("toolchain note").  A node without the
// space's key (domain -1) adds 0 at the table's first entry: the index stays
// inside the table (u[2] + -1 was one word before it — outside the buffer for
// the first table, a fault at full-size C3 with keyless nodes).
KBHIP_HD void commit_aff(const TaskClass& c, const DevTables& t, const NodeCols& nc, int g, int kind) {
    for (int i = 0; i < c.upd_n; ++i) {
        const int32_t* u = t.aff_items + c.upd_off + 3 * i;
        const int typ = u[0];
        const bool to_cnt = typ == 0;
        const int d = to_cnt ? dom_g(nc, u[1], g) : 0;
        const bool apply = (typ == 2 || kind == 1) && d >= 0;
        int32_t* tab = to_cnt ? t.aff_cnt : t.aff_scalar;
        tab[u[2] + (d < 0 ? 0 : d)] += apply ? 1 : 0;  // (a keyless node: +0 at the table's first entry)
    }
}

// Exact inverse of commit_aff (a retracted prediction, or the undo around a
// FitDelta recomputation); same branch-free form.
KBHIP_HD void uncommit_aff(const TaskClass& c, const DevTables& t, const NodeCols& nc, int g, int kind) {
    for (int i = 0; i < c.upd_n; ++i) {
        const int32_t* u = t.aff_items + c.upd_off + 3 * i;
        const int typ = u[0];
        const bool to_cnt = typ == 0;
        const int d = to_cnt ? dom_g(nc, u[1], g) : 0;
        const bool apply = (typ == 2 || kind == 1) && d >= 0;
        int32_t* tab = to_cnt ? t.aff_cnt : t.aff_scalar;
        tab[u[2] + (d < 0 ? 0 : d)] -= apply ? 1 : 0;
    }
}

// Pod-affinity classes the batched pop places (placement 7): predicate terms
// that only ever turn nodes infeasible as pods are placed — existing pods'
// required anti-affinity (EA) and own required anti-affinity (PAA) — with no
// own required affinity (PA: placements make nodes feasible) and no inter-pod
// priority terms (their normalisation moves every node's score).  Lanes keep
// the count-table entries their node's predicate reads in registers.
constexpr int kAffItems = 4;  // EA pairs + PAA the placement tracks per candidate
constexpr int kAffUpd = 8;    // commit updates of the class
KBHIP_HD bool aff_batchable(const TaskClass& c) {
    return c.aff && !c.pred_err && c.pa_space < 0 && c.ipa_n == 0 &&
           c.ea_n + (c.paa_space >= 0 ? 1 : 0) <= kAffItems && c.upd_n <= kAffUpd;
}

// NodeInfo.AddTask for the winner (node_info.go:113-145) + the k8s NodeInfo
// aggregates the predicates/nodeorder read (k8s cache/node_info.go:498-521).
KBHIP_HD void commit_node(const TaskClass& c, const DevTables& t, const NodeCols& nc, int n, int kind) {
    if (c.backfill) { nc.bf_cpu[n] += c.req_cpu; nc.bf_mem[n] += c.req_mem; nc.bf_gpu[n] += c.req_gpu; }
    if (kind == 1) { nc.idle_cpu[n] -= c.req_cpu; nc.idle_mem[n] -= c.req_mem; nc.idle_gpu[n] -= c.req_gpu; }
    else { nc.rel_cpu[n] -= c.req_cpu; nc.rel_mem[n] -= c.req_mem; nc.rel_gpu[n] -= c.req_gpu; }
    nc.pods[n] += 1;
    nc.nzc[n] += c.nz_cpu;
    nc.nzm[n] += c.nz_mem;
    if (c.has_ports)
        for (int w = 0; w < 4; ++w) if (w < port_win(c, nc)) nc.ports[port_at(c, nc, w, n)] |= t.masks[c.pown_off + w];
}

// Exact inverse of commit_node for a batched-path class (integer updates; the
// class's own host-port bits cannot have been set before its commit, since
// they conflict with themselves).  Used to retract a mispredicted pop.
KBHIP_HD void uncommit_node(const TaskClass& c, const DevTables& t, const NodeCols& nc, int n, int kind) {
    if (c.backfill) { nc.bf_cpu[n] -= c.req_cpu; nc.bf_mem[n] -= c.req_mem; nc.bf_gpu[n] -= c.req_gpu; }
    if (kind == 1) { nc.idle_cpu[n] += c.req_cpu; nc.idle_mem[n] += c.req_mem; nc.idle_gpu[n] += c.req_gpu; }
    else { nc.rel_cpu[n] += c.req_cpu; nc.rel_mem[n] += c.req_mem; nc.rel_gpu[n] += c.req_gpu; }
    nc.pods[n] -= 1;
    nc.nzc[n] -= c.nz_cpu;
    nc.nzm[n] -= c.nz_mem;
    if (c.has_ports)
        for (int w = 0; w < 4; ++w) if (w < port_win(c, nc)) nc.ports[port_at(c, nc, w, n)] &= ~t.masks[c.pown_off + w];
}

// Gang bookkeeping after an assignment: allocate.go:191-195 + gang.go:63-66.
KBHIP_HD void after_assign(PopCtrl* ctrl, int i, int kind) {
    if (kind == 1) ctrl->ready_count += 1;  // Pipelined is not an AllocatedStatus (types.go:82-84)
    ctrl->n_done = i + 1;
    if (!ctrl->gang_mode || ctrl->ready_count >= ctrl->min_avail) ctrl->stop = 2;
    else if (i + 1 == ctrl->n_tasks) ctrl->stop = 0;
}

// ---------------------------------------------------------------------------
// The victims of one node (kbhip_head_victims, kbhip_debug_victims): what
// EvictAction::victims_of and the eviction loops of 11_evict.cpp decide, on
// the flat records of the victim state.  Three steps, the first two
// independent per task (a lane each on the device, a loop on the host):
//   vict_stage   task k of the node with its job's and queue's records, and
//                whether the call's loop would hand it to the victim functions
//   vict_link    the first task of the node with k's job / k's queue: where
//                the running sums of one plugin call are kept
//   vict_decide  sequential, in task order: the plugins tier by tier, the
//                intersection, validateVictims, the eviction prefix
// ---------------------------------------------------------------------------
KBHIP_HD bool vict_is_cand(const VictHdr& h, const VictTask& t, int n_jobs, int n_queues) {
    if (!(t.flags & kVictRunCopy) || t.job < 0 || t.job >= n_jobs || t.queue >= n_queues) return false;
    if (h.mode == 1) return t.queue >= 0 && t.queue != h.queue;             // reclaim.go: jobs of other queues
    if (h.mode == 2) return t.queue == h.queue && t.job != h.job;           // preempt.go:104-127
    return t.job == h.job;                                                  // preempt.go:151-181
}
KBHIP_HD void vict_stage(const VictState& st, const VictHdr& h, int at, VictRec& r) {
    r.t = st.task[at];
    r.cand = vict_is_cand(h, r.t, st.n_jobs, st.n_queues) ? 1 : 0;
    r.alive = r.cand;
    r.stamp = 0;
    r.ready = 0;
    r.jfirst = r.qfirst = 0;
    for (int k = 0; k < 3; ++k) r.jalloc[k] = r.qalloc[k] = r.qdes[k] = r.run[k] = 0;
    if (!r.cand) return;
    const VictJob& j = st.job[r.t.job];
    r.ready = j.ready;
    for (int k = 0; k < 3; ++k) r.jalloc[k] = j.alloc[k];
    if (r.t.queue >= 0) {
        const VictQueue& q = st.queue[r.t.queue];
        for (int k = 0; k < 3; ++k) { r.qalloc[k] = q.alloc[k]; r.qdes[k] = q.des[k]; }
    }
}
KBHIP_HD void vict_link(VictRec* rec, int k) {
    if (!rec[k].cand) return;
    int jf = k, qf = k;
    for (int i = k - 1; i >= 0; --i) {
        if (!rec[i].cand) continue;
        if (rec[i].t.job == rec[k].t.job) jf = i;
        if (rec[i].t.queue == rec[k].t.queue) qf = i;
    }
    rec[k].jfirst = jf;
    rec[k].qfirst = qf;
}
KBHIP_HD double vict_share(double l, double r) { return r == 0 ? (l == 0 ? 0 : 1) : l / r; }  // helpers.go:35-48
KBHIP_HD double vict_drf_share(const double* a, const double* total) {  // drf.go:160-170 (Framework::drf_share_of)
    double res = 0;
    for (int k = 0; k < 3; ++k) { const double x = vict_share(a[k], total[k]); if (x > res) res = x; }
    return res;
}
KBHIP_HD bool vict_le_f(const double* a, const double* b) {  // Resource.LessEqual (F3::less_equal)
    return (a[0] < b[0] || fabs(b[0] - a[0]) < (double)kMinCPU) && (a[1] < b[1] || fabs(b[1] - a[1]) < (double)kMinMem) &&
           (a[2] < b[2] || fabs(b[2] - a[2]) < (double)kMinGPU);
}
KBHIP_HD bool vict_le_tol(const int64_t* a, const int64_t* b) {  // EvictAction::le_tol
    return a[0] - b[0] < kMinCPU && a[1] - b[1] < kMinMem && a[2] - b[2] < kMinGPU;
}
// rec[0 .. n): the node's staged tasks.  out_victim: the first min(count, stride) victims' pod indices
// (the caller fills the rest).  Returns the victim count; *evict, *flags as kbhip.h describes them.
KBHIP_HD int vict_decide(const VictHdr& h, VictRec* rec, int n, int stride, int32_t* out_victim, int32_t* evict,
                         int32_t* flags) {
    *evict = 0;
    *flags = 0;
    int ncand = 0;
    for (int k = 0; k < n; ++k) ncand += rec[k].cand;
    if (ncand == 0) return 0;  // every plugin returns nil for no candidates
    bool init = false, decided = false;
    int alive = 0, epoch = 0;
    const double ls = vict_drf_share(h.la, h.total);
    for (int ci = 0; ci < h.n_codes && !decided; ++ci) {
        const int code = h.codes[ci];
        if (code == 0) {  // the tier ends: the first tier with a non-empty intersection decides
            decided = init && alive > 0;
            continue;
        }
        ++epoch;
        alive = 0;
        for (int k = 0; k < n; ++k) {
            VictRec& r = rec[k];
            if (!r.cand) continue;
            bool ans = false;
            if (code == 1) {  // gang.go:107-129
                ans = r.t.min_avail <= r.ready - 1 || r.t.min_avail == 1;
            } else if (code == 2) {  // conformance.go:37-56
                ans = !(r.t.flags & kVictCritical);
            } else if (code == 3) {  // drf.go:84-109: every evictee of the job so far comes off, answered or not
                VictRec& f = rec[r.jfirst];
                if (f.stamp != epoch) { f.stamp = epoch; for (int x = 0; x < 3; ++x) f.run[x] = f.jalloc[x]; }
                for (int x = 0; x < 3; ++x) f.run[x] -= (double)r.t.req[x];
                const double rs = vict_drf_share(f.run, h.total);
                ans = ls < rs || fabs(ls - rs) <= 0.000001;  // shareDelta (drf.go:29)
            } else if (code == 4) {  // proportion.go:159-183: an evictee larger than what is left is skipped
                VictRec& f = rec[r.qfirst];
                if (f.stamp != epoch) { f.stamp = epoch; for (int x = 0; x < 3; ++x) f.run[x] = f.qalloc[x]; }
                const double rq[3] = {(double)r.t.req[0], (double)r.t.req[1], (double)r.t.req[2]};
                if (!(f.run[0] < rq[0] && f.run[1] < rq[1] && f.run[2] < rq[2])) {
                    for (int x = 0; x < 3; ++x) f.run[x] -= rq[x];
                    ans = vict_le_f(f.qdes, f.run);
                }
            }
            if (!ans) r.alive = 0;
            alive += r.alive;
        }
        init = true;
    }
    if (!decided) return 0;
    // validateVictims (preempt.go:355-370), then the eviction loop (reclaim.go / preempt.go:300-320)
    int64_t all[3] = {0, 0, 0}, got[3] = {0, 0, 0}, need[3] = {h.ireq[0], h.ireq[1], h.ireq[2]};
    int w = 0;
    for (int k = 0; k < n; ++k) {
        if (!rec[k].alive) continue;
        for (int x = 0; x < 3; ++x) all[x] += rec[k].t.req[x];
        if (w < stride) out_victim[w] = rec[k].t.pod;
        ++w;
    }
    if (all[0] < h.ireq[0] && all[1] < h.ireq[1] && all[2] < h.ireq[2]) return alive;
    bool stop = false;
    for (int k = 0; k < n && !stop; ++k) {
        if (!rec[k].alive) continue;
        const int64_t* vr = rec[k].t.req;
        *evict += 1;
        for (int x = 0; x < 3; ++x) got[x] += vr[x];
        stop = vict_le_tol(need, vr);
        for (int x = 0; x < 3; ++x) need[x] -= vr[x];
    }
    *flags = 1 | (vict_le_tol(h.ireq, got) ? 2 : 0);  // KBHIP_HEAD_VICTIMS_VALID, _COVERS
    return alive;
}

// ---------------------------------------------------------------------------
// One task's eviction walk (kbhip_walk_victims, kbhip_debug_walk_victims): the
// node loop of preempt.go:259-353 / reclaim.go:115-189 over a list of nodes.
// A node whose victims are valid but do not cover InitResreq is evicted from
// and the loop goes on; the next node's victim functions see those evictions
// through the overlay (kbhip_internal.h) — what on_deallocate / set_status
// (framework.h) do to the job's and the queue's records:
//   walk_ov_job / walk_ov_queue   the entry of an id, or -1
//   vict_stage_walk  vict_stage, then the overlay's deltas on the candidate's
//                    job and queue records
//   walk_step        sequential: vict_decide on the staged node, the capacity
//                    test (a step is all or nothing), the ops, and the evicted
//                    prefix folded into the overlay and, for the task's own
//                    job, into VictHdr::la
// ---------------------------------------------------------------------------
KBHIP_HD void walk_ov_init(WalkOverlay& ov, int cap_j, int cap_q) {
    ov.n_j = ov.n_q = 0;
    ov.cap_j = cap_j < 1 ? 1 : (cap_j > kWalkOvJobs ? kWalkOvJobs : cap_j);
    ov.cap_q = cap_q < 1 ? 1 : (cap_q > kWalkOvQueues ? kWalkOvQueues : cap_q);
}
KBHIP_HD int walk_ov_job(const WalkOverlay& ov, int id) {
    for (int i = 0; i < ov.n_j; ++i) if (ov.j_id[i] == id) return i;
    return -1;
}
KBHIP_HD int walk_ov_queue(const WalkOverlay& ov, int id) {
    for (int i = 0; i < ov.n_q; ++i) if (ov.q_id[i] == id) return i;
    return -1;
}
// the entry of an id, added (with nothing taken off yet) where it is new; -1: the table is full
KBHIP_HD int walk_ov_job_slot(WalkOverlay& ov, int id) {
    int i = walk_ov_job(ov, id);
    if (i >= 0 || ov.n_j >= ov.cap_j) return i;
    i = ov.n_j++;
    ov.j_id[i] = id;
    ov.j_gone[i] = 0;
    for (int x = 0; x < 3; ++x) ov.j_sub[i][x] = 0;
    return i;
}
KBHIP_HD int walk_ov_queue_slot(WalkOverlay& ov, int id) {
    int i = walk_ov_queue(ov, id);
    if (i >= 0 || ov.n_q >= ov.cap_q) return i;
    i = ov.n_q++;
    ov.q_id[i] = id;
    for (int x = 0; x < 3; ++x) ov.q_sub[i][x] = 0;
    return i;
}
KBHIP_HD void vict_stage_walk(const VictState& st, const VictHdr& h, const WalkOverlay& ov, int at, VictRec& r) {
    vict_stage(st, h, at, r);
    if (!r.cand) return;
    const int ji = walk_ov_job(ov, r.t.job);
    if (ji >= 0) {
        r.ready -= ov.j_gone[ji];
        for (int x = 0; x < 3; ++x) r.jalloc[x] -= (double)ov.j_sub[ji][x];
    }
    const int qi = r.t.queue >= 0 ? walk_ov_queue(ov, r.t.queue) : -1;
    if (qi >= 0)
        for (int x = 0; x < 3; ++x) r.qalloc[x] -= (double)ov.q_sub[qi][x];
}
// rec[0 .. n): node `node` (its walk score `score`) staged by vict_stage_walk and linked.  Appends the
// node's ops at out_pod / out_node [c.n_ops ..) and moves c on; c.stop != 0 ends the walk.
KBHIP_HD void walk_step(VictHdr& h, WalkOverlay& ov, WalkCtl& c, VictRec* rec, int n, int node, int score,
                        int32_t* out_pod, int32_t* out_node) {
    int32_t evict = 0, flags = 0;
    c.visited += 1;
    (void)vict_decide(h, rec, n, 0, nullptr, &evict, &flags);
    if (!(flags & 1)) return;  // validateVictims fails: the loop goes on to the next node
    if (c.n_ops + evict + 1 > c.cap_ops) { c.stop = kWalkCapacity; return; }
    const bool covers = (flags & 2) != 0;
    bool carry = !covers;
    if (carry) {  // the walk goes on: the prefix's jobs and queues need their entries (none is kept if one is missing)
        const int nj = ov.n_j, nq = ov.n_q;
        bool full = false;
        for (int k = 0, e = 0; k < n && e < evict && !full; ++k) {
            if (!rec[k].alive) continue;
            ++e;
            full = walk_ov_job_slot(ov, rec[k].t.job) < 0 ||
                   (rec[k].t.queue >= 0 && walk_ov_queue_slot(ov, rec[k].t.queue) < 0);
        }
        if (full) {
            ov.n_j = nj;
            ov.n_q = nq;
            if (c.acted > 0) { c.stop = kWalkCapacity; return; }
            carry = false;  // the first step of a call is taken whatever it touches, and the walk stops behind it
        }
    }
    for (int k = 0, e = 0; k < n && e < evict; ++k) {
        const VictRec& r = rec[k];
        if (!r.alive) continue;
        ++e;
        out_pod[c.n_ops] = r.t.pod;
        out_node[c.n_ops] = node;
        c.n_ops += 1;
        if (!carry) continue;
        const int ji = walk_ov_job(ov, r.t.job);
        ov.j_gone[ji] += 1;
        for (int x = 0; x < 3; ++x) ov.j_sub[ji][x] += r.t.req[x];
        if (r.t.queue >= 0) {
            const int qi = walk_ov_queue(ov, r.t.queue);
            for (int x = 0; x < 3; ++x) ov.q_sub[qi][x] += r.t.req[x];
        }
        if (r.t.job == h.job)  // (KBHIP_VICTIMS_SAME_JOB only) drf.go:88-90: the preemptor's job allocation
            for (int x = 0; x < 3; ++x) h.la[x] -= (double)r.t.req[x];
    }
    c.acted += 1;
    c.last_node = node;
    c.last_score = score;
    if (covers) {
        out_pod[c.n_ops] = c.task;
        out_node[c.n_ops] = node;
        c.n_ops += 1;
        c.stop = kWalkAssigned;
    } else if (!carry) {
        c.stop = kWalkCapacity;
    }
}


}  // namespace kbhip

// kbhip session, part 14: per-node rejection reasons of pending tasks (kbhip_explain_tasks, kbhip_debug_explain)
#include "session.h"

namespace kbhip {

static_assert(KBHIP_EXPLAIN_MAX == kMaxChunk, "one request per chunk slot at most");
static_assert(KBHIP_EXPLAIN_BINS == kWhyBins, "the histogram row of kbhip.h");
static_assert(KBHIP_WHY_FITS_IDLE == kWhyFitsIdle && KBHIP_WHY_FITS_RELEASING == kWhyFitsReleasing &&
                  KBHIP_WHY_RESOURCES == kWhyResources && KBHIP_WHY_POD_COUNT == kWhyPodCount &&
                  KBHIP_WHY_NODE_SELECTOR == kWhyNodeSelector && KBHIP_WHY_HOST_PORTS == kWhyHostPorts &&
                  KBHIP_WHY_UNSCHEDULABLE == kWhyUnschedulable && KBHIP_WHY_TAINTS == kWhyTaints &&
                  KBHIP_WHY_POD_AFFINITY == kWhyPodAffinity && KBHIP_WHY_SCORE_ERROR == kWhyScoreError,
              "node_verdict returns the codes of kbhip.h");
static_assert(KBHIP_WHY_SHORT_CPU == (2 << kWhyShortShift) && KBHIP_WHY_SHORT_MEM == (4 << kWhyShortShift) &&
                  KBHIP_WHY_SHORT_GPU == (8 << kWhyShortShift),
              "the short bits are fit_bits' bits 1..3");

// The verdicts and histograms of n tasks of the session as it stands: the
// tasks' classes go up in one copy from pinned staging, one sweep launch and
// one reduce launch follow, then one copy of the n histograms (and, when asked
// for, one of the n verdict rows) and one wait.  Reads the session state,
// changes nothing: no node row, no visit counter, not fit_task.
int64_t explain_tasks_abi(Session& S, const int32_t* task_ids, int n, uint8_t* out_verdict, int64_t* out_hist,
                          int64_t* out_info) {
    for (int i = 0; i < n; ++i)
        query_task(S, task_ids[i], "kbhip_explain_tasks: task_ids[" + std::to_string(i) + "] ", false);
    query_begin(S, "kbhip_explain_tasks");

    const int N = S.nc.n;
    const int bx = explain_bx(N, n, S.explain_blocks);
    const size_t in_bytes = (size_t)n * sizeof(TaskClass);
    const size_t part_words = (size_t)n * bx * kWhyBins, out_bytes = (size_t)n * kWhyBins * sizeof(int64_t);
    const size_t v_bytes = out_verdict ? (size_t)n * (size_t)N : 0;
    S.h_explain_in.fit((size_t)kMaxChunk * sizeof(TaskClass));
    S.h_explain_out.fit((size_t)kMaxChunk * kWhyBins * sizeof(int64_t));
    if (!S.b_explain_in.p) S.b_explain_in.alloc<TaskClass>(kMaxChunk);
    if (!S.b_explain_out.p) S.b_explain_out.alloc<int64_t>((size_t)kMaxChunk * kWhyBins);
    S.b_explain_part.grow(S.stream, part_words * sizeof(uint32_t), part_words * sizeof(uint32_t));
    if (v_bytes) S.b_explain_v.grow(S.stream, v_bytes, v_bytes);
    for (int i = 0; i < n; ++i) S.h_explain_in.as<TaskClass>()[i] = S.classes[S.pods[task_ids[i]].cls];

    int64_t launches = flush_tables(S);  // evictions / unevicts so far change pod-affinity predicates
    HIPCHK(hipMemcpyAsync(S.b_explain_in.p, S.h_explain_in.p, in_bytes, hipMemcpyHostToDevice, S.stream));
    HIPCHK(launch_explain(S.conf, S.nc, S.tab, (const TaskClass*)S.b_explain_in.p, n, bx,
                          v_bytes ? (uint8_t*)S.b_explain_v.p : nullptr, (uint32_t*)S.b_explain_part.p,
                          (int64_t*)S.b_explain_out.p, S.stream));
    launches += 2;
    HIPCHK(hipMemcpyAsync(S.h_explain_out.p, S.b_explain_out.p, out_bytes, hipMemcpyDeviceToHost, S.stream));
    if (v_bytes) HIPCHK(hipMemcpyAsync(out_verdict, S.b_explain_v.p, v_bytes, hipMemcpyDeviceToHost, S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));
    std::memcpy(out_hist, S.h_explain_out.p, out_bytes);
    if (out_info) {
        out_info[0] = launches;
        out_info[1] = bx;
        out_info[2] = out_verdict ? 1 : 0;
    }
    S.stats.sweeps += n;
    return n;
}

// The same verdicts from the host tables of an encode-only session: node_verdict, the function the
// kernel runs, node by node (as kbhip_debug_replay runs dyn_key).
void debug_explain(const Session& S, int pod, uint8_t* out_verdict, int64_t* out_hist) {
    if (pod < 0 || pod >= (int)S.pods.size() || S.pods[pod].cls < 0)
        throw Error(KBHIP_EINVAL, "kbhip_debug_explain: the task has no task class (not a pending task)");
    const TaskClass& c = S.classes[S.pods[pod].cls];
    int64_t hist[kWhyBins] = {};
    for (int n = 0; n < S.nc.n; ++n) {
        const uint8_t v = node_verdict(S.conf, c, S.tab, S.nc, n);
        if (out_verdict) out_verdict[n] = v;
        const uint32_t bins = verdict_bins(v);
        for (int k = 0; k < kWhyBins; ++k) hist[k] += (bins >> k) & 1u;
    }
    std::memcpy(out_hist, hist, sizeof hist);
}

}  // namespace kbhip

using namespace kbhip;

extern "C" {

int64_t kbhip_explain_tasks(kb_session* s, const int32_t* task_ids, int32_t n_tasks, uint8_t* out_verdict,
                            int64_t* out_hist, int64_t* out_info) {
    ABI_GUARD_S(s, {
        if (n_tasks < 0 || n_tasks > KBHIP_EXPLAIN_MAX)
            throw kbhip::Error(KBHIP_EINVAL, "kbhip_explain_tasks: n_tasks is 0 .. KBHIP_EXPLAIN_MAX (64)");
        if (n_tasks > 0 && (!task_ids || !out_hist))
            throw kbhip::Error(KBHIP_EINVAL, "kbhip_explain_tasks: null task_ids or out_hist");
        kbhip::Session& S = kbhip::device_session(s);
        if (n_tasks == 0) return 0;
        return kbhip::explain_tasks_abi(S, task_ids, n_tasks, out_verdict, out_hist, out_info);
    })
}

}  // extern "C"

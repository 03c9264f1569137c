// kbhip session, part 16: the head victims of several tasks in one call (kbhip_heads_victims)
#include "framework.h"

namespace kbhip {

static_assert(KBHIP_HEADS_VICTIMS_MAX == kMaxChunk && KBHIP_HEADS_VICTIMS_MAX == KBHIP_RANK_HEADS_MAX,
              "one request of kbhip_rank_heads' batch per task");

// For each of n tasks what kbhip_head_victims answers on the session as it stands: kbhip_rank_heads' batch
// (heads_stage / heads_enqueue, the requests' victim headers behind the own-job lists in the same upload),
// kbhip_head_victims' preparation of the two tables (vict_prepare), k_heads_victims on the merged heads where
// the merge left them — one launch, or one per request range where the spill rows of the whole batch would
// exceed option "victims_spill_max" — one copy back, one wait.  Every row is answered against the session
// at the call: nothing is carried from one request to the next.
int64_t heads_victims_abi(Session& S, const int32_t* task_ids, int n, bool by_score, int mode, int cap, int stride,
                          int64_t* out_total, int32_t* out_node, int32_t* out_score, int32_t* out_count,
                          int32_t* out_evict, uint8_t* out_flags, int32_t* out_victim, int32_t* out_first,
                          int64_t* out_info) {
    for (int i = 0; i < n; ++i)
        query_task(S, task_ids[i], "kbhip_heads_victims: task_ids[" + std::to_string(i) + "] ", true);
    query_begin(S, "kbhip_heads_victims");
    if (S.vs_live) vs_spill_check(S, S.vs_max_tasks, cap);  // (a state built below: checked before its upload)
    Framework F(S);
    F.open_plugins();  // drf / proportion as OnSessionOpen leaves them (kbhip_apply_ops opens them the same way)
    VictHdr hdr[kMaxChunk];
    for (int i = 0; i < n; ++i) hdr[i] = make_hdr(S, S.pods[task_ids[i]], mode);
    const VictPrep vp = vict_prepare(S, cap);
    int64_t launches = vp.launches;

    // the victims launches: request ranges whose spill rows fit the bound (no spill: one range)
    const bool spill = S.vs_max_tasks > kVictLds;
    const size_t req_spill = (size_t)cap * S.vs_max_tasks * sizeof(VictRec);
    const int per_range = spill ? (int)std::min<size_t>(n, (size_t)S.vs_spill_max / req_spill) : n;
    if (spill) S.b_vs_spill.grow(S.stream, per_range * req_spill, per_range * req_spill);
    // the rows hold at most the longest node's tasks; a larger stride is filled with -1 here
    const int dstride = std::max(1, std::min(stride, S.vs_max_tasks));
    const size_t key_words = kTopK + 1, key_bytes = (size_t)n * key_words * sizeof(uint64_t),
                 row_words = 3 + (size_t)dstride, out_bytes = key_bytes + (size_t)n * cap * row_words * sizeof(int32_t);
    S.h_vs_out.fit(out_bytes, std::max<size_t>(out_bytes, 4096));
    S.b_vs_out.grow(S.stream, out_bytes, std::max<size_t>(out_bytes, 4096));

    HeadsBatch B;
    heads_stage(S, task_ids, n, by_score, mode, (size_t)n * sizeof(VictHdr), B);
    std::memcpy(B.h_extra, hdr, (size_t)n * sizeof(VictHdr));
    int bx = 0;
    launches += heads_enqueue(S, B, &bx);

    uint8_t* const d_out = (uint8_t*)S.b_vs_out.p;
    const VictState st = vs_device_view(S);
    int64_t vict_launches = 0;
    for (int r0 = 0; r0 < n; r0 += per_range) {
        const int nr = std::min(per_range, n - r0);
        HIPCHK(launch_heads_victims(st, (const VictHdr*)B.d_extra + r0, (const uint64_t*)S.b_heads.p + r0 * key_words,
                                    nr, cap, dstride, S.nc.base, vs_lds_recs(S), vs_spill_rows(S), vs_spill_stride(S),
                                    (uint64_t*)d_out + r0 * key_words,
                                    (int32_t*)(d_out + key_bytes) + (size_t)r0 * cap * row_words, S.stream));
        vict_launches += 1;
    }
    launches += vict_launches;
    HIPCHK(hipMemcpyAsync(S.h_vs_out.p, d_out, out_bytes, hipMemcpyDeviceToHost, S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));

    const uint64_t* const keys = S.h_vs_out.as<uint64_t>();
    const int32_t* const rows = (const int32_t*)(S.h_vs_out.as<uint8_t>() + key_bytes);
    int64_t max_count = 0;
    for (int i = 0; i < n; ++i) {
        const size_t at = (size_t)i * cap;
        out_total[i] = (int64_t)keys[i * key_words + kTopK];
        const int64_t top = head_rows_unpack(keys + i * key_words, rows + at * row_words, cap, stride, dstride, by_score,
                                             out_node + at, out_score ? out_score + at : nullptr, out_count + at,
                                             out_evict + at, out_flags + at, out_victim + at * stride);
        max_count = std::max(max_count, top);
        if (!out_first) continue;
        out_first[i] = -1;
        for (int k = cap - 1; k >= 0; --k)
            if (out_flags[at + k] & KBHIP_HEAD_VICTIMS_VALID) out_first[i] = k;
    }
    head_info_fill(out_info, vp, launches, max_count);
    if (out_info) out_info[5] = vict_launches;
    S.stats.rank_heads += n;
    S.stats.sweeps += n;
    return n;
}

}  // namespace kbhip

using namespace kbhip;

extern "C" {

int64_t kbhip_heads_victims(kb_session* s, const int32_t* task_ids, int32_t n_tasks, int32_t by_score, int32_t victims,
                            int32_t cap, int32_t stride, int64_t* out_total, int32_t* out_node, int32_t* out_score,
                            int32_t* out_count, int32_t* out_evict, uint8_t* out_flags, int32_t* out_victim,
                            int32_t* out_first, int64_t* out_info) {
    ABI_GUARD_S(s, {
        if (n_tasks < 0 || n_tasks > KBHIP_HEADS_VICTIMS_MAX)
            throw kbhip::Error(KBHIP_EINVAL, "kbhip_heads_victims: n_tasks is 0 .. KBHIP_HEADS_VICTIMS_MAX (64)");
        check_cap("kbhip_heads_victims", cap);
        check_stride("kbhip_heads_victims", stride);
        check_by_score("kbhip_heads_victims", by_score);
        check_victims("kbhip_heads_victims", victims);
        if (!task_ids || !out_total || !out_node || !out_count || !out_evict || !out_flags || !out_victim)
            throw kbhip::Error(KBHIP_EINVAL, "kbhip_heads_victims: null task_ids, out_total, out_node, out_count, "
                                             "out_evict, out_flags or out_victim");
        kbhip::Session& S = kbhip::device_session(s);
        if (n_tasks == 0) return 0;
        return kbhip::heads_victims_abi(S, task_ids, n_tasks, by_score != 0, victims, cap, stride, out_total,
                                        out_node, out_score, out_count, out_evict, out_flags, out_victim, out_first,
                                        out_info);
    })
}

}  // extern "C"

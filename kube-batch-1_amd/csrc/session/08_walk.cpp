// kbhip session, part 08: read-outs of the allocate walk (kbhip_walk_visits, kbhip_fit_deltas)
#include "session.h"

namespace kbhip {

// The compaction's scratch (kbhip_walk.hip): ballot words and block offsets, sized once per session.
static int compact_scratch(Session& S, uint64_t** mask, uint32_t** blk) {
    const int nb = compact_blocks(S.nc.n);
    if (S.cmp_blocks != (size_t)nb || !S.b_cmp_mask.p) {
        S.b_cmp_mask.alloc<uint64_t>((size_t)nb * (kBlock / 64));
        S.b_cmp_blk.alloc<uint32_t>((size_t)nb + 1);
        S.cmp_blocks = (size_t)nb;
    }
    *mask = (uint64_t*)S.b_cmp_mask.p;
    *blk = (uint32_t*)S.b_cmp_blk.p;
    return nb;
}

// Scan of the marked blocks; the record count comes back (4 bytes).
static int64_t compact_count(Session& S, uint32_t* blk, int nb) {
    HIPCHK(launch_compact_scan(blk, nb, S.stream));
    uint32_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, blk + nb, sizeof total, hipMemcpyDeviceToHost, S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));
    return (int64_t)total;
}

// Device room for `count` records: node indices and `val_bytes` of values each.
static void compact_records(Session& S, int64_t count, size_t val_bytes) {
    if (S.cmp_node_n < (size_t)count || !S.b_cmp_node.p) {
        S.b_cmp_node.alloc<int32_t>((size_t)count);
        S.cmp_node_n = (size_t)count;
    }
    if (S.cmp_val_bytes < (size_t)count * val_bytes || !S.b_cmp_val.p) {
        S.b_cmp_val.alloc<uint8_t>((size_t)count * val_bytes);
        S.cmp_val_bytes = (size_t)count * val_bytes;
    }
}

// The nodes allocate walks visited since the previous call, ascending, with
// their visit counts (GetAccessibleResource calls, node_info.go:209-211: each
// added Backfilled to Idle once).  The copy back is `count` records; cap <
// count (the size query included): the count alone, nothing cleared.
int64_t walk_visits(Session& S, int32_t* out_node, uint32_t* out_count, int64_t cap) {
    if (S.world != 1) throw Error(KBHIP_EUNSUPPORTED, "kbhip_walk_visits on a node-sharded session");
    ov_quiesce(S);
    uint64_t* mask;
    uint32_t* blk;
    const int nb = compact_scratch(S, &mask, &blk);
    HIPCHK(launch_visit_mark(S.nc, mask, blk, S.stream));
    const int64_t count = compact_count(S, blk, nb);
    if (count == 0 || cap < count) return count;
    compact_records(S, count, sizeof(uint32_t));
    int32_t* d_node = (int32_t*)S.b_cmp_node.p;
    uint32_t* d_cnt = (uint32_t*)S.b_cmp_val.p;
    HIPCHK(launch_visit_scatter(S.nc, mask, blk, d_node, d_cnt, 1, S.stream));
    HIPCHK(hipMemcpyAsync(out_node, d_node, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, S.stream));
    HIPCHK(hipMemcpyAsync(out_count, d_cnt, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost, S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));
    return count;
}

// NodesFitDelta of the task on which the session's last pop stopped unassigned
// (allocate.go:164-167): one record per node of its walk, ascending.  Nothing
// was committed after that walk, so the sweep over the current columns sees
// the state the walk left (its Idle += Backfilled visits applied).  With
// option "time_every" > 0 the three kernels are timed by one HIP-event pair
// (kbhip_stats device_s / timed_launches).
int64_t fit_deltas(Session& S, int pod, int32_t* out_node, int64_t* out_delta, int64_t cap) {
    if (S.world != 1) throw Error(KBHIP_EUNSUPPORTED, "kbhip_fit_deltas on a node-sharded session");
    if (pod < 0 || pod != S.fit_task || pod >= (int)S.pods.size() || S.pods[pod].cls < 0)
        throw Error(KBHIP_EINVAL, "kbhip_fit_deltas: not the task on which the session's most recent pop stopped "
                                  "unassigned (or the session state changed since)");
    ov_quiesce(S);
    const int cls = S.pods[pod].cls;
    const TaskClass& c = S.classes[cls];
    uint64_t* mask;
    uint32_t* blk;
    const int nb = compact_scratch(S, &mask, &blk);
    ctrl_setup(S, 1, &cls, 0, 0, 0, 0, -1, 0);
    if (c.ipa_n > 0) HIPCHK(launch_ipa_minmax(S.nc, S.tab, S.d_ctrl, 0, S.stream));
    const bool timed = S.time_every > 0;
    if (timed) {
        if (!S.ev0) { HIPCHK(hipEventCreate(&S.ev0)); HIPCHK(hipEventCreate(&S.ev1)); }
        HIPCHK(hipEventRecord(S.ev0, S.stream));
    }
    HIPCHK(launch_fit_mark(S.conf, S.nc, S.tab, c, S.d_ctrl, mask, blk, S.stream));
    const int64_t count = compact_count(S, blk, nb);
    const bool copy = count > 0 && cap >= count;
    if (copy) {
        compact_records(S, count, 3 * sizeof(int64_t));
        HIPCHK(launch_fit_scatter(S.nc, c, mask, blk, (int32_t*)S.b_cmp_node.p, (int64_t*)S.b_cmp_val.p, S.stream));
    }
    if (timed) HIPCHK(hipEventRecord(S.ev1, S.stream));
    if (copy) {
        HIPCHK(hipMemcpyAsync(out_node, S.b_cmp_node.p, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, S.stream));
        HIPCHK(hipMemcpyAsync(out_delta, S.b_cmp_val.p, (size_t)count * 3 * sizeof(int64_t), hipMemcpyDeviceToHost,
                              S.stream));
    }
    HIPCHK(hipStreamSynchronize(S.stream));
    if (timed) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, S.ev0, S.ev1));
        S.timed_ms += ms;
        S.timed_n++;
    }
    S.stats.sweeps++;
    return count;
}

}  // namespace kbhip

using namespace kbhip;

extern "C" {

int64_t kbhip_walk_visits(kb_session* s, int32_t* out_node, uint32_t* out_count, int64_t cap) {
    ABI_GUARD_S(s, {
        if (cap < 0 || (cap > 0 && (!out_node || !out_count)))
            throw kbhip::Error(KBHIP_EINVAL, "null output array with cap > 0");
        return kbhip::walk_visits(kbhip::device_session(s), out_node, out_count, cap);
    })
}

int64_t kbhip_fit_deltas(kb_session* s, int32_t task_id, int32_t* out_node, int64_t* out_delta, int64_t cap) {
    ABI_GUARD_S(s, {
        if (cap < 0 || (cap > 0 && (!out_node || !out_delta)))
            throw kbhip::Error(KBHIP_EINVAL, "null output array with cap > 0");
        return kbhip::fit_deltas(kbhip::device_session(s), task_id, out_node, out_delta, cap);
    })
}

}  // extern "C"

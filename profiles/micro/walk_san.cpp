// Host sanitizer run of the eviction walk's overlay and step (walk_ov_*, vict_stage_walk, walk_step,
// kbhip_eval.h): the functions k_walk_victims runs, on synthetic nodes at the staging boundaries, with
// overlays from one entry to the full tables, in all three modes.  CPU only:
//   hipcc -std=c++17 -O1 -g -ffp-contract=off --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -I kube-batch-1_amd/csrc -I include profiles/micro/walk_san.cpp -o walk_san && ./walk_san
#include <cstdio>
#include <vector>

#include "kbhip_eval.h"

using namespace kbhip;

int main() {
    const int sizes[] = {0, 1, 63, 64, 65, 129, 256, 257};
    const int n_nodes = (int)(sizeof(sizes) / sizeof(sizes[0]));
    const int n_jobs = 600, n_queues = 130;  // more than the overlay holds
    std::vector<int32_t> off{0};
    std::vector<VictTask> task;
    uint32_t x = 2463534242u;
    auto rnd = [&x](uint32_t m) { x = x * 1664525u + 1013904223u; return (x >> 8) % m; };
    for (int size : sizes) {
        for (int k = 0; k < size; ++k) {
            const int jb = (int)rnd(n_jobs), pod = (int)task.size();
            task.push_back(VictTask{pod, jb, jb % n_queues, 1 + (int32_t)rnd(3),
                                    {(int64_t)(10 + rnd(60)), (int64_t)1 << (20 + rnd(4)), (int64_t)rnd(3) * 10},
                                    (int32_t)(rnd(8) ? kVictRunCopy : 0) | (rnd(6) ? 0 : kVictCritical), 0});
        }
        off.push_back((int32_t)task.size());
    }
    std::vector<VictJob> job(n_jobs);
    std::vector<VictQueue> queue(n_queues);
    for (int j = 0; j < n_jobs; ++j) job[j] = VictJob{{4000.0 + 50 * j, 8e9, 100.0 * (j % 7)}, 2 + j % 4, 0};
    for (int q = 0; q < n_queues; ++q) queue[q] = VictQueue{{9000.0 * (q + 1), 3e10, 400}, {600.0, 2e9, 10}};
    const VictState st{off.data(), task.data(), job.data(), queue.data(), n_nodes, n_jobs, n_queues, (int32_t)task.size()};
    long ops = 0, acted = 0, capacity = 0, carried = 0;
    const int caps[] = {1, 2, 3, 17, 64, 255, kWalkOvJobs, 100000};
    for (int mode = 1; mode <= 3; ++mode)
        for (int layout = 0; layout < 3; ++layout)
            for (int ov_cap : caps)
                for (int64_t cap_ops : {(int64_t)1, (int64_t)9, (int64_t)300, (int64_t)task.size() + 1}) {
                    VictHdr h{};
                    h.total[0] = 6400000; h.total[1] = 2.5e13; h.total[2] = 160000;
                    h.la[0] = 4500; h.la[1] = 9e9; h.la[2] = 0;
                    h.ireq[0] = 1 << 20; h.ireq[1] = (int64_t)1 << 40; h.ireq[2] = 0;  // never covered: the walk goes on
                    h.mode = mode; h.queue = 0; h.job = 0;
                    const int8_t lay[3][6] = {{1, 2, 0, 3, 4, 0}, {2, 0, 0, 0, 0, 0}, {2, 0, 1, 3, 4, 0}};
                    h.n_codes = layout == 1 ? 2 : 6;
                    for (int i = 0; i < h.n_codes; ++i) h.codes[i] = lay[layout][i];
                    WalkOverlay ov;
                    walk_ov_init(ov, ov_cap, ov_cap);
                    std::vector<int32_t> pod((size_t)cap_ops), node((size_t)cap_ops);  // exactly cap_ops: a slot past it is caught
                    WalkCtl c{0, cap_ops, 0, 0, 0, -1, 0, 1 << 30};
                    for (int i = n_nodes - 1; i >= 0 && c.stop == 0; --i) {  // the large nodes first
                        const int n = off[i + 1] - off[i];
                        std::vector<VictRec> rec(n);  // exactly the node's tasks
                        for (int k = 0; k < n; ++k) vict_stage_walk(st, h, ov, off[i] + k, rec[k]);
                        for (int k = 0; k < n; ++k) vict_link(rec.data(), k);
                        walk_step(h, ov, c, rec.data(), n, i, 0, pod.data(), node.data());
                        if (ov.n_j > ov.cap_j || ov.n_q > ov.cap_q || c.n_ops > cap_ops) { std::printf("bad step\n"); return 1; }
                    }
                    ops += c.n_ops;
                    acted += c.acted;
                    capacity += c.stop == kWalkCapacity;
                    carried += ov.n_j;
                }
    std::printf("walk_san ok: %ld ops on %ld nodes, %ld capacity stops, %ld overlay jobs\n", ops, acted, capacity, carried);
    return ops > 0 && acted > 0 && capacity > 0 && carried > 0 ? 0 : 1;
}

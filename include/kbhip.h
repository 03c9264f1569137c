/*
 * kbhip.h — C ABI of libkbhip.so, the MI355X (gfx950) placement engine for
 * kube-batch's allocate action.
 *
 * The reference has no FFI: its hot path is a set of Go function types that
 * plugins register into a framework.Session.  A per-(task, node) callback
 * across cgo would cost N*T crossings, so the boundary is a batched session
 * engine called once per job pop.  Each entry point below
 * names the reference interface it replaces:
 *
 *   kbhip_session_open   <- framework.OpenSession -> cache.Snapshot()
 *                           (pkg/scheduler/framework/framework.go:29-51,
 *                            pkg/scheduler/cache/cache.go:515-583): the session
 *                           snapshot, serialised as a KBS1 buffer (kbsnap.h),
 *                           is copied, dictionary-encoded and uploaded to HBM.
 *   kbhip_place_job      <- the inner loop of allocateAction.Execute
 *                           (pkg/scheduler/actions/allocate/allocate.go:110-196)
 *                           for one job pop: per task, Session.PredicateFn
 *                           (framework/session_plugins.go:331-348, the
 *                           predicates plugin predicates.go:123-203), Session.
 *                           NodeOrderFn (:350-370, nodeorder.go:252-317),
 *                           util.SelectBestNode (util/sort.go:25-37), the
 *                           fit walk (allocate.go:149-185), Session.Allocate /
 *                           Pipeline node updates (framework/session.go:199-297)
 *                           and the gang JobReadyFn stop (gang.go:63-66).
 *   kbhip_allocate       <- allocateAction.Execute as a whole
 *                           (allocate.go:41-201) with the host-side ordering
 *                           plugins (priority, gang, drf, proportion) run by
 *                           the library's C++ mirror of the Go framework — for
 *                           callers without a Go host (bench, tests).
 *   kbhip_session_close  <- framework.CloseSession (framework.go:53-61).
 *
 * Conventions: every function returns 0 (or a count) on success and a
 * negative KBHIP_E* code on failure; nothing throws or aborts across the ABI.
 * kbhip_last_error() describes the last failure on the calling thread.
 * Inputs are caller-owned and copied; outputs are caller-allocated; the
 * session handle is engine-owned.  One session per calling thread; no host
 * thread of the library outlives a call (kbhip_session_open splits its pod
 * pass over up to 8 worker threads it joins before returning).  Device
 * memory, pinned buffers and streams of a closed session go back to a
 * process-wide pool and serve later sessions.
 *
 * Deviations from SURVEY.md §8(b)'s sketch: kbhip_session_open takes one KBS1
 * buffer that carries the plugin conf too (tiers, nodeorder arguments) instead
 * of separate kb_snapshot / kb_conf structs; node-array sharding over GPUs is
 * kbhip_session_open_shard (rank, world) instead of an n_gpus argument; the
 * open splits its pod pass over worker threads (above).
 *
 * The library has exactly one execution path: HIP on a gfx950 device.  With
 * no usable device every call fails with KBHIP_ENODEV; there is no CPU
 * fallback.
 */
#ifndef KBHIP_H_
#define KBHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KBHIP_OK 0
#define KBHIP_EINVAL (-1)       /* malformed snapshot or arguments */
#define KBHIP_ENODEV (-2)       /* no HIP device / HIP runtime failure */
#define KBHIP_EUNSUPPORTED (-3) /* snapshot uses a feature the engine does not implement */
#define KBHIP_EDEVICE (-4)      /* kernel or copy failed */

/* placement kinds (TaskStatus after the decision) */
#define KBHIP_ALLOCATED 1 /* Session.Allocate -> api.Allocated */
#define KBHIP_PIPELINED 2 /* Session.Pipeline -> api.Pipelined */
#define KBHIP_EVICTED 3   /* Session.Evict / a committed Statement.Evict -> api.Releasing (cache.Evict) */

/* stop reasons of kbhip_place_job */
#define KBHIP_STOP_ALL 0        /* every given task was placed, job not yet ready */
#define KBHIP_STOP_UNASSIGNED 1 /* a task found no node: allocate.go:187-189 */
#define KBHIP_STOP_READY 2      /* JobReady after a placement: allocate.go:191-195 */

typedef struct kb_session kb_session;

/* Engine statistics (cumulative per session). */
typedef struct kbhip_stats {
    double open_s;       /* decode + encode + upload */
    double allocate_s;   /* wall time inside kbhip_allocate */
    double device_s;     /* summed HIP-event duration of the timed sweep launches */
    int64_t pops;        /* job pops */
    int64_t tasks;       /* tasks tried */
    int64_t placed;      /* Allocated + Pipelined */
    int64_t sweeps;      /* full-node sweeps launched */
    int64_t batched_pops;/* pops served by the class-batched path */
    int64_t nodes;       /* nodes in the session */
    int64_t timed_launches; /* sweep launches timed with HIP events (option "time_every") */
    double host_launch_s;   /* host time spent launching batched pop kernels */
    double host_wait_s;     /* host time spent waiting for their results */
    int64_t spec_hits;      /* predicted next pops launched ahead and used (kbhip_allocate) */
    int64_t spec_missed;    /* predicted pops retracted (their node updates undone on device) */
    double alloc_device_s;  /* HIP-event span of kbhip_allocate's device work (first launch to idle) */
    int64_t unassigned_pops; /* job pops that stopped on a task with no node (allocate.go:187-189) */
    int64_t collectives;     /* node-array shards: cross-shard all-gathers + all-reduces issued */
    int64_t rank_requests;   /* reclaim / preempt node rankings served by the what-if batcher ("rank_group") */
    int64_t rank_batch_sum;  /* sum over those of the sessions in the launch that served it */
    int64_t pop_requests;    /* batched allocate pops served by the what-if batcher ("rank_group") */
    int64_t pop_batch_sum;   /* sum over those of the sessions in the launch that served it */
    int64_t comm_reused;     /* 1: kbhip_shard_connect_rccl took a pooled communicator of an earlier session */
    int64_t async_launched;  /* kbhip_place_job_submit: pops launched ahead of their wait */
    int64_t async_retracted; /* ... launches withdrawn (cancelled, or behind a pop that ran synchronously) */
    int64_t async_cancelled; /* tickets withdrawn by kbhip_place_job_cancel */
    int64_t sweep_requests;  /* per-task chunks (allocate's general path, backfill) served by the what-if batcher */
    int64_t sweep_batch_sum; /* sum over those of the sessions per launch that served them */
    double score_sweep_s;    /* kbhip_sweep_scores with "time_every" > 0: summed HIP-event duration of its
                                standalone predicate + score sweep kernel (k_score_sweep) */
    int64_t score_sweeps;    /* ... launches timed */
    int64_t pertask_sweeps;  /* tasks swept one launch each (the general path: k_sweep_argmax) */
    int64_t seq_launches;    /* batched pops with a sequential placement (6: Backfilled nodes, 7: pod affinity) */
    int64_t seq_cut;         /* ... that ended before their chunk (a node outside the list could win next) */
    int64_t seq_none;        /* ... that placed nothing (the task went to the general path) */
    double evict_rank_s;     /* reclaim / preempt: host wall time in the node rankings (device sweep + copy) */
    double evict_walk_s;     /* reclaim / preempt: host wall time walking the ranked nodes (victims, evictions) */
    int64_t evict_visits;    /* reclaim / preempt: nodes whose victims were asked for (Reclaimable / Preemptable) */
    int64_t evict_cands;     /* ... candidates handed to those calls */
    int64_t fit_syncs;       /* allocate: FitDelta histograms recounted after a pop (a job left not Ready) */
    double alloc_setup_s;    /* allocate: host time before the first pop (plugin open, job and queue heaps) */
    double evict_setup_s;    /* reclaim / preempt: host time before the first node ranking (plugin open, node
                                task lists, victim codes, job heaps); part of evict_walk_s */
    int64_t engine_pops;     /* batched pops served by the persistent pop engine (option "engine") */
    int64_t engine_launches; /* launches of the engine's resident grid (one per run of engine pops) */
    int64_t engine_workers;  /* its worker blocks (0: the engine was not used) */
    int64_t engine_owners;   /* list mode (option "engine_lists"): its class-owner blocks (0: sweep mode) */
    int64_t engine_not_resident; /* engine grids that could not become resident (other kernels held CUs)
                                    and were started again */
    int64_t rank_heads;      /* kbhip_rank_nodes calls served by the top-64 kernel (first + cap <= 64) */
    int64_t rank_fulls;      /* ... served by the full device sort */
} kbhip_stats;

/* Library / device probe: returns the number of usable gfx950 devices (>= 0),
 * or KBHIP_ENODEV when the HIP runtime is unusable. */
int kbhip_device_count(void);

/* Open a session from a KBS1 snapshot held in memory (or a file). */
int kbhip_session_open(const void* kbs_bytes, size_t len, int device, kb_session** out);
int kbhip_session_open_file(const char* path, int device, kb_session** out);

/* Place one job pop: tasks (pod indices of the snapshot, already in
 * TaskOrderFn order) are tried in sequence until one is unassigned, the job
 * becomes ready, or the list is exhausted.
 *   gang_mode      1 = the gang JobReadyFn decides, 0 = no JobReadyFn (always Ready)
 *   min_available  JobInfo.MinAvailable
 *   ready_count    tasks of the job currently in AllocatedStatuses
 * Outputs per consumed task: out_node (node index, -1 unassigned), out_kind
 * (KBHIP_ALLOCATED / KBHIP_PIPELINED / 0).  *out_n_done = tasks consumed
 * (including an unassigned one), *out_stop_reason = KBHIP_STOP_*. */
int kbhip_place_job(kb_session* s, const int32_t* task_ids, int32_t n_tasks, int32_t gang_mode,
                    int32_t min_available, int32_t ready_count, int32_t* out_node, uint8_t* out_kind,
                    int32_t* out_n_done, int32_t* out_stop_reason);

/* Asynchronous per-pop entry points: the pipelining kbhip_allocate does
 * internally, for a host that keeps allocate.go's loop
 * (allocate.go:110-196) itself.  While pop e runs, the host predicts pop e+1
 * (assuming e places its tasks as Allocated up to the gang stop), submits it,
 * and only then waits for e; if e's results show the prediction wrong, it
 * cancels e+1 and submits the real next pop.
 *
 * kbhip_place_job_submit queues one job pop with kbhip_place_job's arguments
 * and returns a ticket (>= 0).  A pop runs on the session state that every
 * earlier submitted pop leaves, exactly as a sequence of kbhip_place_job calls
 * would: a pop that is one batched chunk (at most 64 tasks, kMaxChunk, of one
 * task class) is launched at once, up to 4 ahead of the oldest wait; any other pop, and
 * every pop behind it, is launched when the pops ahead of it have been waited
 * for, or runs inside its own wait.
 * kbhip_place_job_wait returns the results of the OLDEST outstanding ticket
 * (outputs as kbhip_place_job); naming any other ticket is KBHIP_EINVAL.
 * kbhip_place_job_cancel withdraws `ticket` and every later one: their device
 * updates are undone and they are never reported.  Returns the number
 * withdrawn.
 * Every call that runs or changes the session (actions, carry, place_job,
 * kbhip_set_option, the kbhip_shard_connect_* calls, read-backs of device
 * state) fails with KBHIP_EINVAL while tickets are outstanding; read-only host
 * queries (kbhip_get_stats, kbhip_gang_unschedulable, kbhip_debug_table) are
 * allowed; kbhip_session_close drops them.
 * KBHIP_EUNSUPPORTED on node-sharded sessions (world > 1): a shard's launch
 * waits inside the cross-rank exchange and a retraction would need every rank
 * to cancel identically; shards use kbhip_place_job. */
int64_t kbhip_place_job_submit(kb_session* s, const int32_t* task_ids, int32_t n_tasks, int32_t gang_mode,
                               int32_t min_available, int32_t ready_count);
int kbhip_place_job_wait(kb_session* s, int64_t ticket, int32_t* out_node, uint8_t* out_kind, int32_t* out_n_done,
                         int32_t* out_stop_reason);
int kbhip_place_job_cancel(kb_session* s, int64_t ticket);

/* Run the whole allocate action.  Outputs the placement log in decision
 * order: pod index, node index, kind.  Returns the number of placements. */
int kbhip_allocate(kb_session* s, int32_t* out_pod, int32_t* out_node, uint8_t* out_kind, int64_t cap);

/* Run the backfill action (actions/backfill/backfill.go:40-70) on the
 * session's current state (normally after kbhip_allocate): every Pending task
 * with an empty InitResreq goes to the first node (lowest index) passing the
 * predicates.  Outputs the placements (all KBHIP_ALLOCATED) like
 * kbhip_allocate; returns their number. */
int kbhip_backfill(kb_session* s, int32_t* out_pod, int32_t* out_node, uint8_t* out_kind, int64_t cap);

/* SURVEY §8(b) per-task entry points, for a Go host that keeps the
 * reference's own backfill / preempt loops and offloads only their sweeps.
 *
 * kbhip_first_fit <- the node loop of backfillAction.Execute
 *   (pkg/scheduler/actions/backfill/backfill.go:51-65): each task, in the
 *   given order, goes to the lowest-index node passing Session.PredicateFn and
 *   is committed with Session.Allocate (framework/session.go:237-297, including
 *   the drf / proportion AllocateFunc and the dispatch of a Ready job).
 *   out_node[i] = node index or -1.  Tasks must be Pending tasks of the
 *   session.  Returns the number placed.
 * kbhip_sweep_scores <- the PredicateFn + NodeOrderFn sweep of preempt()
 *   (pkg/scheduler/actions/preempt/preempt.go:270-287): out_keys[n]
 *   (optional, n_nodes entries) = pack_key(score, n) — score in bits 63..32
 *   biased by 2^31, (0x7fffffff - n) << 1 below — for a node that passes
 *   PredicateFn and has a NodeOrderFn score, 0 otherwise; sorting the keys
 *   descending is util.SelectBestNode's order (util/sort.go:25-37).  The
 *   session state is not changed.  Returns the number of passing nodes.
 * kbhip_rank_nodes <- the node walk of preempt() and of reclaim, ranked on
 *   the device, for a host that keeps the loop over the nodes itself:
 *     by_score 1  the nodes that pass PredicateFn and have a NodeOrderFn
 *                 score, in util.SelectBestNode order (preempt.go:270-287):
 *                 kbhip_sweep_scores' keys sorted descending, so equal scores
 *                 go to the lower node index;
 *     by_score 0  the nodes that pass PredicateFn, in ascending index (the
 *                 node loop of reclaim.go).
 *   Returns the number T of such nodes and writes entries [first, min(T,
 *   first + cap)) of the walk: out_node[i] = the node index, out_score[i]
 *   (optional) = its NodeOrderFn score (0 with by_score 0).  cap 0 with null
 *   outputs is the size query.  A request with first + cap <= 64 and cap > 0
 *   (the head of the walk, where preempt and reclaim usually stop) is served
 *   by one fused predicate + score + top-64 selection sweep: no per-node array
 *   is written and 64 keys plus the count are copied back.  Every other
 *   request runs the full device sort the reclaim / preempt actions use (a
 *   counting sort over the class's score range, or the radix passes: option
 *   "rank_radix") and copies only the entries asked for.  Nothing is kept
 *   between calls: a host that wants the head and then the rest calls twice.
 *   Like kbhip_sweep_scores the call reads the session state and changes
 *   nothing: no node row, no counter of kbhip_walk_visits, and a task
 *   kbhip_fit_deltas would answer for stays answerable.  KBHIP_EINVAL: a null
 *   session, a task without a task class (not a pending task of the session)
 *   or one the session's own actions have placed since, first < 0, cap < 0, cap > 0 with a null out_node, by_score other than 0
 *   or 1, an encode-only session, submitted pops outstanding;
 *   KBHIP_EUNSUPPORTED on node-sharded sessions (as kbhip_sweep_scores);
 *   KBHIP_EDEVICE when the full sort met a score outside the class's range. */
int kbhip_first_fit(kb_session* s, const int32_t* task_ids, int32_t n, int32_t* out_node);
int kbhip_sweep_scores(kb_session* s, int32_t task_id, uint64_t* out_keys);
int64_t kbhip_rank_nodes(kb_session* s, int32_t task_id, int32_t by_score, int64_t first, int32_t* out_node,
                         int32_t* out_score, int64_t cap);

/* kbhip_apply_ops <- the evictions and pipelines a host that keeps reclaim's /
 * preempt's own loop decided since its last ranking: n operations, applied in
 * the given order to the session's host model and to the device exactly as
 * the engine's own reclaim / preempt actions apply theirs, so the next
 * kbhip_rank_nodes / kbhip_sweep_scores / kbhip_first_fit, every later action
 * and every carry-over run on the state the host's loop has reached.
 *   KBHIP_OP_EVICT pod       Session.Evict / Statement.Evict (session.go:331-356,
 *     statement.go:35-67).  pod is Running and so is its node's copy (what the
 *     reclaimee / preemptee filters admit).  Its status becomes Releasing, its
 *     node's Releasing grows by its Resreq, it stops being a pod-affinity
 *     predicate target, the drf / proportion deallocate handlers run.  node[i]
 *     is ignored: the pod's own node is used.
 *   KBHIP_OP_PIPELINE pod, node   Session.Pipeline / Statement.Pipeline
 *     (session.go:199-235, statement.go:96-136).  pod is a Pending task with a
 *     task class, node is in range.  Status Pipelined on node, the node row is
 *     committed with kind Pipelined (pod count, non-zero requests, host ports,
 *     Releasing), the inter-pod fallback node follows, the allocate handlers
 *     run.  No predicate or fit check: the host decided, as ssn.Pipeline does.
 *   KBHIP_OP_UNPIPELINE pod  Statement.unpipeline (statement.go:141-172): the
 *     reverse, for a pod an earlier KBHIP_OP_PIPELINE pipelined.
 *   KBHIP_OP_UNEVICT pod     Statement.unevict (statement.go:81-105), for a pod
 *     an earlier KBHIP_OP_EVICT evicted: Running in the session and a
 *     predicate target again, while its node keeps the Releasing copy (the
 *     failing node.AddTask of the reference): the node's Releasing stays and
 *     the pod is no victim candidate any more.
 * A carry-over ends "earlier": operations do not reach across it.
 * The whole batch is validated first, against the statuses as the batch
 * itself changes them; on a validation error (KBHIP_EINVAL,
 * KBHIP_EUNSUPPORTED) nothing is changed.  A device or allocation failure
 * after validation (KBHIP_EDEVICE) can leave a partly applied batch, as a
 * failed action does: close the session and open a new one.  KBHIP_EINVAL: a
 * null session, a null op, pod or node array with n > 0, n < 0 or above
 * 2^31 - 1, an unknown operation, a pod or a KBHIP_OP_PIPELINE node out of range,
 * an operation that does not fit the pod's status, an encode-only session,
 * submitted pops outstanding; KBHIP_EUNSUPPORTED on node-sharded sessions (as
 * the other per-task calls).  Returns n (0 for an empty batch: nothing done).
 * On the device the batch's node operations are grouped by node on the host
 * and applied by one kernel, a lane per distinct node walking its operations
 * in order; the predicate-target changes of evictions / unevicts follow in
 * one count-table launch, done before the call returns.  *out_launches
 * (optional) = the device kernel launches the call issued: at most 2 whatever
 * n is.  No output record is produced (the host has its decisions), the
 * counters of kbhip_walk_visits are untouched, and a task kbhip_fit_deltas
 * would have answered for is no longer answerable, as after any call that
 * places.  A task pipelined here is not Pending: kbhip_rank_nodes refuses it
 * until a KBHIP_OP_UNPIPELINE. */
#define KBHIP_OP_EVICT 1
#define KBHIP_OP_PIPELINE 2
#define KBHIP_OP_UNPIPELINE 3
#define KBHIP_OP_UNEVICT 4
int64_t kbhip_apply_ops(kb_session* s, const uint8_t* op, const int32_t* pod, const int32_t* node, int64_t n,
                        int64_t* out_launches);

/* kbhip_rank_victim_nodes <- kbhip_rank_nodes' walk without the nodes on which
 * validateVictims (preempt.go:355-370) rejects whatever ssn.Reclaimable /
 * ssn.Preemptable answer.  The candidates of a node are its Running tasks
 * with a Running node copy and a job (what KBHIP_OP_EVICT admits), narrowed by
 * `victims` to what the caller's loop filters for:
 *   KBHIP_VICTIMS_OTHER_QUEUES     jobs of queues other than the task's (reclaim.go)
 *   KBHIP_VICTIMS_QUEUE_OTHER_JOBS the task's queue, jobs other than its own (preempt.go:104-127)
 *   KBHIP_VICTIMS_SAME_JOB         the task's own job (preempt.go:151-181)
 * A node stays in the walk when it has at least one candidate and the sum of
 * the candidates' Resreq is not strictly below the task's InitResreq in all
 * three resources at once (Resource.Less, the test validateVictims applies to
 * the victims).  Victims are a subset of the candidates whatever the plugins
 * and their order, so a node dropped here can yield no victim set that passes
 * validateVictims: a host loop over this walk takes the decisions of the loop
 * over kbhip_rank_nodes' walk, in the same order.
 * Everything else is kbhip_rank_nodes' contract: the returned total and the
 * window [first, first + cap) count kept nodes only; out_score is optional;
 * first + cap <= 64 with cap > 0 is served by the fused top-64 sweep (the
 * test applied by the lane that evaluates the node), anything else by the
 * full device sort followed by a stable compaction of three launches.
 * out_cands[i] (optional) = the candidate count of out_node[i].  out_info
 * (optional, 3 entries) = whether the top-64 sweep served the call, whether
 * the call (re)built the candidate table, the kernel launches it issued.
 * The candidate table — per queue and node the candidates' count and Resreq
 * sums, int64 [queues + 1][4][padded nodes] on the device — is built from the
 * pods by the first call that needs it.  kbhip_apply_ops keeps it current (a
 * KBHIP_OP_EVICT takes the pod off its node's entries inside that call's one
 * node launch; the other operations change no candidate), so a host loop of
 * rankings and operations never rebuilds it.  Every other call that changes
 * pod statuses (the actions, kbhip_place_job and its asynchronous forms,
 * kbhip_first_fit, the carry-overs) leaves it stale, and the next call here
 * rebuilds and uploads it.  Design limit: a table above 512 MB is refused
 * (KBHIP_EUNSUPPORTED, the message names the size).
 * The call changes no node row, no counter of kbhip_walk_visits, and a task
 * kbhip_fit_deltas would answer for stays answerable.  KBHIP_EINVAL: as
 * kbhip_rank_nodes, and `victims` outside 1..3 or a task without a job;
 * KBHIP_EUNSUPPORTED on node-sharded sessions; KBHIP_EDEVICE as
 * kbhip_rank_nodes. */
#define KBHIP_VICTIMS_OTHER_QUEUES 1      /* reclaim.go: Running tasks of jobs in other queues */
#define KBHIP_VICTIMS_QUEUE_OTHER_JOBS 2  /* preempt.go:104-127: same queue, another job */
#define KBHIP_VICTIMS_SAME_JOB 3          /* preempt.go:151-181: the task's own job */
int64_t kbhip_rank_victim_nodes(kb_session* s, int32_t task_id, int32_t by_score, int32_t victims, int64_t first,
                                int32_t* out_node, int32_t* out_score, int32_t* out_cands, int64_t cap,
                                int64_t* out_info);

/* kbhip_rank_heads <- the walk heads of up to KBHIP_RANK_HEADS_MAX tasks of
 * the session as it stands, from one sweep launch, one merge launch and one
 * copy back: a ranking call's fixed cost (upload, launches, copy, wait) paid
 * once per batch instead of once per task.  A host forms such a batch wherever
 * its loop ranks task after task with no operation in between: preempt's
 * within-job phase trying one preemptor per under-request job
 * (preempt.go:151-181), the tasks of one preemptor job until one is assigned
 * (preempt.go:101-138), reclaim's queues each finding no node.
 * For task_ids[i], out_total[i] and row i of the outputs — out_node,
 * out_score (optional), out_cands (optional), n_tasks rows of cap entries —
 * are exactly what kbhip_rank_nodes(task, by_score, 0, .., cap) returns and
 * writes when victims is 0, and what kbhip_rank_victim_nodes(task, by_score,
 * victims, 0, .., cap, ..) returns and writes when victims is one of
 * KBHIP_VICTIMS_* (out_cands entries are 0 with victims 0).  The entries of a
 * row beyond min(cap, total) are -1 (node) and 0 (score, cands): the call
 * defines its whole output.  1 <= cap <= 64.  A task may appear more than
 * once; tasks of different classes, jobs and queues, plain classes,
 * pod-affinity classes and classes with inter-pod priority terms mix freely.
 * Returns n_tasks (0 for n_tasks == 0, which does nothing).  out_info
 * (optional, 3 entries) = whether the call (re)built the candidate table, the
 * kernel launches it issued (2, plus one per distinct class with inter-pod
 * priority terms when by_score is 1, plus one when pod-affinity count changes
 * of earlier operations were still to be applied), the x size of the sweep's
 * grid.  kbhip_stats.rank_heads counts one per answered task.
 * The heads describe the session at the call: a host that prefetches them
 * discards what it has not consumed as soon as it sends a kbhip_apply_ops.
 * The call changes what kbhip_rank_victim_nodes changes — the candidate
 * table's currency — and nothing else.  The whole batch is validated before
 * any device work, and a refused call writes nothing.  KBHIP_EINVAL: a null
 * session, task_ids, out_total or out_node; n_tasks, cap, by_score or victims
 * out of range; a task without a class or not Pending, with victims != 0 a
 * task without a job (the message names the index in task_ids); an
 * encode-only session; submitted pops outstanding.  KBHIP_EUNSUPPORTED: a
 * node-sharded session, a candidate table above 512 MB. */
#define KBHIP_RANK_HEADS_MAX 64
int64_t kbhip_rank_heads(kb_session* s, const int32_t* task_ids, int32_t n_tasks, int32_t by_score,
                         int32_t victims, int32_t cap, int64_t* out_total, int32_t* out_node,
                         int32_t* out_score, int32_t* out_cands, int64_t* out_info);

/* kbhip_head_victims <- the head of a task's pruned walk together with what
 * the victim functions answer on each head node: the step of a host's reclaim
 * / preempt loop between kbhip_rank_victim_nodes and kbhip_apply_ops.
 * Returns the total of kbhip_rank_victim_nodes(task, by_score, victims, 0, ..,
 * cap); out_node / out_score (optional) are exactly that call's head.  For
 * head node i the candidates are its NodeInfo.Tasks in pod-index order that
 * are Running with a Running node copy and a job, narrowed by `victims` as
 * kbhip_rank_victim_nodes narrows them, and
 *   out_count[i]   the length of the list ssn.Reclaimable (victims =
 *                  KBHIP_VICTIMS_OTHER_QUEUES) or ssn.Preemptable (the other
 *                  two) gives (session_plugins.go:67-148: per tier the
 *                  intersection of the enabled plugins' answers, the first
 *                  tier with a non-empty one decides), in candidate order
 *   out_victim[i * stride + k]  the pod indices of that list, k <
 *                  min(count, stride); -1 beyond
 *   out_flags[i]   KBHIP_HEAD_VICTIMS_VALID: the count is > 0 and the
 *                  victims' Resreq sum is not Less than the task's InitResreq
 *                  (validateVictims, preempt.go:355-370);
 *                  KBHIP_HEAD_VICTIMS_COVERS (with VALID only): InitResreq is
 *                  LessEqual the evicted prefix's sum — the loop pipelines here
 *   out_evict[i]   with VALID, how many victims from the front the loop evicts
 *                  before it breaks (reclaim.go / preempt.go:300-320: evict,
 *                  stop when the remaining request is LessEqual the victim's
 *                  Resreq, else subtract and go on); 0 without VALID
 * Rows i >= min(cap, total) are -1 (node, victims) and 0.  out_info (optional,
 * 5 entries): whether the candidate table was rebuilt, whether the victim
 * state was rebuilt, the records patched into it, the kernel launches, the
 * largest out_count (a stride below it truncated a row).
 * The answer is the one kbhip_reclaim / kbhip_preempt would compute at this
 * moment: gang's readyTaskNum, drf's job allocations and total, proportion's
 * allocated / deserved (the plugins are opened by the first call that needs
 * them, as kbhip_apply_ops opens them), conformance's critical pods, and the
 * tiers' enabled victim functions — preempt's for the two preempt modes,
 * reclaim's for KBHIP_VICTIMS_OTHER_QUEUES.
 * The victim state — the nodes' candidate tasks as a CSR of records in node
 * order, one record per job and per queue — is built from the host model by
 * the first call and kept on the device.  kbhip_apply_ops does not make it
 * stale: it notes the pods, jobs and queues it touched, and the next call here
 * uploads those records and applies them in one launch before its sweep (more
 * than option "victims_dirty_max" pods waiting, default 65536: a rebuild).
 * Every other call that changes pod statuses (the actions, kbhip_place_job and
 * its asynchronous forms, kbhip_first_fit, the carry-overs, a kbhip_apply_ops
 * that failed part way) leaves it stale and the next call rebuilds it.
 * Launches: kbhip_rank_victim_nodes' head launches, then one; one copy back.
 * The rows describe the session at the call: a host uses them up to the first
 * node it acts on and discards the rest as soon as it sends a kbhip_apply_ops.
 * The call changes no node row, no counter of kbhip_walk_visits, and a task
 * kbhip_fit_deltas would answer for stays answerable.  The whole call is
 * validated before any device work, and a refused call writes nothing.
 * KBHIP_EINVAL: as kbhip_rank_victim_nodes, cap outside 1..64, stride < 1, a
 * null out_node, out_count, out_evict, out_flags or out_victim.
 * KBHIP_EUNSUPPORTED: a node-sharded session; a victim state above 512 MB (the
 * message names the size); more than 40 victim functions and tiers. */
#define KBHIP_HEAD_VICTIMS_VALID 1  /* validateVictims passes (preempt.go:355-370) */
#define KBHIP_HEAD_VICTIMS_COVERS 2 /* the eviction loop's total covers InitResreq: the loop pipelines here */
int64_t kbhip_head_victims(kb_session* s, int32_t task_id, int32_t by_score, int32_t victims /* KBHIP_VICTIMS_* */,
                           int32_t cap /* 1..64 head nodes */, int32_t stride /* victims kept per node, >= 1 */,
                           int32_t* out_node, int32_t* out_score /* optional */, int32_t* out_count,
                           int32_t* out_evict, uint8_t* out_flags, int32_t* out_victim /* cap rows of stride */,
                           int64_t* out_info /* optional */);

/* kbhip_heads_victims <- kbhip_head_victims for up to KBHIP_HEADS_VICTIMS_MAX
 * tasks in one call: the call's fixed cost (upload, launches, copy, wait) paid
 * once per batch.  A host forms the batch where kbhip_rank_heads names one —
 * task after task asked with no operation in between, as reclaim's and
 * preempt's loops do for the many pending tasks that act on no node.
 * For task_ids[i], out_total[i], row i of out_node, out_score (optional),
 * out_count, out_evict and out_flags (n_tasks rows of cap entries) and rows
 * i * cap .. i * cap + cap - 1 of out_victim (stride entries each) hold exactly
 * what kbhip_head_victims(task_ids[i], by_score, victims, cap, stride, ..)
 * returns and writes on the session as it stands, the -1 / 0 entries beyond
 * min(cap, total) and the -1 tail of each victim row included: the call
 * defines its whole output.  out_first[i] (optional, n_tasks entries) is the
 * index of task i's first head entry with KBHIP_HEAD_VICTIMS_VALID, or -1: the
 * one word a host reads to pass over a task that acts on no node.
 * Every row is answered against the session at the call, with no evictions
 * carried from one task, or one node, to the next: kbhip_head_victims'
 * semantics, not kbhip_walk_victims'.  A host that prefetches uses the rows up
 * to the first task it acts on and discards the rest at its next
 * kbhip_apply_ops.
 * A task may appear more than once; tasks of different classes, jobs and
 * queues, pod-affinity classes and classes with inter-pod priority terms mix
 * freely, as in kbhip_rank_heads.  by_score, victims, cap and stride hold for
 * the whole batch.  Returns n_tasks (0 for n_tasks == 0, which does nothing).
 * out_info (optional, 6 entries): [0] whether the candidate table was rebuilt,
 * [1] whether the victim state was rebuilt, [2] the records patched into it,
 * [3] the kernel launches, [4] the largest out_count of the batch, [5] the
 * victims launches among them.
 * Launches: what kbhip_rank_heads issues for the batch in a victims mode, one
 * patch launch when dirty records were waiting, then the victims launch — one
 * for the batch; only where a node holds more than 256 candidate tasks do the
 * blocks stage into device memory, n_tasks * cap rows of the longest node's
 * length, and a batch whose rows exceed option "victims_spill_max" (bytes,
 * default 256 MB) runs as consecutive ranges of tasks that each fit, one launch
 * per range.  One upload from pinned staging (the control image, the
 * descriptors, the own-job lists and the tasks' victim headers), one copy
 * back, one wait.
 * The call changes the currency of the candidate table and of the victim
 * state and the plugins' open state, and nothing else: no node row, no counter
 * of kbhip_walk_visits, and a task kbhip_fit_deltas would answer for stays
 * answerable.  kbhip_stats.sweeps and kbhip_stats.rank_heads count one per
 * answered task.  The whole batch is validated before any device work, and a
 * refused call writes nothing.  KBHIP_EINVAL: a null session, task_ids,
 * out_total, out_node, out_count, out_evict, out_flags or out_victim; n_tasks
 * outside 0 .. 64, cap outside 1 .. 64, stride < 1, by_score not 0 or 1,
 * victims outside 1 .. 3; a task without a class, not Pending or without a job
 * (the message names the index in task_ids); an encode-only session; submitted
 * pops outstanding.  KBHIP_EUNSUPPORTED: where kbhip_head_victims and
 * kbhip_rank_heads refuse; the cap staging rows of one task above
 * "victims_spill_max" (the message names the size). */
#define KBHIP_HEADS_VICTIMS_MAX 64
int64_t kbhip_heads_victims(kb_session* s, const int32_t* task_ids, int32_t n_tasks, int32_t by_score,
                            int32_t victims /* KBHIP_VICTIMS_* 1..3 */, int32_t cap /* 1..64 */,
                            int32_t stride /* >= 1 */, int64_t* out_total /* n_tasks */,
                            int32_t* out_node /* n_tasks rows of cap */, int32_t* out_score /* optional */,
                            int32_t* out_count, int32_t* out_evict, uint8_t* out_flags /* n_tasks rows of cap */,
                            int32_t* out_victim /* n_tasks * cap rows of stride */,
                            int32_t* out_first /* optional, n_tasks */, int64_t* out_info /* optional, 6 */);

/* kbhip_walk_victims <- one task's whole node loop of preempt()
 * (preempt.go:259-353) or of reclaim (reclaim.go:115-189) over the head of its
 * pruned walk, in one call: the finished batch for kbhip_apply_ops.
 * The head is the one kbhip_head_victims(task, by_score, victims, ..) ranks for
 * the session as it stands.  Its entries are visited in order, and on each the
 * call decides what kbhip_head_victims' row says — against the plugin state as
 * the evictions of the earlier entries of this same call leave it:
 *   no KBHIP_HEAD_VICTIMS_VALID  the node is passed over.
 *   KBHIP_HEAD_VICTIMS_VALID     one KBHIP_OP_EVICT per victim of the evicted
 *     prefix is appended, in victim order, out_node = that node.
 *   and KBHIP_HEAD_VICTIMS_COVERS  KBHIP_OP_PIPELINE task, node follows and the
 *     walk stops with KBHIP_WALK_ASSIGNED.
 *   otherwise  the evictions are carried — each victim's job: drf's allocation
 *     minus Resreq, gang's readyTaskNum minus one; its queue: proportion's
 *     allocation minus Resreq; with KBHIP_VICTIMS_SAME_JOB the preemptor's own
 *     allocation too (drf.go:88-90) — and the walk goes on: the reference's
 *     loop evicts from such a node and tries the next one.
 * Returns the ops written.  out_op / out_pod / out_node can be passed unchanged
 * to kbhip_apply_ops; that batch leaves the session where the reference's loop
 * leaves it for this task.  The walk order is fixed before the first eviction
 * (no ranking reads Releasing), as the reference ranks once per task.
 * `cap` bounds the head entries decided in this call.  after_node >= 0 resumes:
 * head entries whose key is not below the key the head sweep forms for
 * (after_score, after_node) — the score is ignored with by_score 0, where the
 * sweep's keys carry none — are passed over undecided and uncounted: the nodes
 * the loop has left behind.  A host resumes after KBHIP_WALK_CAPACITY (apply the
 * ops, call again after out_info[4] / out_info[5]) and after
 * KBHIP_WALK_HEAD_END while the resume point is inside the new 64-entry head;
 * past the head kbhip_walk_victims_from (below) goes on.
 * A step is all or nothing: when a valid node's prefix plus one slot for a
 * possible pipeline does not fit what is left of cap_ops, or a node the walk
 * would go on from touches more distinct jobs or queues than the carried state
 * holds (256 jobs, 64 queues; option "walk_overlay_max" = k, tests, lowers
 * both to k, 0 = full), the walk stops before that node with
 * KBHIP_WALK_CAPACITY and the ops written are a prefix of the uncapped answer.
 * So that a resumed walk always moves on, the first node a call acts on is
 * taken even when the carried state cannot hold what it touches: its ops are
 * written and the walk stops behind it with KBHIP_WALK_CAPACITY.  (cap_ops
 * below the first step's need has no such way out: KBHIP_WALK_CAPACITY with
 * no node acted on asks for a larger cap_ops.)
 * out_info (optional, 8 entries): [0] the stop reason, [1] the total of the
 * pruned walk (kbhip_head_victims' return value), [2] head entries decided,
 * [3] nodes acted on, [4] the last acted-on node (-1: none), [5] its score (0
 * with by_score 0 or none), [6] kernel launches (kbhip_head_victims' head
 * launches, then one), [7] bit 0: the candidate table was rebuilt, bit 1: the
 * victim state was rebuilt, bits 8 and up: the records patched into it.
 * Read-only as kbhip_head_victims: the carried state lives inside the launch
 * and is discarded; the call changes the currency of the two tables and the
 * plugins' open state, nothing else.  The whole call is validated before any
 * device work, and a refused call writes nothing.  KBHIP_EINVAL: as
 * kbhip_head_victims, cap_ops < 1, a null out_op, out_pod or out_node,
 * after_node outside -1 .. nodes - 1.  KBHIP_EUNSUPPORTED: where
 * kbhip_head_victims refuses. */
#define KBHIP_WALK_ASSIGNED  1 /* a node covered InitResreq: the last op is the task's KBHIP_OP_PIPELINE */
#define KBHIP_WALK_EXHAUSTED 2 /* every node of the walk was visited, none covered */
#define KBHIP_WALK_HEAD_END  3 /* `cap` head entries (or the 64-entry head) used up, the walk has more nodes */
#define KBHIP_WALK_CAPACITY  4 /* the next node's evictions would not fit cap_ops, or the carried state is full */
int64_t kbhip_walk_victims(kb_session* s, int32_t task_id, int32_t by_score, int32_t victims /* KBHIP_VICTIMS_* */,
                           int32_t cap /* 1..64 head entries to visit */,
                           int32_t after_node /* -1: from the top */, int32_t after_score,
                           uint8_t* out_op, int32_t* out_pod, int32_t* out_node, int64_t cap_ops,
                           int64_t* out_info /* optional, 8 */);

/* kbhip_walk_victims_from <- the same node loop over a walk of any length, one
 * window of up to 64 entries per call.
 * The window is the first up to 64 entries of the task's pruned walk
 * (kbhip_rank_victim_nodes' order and test, on the session as it stands) among
 * the nodes whose key is below the resume key: the key the head sweep forms for
 * (after_score, after_node), the score ignored with by_score 0, where the
 * sweep's keys carry none.  Nodes at or above the resume key take no window
 * slot and are not counted.  after_node -1: no bound — the window is
 * kbhip_walk_victims' head.
 * The window's first min(cap, 64) entries are decided in order with
 * kbhip_walk_victims' semantics, unchanged: an entry that is not VALID is passed
 * over, a VALID node's prefix is evicted, a COVERS node also pipelines the task
 * and stops the walk with KBHIP_WALK_ASSIGNED, otherwise the evictions are
 * carried to the entries after it.  cap_ops, the all-or-nothing steps, the
 * carried state's capacities (option "walk_overlay_max"), "the first node a call
 * acts on is taken" and the op format for kbhip_apply_ops are kbhip_walk_victims'.
 * Stop reasons: KBHIP_WALK_ASSIGNED and KBHIP_WALK_CAPACITY as there;
 *   KBHIP_WALK_EXHAUSTED  every node behind the resume point was decided.
 *   KBHIP_WALK_HEAD_END   `cap` or 64 window entries are used up and nodes
 *     remain behind them: apply the ops (if any) and call again from
 *     out_info[4] / out_info[5].
 * The resume point a call returns is the last window entry it passed over or
 * acted on; a node before which the walk stopped with KBHIP_WALK_CAPACITY is not
 * behind it, so the next call meets that node again.  When no entry was passed
 * over or acted on it is the call's own after_node / after_score.
 * Host protocol: call, send the ops through kbhip_apply_ops, and after
 * KBHIP_WALK_HEAD_END or KBHIP_WALK_CAPACITY call again from out_info[4] /
 * out_info[5]; the loop reaches KBHIP_WALK_ASSIGNED or KBHIP_WALK_EXHAUSTED for
 * a walk of any length, and the concatenated ops are the reference's for that
 * task: one ranking and one node loop.  Within a window the walk order is
 * fixed before the first eviction, as in kbhip_walk_victims.  One limit:
 * between two windows the host has applied evictions, and the next window is
 * ranked on the session as it then stands, where the reference ranks once
 * per task.  That is the
 * rank-once order wherever kbhip_walk_victims' own resume is — no ranking reads
 * Releasing, and the victim test of the nodes behind the resume point is
 * untouched — except for task classes whose predicates read pod-affinity
 * targets that an applied eviction removed: for those a node behind the resume
 * point can enter or leave the later windows.
 * out_info (optional, 10 entries): [0] the stop reason, [1] the entries of the
 * pruned walk behind the resume point at the call (the bounded sweep's passing
 * count), [2] entries decided (counted as kbhip_walk_victims counts them: a
 * node refused with KBHIP_WALK_CAPACITY included), [3] nodes acted on, [4] the
 * resume point's node (-1: from the top), [5] its score (0 with by_score 0),
 * [6] kernel launches (kbhip_walk_victims' and one: the pre-pass that decides
 * the window's entries side by side), [7] as kbhip_walk_victims' [7], [8] the
 * last acted-on node (-1: none), [9] the window index of the first entry whose
 * decision against the session as it stands is VALID (-1: none: the walk
 * passes over all of them without its serial loop).
 * Read-only as kbhip_walk_victims.  The whole call is validated before any
 * device work, and a refused call writes nothing.  KBHIP_EINVAL and
 * KBHIP_EUNSUPPORTED: as kbhip_walk_victims. */
int64_t kbhip_walk_victims_from(kb_session* s, int32_t task_id, int32_t by_score, int32_t victims /* KBHIP_VICTIMS_* */,
                                int32_t cap /* 1..64 window entries to decide */,
                                int32_t after_node /* -1: from the top */, int32_t after_score,
                                uint8_t* out_op, int32_t* out_pod, int32_t* out_node, int64_t cap_ops,
                                int64_t* out_info /* optional, 10 */);

/* kbhip_walk_begin / kbhip_walk_next / kbhip_walk_order / kbhip_walk_end <- the
 * same node loop over a walk that is ranked once and kept: the eviction-walk
 * cursor.  A session holds one cursor; kbhip_walk_begin replaces it.
 * kbhip_walk_begin ranks the task's pruned walk once — exactly the order and
 * the victim test of kbhip_rank_victim_nodes(task, by_score, victims, ..) on its
 * full-sort path, on the session as it stands — keeps the ranked keys in a
 * device buffer of the cursor's own, which no other call writes, and returns the
 * walk's total T.  out_info (optional, 4 entries): [0] kernel launches
 * (kbhip_rank_victim_nodes' full-path count: the sort's, the compaction's three,
 * and one when pod-affinity count changes were pending), [1] whether the
 * candidate table was rebuilt, [2] the device bytes the cursor keeps, [3] 1 when
 * the task's class has predicates that read pod-affinity targets (see "Order").
 * KBHIP_EINVAL, KBHIP_EUNSUPPORTED and KBHIP_EDEVICE (a score outside the class
 * range) as kbhip_rank_victim_nodes; a task without a job is refused too.  A
 * call that fails before it overwrites the kept keys — every refusal, and
 * KBHIP_EUNSUPPORTED — leaves an open cursor as it was; after a later failure
 * none is open.
 * kbhip_walk_next decides entries [pos, T) of the kept order in two launches.
 * The scan decides every one of them side by side against the session as it
 * stands (kbhip_head_victims' decision, nothing carried) and yields `first`: the
 * lowest position whose decision is KBHIP_HEAD_VICTIMS_VALID.  The entries
 * [pos, first) are passed over and counted: no eviction of this call precedes
 * them, so that answer is the walk's.  From `first` the serial loop of
 * kbhip_walk_victims runs over at most `cap` entries — the entry at `first`
 * too is decided by it, and no entry behind it by the scan: carried evictions
 * can turn a node that was not VALID into one that is.  cap_ops, the
 * all-or-nothing steps, the carried state's capacities (option
 * "walk_overlay_max"), "the first node a call acts on is taken" and the op
 * format for kbhip_apply_ops are kbhip_walk_victims'.  (An entry whose node holds
 * more candidate tasks than a block stages in LDS, 256, is not decided by the
 * scan: it counts as `first`, and the serial loop decides it exactly and passes
 * it over if it is not VALID.)
 * Stop reasons: KBHIP_WALK_ASSIGNED and KBHIP_WALK_CAPACITY as there;
 *   KBHIP_WALK_EXHAUSTED  position T was reached.
 *   KBHIP_WALK_HEAD_END   `cap` serial entries are used up and entries remain.
 * out_info (optional, 10 entries): [0] the stop reason, [1] T, [2] entries
 * decided — passed over plus visited, a node refused with KBHIP_WALK_CAPACITY
 * counted as kbhip_walk_victims counts it — [3] nodes acted on, [4] the next
 * position: behind the last entry passed over or acted on (a node refused with
 * KBHIP_WALK_CAPACITY is met again), [5] `first` (-1: none), [6] kernel launches
 * (2, plus one when records were patched into the victim state and one when
 * pod-affinity count changes were pending), [7] as kbhip_walk_victims' [7],
 * [8] the last acted-on node (-1: none), [9] the entries the scan decided
 * (informational: a block behind a `first` already found may leave undecided,
 * so first - pos + 1 <= [9] <= T - pos when `first` exists).
 * Returns the ops written; one copy back, one wait.
 * Host protocol: kbhip_walk_begin; then kbhip_walk_next(pos = 0), kbhip_apply_ops,
 * kbhip_walk_next(out_info[4]) .. until KBHIP_WALK_ASSIGNED or
 * KBHIP_WALK_EXHAUSTED.  One ranking per task, and a task that can act on no
 * node is settled by the second call.
 * kbhip_walk_order copies entries [first, first + cap) of the kept order (the
 * nodes; the scores with by_score 1, else 0) and returns T: what a host logs.
 * kbhip_walk_end drops the cursor: 1, or 0 when none was open.
 * Order.  With by_score 1 the kept order is the reference's for every task
 * class: preempt.go:270-288 evaluates the predicates and the scores once,
 * before the node loop.  With by_score 0 the reference tests the predicate at
 * each node as its loop reaches it (reclaim.go:115-117), and the cursor fixed
 * the node set at kbhip_walk_begin; the two differ only for task classes whose
 * predicates read pod-affinity targets that an applied eviction removed.
 * kbhip_walk_begin's out_info[3] names such a class, and for it (by_score 0)
 * kbhip_walk_begin_live below is the exact call.  Pruning is not affected: the
 * evictions of this walk take candidates only off nodes in front of the next
 * position, and a node that other evictions made prunable merely stays in the
 * order and is decided not VALID.
 * Lifetime.  The cursor survives a successful kbhip_apply_ops and every
 * read-only call (the rankings, head, victims, explain and walk queries,
 * kbhip_sweep_scores, stats, read-backs).  Every call that leaves the candidate
 * table and the victim state stale drops it: the actions, kbhip_place_job and
 * its asynchronous forms, kbhip_first_fit, the carry-overs, a kbhip_apply_ops
 * that failed part way; so do kbhip_walk_end, kbhip_walk_begin and
 * kbhip_session_close.
 * Read-only as kbhip_walk_victims.  Each call is validated before any device
 * work, and a refused call writes nothing.  KBHIP_EINVAL (kbhip_walk_next,
 * kbhip_walk_order): no cursor open; kbhip_walk_next also: the cursor's task is
 * no longer Pending (its own KBHIP_OP_PIPELINE was applied), pos outside 0 .. T,
 * cap outside 1 .. 64, cap_ops < 1, a null out_op, out_pod or out_node, an
 * encode-only session, submitted pops outstanding.  KBHIP_EUNSUPPORTED: a
 * node-sharded session. */
int64_t kbhip_walk_begin(kb_session* s, int32_t task_id, int32_t by_score, int32_t victims /* KBHIP_VICTIMS_* */,
                         int64_t* out_info /* optional, 4 */);
int64_t kbhip_walk_next(kb_session* s, int64_t pos, int32_t cap /* 1..64 serial entries */,
                        uint8_t* out_op, int32_t* out_pod, int32_t* out_node, int64_t cap_ops,
                        int64_t* out_info /* optional, 10 */);
int64_t kbhip_walk_order(kb_session* s, int64_t first, int32_t* out_node, int32_t* out_score /* optional */, int64_t cap);
int     kbhip_walk_end(kb_session* s);   /* 1: a cursor was dropped, 0: none was open */

/* kbhip_walk_begin_live <- the cursor opened for reclaim's loop (by_score 0) so
 * that it is exact for every task class: reclaim.go:115-117 tests PredicateFn at
 * each node as the loop reaches it, after the evictions of the nodes before.
 * A class whose predicates read no pod-affinity targets: the call is
 * kbhip_walk_begin(task, 0, victims, ..) in every respect — the kept order,
 * out_info, and what kbhip_walk_next does.
 * A class whose predicates read pod-affinity targets: the cursor is live.  The
 * kept order holds, node index ascending and in by_score 0's key format, every
 * node that passes the class's predicates with the pod-affinity predicate left
 * out (static predicates, pod count and host ports as the by_score 0 ranking
 * tests them) and kbhip_rank_victim_nodes' victim-candidate test; T is that
 * count, at least kbhip_walk_begin's.  No sort runs: out_info[0] counts the
 * launches made (the marks, the compaction's three, one for pending
 * pod-affinity count changes), [1] and [2] as kbhip_walk_begin, [3] is 2.
 * On a live cursor kbhip_walk_next tests the pod-affinity predicate itself, on
 * the count tables as they stand when the call starts (every applied eviction
 * included):
 *   - an entry is VALID only where the predicate holds for its node and the
 *     victims decision is VALID: the scan forms `first` by that rule.  A node of
 *     more than 256 candidate tasks still counts as `first` undecided, the
 *     predicate included.
 *   - the serial loop tests the predicate before it stages an entry; an entry
 *     that fails is passed over, counted in [2] and gives no op.
 *   - the call ends behind the first node it acts on, so [3] is 0 or 1: its
 *     evictions change the predicate's count tables only through
 *     kbhip_apply_ops, and the next call reads them.  The stop reason is then
 *     KBHIP_WALK_ASSIGNED when that node covers, else KBHIP_WALK_HEAD_END while
 *     entries remain and KBHIP_WALK_EXHAUSTED at T (KBHIP_WALK_CAPACITY where
 *     that first step could not be carried, as for every walk call).  A call
 *     that acts on nothing stops as on any cursor.
 * out_info keeps its ten meanings ([4] the next position).  The host protocol is
 * the cursor's; it pays one call per node acted on.  kbhip_walk_order,
 * kbhip_walk_end, the lifetime rules, the refusals (a failure before the kept
 * keys are overwritten leaves an open cursor as it was) and KBHIP_EUNSUPPORTED
 * on a node-sharded session are kbhip_walk_begin's. */
int64_t kbhip_walk_begin_live(kb_session* s, int32_t task_id, int32_t victims /* KBHIP_VICTIMS_* */,
                              int64_t* out_info /* optional, 4 */);

/* kbhip_explain_tasks <- why each node is, or is not, a node of the allocate
 * walk of up to KBHIP_EXPLAIN_MAX pending tasks, on the session as it stands:
 * what the reference logs node by node (allocate.go:128-137, the error
 * ssn.PredicateFn returned) and what its loop then decides.  For task_ids[i]
 * and node n the verdict byte out_verdict[i * n_nodes + n] is the code of the
 * first step that rejects the node, in the reference's order
 * (predicates.go:123-203, then allocate.go:139-146): a node that is
 * unschedulable, tainted and full is KBHIP_WHY_POD_COUNT.  A node no step
 * rejects is in the walk and gets KBHIP_WHY_FITS_IDLE (allocate.go:153 holds:
 * it would be Allocated), KBHIP_WHY_FITS_RELEASING (only allocate.go:173
 * holds: Pipelined) or KBHIP_WHY_RESOURCES (neither), or-ed with the
 * KBHIP_WHY_SHORT_* bits of the resources in which Idle.FitDelta(Resreq) is
 * negative (resource_info.go:134-147; Idle taken as Idle + Backfilled, as
 * kbhip_fit_deltas takes it).  With the predicates plugin off the codes 3..8
 * never occur.  A node's code is in 0..2 exactly where kbhip_sweep_scores
 * gives it a non-zero key.
 * out_hist[i * KBHIP_EXPLAIN_BINS + c], c in 0..9 = the nodes with code c;
 * [10] = 0; [11..13] = the nodes in the walk with the cpu / memory / GPU
 * short bit; [14] = the nodes in the walk; [15] = the node count.  For a task
 * that finds no node ([0] == [1] == 0), [14] and [11..13] are the numbers of
 * JobInfo.FitError (job_info.go:343-372) and [3..9] the reasons of every node
 * that message leaves out.  The library renders no message: the host formats
 * them from these counts.
 * out_verdict is optional (null: no per-node byte is written anywhere, the
 * histogram is the same).  out_info (optional, 3 entries) = the kernel
 * launches issued (2, plus one when pod-affinity count changes of earlier
 * kbhip_apply_ops were still to be applied — they are applied first), the x
 * size of the sweep's grid, whether verdict rows were written.  A task may
 * appear more than once; classes of every kind mix freely.
 * The call is read-only: no node row, no kbhip_walk_visits counter changes,
 * and a task kbhip_fit_deltas would answer for stays answerable.  The whole
 * batch is validated before any device work, and a refused call writes
 * nothing.  Returns n_tasks (0 for n_tasks == 0, which does nothing).
 * KBHIP_EINVAL: a null session, null task_ids or out_hist with n_tasks > 0;
 * n_tasks outside 0 .. KBHIP_EXPLAIN_MAX; a task without a class or not
 * Pending (the message names the index in task_ids); an encode-only session;
 * submitted pops outstanding.  KBHIP_EUNSUPPORTED: a node-sharded session.
 * Option "explain_blocks" = k (tests; 0 = automatic) caps the sweep's grid x. */
#define KBHIP_WHY_FITS_IDLE      0  /* in the walk; allocate.go:153 holds -> would be Allocated */
#define KBHIP_WHY_FITS_RELEASING 1  /* in the walk; only allocate.go:173 holds -> would be Pipelined */
#define KBHIP_WHY_RESOURCES      2  /* in the walk; neither fit holds (allocate.go:164-170) */
#define KBHIP_WHY_POD_COUNT      3  /* predicates.go:127 */
#define KBHIP_WHY_NODE_SELECTOR  4  /* predicates.go:132-143: nodeSelector or required node affinity */
#define KBHIP_WHY_HOST_PORTS     5  /* predicates.go:146-157 */
#define KBHIP_WHY_UNSCHEDULABLE  6  /* predicates.go:160-171 */
#define KBHIP_WHY_TAINTS         7  /* predicates.go:174-185 */
#define KBHIP_WHY_POD_AFFINITY   8  /* predicates.go:188-200, including the task's own invalid selector
                                       (TaskClass::pred_err: the error is returned at this step) */
#define KBHIP_WHY_SCORE_ERROR    9  /* predicates pass, NodeOrderFn errors (allocate.go:140-145, score_err) */
#define KBHIP_WHY_SHORT_CPU 0x10    /* codes 0..2 only: FitDelta(Resreq) negative in cpu / memory / GPU, */
#define KBHIP_WHY_SHORT_MEM 0x20    /* exactly fit_bits' bits 1..3 (resource_info.go:134-147,            */
#define KBHIP_WHY_SHORT_GPU 0x40    /* Idle taken as Idle + Backfilled, as kbhip_fit_deltas takes it)     */
#define KBHIP_EXPLAIN_MAX 64
#define KBHIP_EXPLAIN_BINS 16
int64_t kbhip_explain_tasks(kb_session* s, const int32_t* task_ids, int32_t n_tasks,
                            uint8_t* out_verdict /* optional, n_tasks rows of n_nodes */,
                            int64_t* out_hist   /* n_tasks rows of KBHIP_EXPLAIN_BINS */,
                            int64_t* out_info   /* optional, 3 */);

/* Measurement hook (bench.py's sweep roofline): kbhip_sweep_scores' sweep
 * kernel for each given task, launched back to back on the session stream
 * with no copies in between; *out_mean_us = device time per launch (one
 * HIP-event pair around the sequence, launch boundaries included).  Changes
 * nothing.  KBHIP_EUNSUPPORTED for classes with inter-pod priority terms
 * (their sweep needs a min / max prepass per task). */
int kbhip_time_sweeps(kb_session* s, const int32_t* task_ids, int32_t n, double* out_mean_us);

/* Measurement entry (config C5): the preempt node ranking
 * (PredicateFn + NodeOrderFn sweep + stable counting sort) of n what-if
 * sessions on one device as ONE multi-session launch chain (blockIdx.y =
 * session, each on its own node columns), session i for its pending task
 * task_ids[i]; launched reps times (evict 0: back to back; 2: each behind a
 * 512 MB cache-evicting read), descriptors copied to device memory (mapped 0)
 * or read in place from pinned mapped host memory (1).  *out_us = device
 * microseconds per chain (HIP events).  Classes of the one-pass counting sort
 * only (score range < 256, no inter-pod terms), else KBHIP_EUNSUPPORTED. */
int kbhip_time_rank_multi(kb_session* const* sessions, int32_t n, const int32_t* task_ids, int32_t reps,
                          int32_t evict, int32_t mapped, double* out_us);

/* Run the reclaim action (actions/reclaim/reclaim.go:41-196) / the preempt
 * action (actions/preempt/preempt.go:43-353) on the session's current state.
 * Output records in decision order: (pod, node, KBHIP_EVICTED) for every
 * eviction that reaches the cache (reclaim: each ssn.Evict; preempt: the
 * evictions of a committed Statement, in operation order) and
 * (pod, node, KBHIP_PIPELINED) for every pipelined preemptor (reclaim: each
 * ssn.Pipeline; preempt: those of a committed Statement).  Discarded
 * statements leave no record (and, like the reference, leave the victims'
 * node copies Releasing).  Returns the record count.  On node-sharded
 * sessions every rank calls it collectively and returns the same records:
 * each rank ranks its own nodes, the sorted lists are all-gathered
 * (kbhip_shard_connect_host_gather or kbhip_shard_connect_rccl is required,
 * else KBHIP_EINVAL) and merged, and evictions / pipelines change the rows of
 * the owning rank only.
 * Replaces the reference's reclaimAction.Execute / preemptAction.Execute.
 * If an action fails part-way (negative return) the session's host model may
 * hold a partial action: close it and open a new one. */
int kbhip_reclaim(kb_session* s, int32_t* out_pod, int32_t* out_node, uint8_t* out_kind, int64_t cap);
int kbhip_preempt(kb_session* s, int32_t* out_pod, int32_t* out_node, uint8_t* out_kind, int64_t cap);

/* Carry the session over to the next scheduling session (SURVEY §8(f) row 3,
 * the delta path of cache.go:515-583's per-session Snapshot): the state the
 * scheduler cache holds once this session's binds and evictions reached it —
 * dispatched tasks Bound on their nodes, Allocated-not-dispatched and
 * Pipelined tasks Pending again, evicted pods Releasing — with node rows
 * recomputed on the host and only the changed row runs uploaded (no snapshot
 * parse, no re-encode).  The session can then run its actions again.
 * *out_uploaded_bytes (optional) = bytes sent to the device.  Pod
 * (anti-)affinity count tables are recounted from the carried pod states.
 * On a node-sharded session every rank carries (identically on its
 * replicated host model; each uploads its own rows; no collective).  Pod
 * arrivals, node and PodGroup changes: kbhip_session_carry_snapshot. */
int kbhip_session_carry(kb_session* s, int64_t* out_uploaded_bytes);

/* kbhip_session_carry plus the scheduler cache's events on existing pods
 * between the two sessions (pkg/scheduler/cache/event_handlers.go), applied
 * in order after the carry:
 *   KBHIP_EV_DELETE — deletePod -> deleteTask on NewTaskInfo(pod)
 *     (event_handlers.go:119-165).  A pod of a PodGroup leaves its job and
 *     its node.  A group-less pod's TaskInfo has an empty Job
 *     (api/job_info.go:60-70), so the cache keeps it in its shadow job with
 *     its status and NodeName and only takes it off its node (the pod is
 *     "detached", kbsnap.h p_detached: it still counts for its job's
 *     readiness and the drf / proportion shares; a pending one is allocated
 *     again).  No job is deleted (JobTerminated needs a nil PodGroup).
 *   KBHIP_EV_SUCCEEDED / KBHIP_EV_FAILED — updatePod to a terminal phase
 *     (isTerminated: the task stays in its job, its node no longer counts it).
 * pods[i] are pod indices of the opened snapshot (they stay the session's pod
 * ids; a deleted pod never appears in a later record).  Every event is
 * validated first (KBHIP_EINVAL: index out of range, unknown event, an event
 * on a deleted or detached pod; KBHIP_EUNSUPPORTED: detaching a pod in a
 * session with pod (anti)-affinity terms — the predicate lister's
 * NodeInfo.Filter would leave it out at its own node only) and nothing
 * changes on error. */
enum { KBHIP_EV_DELETE = 1, KBHIP_EV_SUCCEEDED = 2, KBHIP_EV_FAILED = 3 };

/* The next scheduling session from the scheduler cache's snapshot of it
 * (cache.go:515-583 after the informer events of event_handlers.go: pod
 * arrivals, deletions and phase changes, node add / update / delete, PodGroup
 * and queue add / update), re-deriving only what changed.  kbs: the new KBS1
 * snapshot (canonical order, kbsnap.h); old_pod[i] / old_node[n]: the index
 * in THIS session of the new snapshot's pod i / node n, -1 for a new object
 * (a pod whose spec or labels changed — updatePod re-adds it, event_handlers.go
 * :101-110 — is new too).  Afterwards the session's pod and node indices are
 * the new snapshot's.  Fast path when the node set, node labels / taints and
 * the conf are unchanged, no pod carries pod (anti-)affinity terms and new
 * pods have no host ports, nodeSelector or node affinity: mapped pods keep
 * their dictionary ids and task classes, new pods are classed against the
 * kept dictionaries, jobs / queues / plugin state and node rows are
 * re-derived, and only node rows that differ (plus grown class tables) are
 * uploaded.  Any other change re-opens the session in place (same handle,
 * same options; *out_uploaded_bytes = -1).  KBHIP_EUNSUPPORTED on
 * node-sharded sessions; KBHIP_EINVAL for a malformed map.  On error the
 * session may hold a partial state: close it. */
int kbhip_session_carry_snapshot(kb_session* s, const void* kbs, size_t len, const int32_t* old_pod,
                                 const int32_t* old_node, int64_t* out_uploaded_bytes);
int kbhip_session_carry_events(kb_session* s, const int32_t* pods, const uint8_t* events, int64_t n,
                               int64_t* out_uploaded_bytes);

/* Read the device node state: N x 12 int64 (idle, used, releasing,
 * backfilled; cpu/mem/gpu each) of the session's nodes (a shard session: its
 * range [lo, hi) only).  `used` is maintained on the host mirror. */
int kbhip_read_nodes(kb_session* s, int64_t* out, int64_t n_nodes);

int kbhip_get_stats(kb_session* s, kbhip_stats* out);

/* Engine knobs: "batched" = 0 forces the per-task sweep path (tests);
 * "time_every" = k times every k-th sweep launch with HIP events;
 * "bf_batch" = 1 (default) batches pops in sessions with Backfilled nodes
 * (placement 6), 0 = per-task sweeps there;
 * "aff_batch" = 1 (default) batches pops of pod anti-affinity classes
 * (placement 7), 0 = per-task sweeps for them;
 * "aff_fence" = 1 (default) orders a placement-7 pop behind the overlapped
 * pops before it on the device (stream events; the host keeps predicted pops
 * queued), 0 = the host drains the overlap streams first;
 * "rank_radix" = 1 orders reclaim / preempt walks with the wide-range radix
 * passes (four 8-bit counting passes over the score) instead of the one-pass
 * counting sort (tests);
 * "rank_group" = 1 makes this session one of a group of what-if sessions
 * run from concurrent host threads: their allocate pops of placements 6 / 7,
 * their per-task chunks and their reclaim / preempt node rankings are issued
 * as shared multi-session launches (blockIdx.y = session): each request is
 * issued at once together with whatever other sessions' requests are pending
 * (no session waits for another; kbhip_stats
 * rank_batch_sum / rank_requests, pop_batch_sum / pop_requests and
 * sweep_batch_sum / sweep_requests (per-task chunks: allocate's general path
 * and backfill first-fits, k_sweep_argmax_multi) = requests
 * per launch);
 * "rank_first" = k: reclaim / preempt read the first k sorted keys with the count;
 * "keys32" = 1 (default) uses 32-bit selection keys in the batched sweep
 * when the class's score range and the node count fit (same order as the
 * 64-bit key), 0 = always 64-bit;
 * "speculate" = 4 (default) lets kbhip_allocate queue up to that many
 * predicted next job pops behind the running one (0..6; each used only if it
 * is exactly the next pop, retracted on device otherwise: placements are
 * unchanged), 0 = one pop at a time;
 * "engine" = 1 (default) serves eligible batched pops with the persistent pop
 * engine (one resident kernel, a descriptor ring), 0 = launched kernels;
 * "engine_workers" = n caps its worker blocks (0: as many as stay resident);
 * "engine_groups" = g its merger blocks (-1: automatic, 0: none);
 * "engine_lists" = 1 runs the engine in list mode when every eligible class
 * fits (one owner block per task class keeps the class's key of every node,
 * updated from the rows each pop touches), 0 (default) =
 * sweep mode (worker blocks sweep every node per pop);
 * "overlap" = k rotates batched pops over k + 1 streams so that a pop's sweep
 * runs beside the previous k pops' placements, chained on the device (1, the
 * default, or 2); 0 = one stream, one pop kernel at a time;
 * "shard_overlap" = 1 (node-array shards with peer mailboxes and "overlap" >
 * 0): a shard's sweep of pop e runs beside pop e-1's placement, leaving that
 * pop's candidates out and re-evaluating them once its write-back is done;
 * 0 (default) = sweep, exchange and placement one after another;
 * "debug_keys" = 1 records every per-task sweep's per-node keys (tests,
 * read back with kbhip_debug_table "dbg_keys" / "dbg_pods").
 * Measurement and rehearsal options (not part of a scheduler's use):
 * "sweep_variant" = 0..6 the kernel shape of kbhip_sweep_scores (process-wide;
 * 0 default, 4..6 grid-stride forms);
 * "time_sweeps_cold" = 0 warm, 1 write-evict, 2 read-evict the caches before
 * each launch kbhip_time_sweeps times;
 * "group_linger_us" = t (process-wide, tests) keeps a what-if batch open for
 * up to t µs for more sessions' requests;
 * "cu_split" = part * 256 + parts runs this session's streams on CUs
 * [part * C / parts, (part + 1) * C / parts) of the device's C (one-GPU
 * rehearsals of node-array shards).  "time_sweeps_cold" and
 * "cu_split" are not kept across the re-open of
 * kbhip_session_carry_snapshot's slow path. */
int kbhip_set_option(kb_session* s, const char* key, int64_t value);

/* The gang plugin's OnSessionClose after kbhip_allocate (plugins/gang/gang.go:
 * 166-187): the PodGroup Unschedulable condition message of every job that
 * is not Ready — "<m>/<n> tasks in gang unschedulable: <JobInfo.FitError>"
 * (job_info.go:343-372), the FitError from the job's NodesFitDelta as
 * allocate.go:124-126 / 164-167 leave it — one line "<job uid>\t<message>\n"
 * per job, in job UID order; empty when the gang plugin is not in the tiers.
 * Returns the text length; copies it (NUL-terminated) when cap > length. */
int64_t kbhip_gang_unschedulable(kb_session* s, char* out, int64_t cap);

/* Read-outs of the allocate walk (allocate.go:149-185), for a host that keeps
 * the reference's own NodeInfo and JobInfo objects beside the engine.
 *
 * kbhip_walk_visits <- the GetAccessibleResource side effect (node_info.go:
 *   209-211: Idle.Add(Backfilled) mutates Idle in place): every node a task's
 *   walk reaches — the nodes ahead of the chosen one and the chosen one, or
 *   every node of the walk when the task finds none — gets Backfilled added to
 *   its Idle once per visit.  The device applies this to its own Idle column
 *   and counts the visits of every node whose Backfilled is not zero (on the
 *   others the call changes nothing).  The call returns the nodes with a
 *   non-zero count since the previous call, in ascending node index, with
 *   their counts (out_node / out_count, `cap` entries each), clears the
 *   counters it returned and returns the number of entries.  When cap is
 *   smaller than that number (null outputs with cap 0: the size query) only
 *   the number is returned and nothing is cleared.  A host applies
 *   node.GetAccessibleResource() out_count[i] times to node out_node[i] before
 *   it applies the pop's placements; per node, at any quiescent point,
 *     Idle == Idle at open + visits x Backfilled - committed requests.
 *   The backfill, reclaim and preempt actions never call
 *   GetAccessibleResource.  A count multiplies the node's Backfilled as it is
 *   when the host applies it: where a session places backfill-annotated
 *   pending tasks (which raise Backfilled) the counts are read after every
 *   pop.  The counters restart at every carry-over.
 * kbhip_fit_deltas <- job.NodesFitDelta of a task that found no node
 *   (allocate.go:164-167): for the task on which the session's most recent job
 *   pop stopped with KBHIP_STOP_UNASSIGNED (kbhip_place_job / _wait, or the
 *   last pop inside kbhip_allocate), one record per node that passed
 *   PredicateFn and got a NodeOrderFn score — each was visited and did not
 *   fit — in ascending node index: out_node[i] and out_delta[3 i ..] = (cpu,
 *   memory, GPU) of node.Idle.Clone().FitDelta(task.Resreq)
 *   (resource_info.go:134-147: Idle - (Resreq + min) where Resreq > 0, else
 *   Idle), Idle after the walk's own visit.  Nothing is committed after such a
 *   walk, so the records are computed from the current node state by one sweep
 *   that compacts them on the device; only the records are copied back.
 *   Returns their number; copies when cap is at least that.  KBHIP_EINVAL for
 *   any other task_id, and after any later call that runs an action, places a
 *   job or carries the session.  A pop that places every given task and leaves
 *   its job not Ready (KBHIP_STOP_ALL) is not covered: there NodesFitDelta
 *   holds the nodes ahead of the last task's chosen node, which only the state
 *   at walk time gives exactly; kbhip_gang_unschedulable's histogram text
 *   remains the source for those jobs.
 * Both fail with KBHIP_EINVAL while submitted pops are outstanding and with
 * KBHIP_EUNSUPPORTED on node-sharded sessions. */
int64_t kbhip_walk_visits(kb_session* s, int32_t* out_node, uint32_t* out_count, int64_t cap);
int64_t kbhip_fit_deltas(kb_session* s, int32_t task_id, int32_t* out_node, int64_t* out_delta, int64_t cap);

int kbhip_session_close(kb_session* s);

/* Node-array sharding (one process per GPU).  A shard session
 * holds the whole host model but only nodes [lo, hi) of the snapshot on its
 * device, lo = N*rank/world, hi = N*(rank+1)/world (world <= 16).  Every rank
 * runs the same host loop; placements equal the one-GPU session's.
 *   Batched pops (the common case): each shard sweeps its range to its top-64
 *   candidates with their rows; ONE all-gather per pop exchanges them; every
 *   shard runs the identical chunk placement on the merged list (the global
 *   top-64) and writes back the rows it owns.
 *   Per-task pops (pod-affinity classes, Backfilled nodes): the 8-byte
 *   selection key (and the inter-pod affinity min/max) is all-reduced per task.
 * Connect with RCCL (kbhip_rccl_unique_id on one rank, shared out of band, then
 * kbhip_shard_connect_rccl on every rank, collectively: all-gather and
 * all-reduce on the session stream) or with host callbacks (e.g.
 * torch.distributed over gloo): kbhip_shard_connect_host for the all-reduce
 * and kbhip_shard_connect_host_gather for the all-gather; without the latter
 * every pop takes the per-task path. */
#define KBHIP_RED_MAX_U64 0
#define KBHIP_RED_MIN_I64 1
#define KBHIP_RED_MAX_I64 2
#define KBHIP_RED_SUM_I64 3 /* FitDelta counts of a task's walk over the shards */
typedef int (*kbhip_allreduce_fn)(void* ctx, uint64_t* vals, int32_t n, int32_t op);
/* recv <- the `bytes` sent by every rank, concatenated in rank order */
typedef int (*kbhip_allgather_fn)(void* ctx, const void* send, void* recv, int64_t bytes);
int kbhip_session_open_shard(const void* kbs_bytes, size_t len, int device, int32_t rank, int32_t world,
                             kb_session** out);
int kbhip_shard_info(kb_session* s, int32_t* out_rank_world_lo_hi);
int kbhip_rccl_unique_id(void* out, int64_t cap);
/* kbhip_shard_connect_rccl forms the session's communicator with a new
 * ncclCommInitRank, or takes the one a closed earlier session of this process
 * left with the same unique id, rank, world and device (communicators are
 * pooled for the process's lifetime: reuse one unique id across scheduling
 * cycles and the bootstrap is paid once; every rank must then reuse together;
 * kbhip_stats.comm_reused says which happened).  A session on which an ABI
 * call failed while it was connected, or whose communicator reports an
 * asynchronous error, aborts the communicator at close instead of pooling it. */
int kbhip_shard_connect_rccl(kb_session* s, const void* unique_id, int64_t len);
int kbhip_shard_connect_host(kb_session* s, kbhip_allreduce_fn fn, void* ctx);
/* Peer mailboxes for the batched pops of a shard session (SURVEY §8(e)'s
 * device-side exchange): every rank's device holds a mailbox (exportable
 * device memory, uncached where the runtime allows); fn all-gathers the
 * ranks' IPC handles once (every rank calls this collectively), each rank
 * maps the others' (hipIpcOpenMemHandle: xGMI across GPUs, the same memory for
 * ranks sharing one GPU).  Per batched pop every shard's sweep kernel writes
 * its top-64 with rows into every rank's mailbox and raises a flag; each
 * rank's placement kernel waits for the W flags on the device — no host
 * step and no collective launch per pop.  Takes precedence over the RCCL /
 * host all-gather for batched pops; per-task pops still use the all-reduce
 * of kbhip_shard_connect_rccl / kbhip_shard_connect_host.  Mailboxes and
 * mappings are kept per process and reused by later sessions. */
int kbhip_shard_connect_mailbox(kb_session* s, kbhip_allgather_fn fn, void* ctx);
/* Ranks that are threads of one process on one device (a rehearsal; one
 * process per GPU is the deployment): a rank's placement kernel spins on the
 * other ranks' flags, so their chained kernels must never share a hardware
 * queue.  kbhip_shard_connect_mailbox returns KBHIP_EUNSUPPORTED (every rank
 * of the group, after the all-gather) unless all ranks' streams fit in the
 * process's queues (GPU_MAX_HW_QUEUES, default 4).  This query gives the
 * same verdict without a device: 1 when ranks_on_device ranks fit in
 * hw_queues queues (hw_queues <= 0: the environment's), else 0. */
int kbhip_shard_mailbox_fits(int32_t ranks_on_device, int32_t hw_queues);
int kbhip_shard_connect_host_gather(kb_session* s, kbhip_allgather_fn fn, void* ctx);

/* Test support (not part of the placement path): encode a snapshot without a
 * device and read the compiled host tables back by name.  Tables (int32):
 *   "dims"       n_nodes, npad, n_spaces, n_classes
 *   "pod_class"  task class of every pod (-1: not a pending task)
 *   "class_aff"  per class 16 fields: aff, pred_err, ea_off, ea_n, pa_space,
 *                pa_cnt, pa_total, pa_self, paa_space, paa_cnt, ipa_off, ipa_n,
 *                upd_off, upd_n, score_err, 0
 *   "aff_dom"    [n_spaces][npad] topology domain ids
 *   "aff_cnt", "aff_scalar", "aff_items"  pod-affinity count tables / programs
 *   "node_idle", "node_backfilled"  (encode-only sessions) int64 [n_nodes][3]:
 *                cpu, memory, GPU of the host tables kbhip_debug_replay mutates
 *   "node_visits"  (encode-only sessions) uint32 [n_nodes]: the walk visit
 *                counters of kbhip_walk_visits as the replay counts them
 *   "pod_job", "pod_queue"  the session job / queue of every pod (-1: none)
 *   "job_ready"  gang's readyTaskNum of every job; "job_drf_alloc" (double
 *                [n_jobs][3]), "queue_allocated", "queue_deserved" (double
 *                [n_queues][3]): drf's and proportion's state — reading one of
 *                these four opens the plugins if no call has yet
 *   "victim_state"  int64 [4]: kbhip_head_victims' last state build — bytes
 *                uploaded, host microseconds, candidate tasks, longest node
 * kbhip_debug_table returns the table size in bytes and copies it when
 * cap_bytes is large enough.  Sessions from kbhip_debug_encode reject every
 * call that needs a device (KBHIP_EINVAL). */
int kbhip_debug_encode(const void* kbs_bytes, size_t len, kb_session** out);
int64_t kbhip_debug_table(kb_session* s, const char* name, void* out, int64_t cap_bytes);
/* Test support: replay a given decision sequence on an encode-only session's
 * host tables with the kernels' own per-node arithmetic (kbhip_eval.h).  Step
 * i tries task pods[i] (modes[i]: 0 allocate, 1 backfill): the selection key
 * of every node, as the device sweep computes it before the step's commit, is
 * written to out_keys[i * n_nodes + node]; then nodes[i] (-1: unassigned) is
 * committed with kinds[i] (KBHIP_ALLOCATED / KBHIP_PIPELINED).  No placement
 * decision is made here: the sequence comes from the caller (the tests take
 * it from the CPU oracle and compare the keys with the oracle's). */
int kbhip_debug_replay(kb_session* s, int32_t n_steps, const int32_t* pods, const int32_t* modes,
                       const int32_t* nodes, const uint8_t* kinds, uint64_t* out_keys);
/* Test support: kbhip_explain_tasks for one task on an encode-only session's
 * host tables, by the function the kernel runs (node_verdict, kbhip_eval.h):
 * out_verdict (optional, n_nodes bytes) and out_hist (KBHIP_EXPLAIN_BINS) as
 * that call defines them.  KBHIP_EINVAL: a null session or out_hist, a session
 * with a device, a task without a class. */
int kbhip_debug_explain(kb_session* s, int32_t task_id, uint8_t* out_verdict, int64_t* out_hist);
/* Test support: kbhip_head_victims' row for one node on an encode-only
 * session's host tables, by the functions the kernel runs (vict_stage,
 * vict_link, vict_decide, kbhip_eval.h): the count, the evicted prefix, the
 * flags and `stride` victims as that call defines them, whether or not the
 * node is in the task's walk.  KBHIP_EINVAL: a null session or output, a
 * session with a device, a task without a class or a job, victims outside
 * 1..3, a node out of range, stride < 1. */
int kbhip_debug_victims(kb_session* s, int32_t task_id, int32_t victims, int32_t node, int32_t stride,
                        int32_t* out_count, int32_t* out_evict, uint8_t* out_flags, int32_t* out_victim);
/* Test support: kbhip_walk_victims' node loop over the caller's node list
 * (n_nodes entries, visited in the given order, whether or not they are in the
 * task's walk) on an encode-only session's host tables, by the functions the
 * kernel runs (vict_stage_walk, vict_link, walk_step, kbhip_eval.h).  Returns
 * the ops written; out_op / out_pod / out_node as that call defines them;
 * out_info (optional, 8): the stop reason (never KBHIP_WALK_HEAD_END), n_nodes,
 * the entries visited, the nodes acted on, the last acted-on node, then zeros.
 * Option "walk_overlay_max" applies.  KBHIP_EINVAL: a null session, output or
 * node list, a session with a device, a task without a class or a job,
 * victims outside 1..3, a node out of range, n_nodes < 0, cap_ops < 1. */
int64_t kbhip_debug_walk_victims(kb_session* s, int32_t task_id, int32_t victims, const int32_t* nodes,
                                 int32_t n_nodes, int64_t cap_ops, uint8_t* out_op, int32_t* out_pod,
                                 int32_t* out_node, int64_t* out_info);

const char* kbhip_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* KBHIP_H_ */

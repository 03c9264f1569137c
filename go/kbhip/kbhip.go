// Package kbhip binds libkbhip.so (include/kbhip.h), the MI355X placement
// engine for kube-batch's allocate hot path, into the reference scheduler's
// framework (pkg/scheduler/framework/interface.go:20-40).
//
// NOT COMPILED HERE: this image has no Go toolchain (DESIGN.md §1).  The file
// is the binding a maintainer adds under
// pkg/scheduler/actions/allocatehip/ of the reference tree; the C ABI it calls
// is exercised from Python (ctypes, tests/) and C++ (kube-batch-1_amd/host/
// kbhost.cpp, the same host loop as allocate_hip.go) in this repository.
package kbhip

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../kube-batch-1_amd/_build -lkbhip -Wl,-rpath,${SRCDIR}/../../kube-batch-1_amd/_build
#include <stdlib.h>
#include "kbhip.h"
*/
import "C"

import (
	"fmt"
	"unsafe"
)

// Placement kinds and pop stop reasons (include/kbhip.h:70-77).
const (
	Allocated = C.KBHIP_ALLOCATED // Session.Allocate -> api.Allocated
	Pipelined = C.KBHIP_PIPELINED // Session.Pipeline -> api.Pipelined

	StopAll        = C.KBHIP_STOP_ALL        // every task of the pop was placed, the job is not yet ready
	StopUnassigned = C.KBHIP_STOP_UNASSIGNED // a task found no node (allocate.go:187-189)
	StopReady      = C.KBHIP_STOP_READY      // JobReady after a placement (allocate.go:191-195)
)

// Engine is one scheduling session on the device (kbhip_session_open .. close).
type Engine struct {
	s *C.kb_session
}

func lastErr(what string, rc C.int) error {
	return fmt.Errorf("kbhip %s: %d: %s", what, int(rc), C.GoString(C.kbhip_last_error()))
}

// DeviceCount is the number of gfx950 devices the library sees.
func DeviceCount() int { return int(C.kbhip_device_count()) }

// Open uploads a KBS1 snapshot (EncodeSession) to `device` (cache.go:515-583's
// Snapshot as the device's node columns, task classes and host model).
func Open(snapshot []byte, device int) (*Engine, error) {
	if len(snapshot) == 0 {
		return nil, fmt.Errorf("kbhip: empty snapshot")
	}
	var s *C.kb_session
	rc := C.kbhip_session_open(unsafe.Pointer(&snapshot[0]), C.size_t(len(snapshot)), C.int(device), &s)
	if rc < 0 {
		return nil, lastErr("session_open", rc)
	}
	return &Engine{s: s}, nil
}

// Close ends the session (kbhip_session_close).
func (e *Engine) Close() {
	if e.s != nil {
		C.kbhip_session_close(e.s)
		e.s = nil
	}
}

// SetOption sets an engine option (kbhip_set_option: "engine", "engine_lists",
// "speculate", ...).
func (e *Engine) SetOption(key string, value int64) error {
	k := C.CString(key)
	defer C.free(unsafe.Pointer(k))
	if rc := C.kbhip_set_option(e.s, k, C.int64_t(value)); rc < 0 {
		return lastErr("set_option "+key, rc)
	}
	return nil
}

// Placement is one entry of the placement log, in decision order: the
// snapshot's pod and node indices and Allocated / Pipelined.
type Placement struct {
	Pod, Node int32
	Kind      uint8
}

// Allocate runs the whole allocate action on the device with the host
// ordering in C++ (kbhip_allocate) and returns the placement log.
func (e *Engine) Allocate(capacity int) ([]Placement, error) {
	if capacity < 1 {
		capacity = 1
	}
	pods := make([]int32, capacity)
	nodes := make([]int32, capacity)
	kinds := make([]uint8, capacity)
	n := C.kbhip_allocate(e.s, (*C.int32_t)(unsafe.Pointer(&pods[0])), (*C.int32_t)(unsafe.Pointer(&nodes[0])),
		(*C.uint8_t)(unsafe.Pointer(&kinds[0])), C.int64_t(capacity))
	if n < 0 {
		return nil, lastErr("allocate", n)
	}
	out := make([]Placement, int(n))
	for i := range out {
		out[i] = Placement{Pod: pods[i], Node: nodes[i], Kind: kinds[i]}
	}
	return out, nil
}

// PlaceJob runs one job pop (allocate.go:110-196 for the tasks of one job,
// already in TaskOrderFn order): per consumed task its node (-1: unassigned)
// and kind, and the stop reason.
func (e *Engine) PlaceJob(taskIDs []int32, gang bool, minAvailable, readyCount int32) (
	nodes []int32, kinds []uint8, stop int32, err error) {
	n := len(taskIDs)
	if n == 0 {
		return nil, nil, StopAll, nil
	}
	nodes = make([]int32, n)
	kinds = make([]uint8, n)
	var done, st C.int32_t
	rc := C.kbhip_place_job(e.s, (*C.int32_t)(unsafe.Pointer(&taskIDs[0])), C.int32_t(n), boolI32(gang),
		C.int32_t(minAvailable), C.int32_t(readyCount),
		(*C.int32_t)(unsafe.Pointer(&nodes[0])), (*C.uint8_t)(unsafe.Pointer(&kinds[0])), &done, &st)
	if rc < 0 {
		return nil, nil, 0, lastErr("place_job", rc)
	}
	return nodes[:done], kinds[:done], int32(st), nil
}

// Submit queues a job pop (kbhip_place_job_submit) and returns its ticket;
// Wait returns the oldest outstanding pop's results; Cancel withdraws a ticket
// and every later one (their device updates are undone).
func (e *Engine) Submit(taskIDs []int32, gang bool, minAvailable, readyCount int32) (int64, error) {
	if len(taskIDs) == 0 {
		return -1, fmt.Errorf("kbhip submit: empty pop")
	}
	t := C.kbhip_place_job_submit(e.s, (*C.int32_t)(unsafe.Pointer(&taskIDs[0])), C.int32_t(len(taskIDs)),
		boolI32(gang), C.int32_t(minAvailable), C.int32_t(readyCount))
	if t < 0 {
		return -1, lastErr("place_job_submit", C.int(t))
	}
	return int64(t), nil
}

func (e *Engine) Wait(ticket int64, n int) (nodes []int32, kinds []uint8, stop int32, err error) {
	nodes = make([]int32, n)
	kinds = make([]uint8, n)
	var done, st C.int32_t
	rc := C.kbhip_place_job_wait(e.s, C.int64_t(ticket), (*C.int32_t)(unsafe.Pointer(&nodes[0])),
		(*C.uint8_t)(unsafe.Pointer(&kinds[0])), &done, &st)
	if rc < 0 {
		return nil, nil, 0, lastErr("place_job_wait", rc)
	}
	return nodes[:done], kinds[:done], int32(st), nil
}

func (e *Engine) Cancel(ticket int64) { C.kbhip_place_job_cancel(e.s, C.int64_t(ticket)) }

// Visit is one entry of kbhip_walk_visits: a node the allocate walks reached
// and how many times (each time node.GetAccessibleResource() added the node's
// Backfilled to its Idle, node_info.go:209-211).
type Visit struct {
	Node  int32
	Count uint32
}

// WalkVisits returns the nodes with Backfilled resources that the walks since
// the previous call visited, in ascending node index, and clears the counts.
func (e *Engine) WalkVisits() ([]Visit, error) {
	n := C.kbhip_walk_visits(e.s, nil, nil, 0)
	if n < 0 {
		return nil, lastErr("walk_visits", C.int(n))
	}
	if n == 0 {
		return nil, nil
	}
	nodes := make([]int32, int(n))
	counts := make([]uint32, int(n))
	if m := C.kbhip_walk_visits(e.s, (*C.int32_t)(unsafe.Pointer(&nodes[0])),
		(*C.uint32_t)(unsafe.Pointer(&counts[0])), n); m < 0 {
		return nil, lastErr("walk_visits", C.int(m))
	}
	out := make([]Visit, int(n))
	for i := range out {
		out[i] = Visit{Node: nodes[i], Count: counts[i]}
	}
	return out, nil
}

// FitDelta is one record of kbhip_fit_deltas: node.Idle.Clone().FitDelta(
// task.Resreq) of a node the task's walk visited (allocate.go:164-167).
type FitDelta struct {
	Node                     int32
	MilliCPU, Memory, MilliGPU int64
}

// FitDeltas returns job.NodesFitDelta for the task on which the most recent
// pop stopped unassigned, in ascending node index.
func (e *Engine) FitDeltas(task int32) ([]FitDelta, error) {
	n := C.kbhip_fit_deltas(e.s, C.int32_t(task), nil, nil, 0)
	if n < 0 {
		return nil, lastErr("fit_deltas", C.int(n))
	}
	if n == 0 {
		return nil, nil
	}
	nodes := make([]int32, int(n))
	deltas := make([]int64, 3*int(n))
	if m := C.kbhip_fit_deltas(e.s, C.int32_t(task), (*C.int32_t)(unsafe.Pointer(&nodes[0])),
		(*C.int64_t)(unsafe.Pointer(&deltas[0])), n); m < 0 {
		return nil, lastErr("fit_deltas", C.int(m))
	}
	out := make([]FitDelta, int(n))
	for i := range out {
		out[i] = FitDelta{Node: nodes[i], MilliCPU: deltas[3*i], Memory: deltas[3*i+1], MilliGPU: deltas[3*i+2]}
	}
	return out, nil
}

// RankNodes returns entries [first, first+n) of the ranked node walk of a
// Pending task (kbhip_rank_nodes) and the walk's length: byScore true is
// preempt()'s walk (preempt.go:270-287: the nodes passing PredicateFn with a
// NodeOrderFn score, in util.SelectBestNode order), false reclaim's (the
// passing nodes in index order, scores 0).  first+n <= 64 is served by the
// top-64 kernel, any other window by the full device sort; n = 0 asks for the
// length alone.  The session state is not changed.
func (e *Engine) RankNodes(task int32, byScore bool, first, n int64) (total int64, nodes, scores []int32, err error) {
	if n < 0 || first < 0 {
		return 0, nil, nil, fmt.Errorf("kbhip rank_nodes: negative window")
	}
	var pn, ps *C.int32_t
	if n > 0 { // &nodes[0] of an empty slice panics
		nodes = make([]int32, n)
		scores = make([]int32, n)
		pn = (*C.int32_t)(unsafe.Pointer(&nodes[0]))
		ps = (*C.int32_t)(unsafe.Pointer(&scores[0]))
	}
	t := C.kbhip_rank_nodes(e.s, C.int32_t(task), boolI32(byScore), C.int64_t(first), pn, ps, C.int64_t(n))
	if t < 0 {
		return 0, nil, nil, lastErr("rank_nodes", C.int(t))
	}
	got := int64(t) - first
	if got < 0 {
		got = 0
	}
	if got > n {
		got = n
	}
	return int64(t), nodes[:got], scores[:got], nil
}

// The victim kinds of RankVictimNodes (KBHIP_VICTIMS_*): whose Running tasks
// the caller's loop filters for.
const (
	VictimsOtherQueues    int32 = 1 // reclaim.go: jobs of other queues
	VictimsQueueOtherJobs int32 = 2 // preempt.go:104-127: the task's queue, other jobs
	VictimsSameJob        int32 = 3 // preempt.go:151-181: the task's own job
)

// VictimWalkInfo says how a RankVictimNodes call was served.
type VictimWalkInfo struct {
	Head     bool  // by the top-64 kernel
	Rebuilt  bool  // the call (re)built the candidate table
	Launches int64 // kernel launches issued
}

// RankVictimNodes is RankNodes without the nodes that can yield no victim set
// for the task (kbhip_rank_victim_nodes): nodes with no candidate of the
// given kind, or whose candidates' Resreq sum is strictly below the task's
// InitResreq in all three resources — the nodes validateVictims rejects
// whatever the plugins answer.  cands[i] is the candidate count of nodes[i].
// The host loop over this walk decides what the loop over RankNodes' walk
// decides, in the same order.  ApplyOps keeps the device's candidate table
// current; any other call that changes pod statuses makes the next call here
// rebuild it.
func (e *Engine) RankVictimNodes(task int32, byScore bool, victims int32, first, n int64) (total int64, nodes, scores, cands []int32, info VictimWalkInfo, err error) {
	if n < 0 || first < 0 {
		return 0, nil, nil, nil, info, fmt.Errorf("kbhip rank_victim_nodes: negative window")
	}
	var pn, ps, pc *C.int32_t
	if n > 0 { // &nodes[0] of an empty slice panics
		nodes = make([]int32, n)
		scores = make([]int32, n)
		cands = make([]int32, n)
		pn = (*C.int32_t)(unsafe.Pointer(&nodes[0]))
		ps = (*C.int32_t)(unsafe.Pointer(&scores[0]))
		pc = (*C.int32_t)(unsafe.Pointer(&cands[0]))
	}
	var raw [3]C.int64_t
	t := C.kbhip_rank_victim_nodes(e.s, C.int32_t(task), boolI32(byScore), C.int32_t(victims), C.int64_t(first),
		pn, ps, pc, C.int64_t(n), &raw[0])
	if t < 0 {
		return 0, nil, nil, nil, info, lastErr("rank_victim_nodes", C.int(t))
	}
	info = VictimWalkInfo{Head: raw[0] != 0, Rebuilt: raw[1] != 0, Launches: int64(raw[2])}
	got := int64(t) - first
	if got < 0 {
		got = 0
	}
	if got > n {
		got = n
	}
	return int64(t), nodes[:got], scores[:got], cands[:got], info, nil
}

// RankHeadsMax is the most tasks one RankHeads call answers (KBHIP_RANK_HEADS_MAX).
const RankHeadsMax = int(C.KBHIP_RANK_HEADS_MAX)

// Head is one task's answer of RankHeads: the walk's length and its first
// min(cap, Total) entries (Cands all 0 with victims 0).
type Head struct {
	Total  int64
	Nodes  []int32
	Scores []int32
	Cands  []int32
}

// HeadsInfo says how a RankHeads call was served.
type HeadsInfo struct {
	Rebuilt  bool  // the call (re)built the candidate table
	Launches int64 // kernel launches issued: 2, plus one per distinct class with inter-pod priority terms
	GridX    int64 // the x size of the sweep's grid
}

// RankHeads answers the walk heads of up to RankHeadsMax Pending tasks in one
// sweep launch, one merge launch and one copy (kbhip_rank_heads): heads[i] is
// what RankNodes(tasks[i], byScore, 0, cap) returns with victims 0, and what
// RankVictimNodes(tasks[i], byScore, victims, 0, cap) returns with one of the
// Victims* kinds.  1 <= cap <= 64; a task may appear more than once.  The
// heads describe the session at the call: a host that prefetches them for the
// tasks its loop will rank next discards what it has not consumed as soon as
// it sends an ApplyOps.  The session state is not changed.
func (e *Engine) RankHeads(tasks []int32, byScore bool, victims int32, cap int) (heads []Head, info HeadsInfo, err error) {
	if len(tasks) == 0 { // &tasks[0] of an empty slice panics
		return nil, info, nil
	}
	if len(tasks) > RankHeadsMax || cap < 1 || cap > 64 {
		return nil, info, fmt.Errorf("kbhip rank_heads: %d tasks (1..%d), cap %d (1..64)", len(tasks), RankHeadsMax, cap)
	}
	n := len(tasks)
	total := make([]int64, n)
	nodes := make([]int32, n*cap)
	scores := make([]int32, n*cap)
	cands := make([]int32, n*cap)
	var raw [3]C.int64_t
	if r := C.kbhip_rank_heads(e.s, (*C.int32_t)(unsafe.Pointer(&tasks[0])), C.int32_t(n), boolI32(byScore),
		C.int32_t(victims), C.int32_t(cap), (*C.int64_t)(unsafe.Pointer(&total[0])),
		(*C.int32_t)(unsafe.Pointer(&nodes[0])), (*C.int32_t)(unsafe.Pointer(&scores[0])),
		(*C.int32_t)(unsafe.Pointer(&cands[0])), &raw[0]); r < 0 {
		return nil, info, lastErr("rank_heads", C.int(r))
	}
	info = HeadsInfo{Rebuilt: raw[0] != 0, Launches: int64(raw[1]), GridX: int64(raw[2])}
	heads = make([]Head, n)
	for i := range heads {
		k := total[i]
		if k > int64(cap) {
			k = int64(cap)
		}
		lo, hi := i*cap, i*cap+int(k)
		heads[i] = Head{Total: total[i], Nodes: nodes[lo:hi:hi], Scores: scores[lo:hi:hi], Cands: cands[lo:hi:hi]}
	}
	return heads, info, nil
}

// The flag bits of a HeadVictim (KBHIP_HEAD_VICTIMS_*).
const (
	HeadVictimsValid  = uint8(C.KBHIP_HEAD_VICTIMS_VALID)
	HeadVictimsCovers = uint8(C.KBHIP_HEAD_VICTIMS_COVERS)
)

// HeadVictim is one head node of HeadVictims: what ssn.Reclaimable /
// ssn.Preemptable answer on it (Count victims, the first min(Count, stride) of
// them in Victims), whether validateVictims passes (Flags & HeadVictimsValid),
// how many victims from the front the eviction loop evicts (Evict) and whether
// it then pipelines the task here (Flags & HeadVictimsCovers).
type HeadVictim struct {
	Node, Score  int32
	Count, Evict int32
	Flags        uint8
	Victims      []int32
}

// HeadVictimsInfo says what a HeadVictims call did (out_info of kbhip_head_victims).
type HeadVictimsInfo struct {
	Rebuilt      bool  // the candidate table was built by this call
	StateRebuilt bool  // the victim state was built by this call
	Patched      int64 // records of earlier ApplyOps batches patched into it
	Launches     int64 // kernel launches issued
	MaxCount     int64 // the largest Count: a stride below it truncated a row
}

// headVictimAt is head entry `at` of the calls' output arrays (victim rows of stride words).
func headVictimAt(nodes, scores, counts, evicts []int32, flags []uint8, rows []int32, at, stride int) HeadVictim {
	n := int(counts[at])
	if n > stride {
		n = stride
	}
	lo := at * stride
	return HeadVictim{Node: nodes[at], Score: scores[at], Count: counts[at], Evict: evicts[at], Flags: flags[at],
		Victims: rows[lo : lo+n : lo+n]}
}

// HeadVictims answers the head of RankVictimNodes' walk together with the
// victim decision on each head node (kbhip_head_victims): the step of a
// reclaim / preempt loop between the ranking and ApplyOps.  1 <= cap <= 64,
// stride >= 1.  The rows describe the session at the call: use them up to the
// first node acted on and discard the rest once an ApplyOps is sent.
func (e *Engine) HeadVictims(task int32, byScore bool, victims int32, cap, stride int) (total int64, heads []HeadVictim, info HeadVictimsInfo, err error) {
	if cap < 1 || cap > 64 || stride < 1 { // (also keeps &x[0] below off empty slices)
		return 0, nil, info, fmt.Errorf("kbhip head_victims: cap %d (1..64), stride %d (>= 1)", cap, stride)
	}
	nodes, scores := make([]int32, cap), make([]int32, cap)
	counts, evicts := make([]int32, cap), make([]int32, cap)
	flags := make([]uint8, cap)
	rows := make([]int32, cap*stride)
	var raw [5]C.int64_t
	t := C.kbhip_head_victims(e.s, C.int32_t(task), boolI32(byScore), C.int32_t(victims), C.int32_t(cap),
		C.int32_t(stride), (*C.int32_t)(unsafe.Pointer(&nodes[0])), (*C.int32_t)(unsafe.Pointer(&scores[0])),
		(*C.int32_t)(unsafe.Pointer(&counts[0])), (*C.int32_t)(unsafe.Pointer(&evicts[0])),
		(*C.uint8_t)(unsafe.Pointer(&flags[0])), (*C.int32_t)(unsafe.Pointer(&rows[0])), &raw[0])
	if t < 0 {
		return 0, nil, info, lastErr("head_victims", C.int(t))
	}
	info = HeadVictimsInfo{Rebuilt: raw[0] != 0, StateRebuilt: raw[1] != 0, Patched: int64(raw[2]),
		Launches: int64(raw[3]), MaxCount: int64(raw[4])}
	k := int(t)
	if int64(t) > int64(cap) {
		k = cap
	}
	heads = make([]HeadVictim, k)
	for i := range heads {
		heads[i] = headVictimAt(nodes, scores, counts, evicts, flags, rows, i, stride)
	}
	return int64(t), heads, info, nil
}

// HeadsVictimsMax is the most tasks one HeadsVictims call answers (KBHIP_HEADS_VICTIMS_MAX).
const HeadsVictimsMax = int(C.KBHIP_HEADS_VICTIMS_MAX)

// TaskHeadVictims is one task's answer of HeadsVictims: what HeadVictims
// returns for it, and First, the index in Heads of the first entry with
// HeadVictimsValid (-1: the task acts on none of its head nodes).
type TaskHeadVictims struct {
	Total int64
	First int32
	Heads []HeadVictim
}

// HeadsVictimsInfo says what a HeadsVictims call did (out_info of kbhip_heads_victims).
type HeadsVictimsInfo struct {
	HeadVictimsInfo
	VictimLaunches int64 // the victims launches among Launches: 1 unless the spill bound split the batch
}

// HeadsVictims answers HeadVictims for up to HeadsVictimsMax Pending tasks in
// one call (kbhip_heads_victims): out[i] is what HeadVictims(tasks[i], byScore,
// victims, cap, stride) returns on the session as it stands.  Every task is
// answered against the session at the call — no eviction is carried from one
// task to the next.  A host that prefetches uses the answers up to the first
// task it acts on and discards the rest once an ApplyOps is sent; First lets it
// pass over the tasks that act on no node.  A task may appear more than once.
func (e *Engine) HeadsVictims(tasks []int32, byScore bool, victims int32, cap, stride int) (out []TaskHeadVictims, info HeadsVictimsInfo, err error) {
	if len(tasks) == 0 { // &tasks[0] of an empty slice panics
		return nil, info, nil
	}
	if len(tasks) > HeadsVictimsMax || cap < 1 || cap > 64 || stride < 1 {
		return nil, info, fmt.Errorf("kbhip heads_victims: %d tasks (1..%d), cap %d (1..64), stride %d (>= 1)",
			len(tasks), HeadsVictimsMax, cap, stride)
	}
	n := len(tasks)
	total := make([]int64, n)
	nodes, scores := make([]int32, n*cap), make([]int32, n*cap)
	counts, evicts := make([]int32, n*cap), make([]int32, n*cap)
	flags := make([]uint8, n*cap)
	rows := make([]int32, n*cap*stride)
	first := make([]int32, n)
	var raw [6]C.int64_t
	if r := C.kbhip_heads_victims(e.s, (*C.int32_t)(unsafe.Pointer(&tasks[0])), C.int32_t(n), boolI32(byScore),
		C.int32_t(victims), C.int32_t(cap), C.int32_t(stride), (*C.int64_t)(unsafe.Pointer(&total[0])),
		(*C.int32_t)(unsafe.Pointer(&nodes[0])), (*C.int32_t)(unsafe.Pointer(&scores[0])),
		(*C.int32_t)(unsafe.Pointer(&counts[0])), (*C.int32_t)(unsafe.Pointer(&evicts[0])),
		(*C.uint8_t)(unsafe.Pointer(&flags[0])), (*C.int32_t)(unsafe.Pointer(&rows[0])),
		(*C.int32_t)(unsafe.Pointer(&first[0])), &raw[0]); r < 0 {
		return nil, info, lastErr("heads_victims", C.int(r))
	}
	info = HeadsVictimsInfo{HeadVictimsInfo: HeadVictimsInfo{Rebuilt: raw[0] != 0, StateRebuilt: raw[1] != 0,
		Patched: int64(raw[2]), Launches: int64(raw[3]), MaxCount: int64(raw[4])}, VictimLaunches: int64(raw[5])}
	out = make([]TaskHeadVictims, n)
	for t := range out {
		k := int64(cap)
		if total[t] < k {
			k = total[t]
		}
		heads := make([]HeadVictim, k)
		for i := range heads {
			heads[i] = headVictimAt(nodes, scores, counts, evicts, flags, rows, t*cap+i, stride)
		}
		out[t] = TaskHeadVictims{Total: total[t], First: first[t], Heads: heads}
	}
	return out, info, nil
}

// The stop reasons of WalkVictims (KBHIP_WALK_*).
const (
	WalkAssigned  = int(C.KBHIP_WALK_ASSIGNED)  // a node covered InitResreq: the last op pipelines the task
	WalkExhausted = int(C.KBHIP_WALK_EXHAUSTED) // every node of the walk was visited, none covered
	WalkHeadEnd   = int(C.KBHIP_WALK_HEAD_END)  // cap entries or the 64-entry head used up, the walk has more nodes
	WalkCapacity  = int(C.KBHIP_WALK_CAPACITY)  // the next step does not fit capOps or the carried state
)

// WalkVictimsInfo says how a WalkVictims call ended and what it did (out_info
// of kbhip_walk_victims).
type WalkVictimsInfo struct {
	Stop         int   // a Walk* reason
	Total        int64 // nodes in the pruned walk
	Visited      int64 // head entries decided
	Acted        int64 // nodes evicted from
	LastNode     int32 // the last acted-on node, -1 if none: where a resumed call goes on
	LastScore    int32 // its score (0 with byScore false)
	Launches     int64
	Rebuilt      bool  // the candidate table was built by this call
	StateRebuilt bool  // the victim state was built by this call
	Patched      int64 // records of earlier ApplyOps batches patched into it
}

// WalkVictims runs one task's whole eviction walk over the head of its pruned
// walk (kbhip_walk_victims): the node loop of preempt() / reclaim with the
// evictions of each node carried to the next.  ops / pods / nodes go to
// ApplyOps unchanged.  afterNode < 0 starts at the top; after a WalkCapacity
// or WalkHeadEnd stop apply the ops and call again with LastNode / LastScore.
// 1 <= cap <= 64, capOps >= 1.
func (e *Engine) WalkVictims(task int32, byScore bool, victims int32, cap int, afterNode, afterScore int32, capOps int) (ops []uint8, pods, nodes []int32, info WalkVictimsInfo, err error) {
	if cap < 1 || cap > 64 || capOps < 1 { // (also keeps &x[0] below off empty slices)
		return nil, nil, nil, info, fmt.Errorf("kbhip walk_victims: cap %d (1..64), capOps %d (>= 1)", cap, capOps)
	}
	ops, pods, nodes = make([]uint8, capOps), make([]int32, capOps), make([]int32, capOps)
	var raw [8]C.int64_t
	n := C.kbhip_walk_victims(e.s, C.int32_t(task), boolI32(byScore), C.int32_t(victims), C.int32_t(cap),
		C.int32_t(afterNode), C.int32_t(afterScore), (*C.uint8_t)(unsafe.Pointer(&ops[0])),
		(*C.int32_t)(unsafe.Pointer(&pods[0])), (*C.int32_t)(unsafe.Pointer(&nodes[0])), C.int64_t(capOps), &raw[0])
	if n < 0 {
		return nil, nil, nil, info, lastErr("walk_victims", C.int(n))
	}
	info = WalkVictimsInfo{Stop: int(raw[0]), Total: int64(raw[1]), Visited: int64(raw[2]), Acted: int64(raw[3]),
		LastNode: int32(raw[4]), LastScore: int32(raw[5]), Launches: int64(raw[6]), Rebuilt: raw[7]&1 != 0,
		StateRebuilt: raw[7]&2 != 0, Patched: int64(raw[7]) >> 8}
	return ops[:n], pods[:n], nodes[:n], info, nil
}

// WalkVictimsFromInfo says how a WalkVictimsFrom call ended and what it did
// (out_info of kbhip_walk_victims_from).
type WalkVictimsFromInfo struct {
	Stop         int   // a Walk* reason: WalkExhausted = every node behind the resume point was decided, WalkHeadEnd = the window is used up and nodes remain
	Remaining    int64 // entries of the pruned walk behind the resume point at the call
	Visited      int64 // window entries decided
	Acted        int64 // nodes evicted from
	ResumeNode   int32 // the resume point: the last entry passed over or acted on (the call's own afterNode if none)
	ResumeScore  int32 // its score (0 with byScore false)
	Launches     int64
	Rebuilt      bool  // the candidate table was built by this call
	StateRebuilt bool  // the victim state was built by this call
	Patched      int64 // records of earlier ApplyOps batches patched into it
	LastNode     int32 // the last acted-on node, -1 if none
	FirstValid   int32 // window index of the first entry VALID against the session as it stands, -1 if none
}

// WalkVictimsFrom runs one window (up to 64 entries) of a task's eviction walk
// behind a resume point (kbhip_walk_victims_from).  ops / pods / nodes go to
// ApplyOps unchanged.  afterNode < 0 starts at the top; after a WalkHeadEnd or
// WalkCapacity stop apply the ops and call again with ResumeNode /
// ResumeScore: the loop reaches WalkAssigned or WalkExhausted for a walk of
// any length.  1 <= cap <= 64, capOps >= 1.
func (e *Engine) WalkVictimsFrom(task int32, byScore bool, victims int32, cap int, afterNode, afterScore int32, capOps int) (ops []uint8, pods, nodes []int32, info WalkVictimsFromInfo, err error) {
	if cap < 1 || cap > 64 || capOps < 1 { // (also keeps &x[0] below off empty slices)
		return nil, nil, nil, info, fmt.Errorf("kbhip walk_victims_from: cap %d (1..64), capOps %d (>= 1)", cap, capOps)
	}
	ops, pods, nodes = make([]uint8, capOps), make([]int32, capOps), make([]int32, capOps)
	var raw [10]C.int64_t
	n := C.kbhip_walk_victims_from(e.s, C.int32_t(task), boolI32(byScore), C.int32_t(victims), C.int32_t(cap),
		C.int32_t(afterNode), C.int32_t(afterScore), (*C.uint8_t)(unsafe.Pointer(&ops[0])),
		(*C.int32_t)(unsafe.Pointer(&pods[0])), (*C.int32_t)(unsafe.Pointer(&nodes[0])), C.int64_t(capOps), &raw[0])
	if n < 0 {
		return nil, nil, nil, info, lastErr("walk_victims_from", C.int(n))
	}
	info = WalkVictimsFromInfo{Stop: int(raw[0]), Remaining: int64(raw[1]), Visited: int64(raw[2]),
		Acted: int64(raw[3]), ResumeNode: int32(raw[4]), ResumeScore: int32(raw[5]), Launches: int64(raw[6]),
		Rebuilt: raw[7]&1 != 0, StateRebuilt: raw[7]&2 != 0, Patched: int64(raw[7]) >> 8, LastNode: int32(raw[8]),
		FirstValid: int32(raw[9])}
	return ops[:n], pods[:n], nodes[:n], info, nil
}

// WalkBeginInfo says what a WalkBegin call did (out_info of kbhip_walk_begin).
type WalkBeginInfo struct {
	Launches        int64
	Rebuilt         bool  // the candidate table was built by this call
	Bytes           int64 // device bytes the cursor keeps
	AffinityTargets bool  // the task's class has predicates that read pod-affinity targets: with byScore false WalkVictimsFrom is the closer call
}

// WalkBegin ranks the task's pruned walk once and keeps it on the device as
// the session's eviction-walk cursor (kbhip_walk_begin), replacing an earlier
// one.  Returns the walk's total.
func (e *Engine) WalkBegin(task int32, byScore bool, victims int32) (total int64, info WalkBeginInfo, err error) {
	var raw [4]C.int64_t
	n := C.kbhip_walk_begin(e.s, C.int32_t(task), boolI32(byScore), C.int32_t(victims), &raw[0])
	if n < 0 {
		return 0, info, lastErr("walk_begin", C.int(n))
	}
	info = WalkBeginInfo{Launches: int64(raw[0]), Rebuilt: raw[1] != 0, Bytes: int64(raw[2]), AffinityTargets: raw[3] != 0}
	return int64(n), info, nil
}

// WalkBeginLive opens the cursor for reclaim's order (kbhip_walk_begin_live),
// exact for every task class.  For a class whose predicates read pod-affinity
// targets the cursor is live (live true): the kept order leaves that predicate
// out, WalkNext tests it on the count tables as they stand and returns behind
// the first node it acts on, so the host calls ApplyOps and WalkNext once per
// acting node.  For any other class the call is WalkBegin(task, false, victims).
// (Source only: no Go toolchain has compiled this declaration.)
func (e *Engine) WalkBeginLive(task int32, victims int32) (total int64, info WalkBeginInfo, live bool, err error) {
	var raw [4]C.int64_t
	n := C.kbhip_walk_begin_live(e.s, C.int32_t(task), C.int32_t(victims), &raw[0])
	if n < 0 {
		return 0, info, false, lastErr("walk_begin_live", C.int(n))
	}
	info = WalkBeginInfo{Launches: int64(raw[0]), Rebuilt: raw[1] != 0, Bytes: int64(raw[2]), AffinityTargets: raw[3] != 0}
	return int64(n), info, raw[3] == 2, nil
}

// WalkNextInfo says how a WalkNext call ended and what it did (out_info of
// kbhip_walk_next).
type WalkNextInfo struct {
	Stop         int   // a Walk* reason: WalkExhausted = the end of the kept order was reached, WalkHeadEnd = cap serial entries are used up and entries remain
	Total        int64 // entries of the kept order
	Decided      int64 // entries passed over and visited
	Acted        int64 // nodes evicted from
	Next         int64 // the position the next call goes on from
	First        int64 // the first position that could act against the session as it stands, -1 if none
	Launches     int64
	Rebuilt      bool  // the candidate table was built by this call
	StateRebuilt bool  // the victim state was built by this call
	Patched      int64 // records of earlier ApplyOps batches patched into it
	LastNode     int32 // the last acted-on node, -1 if none
	Scanned      int64 // entries the side-by-side scan decided
}

// WalkNext runs the cursor's walk from position pos of the kept order
// (kbhip_walk_next): the entries that cannot act are passed over in one
// launch, the serial walk covers up to cap entries from the first that can.
// ops / pods / nodes go to ApplyOps unchanged; after a WalkHeadEnd or
// WalkCapacity stop apply the ops and call again with Next.  1 <= cap <= 64,
// capOps >= 1.
func (e *Engine) WalkNext(pos int64, cap int, capOps int) (ops []uint8, pods, nodes []int32, info WalkNextInfo, err error) {
	if cap < 1 || cap > 64 || capOps < 1 { // (also keeps &x[0] below off empty slices)
		return nil, nil, nil, info, fmt.Errorf("kbhip walk_next: cap %d (1..64), capOps %d (>= 1)", cap, capOps)
	}
	ops, pods, nodes = make([]uint8, capOps), make([]int32, capOps), make([]int32, capOps)
	var raw [10]C.int64_t
	n := C.kbhip_walk_next(e.s, C.int64_t(pos), C.int32_t(cap), (*C.uint8_t)(unsafe.Pointer(&ops[0])),
		(*C.int32_t)(unsafe.Pointer(&pods[0])), (*C.int32_t)(unsafe.Pointer(&nodes[0])), C.int64_t(capOps), &raw[0])
	if n < 0 {
		return nil, nil, nil, info, lastErr("walk_next", C.int(n))
	}
	info = WalkNextInfo{Stop: int(raw[0]), Total: int64(raw[1]), Decided: int64(raw[2]), Acted: int64(raw[3]),
		Next: int64(raw[4]), First: int64(raw[5]), Launches: int64(raw[6]), Rebuilt: raw[7]&1 != 0,
		StateRebuilt: raw[7]&2 != 0, Patched: int64(raw[7]) >> 8, LastNode: int32(raw[8]), Scanned: int64(raw[9])}
	return ops[:n], pods[:n], nodes[:n], info, nil
}

// WalkOrder copies entries [first, first+cap) of the cursor's kept order
// (kbhip_walk_order): the nodes and, with byScore, their scores.  Returns the
// walk's total.
func (e *Engine) WalkOrder(first int64, cap int) (total int64, nodes, scores []int32, err error) {
	if first < 0 || cap < 0 {
		return 0, nil, nil, fmt.Errorf("kbhip walk_order: first %d, cap %d (>= 0)", first, cap)
	}
	nodes, scores = make([]int32, cap+1), make([]int32, cap+1) // (+1 keeps &x[0] off empty slices)
	n := C.kbhip_walk_order(e.s, C.int64_t(first), (*C.int32_t)(unsafe.Pointer(&nodes[0])),
		(*C.int32_t)(unsafe.Pointer(&scores[0])), C.int64_t(cap))
	if n < 0 {
		return 0, nil, nil, lastErr("walk_order", C.int(n))
	}
	k := int64(n) - first
	if k < 0 {
		k = 0
	}
	if k > int64(cap) {
		k = int64(cap)
	}
	return int64(n), nodes[:k], scores[:k], nil
}

// WalkEnd drops the cursor (kbhip_walk_end); whether one was open.
func (e *Engine) WalkEnd() (bool, error) {
	r := C.kbhip_walk_end(e.s)
	if r < 0 {
		return false, lastErr("walk_end", r)
	}
	return r != 0, nil
}

// The verdict codes of ExplainTasks (KBHIP_WHY_*): the low four bits of a
// verdict byte; the WhyShort* bits accompany the codes 0..2.
const (
	WhyFitsIdle      = uint8(C.KBHIP_WHY_FITS_IDLE)
	WhyFitsReleasing = uint8(C.KBHIP_WHY_FITS_RELEASING)
	WhyResources     = uint8(C.KBHIP_WHY_RESOURCES)
	WhyPodCount      = uint8(C.KBHIP_WHY_POD_COUNT)
	WhyNodeSelector  = uint8(C.KBHIP_WHY_NODE_SELECTOR)
	WhyHostPorts     = uint8(C.KBHIP_WHY_HOST_PORTS)
	WhyUnschedulable = uint8(C.KBHIP_WHY_UNSCHEDULABLE)
	WhyTaints        = uint8(C.KBHIP_WHY_TAINTS)
	WhyPodAffinity   = uint8(C.KBHIP_WHY_POD_AFFINITY)
	WhyScoreError    = uint8(C.KBHIP_WHY_SCORE_ERROR)
	WhyShortCPU      = uint8(C.KBHIP_WHY_SHORT_CPU)
	WhyShortMem      = uint8(C.KBHIP_WHY_SHORT_MEM)
	WhyShortGPU      = uint8(C.KBHIP_WHY_SHORT_GPU)
)

// ExplainMax is the most tasks one ExplainTasks call answers, ExplainBins the
// length of a task's histogram.
const (
	ExplainMax  = int(C.KBHIP_EXPLAIN_MAX)
	ExplainBins = int(C.KBHIP_EXPLAIN_BINS)
)

// Explanation is one task's answer of ExplainTasks.  Hist[c], c in 0..9, counts
// the nodes with code c; Hist[11..13] the nodes of the walk short of cpu /
// memory / GPU; Hist[14] the walk; Hist[15] the nodes.  Verdict (nil unless
// asked for) holds one byte per node.
type Explanation struct {
	Hist    [16]int64
	Verdict []uint8
}

// ExplainInfo says how an ExplainTasks call was served.
type ExplainInfo struct {
	Launches int64 // kernel launches issued: 2, plus one when pod-affinity count changes were still to be applied
	GridX    int64 // the x size of the sweep's grid
	Rows     bool  // per-node verdicts were written
}

// ExplainTasks answers, for up to ExplainMax Pending tasks of the session as it
// stands, why each node is or is not in the task's allocate walk
// (kbhip_explain_tasks): the first step of predicates.go:123-203 that rejects
// the node, a NodeOrderFn error, or how the node fits.  nNodes is the session's
// node count; verdicts false skips the per-node bytes (the histograms are the
// same).  The session state is not changed.
func (e *Engine) ExplainTasks(tasks []int32, verdicts bool, nNodes int) (out []Explanation, info ExplainInfo, err error) {
	if len(tasks) == 0 { // &tasks[0] of an empty slice panics
		return nil, info, nil
	}
	if len(tasks) > ExplainMax || nNodes < 0 {
		return nil, info, fmt.Errorf("kbhip explain_tasks: %d tasks (1..%d), %d nodes", len(tasks), ExplainMax, nNodes)
	}
	n := len(tasks)
	hist := make([]int64, n*ExplainBins)
	var rows []uint8
	var rowsPtr *C.uint8_t
	if verdicts && nNodes > 0 {
		rows = make([]uint8, n*nNodes)
		rowsPtr = (*C.uint8_t)(unsafe.Pointer(&rows[0]))
	}
	var raw [3]C.int64_t
	if r := C.kbhip_explain_tasks(e.s, (*C.int32_t)(unsafe.Pointer(&tasks[0])), C.int32_t(n), rowsPtr,
		(*C.int64_t)(unsafe.Pointer(&hist[0])), &raw[0]); r < 0 {
		return nil, info, lastErr("explain_tasks", C.int(r))
	}
	info = ExplainInfo{Launches: int64(raw[0]), GridX: int64(raw[1]), Rows: raw[2] != 0}
	out = make([]Explanation, n)
	for i := range out {
		copy(out[i].Hist[:], hist[i*ExplainBins:(i+1)*ExplainBins])
		if rows != nil {
			out[i].Verdict = rows[i*nNodes : (i+1)*nNodes : (i+1)*nNodes]
		}
	}
	return out, info, nil
}

// Op is one decision of a host-kept reclaim / preempt loop for ApplyOps.
// Node is read for OpPipeline only (an eviction uses the pod's own node).
type Op struct {
	Kind uint8
	Pod  int32
	Node int32
}

// The operation kinds of ApplyOps (KBHIP_OP_*).
const (
	OpEvict      = uint8(C.KBHIP_OP_EVICT)      // Session.Evict / Statement.Evict
	OpPipeline   = uint8(C.KBHIP_OP_PIPELINE)   // Session.Pipeline / Statement.Pipeline
	OpUnpipeline = uint8(C.KBHIP_OP_UNPIPELINE) // Statement.unpipeline (a discarded statement)
	OpUnevict    = uint8(C.KBHIP_OP_UNEVICT)    // Statement.unevict (the node keeps its Releasing copy)
)

// ApplyOps hands the engine what the host's own reclaim / preempt loop decided
// since its last ranking (kbhip_apply_ops), in order: the session's host model
// and the device node rows change exactly as under the engine's own actions,
// so the next RankNodes sees them.  The batch is validated as a whole; on an
// error nothing is changed.  Returns the device kernel launches issued (at
// most 2 whatever len(ops) is).
func (e *Engine) ApplyOps(ops []Op) (launches int64, err error) {
	if len(ops) == 0 { // &kind[0] of an empty slice panics
		return 0, nil
	}
	kind := make([]uint8, len(ops))
	pod := make([]int32, len(ops))
	node := make([]int32, len(ops))
	for i, o := range ops {
		kind[i], pod[i], node[i] = o.Kind, o.Pod, o.Node
	}
	var l C.int64_t
	if n := C.kbhip_apply_ops(e.s, (*C.uint8_t)(unsafe.Pointer(&kind[0])), (*C.int32_t)(unsafe.Pointer(&pod[0])),
		(*C.int32_t)(unsafe.Pointer(&node[0])), C.int64_t(len(ops)), &l); n < 0 {
		return 0, lastErr("apply_ops", C.int(n))
	}
	return int64(l), nil
}

// GangUnschedulable is the gang plugin's OnSessionClose text after Allocate
// (gang.go:166-187): "<job uid>\t<message>\n" per job that is not ready.
func (e *Engine) GangUnschedulable() (string, error) {
	n := C.kbhip_gang_unschedulable(e.s, nil, 0)
	if n < 0 {
		return "", lastErr("gang_unschedulable", C.int(n))
	}
	buf := make([]byte, int(n)+1)
	C.kbhip_gang_unschedulable(e.s, (*C.char)(unsafe.Pointer(&buf[0])), C.int64_t(len(buf)))
	return string(buf[:n]), nil
}

// Stats are the session's counters (kbhip_stats, include/kbhip.h).
func (e *Engine) Stats() (C.kbhip_stats, error) {
	var st C.kbhip_stats
	if rc := C.kbhip_get_stats(e.s, &st); rc < 0 {
		return st, lastErr("get_stats", rc)
	}
	return st, nil
}

func boolI32(b bool) C.int32_t {
	if b {
		return 1
	}
	return 0
}

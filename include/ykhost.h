/*
 * ykhost.h — C API of libykhost.so: the host-side mirror of the reference's predicate interface.
 *
 * In the real system this layer is Go: a `gpuPredicateManager` in pkg/plugin/predicates that keeps an encoded
 * mirror of pkg/cache/external.SchedulerCache and talks to libykpred.so through cgo. Go is not
 * available in this image, so the same layer is written in C++ above the SAME C ABI (include/ykpred.h) and
 * exposed here so that tests and bench.py can drive it with Kubernetes-JSON objects. Names follow the reference:
 *
 *   ykhost_predicates            PredicateManager.Predicates(pod, node, allocate) (string, error)
 *                                /root/reference/pkg/plugin/predicates/predicate_manager.go:134-139
 *   ykhost_preemption_predicates PredicateManager.PreemptionPredicates(pod, node, victims, startIndex) int   (:141-179)
 *   ykhost_set_plugins           newPredicateManagerInternal(handle, resPre, allocPre, resFilt, allocFilt) (:378-424)
 *   ykhost_update_node / ykhost_remove_node / ykhost_update_pod / ykhost_remove_pod / ykhost_assume_pod /
 *   ykhost_forget_pod            SchedulerCache.UpdateNode / RemoveNode / UpdatePod / RemovePod / AssumePod / ForgetPod
 *                                /root/reference/pkg/cache/external/scheduler_cache.go:148-239,303-484
 *   ykhost_evaluate              the batched form of the core's loop over (ask, node) → Predicates()
 *
 * All functions return >= 0 on success, negative on error (text via ykhost_last_error). One lock per handle serialises
 * the entry points: the reference's callers hold read locks only (pkg/cache/context.go:697,709), so several threads may be
 * inside ykhost_predicates at once.
 */
#ifndef YKHOST_H_
#define YKHOST_H_
#include <stdint.h>

#include "ykpred.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ykhost ykhost_t;

/* NULL on failure (no GPU ⇒ failure). device < 0 makes a mirror-only handle: cache bookkeeping, request vectors and
 * snapshot dumps work, every evaluation fails (there is no CPU evaluation path). */
ykhost_t* ykhost_create(int32_t device, char* err, int32_t errlen);
void ykhost_destroy(ykhost_t* h);
const char* ykhost_last_error(const ykhost_t* h);

/* plugin lists of the four phases; defaults = NewPredicateManager (predicate_manager.go:321-373) */
int32_t ykhost_set_plugins(ykhost_t* h, uint32_t reservation_prefilters, uint32_t allocation_prefilters,
                           uint32_t reservation_filters, uint32_t allocation_filters);

/* --- cluster state (SchedulerCache mirror). JSON uses Kubernetes field names; see INTEGRATION.md. */
int32_t ykhost_load_snapshot(ykhost_t* h, const char* json); /* {"nodes":[{..., "pods":[...]}], "pods":[pending asks]} — replaces all state */
/* The six functions below restate the bookkeeping of scheduler_cache.go (podsMap / assignedPods / assumedPods /
 * orphanedPods), pinned by the scenarios of pkg/cache/external/scheduler_cache_test.go (tests/test_host_cache.py). */
int32_t ykhost_update_node(ykhost_t* h, const char* node_json);  /* → number of orphaned pods the (new) node adopted (:165-172) */
int32_t ykhost_remove_node(ykhost_t* h, const char* node_name);  /* → number of pods orphaned; assumed pods are reverted to pending (:205-219);
                                                                    unknown node: 0 */
/* → 1, or 0 when the pod was stored as an orphan (spec.nodeName names an unknown node, :352-360). spec.nodeName set ⇒
 * accounted on that node; unset ⇒ a pending ask (it inherits the node of the cached version, :336-339). status.phase
 * Running clears the assumed mark, Failed / Succeeded drops the pod (:344-347,374-383). */
int32_t ykhost_update_pod(ykhost_t* h, const char* pod_json);
int32_t ykhost_remove_pod(ykhost_t* h, const char* uid);         /* → 1 removed, 0 unknown uid (:390-417) */
/* Host ports follow framework.NodeInfo.UsedPorts, a SET of (ip, protocol, port): a pod that leaves its node takes its triples with
 * it even where another pod of the node holds the identical triple (no kubelet admits two such pods); the next AddPod puts them
 * back. A snapshot that is dumped and loaded again starts from the union of the pods' ports. */
/* The two update hooks for MANY objects at once — what the start-up replay of the informer caches amounts to
 * (Context.InitializeState, /root/reference/pkg/cache/context.go:1411-1484: every node, then every pod). `text` holds `len`
 * bytes of JSON documents one after the other (newline- or comma-separated; the body of a JSON array works): one cgo crossing,
 * one lock, and the pods share the template memo (pods of one Deployment / task group differ in name and uid only: all but the
 * first skip the JSON tree). → documents applied; on a malformed or rejected document -1 - (documents applied before it). */
int32_t ykhost_update_nodes_batch(ykhost_t* h, const char* text, int64_t len);
int32_t ykhost_update_pods_batch(ykhost_t* h, const char* text, int64_t len);
/* AssumePod: the cached pod gets spec.nodeName = node and is accounted there (moved from a node it was assumed on
 * before); the ask keeps its index (row) and is skipped by dump. Unknown pod / node: error. */
int32_t ykhost_assume_pod(ykhost_t* h, const char* uid, const char* node_name);
/* ForgetPod: the assumed mark is dropped; the cached pod keeps its node name and STAYS accounted on the node
 * (scheduler_cache.go:471-476 re-runs updatePod on the cached pod). → 1, or 0 for an unknown uid. */
int32_t ykhost_forget_pod(ykhost_t* h, const char* uid);
/* cache introspection: bit0 in podsMap, bit1 assigned (accounted on a node), bit2 assumed, bit3 orphan, bit4 holds an ask
 * row; node_out = spec.nodeName of the cached pod. 0 = unknown uid. */
int32_t ykhost_pod_state(ykhost_t* h, const char* uid, char* node_out, int32_t node_len);
int32_t ykhost_node_pod_count(ykhost_t* h, const char* node_name); /* len(NodeInfo.Pods), -1 = unknown node */

/* Gang scheduling. `task_groups_json` is the value of the pod annotation yunikorn.apache.org/task-groups (TaskGroup schema,
 * /root/reference/pkg/cache/amprotocol.go:47-57). ykhost_validate_task_groups restates GetTaskGroupsFromAnnotation +
 * validateTaskGroupResources (pkg/cache/utils.go:33-121: name / minMember / minResource present, no negative quantity, no
 * int64 overflow of minMember x minResource or of the cross-group aggregate, no cpu/vcore or explicit-"pods" collision) →
 * number of groups, negative = rejected (reason in ykhost_last_error). ykhost_add_task_groups also creates the minMember
 * placeholder pods of every group as pending asks, built like newPlaceholder (pkg/cache/placeholder.go:40-157): identical
 * labels (+ app id, queue), requests = minResource, nodeSelector, tolerations, affinity, topologySpreadConstraints — one
 * pod class per group. `app_json`: {"applicationId", "queue", "namespace"}. → number of placeholders created. */
int32_t ykhost_validate_task_groups(ykhost_t* h, const char* task_groups_json);
int32_t ykhost_add_task_groups(ykhost_t* h, const char* app_json, const char* task_groups_json);

/* The scheduler-interface callbacks as the core issues them — by allocation key (pod UID) and node id:
 * Context.IsPodFitNode (/root/reference/pkg/cache/context.go:696-716) behind AsyncRMCallback.Predicates
 * (pkg/cache/scheduler_callback.go:203-205). → 1 fit (err = ""), 0 does not fit (err = "failed plugin: '<name>'\n<message>",
 * the errors.Join of :713), YKHOST_E_POD_NOT_FOUND / YKHOST_E_NODE_NOT_FOUND with the texts of ErrorPodNotFound /
 * ErrorNodeNotFound (:66-69), YKHOST_E_NOT_AN_ASK for a cached pod that holds no ask row. */
#define YKHOST_E_POD_NOT_FOUND (-10)
#define YKHOST_E_NODE_NOT_FOUND (-11)
#define YKHOST_E_NOT_AN_ASK (-12)
#define YKHOST_E_UNSUPPORTED (-13) /* the ask is not evaluated by the engine (volumes, DRA claims, dictionary limits, specs the API
                                      server rejects): the caller's CPU PredicateManager answers this one; msg / err = the reason */
int32_t ykhost_is_pod_fit_node(ykhost_t* h, const char* allocation_key, const char* node_id, int32_t allocate, char* err, int32_t err_len);
/* Context.IsPodFitNodeViaPreemption (context.go:718-742) behind AsyncRMCallback.PreemptionPredicates
 * (scheduler_callback.go:207-216): → Index, or -1 for {Success: false} (no prefix of victims helps, unknown ask or node). */
int32_t ykhost_is_pod_fit_node_via_preemption(ykhost_t* h, const char* allocation_key, const char* node_id,
                                              const char* const* preempt_allocation_keys, int32_t num_keys, int32_t start_index);

/* synthetic KWOK-style cluster, replaces all state */
typedef struct ykhost_kwok {
  uint64_t seed;
  int32_t num_nodes;
  int32_t num_pods;
  int32_t num_templates;   /* distinct pod templates ("deployments"); 0 = every pod draws its own */
  int32_t node_affinity;   /* 0 = pods carry no nodeSelector/affinity (configs 1-2), 1 = config-3 mix */
  int32_t tolerations;     /* 0 = no tolerations and no node taints (config 1), 1 = KWOK taints + tolerations */
  int32_t unique_requests; /* 1 = adversarial: every pod a distinct cpu request (no signature sharing) */
  int32_t gang_size;       /* >0: pods are gang placeholders, `gang_size` identical members per task group */
  int32_t node_index_offset; /* node-sharded clusters: this shard holds global nodes [offset, offset+num_nodes); every node
                                draws from a stream keyed by its global index, so a shard holds exactly those nodes of the
                                unsharded cluster; pod draws depend on `seed` only (identical on all shards) */
  int32_t spread;            /* 1 = 10 % of the templates carry one DoNotSchedule zone-spread constraint (configs[4]) */
  int32_t total_nodes;       /* node-sharded clusters: node count of the whole cluster (0 = num_nodes); the asks' node pins
                                and matchFields names are drawn against it, so every shard holds the same asks */
  int32_t reserved[2];
} ykhost_kwok_t;
int32_t ykhost_generate_kwok(ykhost_t* h, const ykhost_kwok_t* cfg);

int32_t ykhost_num_nodes(const ykhost_t* h);
int32_t ykhost_num_pods(const ykhost_t* h); /* pending asks */
int32_t ykhost_pod_index(const ykhost_t* h, const char* uid);       /* index among pending asks, -1 = unknown */
int32_t ykhost_node_index(const ykhost_t* h, const char* node_name); /* -1 = unknown */

/* Serialises pending pods `pods[0..np)` (NULL = all) and nodes `nodes[0..nn)` (NULL = all, with their assigned pods)
 * as a snapshot document. Returns the required length (incl. NUL); writes at most `len` bytes. */
int64_t ykhost_dump_snapshot(ykhost_t* h, const int32_t* pods, int32_t np, const int32_t* nodes, int32_t nn, char* out, int64_t len);
/* The mirror's objects as the newline-separated documents the cache hooks would deliver: kind 0 = Node objects, 1 = pods on
 * nodes (spec.nodeName, status.phase Running), 2 = pending asks. Feeds ykhost_update_*_batch in bench.py's ingest leg and tests.
 * ykhost_ingest_stats: out[0] = pod documents that reused a known template without a parse, out[1] = full parses. */
int64_t ykhost_dump_documents(ykhost_t* h, int32_t kind, char* out, int64_t len);
int32_t ykhost_ingest_stats(ykhost_t* h, int64_t* out2);
/* Where the time of the pod batches went (summed over the handle's life): out[0] = scanning threads of the last batch that was
 * cut into pieces, out[1] = microseconds of the parallel scan, out[2] = microseconds of the ordered cache pass on the calling
 * thread (or of the bulk pass), out[3] = batches that took the parallel path, out[4] = those of them whose cache pass was the
 * bulk pass on every core (all pods new, everything to be re-encoded anyway — the start-up replay). */
int32_t ykhost_ingest_timing(ykhost_t* h, int64_t* out5);
/* on != 0: ykhost_dump_snapshot writes runs of on-node pods that share a pod template once, with "replicas": k (the loaders
 * expand them; their uids get a "#r" suffix) — what keeps the dump of a 50 000-node cluster small enough to hand to the
 * oracle for full-grid parity. */
int32_t ykhost_set_dump_compact(ykhost_t* h, int32_t on);

/* The encoded (structure-of-arrays) tables that cross the C ABI, as JSON (64-bit masks as hex strings); works on a
 * mirror-only handle. For encoder tests on machines without a device. Returns the required length like dump_snapshot. */
int64_t ykhost_encoded_tables_json(ykhost_t* h, char* out, int64_t len);

/* encode + upload whatever changed since the last sync (called implicitly by the functions below) */
int32_t ykhost_sync(ykhost_t* h);
ykpred_engine_t* ykhost_engine(ykhost_t* h); /* the underlying engine, for layout / readback / timing calls */

/* Node-sharded clusters (one handle per GPU, each mirroring a contiguous shard of the nodes and all asks): the shards agree
 * on one bitmap row stride (that of the largest shard) so that ykpred_gather_bitmap yields the regular layout
 * [world][P][row_stride]; ykhost_comm_init uploads the tables and attaches the RCCL communicator to the engine
 * (ykpred_comm_init). The gather / decision exchange are then called on ykhost_engine(h). */
int32_t ykhost_set_row_stride(ykhost_t* h, int32_t words /* multiple of 16; 0 = automatic */);
int32_t ykhost_set_row_capacity(ykhost_t* h, int32_t rows /* physical bitmap rows every shard allocates; 0 = automatic */);
int32_t ykhost_comm_init(ykhost_t* h, const uint8_t* id /* [YKPRED_COMM_ID_BYTES] */, int32_t rank, int32_t world, int32_t node_offset);
/* The shards' topology dictionaries are made cluster-wide inside ykhost_comm_init: every shard exports its node-side share
 * (the values of every topology key on its nodes, the templates of its pods that carry required anti-affinity terms, its first
 * and last NodeID), the shards all-gather the exports (ykpred_comm_allgather_bytes), and each keeps the union as the floor of
 * every later re-encode — domain id d is the same value and count class s the same class on every shard, so the histograms
 * the engine sums line up cell by cell. When the union changes the dictionary shape the engine is re-created and adopts the
 * communicator (ykpred_comm_adopt); the digest of the dictionaries goes to the engine (ykpred_set_dictionary_digest). The merge also checks the name-sorted contract (every
 * NodeID of shard r sorts before every NodeID of shard r + 1) and refuses, on every rank alike, when it is broken.
 * The two halves are callable on their own (mirror-only handles included):
 *   ykhost_topology_export  this shard's export; returns the required length (like dump_snapshot). Not a pure query: a
 *                           device handle syncs first (uploads what changed), a mirror-only handle re-encodes its objects
 *   ykhost_topology_merge   `len` bytes of every shard's export in rank order, each followed by a NUL byte */
int64_t ykhost_topology_export(ykhost_t* h, char* out, int64_t len);
int32_t ykhost_topology_merge(ykhost_t* h, const char* blobs, int64_t len);
int32_t ykhost_comm_destroy(ykhost_t* h);

/* batched evaluation of every pending ask against every node: phase selects the plugin lists */
int32_t ykhost_evaluate(ykhost_t* h, int32_t allocate, uint32_t options /* YKPRED_OUT_* | YKPRED_EVAL_* */);

/* Like ykhost_evaluate, but when only node rows changed since the last evaluation of this phase (AssumePod / ForgetPod /
 * pods added to or removed from nodes) it patches just those node columns (ykpred_eval_nodes). *columns_patched receives
 * the number of columns re-evaluated, or -1 when a full evaluation was required. On a node-sharded handle (ykhost_comm_init)
 * whose asks carry topology constraints the call is COLLECTIVE: every shard's host makes it for the step, with or without
 * changes of its own — the engine exchanges the topology histograms inside. */
int32_t ykhost_evaluate_dirty(ykhost_t* h, int32_t allocate, uint32_t options, int32_t* columns_patched);

/* PredicateManager.Predicates for pending pod #pod on node #node. Returns 1 = fits ("", nil), 0 = error returned.
 * plugin receives the failing plugin name ("" when a PreFilter plugin rejected the pod), msg the status message. */
int32_t ykhost_predicates(ykhost_t* h, int32_t pod, int32_t node, int32_t allocate, char* plugin, int32_t plugin_len, char* msg,
                          int32_t msg_len);
/* The callbacks above are served from the RESIDENT answer whenever an evaluation of the phase is current: on the first
 * callback after ykhost_evaluate the class-compressed bitmap ([classes][row_words]; YKHOST_RESIDENT_MB, default 256, bounds it —
 * beyond that one row per ask) is mirrored to the host, and a callback becomes ask → class → bit. A node whose column changed
 * since (AssumePod between two asks) is answered per pair from the tables; a pair that does not fit costs one packed
 * whole-class query for its failing plugin (cached). Without a current evaluation: one ykpred_query_pod per ask, as before.
 * ykhost_candidates: the first k feasible nodes of the ask in bin-pack order — the node loop of the core in one call.
 * → nodes written, YKPRED_E_STATE (-4) if no evaluation WITH decisions is current. ykhost_resident_stats: out[0] callbacks served
 * from the mirror, [1] per pair (changed column), [2] by whole-ask queries, [3] answer fetches, [4] failing-plugin fetches. */
int32_t ykhost_candidates(ykhost_t* h, int32_t pod, int32_t allocate, int32_t k, int32_t* out_nodes /* [k] */);
int32_t ykhost_resident_stats(ykhost_t* h, int64_t* out5);

/* One scheduling ROUND with conflict-resolved decisions — what the core's loop decides for the asks asks[0..n) (indices into
 * the ask table, in decision order; NULL = asks 0..n-1): ask i is decided with asks 0..i-1 ASSUMED on their nodes (the core
 * decides an ask, AsyncRMCallback.UpdateAllocation → Context.AssumePod runs, scheduler_callback.go:49-98 / context.go:828-885,
 * and the next Predicates() call sees the node's new Requested / pod list). out_nodes[i] = node index, -1 = no node fits,
 * -2 = the ask is routed to the CPU manager (not evaluated by the engine) and takes no part in the round.
 * The whole round is ONE device call (ykpred_allocate_round): node resources, pod slots, host ports and the match counts behind
 * PodTopologySpread / InterPodAffinity are kept live on the device (the host uploads what a pod of every spec adds to its node:
 * ykpred_set_spec_effects); the engine runs it with its sequential kernel or in batches — parallel proposals, the loop replayed on
 * the host — whichever the ask list favours, with identical decisions (ykpred.h: ykpred_allocate_round, ykpred_get_round_info). Only when those effects are withheld (YKHOST_ROUND_ON_HOST=1, tests) does the host decide ask by ask
 * (decision → AssumePod → column patch → next decision) — that path needs apply != 0 to see its own allocations and refuses
 * apply == 0 with YKHOST_E_UNSUPPORTED.
 * NODE-SHARDED cluster (a communicator with world > 1 is attached to the engine): the call is COLLECTIVE — every rank calls with the
 * same asks in the same order — and node indices in out_nodes are indices in the WHOLE cluster (this shard's node 0 = its
 * node_offset), identical on every rank; an ask that went to another shard's node is assumed here as well (it leaves the pending
 * asks) without touching a node of this mirror. Topology constraints are part of the collective form (the owner of an accepted node
 * hands what its assume added to the histograms to the other shards: ykpred.h). A sharded round the collective form does not cover
 * (spec effects withheld; a pod that moves more histogram cells than a delta record holds) returns YKHOST_E_UNSUPPORTED — it is never
 * decided shard by shard.
 * apply != 0: every ask that got a node is assumed in the mirror exactly as ykhost_assume_pod would. → number of asks that got a
 * node, or a negative error. ykhost_round_stats: out[0] rounds decided by one device call, [1] asks decided in them, [2] asks
 * decided ask by ask, [3] asks routed. */
int32_t ykhost_allocate_round(ykhost_t* h, int32_t n, const int32_t* asks, int32_t apply, int32_t* out_nodes /* [n] */);
int32_t ykhost_round_stats(ykhost_t* h, int64_t* out4);

/* WHY an ask fits nowhere (ykpred.h: ykpred_explain) — the text kube-scheduler prints for an unschedulable pod and the shim can put
 * into the Message of the PodScheduled=False / Unschedulable condition (/root/reference/pkg/cache/context.go:1272-1285).
 *   ykhost_explain          syncs, picks the phase's plugin lists and makes ONE engine call for the listed asks (NULL = asks 0..n-1):
 *                           out_bins[i] = the YKPRED_EXPLAIN_BINS histogram of ask i over all nodes. An ask routed to the CPU manager
 *                           gets [10] = N without a device call. A mirror-only handle fails like every other evaluation. On a
 *                           node-sharded handle the call is collective and the bins are cluster-wide.
 *   ykhost_explain_format   a PURE function of the bins and the handle's resource names (works on a mirror-only handle):
 *                           total = bins[0] + ... + bins[10]; total == 0 gives "no nodes available to schedule pods"; otherwise
 *                           "<bins[9]>/<total> nodes are available" + ": <count> <text>, <count> <text>." (or just "." without entries) —
 *                           one entry per reason text with a count > 0, entries of equal text merged, the entry strings sorted
 *                           bytewise ("10 x" before "2 y", as upstream sorts them). The wording is kube-scheduler's FitError (upstream
 *                           wording, not reference-held); the texts are those of the per-pair messages. The taint entry is the generic
 *                           "node(s) had untolerated taint": upstream's per-taint {key: value} breakdown is out of scope.
 *                           → required length incl. NUL; writes at most `len` bytes.
 *   ykhost_explain_message  explain + format for one ask by allocation key (pod UID). → required length, or
 *                           YKHOST_E_POD_NOT_FOUND / YKHOST_E_NOT_AN_ASK as ykhost_is_pod_fit_node, YKHOST_E_UNSUPPORTED with the
 *                           routing reason in `out` for an ask the engine does not evaluate. */
int32_t ykhost_explain(ykhost_t* h, int32_t n, const int32_t* asks /* NULL = asks 0..n-1 */, int32_t allocate, int32_t* out_bins /* [n][32] */);
int64_t ykhost_explain_format(ykhost_t* h, const int32_t* bins /* [32] */, char* out, int64_t len);
int64_t ykhost_explain_message(ykhost_t* h, const char* allocation_key, int32_t allocate, char* out, int64_t len);

/* HOW MANY copies of an ask the cluster can still place (ykpred.h: ykpred_headroom) — what the gang path otherwise learns by waiting
 * out placeholderTimeoutInSeconds. Always with the ALLOCATION-phase plugin lists: the reservation lists carry no NodeResourcesFit.
 *   ykhost_headroom         syncs and makes ONE engine call for the listed asks (NULL = asks 0..n-1): out_cells[i] = the
 *                           YKPRED_HEADROOM_CELLS cells of ask i over all nodes. An ask routed to the CPU manager gets status [3] = 1
 *                           without a device call. A mirror-only handle fails like every other evaluation. On a node-sharded handle
 *                           the call is collective and the cells are cluster-wide.
 *   ykhost_headroom_nodes   replicas of ONE ask on every node (ykpred_headroom_pod): which nodes take how many copies; -1 everywhere
 *                           for a coupled ask, 0 everywhere for a routed one; this shard's nodes on a node-sharded handle.
 *   ykhost_headroom_by_key  ykhost_headroom for one ask by allocation key (pod UID). → 0, or YKHOST_E_POD_NOT_FOUND /
 *                           YKHOST_E_NOT_AN_ASK as ykhost_is_pod_fit_node, YKHOST_E_UNSUPPORTED (with out16[3] = 1) for an ask the
 *                           engine does not evaluate. */
int32_t ykhost_headroom(ykhost_t* h, int32_t n, const int32_t* asks /* NULL = asks 0..n-1 */, int64_t* out_cells /* [n][16] */);
int32_t ykhost_headroom_nodes(ykhost_t* h, int32_t pod, int32_t* out /* [N] */);
int32_t ykhost_headroom_by_key(ykhost_t* h, const char* allocation_key, int64_t* out16 /* [16] */);

/* Headroom per TOPOLOGY DOMAIN (ykpred.h: ykpred_headroom_groups) — which zone, rack or host still takes all minMember members of a gang
 * with a locality requirement, and which of them is the tightest fit: the value a shim adds to the placeholders' nodeSelector. The groups
 * are derived from a node LABEL KEY in the mirror: group ids are the ranks of the bytewise-sorted distinct values of the key, a node
 * without the label is in no group (-1). The column is kept per (key, node-table epoch). Always the ALLOCATION-phase plugin lists.
 *   ykhost_headroom_domains        syncs and makes ONE engine call for the listed asks (NULL = asks 0..n-1) with want[i] members each (NULL
 *                                  = 1): out_summary[i] = the YKPRED_GROUP_SUMMARY cells; out_groups (may be NULL) [i][G + 1]
 *                                  [YKPRED_GROUP_CELLS] = { copies, nodes } per domain, row G for the nodes without the label;
 *                                  groups_cap = the int64 cells out_groups holds (YKPRED_E_INVALID when fewer than n * (G + 1) * 2).
 *                                  → G >= 0, the number of domains, or an error < 0. A routed ask gets status 1 without a device call.
 *                                  On a node-sharded handle the call is COLLECTIVE: the shards unite their value lists
 *                                  (ykpred_comm_allgather_bytes, lengths first), so ids, rows and summaries are cluster-wide.
 *                                  Every rank passes the same asks, wants, key and capacity: the engine's agreement step turns a
 *                                  bad index or want on one rank into the same error on all of them.
 *   ykhost_domain_values           the values of the key in id order as a JSON array → the length needed (with the terminator), as
 *                                  ykhost_explain_format. Collective on a node-sharded handle for the same reason.
 *   ykhost_headroom_domain_by_key  ONE crossing for one ask by allocation key (pod UID): the summary, and the domain with the most
 *                                  copies / the tightest domain that holds `want` as label VALUES ("" when there is none). → 0, or the
 *                                  errors of ykhost_headroom_by_key (YKHOST_E_UNSUPPORTED with out_summary[0] = 1). */
int32_t ykhost_headroom_domains(ykhost_t* h, int32_t n, const int32_t* pods /* NULL = asks 0..n-1 */, const int64_t* want /* [n], NULL = all 1 */,
                                const char* label_key, int64_t* out_summary /* [n][8] */, int64_t* out_groups /* [n][G + 1][2], may be NULL */,
                                int64_t groups_cap);
int64_t ykhost_domain_values(ykhost_t* h, const char* label_key, char* out, int64_t len);
int32_t ykhost_headroom_domain_by_key(ykhost_t* h, const char* allocation_key, const char* label_key, int64_t want, int64_t* out_summary /* [8] */,
                                      char* best, int64_t best_len, char* tightest, int64_t tightest_len);

/* Headroom of asks with ONE hard spread constraint (ykpred.h: ykpred_headroom_spread) — the fallback when ykhost_headroom reports an ask
 * as coupled (status 2): how many placeholders of a task group with topologySpreadConstraints the cluster still takes, and in which
 * domains. Always the ALLOCATION-phase plugin lists. Domain ids are the ranks of the bytewise-sorted values of the constraint's key.
 *   ykhost_headroom_spread          syncs and makes ONE engine call for the listed asks (NULL = asks 0..n-1): out_cells[i] = the
 *                                   YKPRED_SPREAD_HEADROOM_CELLS cells. A routed ask gets status 1 without a device call. → 0 or an error.
 *                                   Collective on a node-sharded handle: every rank passes the same asks.
 *   ykhost_headroom_spread_domains  one ask: the cells, its per-domain rows out_rows[d] = { cnt, cap, nodes, copies } and the domains' label
 *                                   VALUES in id order as a JSON array (as ykhost_domain_values; "[]" at a status other than 0) → the
 *                                   number of domains D (0 at a status other than 0), or an error < 0. With max_domains < D nothing but
 *                                   the cells is written: call again with room for D (as ykhost_explain_format reports a length).
 *   ykhost_headroom_spread_by_key   ONE crossing for one ask by allocation key (pod UID): the cells, and the domain with the most copies
 *                                   as a label VALUE ("" when there is none). → 0, or the errors of ykhost_headroom_by_key
 *                                   (YKHOST_E_UNSUPPORTED with out16[3] = 1). */
int32_t ykhost_headroom_spread(ykhost_t* h, int32_t n, const int32_t* asks /* NULL = asks 0..n-1 */, int64_t* out_cells /* [n][16] */);
int32_t ykhost_headroom_spread_domains(ykhost_t* h, int32_t pod, int64_t* out_summary /* [16] */, int64_t* out_rows /* [max_domains][4] */,
                                       int32_t max_domains, char* values, int64_t values_len);
int32_t ykhost_headroom_spread_by_key(ykhost_t* h, const char* allocation_key, int64_t* out16 /* [16] */, char* best, int64_t best_len);

/* Headroom of asks with required pod (anti-)affinity (ykpred.h: ykpred_headroom_affinity) — the other fallback when ykhost_headroom
 * reports an ask as coupled (status 2): how many placeholders of a task group with "one executor per host" (or any required
 * podAffinity / podAntiAffinity whose copies meet on one topology key) the cluster still takes, and in which domains. Always the
 * ALLOCATION-phase plugin lists. Each call syncs and uploads the spec effects when the spec table moved since the last upload.
 *   ykhost_headroom_affinity          ONE engine call for the listed asks (NULL = asks 0..n-1): out_cells[i] = the
 *                                     YKPRED_AFFINITY_HEADROOM_CELLS cells. A routed ask gets status 1 without a device call. → 0 or an
 *                                     error. Collective on a node-sharded handle: every rank passes the same asks.
 *   ykhost_headroom_affinity_domains  one ask at status 0 or 4: the cells, its rows out_rows[d] = { cnt, cap, nodes, copies } per domain
 *                                     with the OUTSIDE row (nodes without the key) at out_rows[D], and the domains' label VALUES in id
 *                                     order as a JSON array → D, or an error < 0; 0 and "[]" at any other status. out_rows holds
 *                                     max_domains + 1 rows; with max_domains < D nothing but the cells is written: call again with room.
 *   ykhost_headroom_affinity_by_key   ONE crossing for one ask by allocation key (pod UID): the cells, and the domain with the most
 *                                     copies as a label VALUE ("" when there is none). → 0, or the errors of ykhost_headroom_by_key
 *                                     (YKHOST_E_UNSUPPORTED with out16[3] = 1). */
int32_t ykhost_headroom_affinity(ykhost_t* h, int32_t n, const int32_t* asks /* NULL = asks 0..n-1 */, int64_t* out_cells /* [n][16] */);
int32_t ykhost_headroom_affinity_domains(ykhost_t* h, int32_t pod, int64_t* out_summary /* [16] */, int64_t* out_rows /* [max_domains + 1][4] */,
                                         int32_t max_domains, char* values, int64_t values_len);
int32_t ykhost_headroom_affinity_by_key(ykhost_t* h, const char* allocation_key, int64_t* out16 /* [16] */, char* best, int64_t best_len);

/* PREEMPTION REACH (ykpred.h: ykpred_preempt_reach) — can preemption help an ask at all, and on which nodes? — asked before the core
 * builds a victim list per node and walks the nodes through PreemptionPredicates. The mirror keeps what the reference's shim reads of a
 * pod for preemption: spec.priority (0 when missing), spec.preemptionPolicy and the pod-level opt-out annotation
 * yunikorn.apache.org/allow-preemption: "false". Always the ALLOCATION-phase plugin lists, as the reference uses for preemption.
 *   ykhost_set_preemption_tiers  ascending priority bounds b[0] < ... < b[T-1], 1 <= T <= 8. A pod on a node is in tier t = the smallest
 *                                t with priority < b[t]; a pod of priority >= b[T-1], an opted-out pod and a pod on no node are in no
 *                                tier and never victims. T == 0 switches the feature off and drops the device table. Nothing is built or
 *                                uploaded until the bounds are set. The LIMIT of an ask = the number of bounds <= its priority, 0 with
 *                                preemptionPolicy: Never.
 *   ykhost_preempt_reach         syncs, brings the device's reclaim table up to date — whole after a node was added or removed or the
 *                                bounds changed, else only the columns of the nodes whose pods changed (add / remove / update / assume /
 *                                forget) — and makes ONE engine call for the listed asks (NULL = asks 0..n-1): out_cells[i] = the
 *                                YKPRED_REACH_CELLS cells. An ask routed to the CPU manager gets status [10] = 1 without a device call.
 *                                YKPRED_E_STATE without tiers. Collective on a node-sharded handle: every rank passes the same asks.
 *   ykhost_preempt_reach_nodes   the level of ONE ask on every node (ykpred_preempt_reach_pod), -1 = never: the shortlist the caller
 *                                walks for the real victim selection; this shard's nodes on a node-sharded handle.
 *   ykhost_preempt_reach_by_key  ONE crossing for one ask by allocation key (pod UID): the cells, and the best node ([13]) by NAME (""
 *                                when there is none, or when it lies on another shard). → 0, or the errors of ykhost_headroom_by_key
 *                                (YKHOST_E_UNSUPPORTED with out16[10] = 1).
 *   ykhost_reclaim_table         the planes the mirror would upload, copied out: dims = { T, R, KP, N }; requests [T][R][N], pods [T][N],
 *                                ports_after [T][KP][N] (any of the three may be NULL: only the dims come back). Works on a mirror-only
 *                                handle: the table can be checked without a device. */
int32_t ykhost_set_preemption_tiers(ykhost_t* h, const int32_t* bounds, int32_t num_tiers);
int32_t ykhost_preempt_reach(ykhost_t* h, int32_t n, const int32_t* asks /* NULL = asks 0..n-1 */, int64_t* out_cells /* [n][16] */);
int32_t ykhost_preempt_reach_nodes(ykhost_t* h, int32_t pod, int32_t* out /* [N] */);
int32_t ykhost_preempt_reach_by_key(ykhost_t* h, const char* allocation_key, int64_t* out16 /* [16] */, char* best_node_name, int64_t len);
int32_t ykhost_reclaim_table(ykhost_t* h, int32_t* dims /* [4] */, int64_t* requests, int32_t* pods, uint64_t* ports_after);
/* The limits of the listed asks (NULL = asks 0..n-1) as the mirror derives them, after the sync and the reclaim-table update of
 * ykhost_preempt_reach and without an engine query: what a caller of ykpred_preempt_reach with plugin lists of its own passes on. */
int32_t ykhost_preempt_limits(ykhost_t* h, int32_t n, const int32_t* asks /* NULL = asks 0..n-1 */, int32_t* out_limits /* [n] */);

/* PREEMPTION EXPLAIN (ykpred.h: ykpred_preempt_explain) — WHY an ask is still pending with preemption on: the second sentence of
 * kube-scheduler's message for an unschedulable pod, "preemption: 0/5000 nodes are available: 3000 Preemption is not helpful for
 * scheduling, 1500 No preemption victims found for incoming pod, 500 Insufficient memory.", behind ykhost_explain's first one. The tiers
 * are those of ykhost_set_preemption_tiers, the limits are derived and the reclaim table is kept up to date exactly as for
 * ykhost_preempt_reach; always the ALLOCATION-phase plugin lists.
 *   ykhost_preempt_explain          syncs and makes ONE engine call for the listed asks (NULL = asks 0..n-1): out_cells[i] = the
 *                                   YKPRED_PREEMPT_EXPLAIN_CELLS cells. An ask routed to the CPU manager gets [10] = N and status [30] = 1
 *                                   without a device call. YKPRED_E_STATE without tiers. Collective on a node-sharded handle: every rank
 *                                   passes the same asks.
 *   ykhost_preempt_explain_nodes    the per-node word of ONE ask on every node (ykpred_preempt_explain_pod); this shard's nodes on a
 *                                   node-sharded handle.
 *   ykhost_preempt_explain_format   a PURE function of the cells and the handle's resource names (works on a mirror-only handle):
 *                                   total = cells[0] + ... + cells[11]; "preemption: <cells[11]>/<total> nodes are available" + the
 *                                   entries in ykhost_explain_format's style (counts > 0 only, equal texts merged, the entry strings
 *                                   sorted bytewise; "0/0 nodes are available." for an empty total): [25] "Preemption is not helpful
 *                                   for scheduling", [24] "No preemption victims found for incoming pod", [27] the NodePorts text and
 *                                   [12] the too-many-pods text of the per-pair messages, [16 + r] "Insufficient <resource r>", [10]
 *                                   the routed-ask text of ykhost_explain_format. A not-enough node whose last failure is a frozen
 *                                   plugin behind NodeResourcesFit is in [26] and has no entry. The wording is kube-scheduler's
 *                                   PostFilter message of the default preemption plugin (upstream wording, not reference-held).
 *                                   → required length incl. NUL; writes at most `len` bytes.
 *   ykhost_preempt_explain_message  ONE crossing for one ask by allocation key (pod UID): ykhost_explain_format's sentence of the
 *                                   allocation phase, a space, then the preemption sentence — as kube-scheduler joins them. → required
 *                                   length, or the errors of ykhost_explain_message. */
int32_t ykhost_preempt_explain(ykhost_t* h, int32_t n, const int32_t* asks /* NULL = asks 0..n-1 */, int64_t* out_cells /* [n][32] */);
int32_t ykhost_preempt_explain_nodes(ykhost_t* h, int32_t pod, uint32_t* out /* [N] */);
int64_t ykhost_preempt_explain_format(ykhost_t* h, const int64_t* cells /* [32] */, char* out, int64_t len);
int64_t ykhost_preempt_explain_message(ykhost_t* h, const char* allocation_key, char* out, int64_t len);

/* PREEMPTION HEADROOM (ykpred.h: ykpred_preempt_headroom) — can preemption up to the ask's priority place the whole gang, at which level,
 * and at the cost of how many resident pods? — asked where a task group creates its minMember placeholders, before the timeout wait.
 * The tiers are those of ykhost_set_preemption_tiers, the limits are derived and the reclaim table is kept up to date exactly as for
 * ykhost_preempt_reach; always the ALLOCATION-phase plugin lists.
 *   ykhost_preempt_headroom         ONE engine call for the listed asks (NULL = asks 0..n-1) with their wants (NULL = 1 each; a want
 *                                   < 1 is YKPRED_E_INVALID): out_cells[i] = the YKPRED_PREEMPT_HEADROOM_CELLS cells. An ask routed to the
 *                                   CPU manager gets status [27] = 1 without a device call. YKPRED_E_STATE without tiers. Collective on a
 *                                   node-sharded handle: every rank passes the same asks and wants.
 *   ykhost_preempt_headroom_nodes   rep_L of ONE ask on every node, L = 0..limit (ykpred_preempt_headroom_pod): out holds
 *                                   [limit+1][N] — size it for [tiers+1][N] —, *out_limit the ask's limit; this shard's nodes on a
 *                                   node-sharded handle.
 *   ykhost_preempt_headroom_by_key  ONE crossing for one ask by allocation key (pod UID) and its want: the 32 cells. → 0, or the
 *                                   errors of ykhost_headroom_by_key (YKHOST_E_UNSUPPORTED with out32[27] = 1). */
int32_t ykhost_preempt_headroom(ykhost_t* h, int32_t n, const int32_t* asks /* NULL = asks 0..n-1 */, const int64_t* wants /* NULL = 1 */,
                                int64_t* out_cells /* [n][32] */);
int32_t ykhost_preempt_headroom_nodes(ykhost_t* h, int32_t pod, int32_t* out /* [limit+1][N] */, int32_t* out_limit);
int32_t ykhost_preempt_headroom_by_key(ykhost_t* h, const char* allocation_key, int64_t want, int64_t* out32 /* [32] */);

/* PREEMPTION VICTIMS (ykpred.h: ykpred_preempt_victims) — the shortest victim prefix on every node in one pass: what the core's loop of
 * one PreemptionPredicates callback per candidate node answers, from resident state. Tiers, limits and victim eligibility are those of
 * ykhost_set_preemption_tiers; order(n) = the pods of node n that are in a tier, sorted by (priority ascending, uid ascending
 * bytewise); always the ALLOCATION-phase plugin lists. The mirror keeps the victim table — one segment per node with a capacity of
 * count + count / 2 + 4 rows — and NOTHING of it is derived or uploaded before the first call of this group: at a call it patches the
 * segments of the nodes whose pods changed (add / remove / update / assume / forget), or derives and uploads the whole table after a
 * bounds change, an engine re-creation or a segment that outgrew its capacity.
 *   ykhost_preempt_victims         syncs, brings the reclaim and the victim table up to date and makes ONE engine call for the listed
 *                                  asks (NULL = asks 0..n-1): out_cells[i] = the YKPRED_VICTIM_CELLS cells. An ask routed to the CPU
 *                                  manager gets status [3] = 1 without a device call. YKPRED_E_STATE without tiers. Collective on a
 *                                  node-sharded handle: every rank passes the same asks.
 *   ykhost_preempt_victims_nodes   need of ONE ask on every node (ykpred_preempt_victims_pod): 0 fits as it stands, k >= 1 the first k
 *                                  pods of order(n) must go, -1 never; this shard's nodes on a node-sharded handle.
 *   ykhost_victim_list             the uids of order(node) in tiers < limit, NUL-separated (each uid followed by one NUL), *count of
 *                                  them: the first `need` of them are the victims. A buffer too short holds the uids that fit whole;
 *                                  *count is always the full number. Works on a mirror-only handle.
 *   ykhost_preempt_victims_by_key  ONE crossing for one ask by allocation key (pod UID): the cells, the best node ([6]) by NAME and the
 *                                  uids of its prefix of [7] pods, NUL-separated ("" / nothing when there is none, or when the node
 *                                  lies on another shard). → 0, or the errors of ykhost_headroom_by_key (YKHOST_E_UNSUPPORTED with
 *                                  out16[3] = 1).
 *   ykhost_victim_table            the table as the mirror keeps it (patched, not derived afresh), copied out: dims = { T, R, KP, N, P };
 *                                  seg_base [N], seg_cap [N], tier_end [T][N], cum [R][P], ports_after [KP][P] (any NULL: only the
 *                                  dims come back). Works on a mirror-only handle: the table and its patching can be checked without a
 *                                  device.
 *   ykhost_victim_stats            out2 = { whole tables derived, segments patched } so far. */
int32_t ykhost_preempt_victims(ykhost_t* h, int32_t n, const int32_t* asks /* NULL = asks 0..n-1 */, int64_t* out_cells /* [n][16] */);
int32_t ykhost_preempt_victims_nodes(ykhost_t* h, int32_t pod, int32_t* out /* [N] */);
int32_t ykhost_victim_list(ykhost_t* h, int32_t node, int32_t limit, char* uids_buf, int64_t len, int32_t* count);
int32_t ykhost_preempt_victims_by_key(ykhost_t* h, const char* allocation_key, int64_t* out16 /* [16] */, char* best_node_name, int64_t name_len,
                                      char* victim_uids, int64_t uids_len);
int32_t ykhost_victim_table(ykhost_t* h, int32_t* dims /* [5] */, int32_t* seg_base, int32_t* seg_cap, int32_t* tier_end, int64_t* cum,
                            uint64_t* ports_after);
int32_t ykhost_victim_stats(ykhost_t* h, int64_t* out2 /* [2] */);

/* PREEMPTION ROUND (ykpred.h: ykpred_preempt_round) — conflict-resolved victim plans for a list of asks: what the caller's loop of
 * ykhost_preempt_victims_by_key, ykhost_remove_pod per victim and ykhost_assume_pod per ask answers, in one call that changes nothing
 * in the mirror or on the device. The asks are processed in list order, each under the state the earlier ones left behind; a repeated
 * ask is one more copy (a gang). Limits are the mirror's (ykhost_set_preemption_tiers); always the ALLOCATION-phase plugin lists.
 *   ykhost_preempt_round          syncs, brings the reclaim and the victim table up to date as ykhost_preempt_victims does and makes ONE
 *                                 engine call: out_cells[i] = the YKPRED_PREEMPT_ROUND_CELLS cells of ask i of the list (NULL = asks
 *                                 0..n-1), out_summary = the 8 summary cells. An ask routed to the CPU manager gets outcome 3 without
 *                                 taking a turn. Collective on a node-sharded handle: every rank passes the same asks.
 *   ykhost_preempt_round_by_keys  ONE crossing: allocation keys (pod UIDs) in; beside the cells, node_names receives per ask the node
 *                                 by NAME ("" at outcome 2..4, or when the node lies on another shard), each followed by one NUL, and
 *                                 victim_uids the uids of order(node)[from .. from + extra) of every ask in list order, each followed by
 *                                 one NUL (ask i owns the next cells[i][3] of them). needed2 = { bytes of names, bytes of uids } the
 *                                 answer needs; a buffer too short holds what fits whole. YKHOST_E_POD_NOT_FOUND / YKHOST_E_NOT_AN_ASK
 *                                 for a key that names no ask (nothing is computed).
 *   ykhost_preempt_gang_by_key    the same over `want` copies of one ask: where the gang goes and at whose cost (ykhost_preempt_headroom
 *                                 says only whether it fits at a level).
 *   ykhost_victim_range           the uids of order(node)[from .. from + count), NUL-separated, *got of them, *needed bytes: the slice
 *                                 the by-keys call hands out. Works on a mirror-only handle. */
int32_t ykhost_preempt_round(ykhost_t* h, int32_t n, const int32_t* asks /* NULL = asks 0..n-1 */, int64_t* out_cells /* [n][8] */,
                             int64_t* out_summary /* [8] */);
int32_t ykhost_preempt_round_by_keys(ykhost_t* h, int32_t n, const char* const* allocation_keys, int64_t* out_cells /* [n][8] */,
                                     int64_t* out_summary /* [8] */, char* node_names, int64_t names_len, char* victim_uids, int64_t uids_len,
                                     int64_t* needed2 /* [2] or NULL */);
int32_t ykhost_preempt_gang_by_key(ykhost_t* h, const char* allocation_key, int32_t want, int64_t* out_cells /* [want][8] */,
                                   int64_t* out_summary /* [8] */, char* node_names, int64_t names_len, char* victim_uids, int64_t uids_len,
                                   int64_t* needed2 /* [2] or NULL */);
int32_t ykhost_victim_range(ykhost_t* h, int32_t node, int32_t from, int32_t count, char* uids_buf, int64_t len, int32_t* got, int64_t* needed);

/* PREEMPTION ROUND WITH LIVE TOPOLOGY HISTOGRAMS (ykpred.h: ykpred_preempt_round_live) — ykhost_preempt_round for lists that hold asks with
 * a hard topology spread, required pod affinity or anti-affinity: no ask is settled as coupled (outcome 4 never occurs), every ask takes
 * its turn against the histograms as the earlier placements AND the earlier victims left them. What the caller's loop of
 * ykhost_preempt_victims_by_key, ykhost_remove_pod per victim and ykhost_assume_pod per ask answers for such asks, in one call that
 * changes nothing in the mirror or on the device.
 *   ykhost_preempt_round_live          as ykhost_preempt_round; before the engine call the specs' effects and the VICTIM-EFFECTS PLANE
 *                                      are brought up to date. The mirror derives no plane before the first live call (or
 *                                      ykhost_victim_effects); from then on victims_refresh patches it with the segments of changed nodes
 *                                      and derives it anew when the selector classes move or a class gains its first contributing
 *                                      victim. out_counts [counts_len] / out_minima [minima_len] (each may be NULL) receive the
 *                                      round-local histograms after the last turn, as far as they fit; hist_needed2 (may be NULL) =
 *                                      { histogram cells, constraints }. out_summary[7] = (turn, constraint) pairs that moved a cell.
 *   ykhost_preempt_round_live_by_keys  ykhost_preempt_round_by_keys over the live round, one crossing.
 *   ykhost_preempt_gang_live_by_key    ykhost_preempt_gang_by_key over the live round: where a gang with a zone spread or a "one per
 *                                      host" rule goes and at whose cost.
 *   ykhost_victim_effects              the plane as the mirror keeps it, copied out: dims = { KS, KA, P, planes derived, segments
 *                                      patched }; class_col [KS] (-1: no column), cum [KA][P] prefix sums within the segment (either
 *                                      NULL: only the dims come back). Works on a mirror-only handle. */
int32_t ykhost_preempt_round_live(ykhost_t* h, int32_t n, const int32_t* asks /* NULL = asks 0..n-1 */, int64_t* out_cells /* [n][8] */,
                                  int64_t* out_summary /* [8] */, int32_t* out_counts, int64_t counts_len, int32_t* out_minima, int64_t minima_len,
                                  int64_t* hist_needed2 /* [2] or NULL */);
int32_t ykhost_preempt_round_live_by_keys(ykhost_t* h, int32_t n, const char* const* allocation_keys, int64_t* out_cells /* [n][8] */,
                                          int64_t* out_summary /* [8] */, char* node_names, int64_t names_len, char* victim_uids, int64_t uids_len,
                                          int64_t* needed2 /* [2] or NULL */);
int32_t ykhost_preempt_gang_live_by_key(ykhost_t* h, const char* allocation_key, int32_t want, int64_t* out_cells /* [want][8] */,
                                        int64_t* out_summary /* [8] */, char* node_names, int64_t names_len, char* victim_uids, int64_t uids_len,
                                        int64_t* needed2 /* [2] or NULL */);
int32_t ykhost_victim_effects(ykhost_t* h, int32_t* dims /* [5] */, int32_t* class_col, int32_t* cum);

/* Engine calls that came back YKPRED_E_DEVICE / YKPRED_E_NOMEM so far (failed allocation, lost device). Each one marks the whole
 * device state stale: the failing call returns its error (Predicates() < 0: the Go manager routes the ask to the CPU predicate
 * manager — SURVEY.md §5, "must degrade, never fail scheduling"), the mirror stays intact, and the next ykhost_sync /
 * ykhost_evaluate re-uploads every table and runs a full pass. */
int64_t ykhost_device_errors(ykhost_t* h);

/* victims: UIDs of pods assigned to the node (NULL / unknown UID = nil victim). Returns the index or -1. */
int32_t ykhost_preemption_predicates(ykhost_t* h, int32_t pod, int32_t node, const char* const* victim_uids, int32_t num_victims,
                                     int32_t start_index);

/* Batched form: query q = (pods[q], nodes[q], victim UIDs victim_uids[victim_off[q] .. victim_off[q+1]), start_index[q]). */
int32_t ykhost_preemption_predicates_batch(ykhost_t* h, int32_t num_queries, const int32_t* pods, const int32_t* nodes,
                                           const int32_t* victim_off, const char* const* victim_uids, const int32_t* start_index,
                                           int32_t* out_index);

/* Individual routing: 1 = pending pod #pod is evaluated on the device, 0 = it is routed to the CPU predicate manager
 * (`reason` says why). ykhost_routing_stats: out[0] = asks marked unsupported at the last encode, out[1] = Predicates() calls
 * answered YKHOST_E_UNSUPPORTED so far (what the Go side exports as its fallback counter), out[2] = new asks whose selector
 * requirements were added to the dictionaries in place (one label-word column uploaded, nothing re-encoded). */
int32_t ykhost_ask_supported(ykhost_t* h, int32_t pod, char* reason, int32_t reason_len);
int32_t ykhost_routing_stats(ykhost_t* h, int64_t* out3);

/* request vector of pending pod #pod as JSON {"cpu": milli, "memory": bytes, ...} */
int32_t ykhost_pod_request_json(ykhost_t* h, int32_t pod, char* out, int32_t len);

/* encoder statistics: out[0]=R, [1]=KT, [2]=W, [3]=#taints, [4]=#requirements, [5]=#templates, [6]=#specs, [7]=last encode µs */
int32_t ykhost_stats(const ykhost_t* h, int64_t* out8);

#ifdef __cplusplus
}
#endif
#endif /* YKHOST_H_ */

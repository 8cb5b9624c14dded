/*
 * ykpred.h — C ABI of libykpred.so, the MI355X (gfx950) batched predicate engine.
 *
 * This is the drop-in boundary for the yunikorn-k8shim predicate hot path. A Go
 * `gpuPredicateManager` implementing the reference's
 *     type PredicateManager interface { EventsToRegister; Predicates; PreemptionPredicates }
 *     (/root/reference/pkg/plugin/predicates/predicate_manager.go:47-55)
 * binds these entry points through cgo (binding sketch: INTEGRATION.md) and is installed at the one
 * construction site /root/reference/pkg/cache/context.go:130; pkg/shim and the scheduler-interface
 * callback (/root/reference/pkg/cache/scheduler_callback.go:203-216) stay untouched.
 *
 * Conventions
 *   - plain C types, caller-owned flat arrays (structure-of-arrays), copied during the call: the library
 *     never retains a caller pointer (cgo rule: no Go pointers kept after return);
 *   - every function returns YKPRED_OK (0) or a negative YKPRED_E_* code; ykpred_last_error() gives text;
 *   - no CPU fallback exists in this library: if the HIP device is missing, create() fails;
 *   - evals may run concurrently with queries only if the caller serialises them against uploads — the same
 *     contract the reference gets from Context.lock / SchedulerCache.lock (context.go:697,709).
 *
 * What replaces what
 *   ykpred_set_nodes / ykpred_update_node   the per-call reads of framework.NodeInfo{Allocatable, Requested,
 *                                           Pods, Node().Spec/Labels} (scheduler_cache.go:84-145, a14 in SURVEY §8a)
 *   ykpred_set_specs / ykpred_set_pods      the pod side of every Predicates(pod, ...) call: the request vector of
 *                                           pkg/common/resource.go:56-109 and the toleration / node-selector ASTs,
 *                                           pre-encoded once per pod update instead of once per (pod,node) pair
 *   ykpred_eval                             the P×N loop of Predicates() calls: runPreFilterPlugins +
 *                                           runFilterPlugins (predicate_manager.go:221-283) for every pending
 *                                           ask against every node of one snapshot
 *   ykpred_query                            one Predicates() result: fit + first failing plugin (:206-219)
 *   ykpred_preemption                       PreemptionPredicates (:141-179)
 */
#ifndef YKPRED_H_
#define YKPRED_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* (ykpred_preempt_explain + ykpred_preempt_explain_pod + YKPRED_PREEMPT_EXPLAIN_CELLS arrived WITHIN version 4 too:
 *    dlsym("ykpred_preempt_explain"))
 * (ykpred_preempt_round_live + ykpred_histogram_dims + ykpred_set_victim_effects + ykpred_update_victim_effects_node + ykpred_victim_effects_t arrived WITHIN
 *    version 4 too: dlsym("ykpred_preempt_round_live"))
 * (ykpred_preempt_round + YKPRED_PREEMPT_ROUND_CELLS arrived WITHIN version 4 too: dlsym("ykpred_preempt_round"))
 * (ykpred_preempt_victims + ykpred_preempt_victims_pod + ykpred_set_victims + ykpred_update_victims_node + YKPRED_VICTIM_CELLS arrived
 *    WITHIN version 4 too: dlsym("ykpred_preempt_victims"))
 * (ykpred_preempt_headroom + ykpred_preempt_headroom_pod + YKPRED_PREEMPT_HEADROOM_CELLS arrived WITHIN version 4 too:
 *    dlsym("ykpred_preempt_headroom"))
 * (ykpred_preempt_reach + ykpred_preempt_reach_pod + ykpred_set_reclaim + ykpred_update_reclaim_node + YKPRED_REACH_CELLS arrived
 *    WITHIN version 4 too: dlsym("ykpred_preempt_reach"))
 * (ykpred_headroom_affinity + ykpred_headroom_affinity_pod + YKPRED_AFFINITY_HEADROOM_CELLS arrived WITHIN version 4 too:
 *    dlsym("ykpred_headroom_affinity"))
 * (ykpred_headroom_spread + ykpred_headroom_spread_pod + YKPRED_SPREAD_HEADROOM_CELLS arrived WITHIN version 4 too:
 *    dlsym("ykpred_headroom_spread"))
 * (ykpred_headroom_groups + YKPRED_GROUP_CELLS / YKPRED_GROUP_SUMMARY arrived WITHIN version 4 too: dlsym("ykpred_headroom_groups"))
 * (ykpred_headroom + ykpred_headroom_pod + YKPRED_HEADROOM_CELLS arrived WITHIN version 4 as well, detected the same way:
 *    dlsym("ykpred_headroom"))
 * (ykpred_explain + YKPRED_EXPLAIN_BINS arrived WITHIN version 4, without a bump: a host that needs the call detects it by the
 *    exported symbol — dlsym("ykpred_explain") — not by the version number)
 * 4: ykpred_set_spec_effects + ykpred_spec_effects_t, ykpred_comm_info (round 5 added them without a bump: a host built against the
 *    header could not tell an older library apart), ykpred_layout_t.sweep_rows / index_rows_walked / run_rows / fused_rows, ykpred_get_round_info
 * 3: ykpred_eval_args_t.bitmap_rows (a caller-owned bitmap states its size), ykpred_peek_row (the resident
 *    answer served to single Predicates() callbacks), ykpred_eval_nodes is collective on a sharded engine with topology signatures
 * 2: bitmap rows addressed through ykpred_layout_t.row_of_pod, ykpred_nodes_t.name_rank, per-ask unsupported flag, communicator /
 *    gather / exchange entry points (version 1 = the round-1 ABI: rows in ask order, no collectives) */
#define YKPRED_ABI_VERSION 4

/* status codes */
#define YKPRED_OK 0
#define YKPRED_E_INVALID (-1)   /* bad argument / inconsistent sizes */
#define YKPRED_E_DEVICE (-2)    /* HIP runtime error (message in ykpred_last_error) */
#define YKPRED_E_NOMEM (-3)     /* device or host allocation failed */
#define YKPRED_E_STATE (-4)     /* call sequence error (e.g. eval before nodes/specs/pods were uploaded) */
#define YKPRED_E_UNSUPPORTED (-5)

/* Plugin bits. Bit order = Filter order of predicate_manager.go:339-352. */
#define YKPRED_PLUGIN_NODE_UNSCHEDULABLE (1u << 0)
#define YKPRED_PLUGIN_NODE_NAME (1u << 1)
#define YKPRED_PLUGIN_TAINT_TOLERATION (1u << 2)
#define YKPRED_PLUGIN_NODE_AFFINITY (1u << 3)
#define YKPRED_PLUGIN_NODE_PORTS (1u << 4)
#define YKPRED_PLUGIN_NODE_RESOURCES_FIT (1u << 5)
#define YKPRED_PLUGIN_POD_TOPOLOGY_SPREAD (1u << 6)
#define YKPRED_PLUGIN_INTER_POD_AFFINITY (1u << 7)
#define YKPRED_PLUGIN_ALL 0xffu

/* "failing plugin" codes returned by ykpred_query (0 = "" — a PreFilter plugin rejected the pod, :236-238) */
#define YKPRED_CODE_NONE 0
#define YKPRED_CODE_NODE_UNSCHEDULABLE 1
#define YKPRED_CODE_NODE_NAME 2
#define YKPRED_CODE_TAINT_TOLERATION 3
#define YKPRED_CODE_NODE_AFFINITY 4
#define YKPRED_CODE_NODE_PORTS 5
#define YKPRED_CODE_NODE_RESOURCES_FIT 6
#define YKPRED_CODE_POD_TOPOLOGY_SPREAD 7
#define YKPRED_CODE_INTER_POD_AFFINITY 8
#define YKPRED_CODE_UNSUPPORTED 255 /* the ask's spec carries YKPRED_SPEC_UNSUPPORTED: not evaluated, route it to the CPU manager */

/* reason bits returned by ykpred_query next to the plugin code (the host composes the status message) */
#define YKPRED_REASON_TOO_MANY_PODS (1u << 0)
#define YKPRED_REASON_PREFILTER_NODE_NOT_ELIGIBLE (1u << 1)
#define YKPRED_REASON_PREFILTER_REJECTED (1u << 2)
#define YKPRED_REASON_MISSING_TOPOLOGY_LABEL (1u << 3)
#define YKPRED_REASON_RESOURCE_SHIFT 8 /* bit (8+r) set: insufficient resource dimension r */

/* node flags */
#define YKPRED_NODE_UNSCHEDULABLE (1u << 0)

/* spec flags */
#define YKPRED_SPEC_TOLERATES_UNSCHEDULABLE (1u << 0) /* tolerates node.kubernetes.io/unschedulable:NoSchedule */
#define YKPRED_SPEC_AFFINITY_SKIP (1u << 1)           /* NodeAffinity.PreFilter returns Skip (no selector, no required affinity) */
#define YKPRED_SPEC_PREFILTER_REJECT (1u << 2)        /* NodeAffinity.PreFilter: conflicting metadata.name terms */
#define YKPRED_SPEC_PREFILTER_NAMES (1u << 3)         /* NodeAffinity.PreFilter returned a NodeNames set (pre_terms) */
#define YKPRED_SPEC_UNSUPPORTED (1u << 4)             /* the host could not encode this ask (volumes, DRA claims, dictionary limits ...):
                                                         its bitmap row is all zero, its count 0, its decision -1 and every query
                                                         answers YKPRED_CODE_UNSUPPORTED, whatever the plugin lists — the host
                                                         routes exactly these asks to the CPU predicate manager */

/* special values for pods.node_name_index */
#define YKPRED_NO_NODE_NAME (-1)      /* pod.Spec.NodeName == "" */
#define YKPRED_UNKNOWN_NODE_NAME (-2) /* names a node that is not in the table: matches no node */

typedef struct ykpred_engine ykpred_engine_t;

typedef struct ykpred_config {
  int32_t abi_version;      /* YKPRED_ABI_VERSION */
  int32_t device;           /* HIP device ordinal */
  int32_t num_resources;    /* R >= 3: 0 = cpu (milli), 1 = memory, 2 = ephemeral-storage, 3.. = scalar resources */
  int32_t taint_words;      /* KT >= 1: 64-bit words of the taint dictionary */
  int32_t label_words;      /* W  >= 1: 64-bit words of the node-selector requirement dictionary */
  int32_t topology_keys;    /* KD >= 0: topology keys used by hard spread constraints */
  int32_t selector_classes; /* KS >= 0: distinct (namespace, labelSelector) classes of spread constraints */
  int32_t port_words;       /* KP >= 0: 64-bit words of the host-port dictionary (NodePorts) */
  int32_t reserved[8];      /* [0..7]: engine tunables for experiments, 0 = defaults; [3] == 1 replays a repeated
                               ykpred_eval as a hipGraph (opt-in: measured equal to plain launches); [4] = number of distinct
                               request values per resource dimension from which the sorted-walk plane kernels are used (256);
                               [5] = average members per combine chunk below which the wave-per-chunk combine runs (16, -1 never);
                               [6] = band height of the zone-A row layout in windows (4..256, multiple of 4; 0 = chosen from the row
                               length so that classes of ~100 asks still get band rows; -1 = no band layout); [7] unused.
                               The tests force paths through the environment instead: YKPRED_TUNE="walk_rows=1,sig_wpl=2,..." */
} ykpred_config_t;

/* Node table, structure-of-arrays. Arrays documented [A][count] are A consecutive runs of `count` values. */
typedef struct ykpred_nodes {
  int32_t count;
  const int64_t* allocatable;    /* [R][count]   NodeInfo.Allocatable */
  const int64_t* requested;      /* [R][count]   NodeInfo.Requested (assumed pods included) */
  const int32_t* allowed_pods;   /* [count]      Allocatable.AllowedPodNumber */
  const int32_t* pod_count;      /* [count]      len(NodeInfo.Pods) */
  const uint32_t* flags;         /* [count]      YKPRED_NODE_* */
  const uint64_t* taint_bits;    /* [KT][count]  bit t: node carries dictionary taint t (NoSchedule/NoExecute only) */
  const uint64_t* label_bits;    /* [W][count]   bit q: node satisfies dictionary requirement q */
  const int32_t* domain_id;      /* [KD][count]  id of the node's value for topology key k, -1 = label missing */
  const int32_t* selector_count; /* [KS][count]  # pods on the node matching selector class s */
  const int32_t* domain_sizes;   /* [KD]         number of distinct values (domain ids 0..size-1) of topology key k */
  const uint64_t* port_bits;     /* [KP][count]  bit k: some pod on the node uses a host port that conflicts with dictionary
                                                 port k (HostPortInfo.CheckConflict: same protocol+port, equal or wildcard IP) */
  const int32_t* name_rank;      /* [count]      position of the node's NodeID in lexicographic order: the tie-break of the
                                                 bin-pack order between nodes of equal score (yunikorn-core sorts by score,
                                                 then node id). NULL = ties by node index. In a node-sharded cluster the
                                                 shards are ranges of a name-sorted node list, in any insertion order
                                                 inside a shard: between shards the tie-break is the shard (lower rank
                                                 first), inside one this rank — together the cluster's NodeID order. */
} ykpred_nodes_t;

/* One topology constraint of a pod spec: a hard (DoNotSchedule) topology spread constraint, or one InterPodAffinity
 * rule. All kinds share the mechanics "per-node match counts (selector_count) → histogram per topology domain → test of
 * the candidate node's domain"; a spec's PodTopologySpread constraints must precede its InterPodAffinity ones. */
typedef struct ykpred_spread {
  int32_t topology_key;   /* index into domain_id[KD] */
  int32_t selector_class; /* index into selector_count[KS]; -1 = counts nothing (nil / empty selector) */
  int32_t max_skew;       /* SPREAD only */
  int32_t min_domains;    /* SPREAD only; nil => 1 */
  int32_t self_match;     /* SPREAD: the pod's labels match the selector. POD_AFFINITY: the pod matches ALL its own
                             affinity terms (same value on every affinity term of the spec) */
  uint32_t flags;         /* SPREAD only. bit0: nodeAffinityPolicy == Honor, bit1: nodeTaintsPolicy == Honor */
  int32_t kind;           /* YKPRED_CONSTRAINT_* */
  int32_t reserved;
} ykpred_spread_t;
#define YKPRED_SPREAD_HONOR_AFFINITY (1u << 0)
#define YKPRED_SPREAD_HONOR_TAINTS (1u << 1)
#define YKPRED_CONSTRAINT_SPREAD 0
#define YKPRED_CONSTRAINT_POD_AFFINITY 1          /* selector_class counts pods matching ALL required affinity terms of the spec */
#define YKPRED_CONSTRAINT_POD_ANTI_AFFINITY 2     /* selector_class counts pods matching this required anti-affinity term */
#define YKPRED_CONSTRAINT_EXISTING_ANTI_AFFINITY 3 /* selector_class counts (pod, anti-affinity term on this key) pairs matching the spec's pod */

/* Pod specs (one per distinct pod template / task group; pods reference them by index). */
typedef struct ykpred_specs {
  int32_t count;
  const int64_t* requests;       /* [count][R]  upstream PodRequests: cpu milli, others Value() */
  const uint64_t* tolerated;     /* [count][KT] bit t: some toleration tolerates dictionary taint t */
  const uint32_t* flags;         /* [count]     YKPRED_SPEC_* */
  const int32_t* aff_term_off;   /* [count+1]   Filter DNF: spec s owns aff_terms rows [off[s], off[s+1]) */
  const uint64_t* aff_terms;     /* [n][W]      a term matches a node iff (label_bits & term) == term;
                                                no rows = matches no node; one all-zero row = matches every node */
  const int32_t* pre_term_off;   /* [count+1]   PreFilter NodeNames set as DNF (only if YKPRED_SPEC_PREFILTER_NAMES) */
  const uint64_t* pre_terms;     /* [m][W] */
  const int32_t* spread_off;     /* [count+1]   may be NULL when no spec has hard spread constraints */
  const ykpred_spread_t* spread; /* [k] */
  const uint64_t* wanted_ports;  /* [count][KP] bit k: the pod requests dictionary host port k (NodePorts); may be NULL if KP == 0 */
} ykpred_specs_t;

typedef struct ykpred_pods {
  int32_t count;
  const int32_t* spec_index;      /* [count] */
  const int32_t* node_name_index; /* [count] node index named by pod.Spec.NodeName, or YKPRED_NO_/UNKNOWN_NODE_NAME */
} ykpred_pods_t;

#define YKPRED_OUT_BITMAP (1u << 0)    /* P x N feasibility bitmap */
#define YKPRED_OUT_COUNTS (1u << 1)    /* per-pod number of feasible nodes */
#define YKPRED_OUT_DECISIONS (1u << 2) /* per-pod best feasible node under the bin-pack order (-1 = none) */
#define YKPRED_OUT_DECISION_KEYS (1u << 3) /* per-pod order key of that node (int64; INT64_MAX = none): lets shards of a
                                              node-sharded cluster pick the global best with one MIN all-reduce */
#define YKPRED_EVAL_PROFILE (1u << 8)  /* bracket every kernel with HIP events (see ykpred_last_timing) */
#define YKPRED_EVAL_DIRECT (1u << 9)   /* use the per-pair reference kernel instead of the plane/class path */
#define YKPRED_EVAL_SPREAD_COUNT_ONLY (1u << 10)   /* node-sharded clusters: only build this shard's PodTopologySpread
                                                      histograms (layout.spread_counts / spread_present) and return */
#define YKPRED_EVAL_SPREAD_COUNTS_READY (1u << 11) /* the histograms already hold the cluster-wide (all-reduced) values */
#define YKPRED_EVAL_SKIP_BITMAP (1u << 12)         /* refresh planes / counts scatter / decisions only; the bitmap and the class
                                                      counts are already current (used by ykpred_eval_nodes) */
#define YKPRED_EVAL_DIRTY_CLASSES (1u << 13)       /* internal (ykpred_eval_nodes): rewrite only the rows of classes whose topology
                                                      signature changed (flagged on the device), keep every other row */

typedef struct ykpred_eval_args {
  uint32_t prefilter_plugins; /* enabled PreFilter plugins (YKPRED_PLUGIN_* bits) */
  uint32_t filter_plugins;    /* enabled Filter plugins */
  uint32_t options;           /* YKPRED_OUT_* | YKPRED_EVAL_* */
  uint32_t bitmap_rows;       /* caller-owned bitmap: the physical rows it holds (row_stride words each). The engine never writes
                                 a row >= bitmap_rows: an evaluation or ask-table patch that would need one fails with
                                 YKPRED_E_INVALID / invalidates the evaluation instead. 0 = ykpred_set_row_capacity rows (one
                                 of the two must be given with a caller-owned bitmap) */
  void* bitmap;               /* optional caller-owned DEVICE buffer of bitmap_rows x row_stride x 8 bytes; NULL = engine-owned */
  void* stream;               /* hipStream_t to launch on; NULL = the engine's own stream */
  void* counts;               /* optional caller-owned DEVICE int32[P]; NULL = engine-owned */
  void* decisions;            /* optional caller-owned DEVICE int32[P]; NULL = engine-owned */
  void* decision_keys;        /* optional caller-owned DEVICE int64[P]; NULL = engine-owned */
} ykpred_eval_args_t;

typedef struct ykpred_layout {
  int32_t num_nodes;  /* N */
  int32_t num_pods;   /* P */
  int32_t num_specs;
  int32_t num_classes;
  int32_t row_words;   /* ceil(N/64): meaningful 64-bit words per bitmap row */
  int32_t row_stride;  /* words between consecutive rows (>= row_words, multiple of 16 = 128 B; padding words are 0) */
  int32_t num_chunks;
  int32_t plane_rows;  /* total signature planes evaluated per eval */
  uint64_t bitmap_bytes;
  void* bitmap;        /* device pointer of the last evaluated bitmap; rows are addressed through row_of_pod (below) */
  void* counts;        /* device int32[P] */
  void* decisions;     /* device int32[P] */
  void* decision_keys; /* device int64[P] */
  void* spread_counts;  /* device int32[spread_cells]: matching pods per (spread constraint, topology domain) — SUM across shards */
  void* spread_present; /* device int32[spread_cells]: 1 = an eligible node carries the domain — MAX across shards */
  int64_t spread_cells;
  int32_t num_rows;     /* physical rows of the bitmap (>= num_pods: rows are laid out for the writer and never reused between two
                           class builds); bitmap_bytes = num_rows * row_stride * 8 — what a caller-owned bitmap must hold */
  int32_t band_rows;    /* rows [0, band_rows) are written by the band writer (k_expand_bands), the rest class by class (k_combine) */
  void* row_of_pod;     /* device int32[P]: the bitmap row of pod p. Bit (n & 63) of word [row_of_pod[p] * row_stride + (n >> 6)]
                           says whether pod p fits node n */
  int32_t index_rows;   /* of plane_rows: request-value rows of many-valued resource dimensions, kept as INDEX rows (one byte per
                           64-node word instead of an 8-byte plane word) */
  int32_t band_steps;   /* band height (windows) the current row layout was built with */
  int32_t sweep_rows;   /* rows of zone B laid out as RUNS of one signature in ascending order of a many-valued request dimension:
                           a full pass writes them with k_sweep_rows (a row = its predecessor minus the nodes the larger value loses) */
  int32_t index_rows_walked; /* of index_rows: the ones a full pass still materialises (k_dim_walk) — the sweep runs read none */
  int32_t run_rows;     /* rows of zone B whose classes (no index row, staged request-value rows) are written run by run: k_class_runs */
  int32_t fused_rows;   /* rows of zone B whose classes no run kernel takes and whose rows are plain plane rows: written from records resolved
                           at class-build time (k_fused_rows) */
} ykpred_layout_t;

#define YKPRED_MAX_TIMED_KERNELS 24
typedef struct ykpred_timing {
  int32_t num_kernels;
  float total_ms;                         /* first launch to last completion, device time */
  float kernel_ms[YKPRED_MAX_TIMED_KERNELS];
  const char* kernel_name[YKPRED_MAX_TIMED_KERNELS];
} ykpred_timing_t;

/* lifecycle */
int32_t ykpred_create(const ykpred_config_t* cfg, ykpred_engine_t** out);
void ykpred_destroy(ykpred_engine_t* e);
const char* ykpred_last_error(const ykpred_engine_t* e); /* e may be NULL: error of the last failed create() */
int32_t ykpred_abi_version(void);

/* state upload (externally serialised against evals) */
int32_t ykpred_set_nodes(ykpred_engine_t* e, const ykpred_nodes_t* nodes);
int32_t ykpred_update_node(ykpred_engine_t* e, int32_t index, const ykpred_nodes_t* one_node); /* count must be 1 */
/* Dictionary growth without a re-upload: replaces ONE 64-bit word column of label_bits ([count] values, one per node) — how a
 * requirement that no spec used before gets its bit. Bits that no uploaded spec references may change freely: the last
 * evaluation stays valid. */
int32_t ykpred_update_label_word(ykpred_engine_t* e, int32_t word, const uint64_t* column /* [N] */);
/* A table whose first specs are byte-identical to the previous one (new specs appended) keeps the engine's pod classes and
 * the last evaluation valid, so that a new pod template is followed by ykpred_update_pods / ykpred_eval_pods, not by a full
 * pass (unless the new specs bring a new topology-constraint signature). */
int32_t ykpred_set_specs(ykpred_engine_t* e, const ykpred_specs_t* specs);
int32_t ykpred_set_pods(ykpred_engine_t* e, const ykpred_pods_t* pods);

/* evaluation of every pending pod against every node of the uploaded snapshot */
int32_t ykpred_eval(ykpred_engine_t* e, const ykpred_eval_args_t* args);
/* Incremental form for the sequential scheduling loop (AssumePod / ForgetPod / UpdateNode between two asks,
 * /root/reference/pkg/cache/context.go:828-898): after ykpred_update_node on `num_nodes` nodes, re-evaluates ONLY those
 * node columns of the bitmap produced by the last ykpred_eval (same plugin lists, same output buffers) and patches the
 * feasible counts; decisions are recomputed when YKPRED_OUT_DECISIONS is set. With PodTopologySpread / InterPodAffinity
 * signatures active the histograms are rebuilt (they couple all nodes), the signatures whose PreFilter state moved are
 * found on the device, and the classes that use them get their WHOLE rows rewritten — all other classes still only the
 * touched columns. YKPRED_E_STATE if there is no matching previous evaluation. On a node-sharded engine (communicator attached)
 * with topology signatures the call is COLLECTIVE: every shard enters it — with its own, possibly empty, node list — and
 * performs exactly the histogram exchange of a full ykpred_eval (SUM of matches, MAX of "domain present"), so a shard may
 * answer the same step with ykpred_eval instead. Hosts that move the histograms themselves split the call like ykpred_eval:
 * YKPRED_EVAL_SPREAD_COUNT_ONLY (rebuild this shard's histograms, return), then YKPRED_EVAL_SPREAD_COUNTS_READY. */
int32_t ykpred_eval_nodes(ykpred_engine_t* e, const ykpred_eval_args_t* args, int32_t num_nodes, const int32_t* node_index);
/* Row-level maintenance of the ask table (SchedulerCache.UpdatePod for a new / changed / finished ask,
 * /root/reference/pkg/cache/external/scheduler_cache.go:303-388) without re-uploading it: the table gets `num_pods_after`
 * rows (rows beyond it are dropped, every appended row must be listed) and the `count` listed rows (each at most once) take
 * new (spec, nodeName) values. The engine moves those rows between pod classes in O(count); their bitmap rows are stale
 * until ykpred_eval_pods (or a full ykpred_eval) has run. The specs must already be uploaded. */
int32_t ykpred_update_pods(ykpred_engine_t* e, int32_t num_pods_after, int32_t count, const int32_t* rows, const int32_t* spec_index,
                           const int32_t* node_name_index);
/* Re-evaluates ONLY the listed bitmap rows (per pair, against every node) into the bitmap of the last ykpred_eval (same
 * plugin lists, same output buffers; engine-owned outputs grow with the table, caller-owned ones must already hold
 * layout.num_pods rows), with their feasible counts and — YKPRED_OUT_DECISIONS / _KEYS — their decisions.
 * YKPRED_E_STATE if there is no matching previous evaluation, or decisions are requested while the bin-pack order of
 * the last evaluation is stale (a node changed since). */
int32_t ykpred_eval_pods(ykpred_engine_t* e, const ykpred_eval_args_t* args, int32_t num_rows, const int32_t* rows);
int32_t ykpred_synchronize(ykpred_engine_t* e);
int32_t ykpred_get_layout(const ykpred_engine_t* e, ykpred_layout_t* out);
int32_t ykpred_last_timing(const ykpred_engine_t* e, ykpred_timing_t* out);
/* Engine counters since create: out[0] full evaluations, [1] ykpred_eval_nodes calls, [2] ykpred_eval_pods calls, [3] query calls,
 * [4] bitmap gathers, [5] table uploads / patches. Every upload / eval / gather entry point is also bracketed by a roctx
 * range ("ykpred:eval", "ykpred:upload_nodes", "ykpred:gather_bitmap" ...) when the process runs under a profiler that has
 * the marker library mapped, or with YKPRED_ROCTX=1. */
int32_t ykpred_get_counters(const ykpred_engine_t* e, int64_t* out6);

/* readback (device -> caller host buffers); each implies a synchronize */
int32_t ykpred_read_bitmap(ykpred_engine_t* e, int32_t first_pod, int32_t num_pods, uint64_t* out /* [num_pods][row_words] */);
int32_t ykpred_read_counts(ykpred_engine_t* e, int32_t* out /* [P] */);
int32_t ykpred_read_decisions(ykpred_engine_t* e, int32_t* out /* [P] */);
int32_t ykpred_read_scores(ykpred_engine_t* e, double* out /* [N] bin-pack score per node */);
int32_t ykpred_bitmap_checksum(ykpred_engine_t* e, uint64_t* out); /* order-independent hash of (pod,word,value) */
/* Parity support for bitmaps too large to read back (50k x 1M = 6.27 GB): the rows of the listed pods, densely; the pod →
 * class map with one representative pod per class (-1 = class without live member); and the number of bitmap words that
 * differ between a pod's row and the row of its class's representative, plus non-zero padding words. With these a checker
 * evaluates ONE pod per class against every node on the CPU and still covers every (pod, node) pair of the bitmap. */
int32_t ykpred_read_rows(ykpred_engine_t* e, int32_t n, const int32_t* pod_index, uint64_t* out /* [n][row_words] */);
int32_t ykpred_read_row_map(ykpred_engine_t* e, int32_t* out /* [P]: layout.row_of_pod on the host */);
int32_t ykpred_read_pod_classes(ykpred_engine_t* e, int32_t* pod_class /* [P] or NULL */, int32_t* class_rep /* [num_classes] or NULL */);
int32_t ykpred_check_class_rows(ykpred_engine_t* e, uint64_t* bad_words);

/* CONFLICT-RESOLVED decisions: the sequential loop yunikorn-core drives through the shim. For asks[0], asks[1], ... in this
 * order: the first node of the bin-pack order that passes Predicates() under the state the EARLIER asks of the round left
 * behind (AsyncRMCallback.Predicates, /root/reference/pkg/cache/scheduler_callback.go:203-205 → Context.IsPodFitNode,
 * context.go:696-716), then AssumePod (context.go:828-885 → SchedulerCache.AssumePod, scheduler_cache.go:443-461 →
 * NodeInfo.AddPod): the node's Requested grows by the ask's request vector, len(Pods) by one, its bin-pack score moves.
 * out_nodes[i] = node index or -1 (no node fits; nothing is assumed for that ask). The engine's TABLES ARE NOT CHANGED — the
 * round runs on a scratch copy of the node columns; the caller applies the allocations the core accepts through the cache
 * hooks (ykhost_assume_pod → ykpred_update_node) as it does for any AssumePod.
 * Needs a current evaluation WITH decisions of the same plugin lists (YKPRED_E_STATE otherwise). YKPRED_E_UNSUPPORTED — decide ask by
 * ask instead — when something other than node resources couples the asks of the round (active PodTopologySpread /
 * InterPodAffinity signatures, an ask that requests a host port) while the specs' effects (ykpred_set_spec_effects, below) are not
 * uploaded for the current spec table.
 * ONE GPU, two forms with identical decisions. SEQUENTIAL: one workgroup runs the loop (k_allocate_round; the asks are a dependency
 * chain, the parallelism is inside an ask) — a run of asks of one spec that lands on one node is decided by arithmetic (millions of
 * asks per second), every other ask costs ~10 us. BATCHED: the asks of a batch are proposed in parallel against one frozen state
 * (k_round_propose: a workgroup per ask, its 8 best feasible nodes with the columns their keys are made of), every ask is evaluated
 * against every node the batch proposed (k_round_cross: a bit per pair), the host replays the loop over the batch exactly — an
 * accepted node by its bit + NodeResourcesFit on the exchanged columns, a candidate that is full by the next entry of the ask's
 * list — and the accepted pods are assumed node by node: 100 k -> 570 k asks/s on a 20 000-ask round of configs[2]. Chosen per round
 * (YKPRED_TUNE round_batched: -1 = by the list, the default; 0 / 1 = never / always): batched for rounds of 512 asks and more
 * without live topology constraints whose mean run of one spec is shorter than four asks. ykpred_get_round_info counts both.
 * NODE-SHARDED engines (communicator attached, world > 1): the call is COLLECTIVE — every rank passes the same asks in the same
 * order — and out_nodes holds GLOBAL node indices (the winner's shard offset + its index there), identical on every rank. The
 * round always runs in batches: proposals and pair bits of a batch in ONE all-gather, the same replay on every rank, the owners
 * assume (engine.hip has the rule and its proof sketch). Equal keys across shards are ordered by global node index, as in
 * ykpred_exchange_decisions. Before the first batch the ranks agree on status, ask count and a hash of the ask list (a rank that
 * cannot run the round makes every rank return the same error). With active topology signatures the histograms are cluster-wide
 * state on every shard: the owner of an accepted node records what its assume added (constraint, domain, count), a second
 * all-gather of the batch hands the records to the other shards, and a batch ends in front of the first ask whose topology signature
 * counts a selector class an accepted pod of the batch added to (its verdicts may have turned from fail to fit anywhere).
 * YKPRED_E_UNSUPPORTED when one pod moves more than 10 histogram cells (every rank sees the same record and stops). */
int32_t ykpred_allocate_round(ykpred_engine_t* e, uint32_t prefilter_plugins, uint32_t filter_plugins, int32_t n_asks,
                              const int32_t* asks /* host, [n_asks] ask indices in decision order */, int32_t* out_nodes /* host, [n_asks] */);
/* How the rounds so far were decided: out[0] rounds run in batches, [1] their asks, [2] their batches, [3] collective exchanges of
 * sharded rounds (proposals + histogram deltas), [4] rounds run by the sequential kernel, [5] their asks. */
int32_t ykpred_get_round_info(const ykpred_engine_t* e, int64_t* out6);
/* What NodeInfo.AddPod (behind SchedulerCache.AssumePod, /root/reference/pkg/cache/external/scheduler_cache.go:443-461) adds to a
 * node BESIDES the pod's request vector and len(Pods) += 1, per pod spec — the part of the upstream NodeInfo the Filters of
 * predicate_manager.go:339-352 read again for the NEXT ask: UsedPorts (NodePorts), and the pod itself in Pods / PodsWithAffinity /
 * PodsWithRequiredAntiAffinity, which this ABI encodes as the per-node match counts selector_count[KS][N] (PodTopologySpread's
 * countPodsMatchSelector, InterPodAffinity's topologyToMatchedTermCount). A pod's contribution to a count column is a function of
 * (column, pod template) alone, so the host states it once per spec:
 *   contrib_*      spec s adds contrib_count[k] to column contrib_class[k] of the node it lands on, k in [contrib_off[s], contrib_off[s+1])
 *   occupied_ports [count][KP] bit k: once a pod of the spec is on a node, the node's port_bits gain bit k (HostPortInfo.CheckConflict of
 *                  the pod's host ports against dictionary port k)
 * With the effects of the CURRENT spec table uploaded (ykpred_set_specs drops them), ykpred_allocate_round keeps the topology
 * histograms and the port words of its scratch state current ask by ask on the device, and active PodTopologySpread /
 * InterPodAffinity signatures or host-port asks no longer make it return YKPRED_E_UNSUPPORTED. The shards' dictionaries must
 * list the selector classes of every template that can be ASSUMED during a round, not only of the pods already on nodes (the
 * host encoder does: encoder.h, existing_anti_templates_). */
typedef struct ykpred_spec_effects {
  int32_t count;                  /* == the uploaded spec table's count */
  const int32_t* contrib_off;     /* [count+1]; NULL = no spec adds to any count column */
  const int32_t* contrib_class;   /* [contrib_off[count]] column of selector_count, 0 <= class < KS */
  const int32_t* contrib_count;   /* [contrib_off[count]] > 0 */
  const uint64_t* occupied_ports; /* [count][KP]; NULL = no spec occupies a dictionary host port (or KP == 0) */
} ykpred_spec_effects_t;
int32_t ykpred_set_spec_effects(ykpred_engine_t* e, const ykpred_spec_effects_t* fx /* NULL: drop the uploaded effects */);

/* Debugging aid (no reference counterpart). With YKPRED_GUARD_PAGES=1 (2) in the environment every device block of the engine
 * ends (starts) on the last (first) byte of its mapping with an unmapped granule behind (in front of) it. The self-test proves the
 * guard is armed: it allocates a block the same way and reads `offset` bytes past its end (offset >= 0) or |offset| bytes in front
 * of its start (offset < 0). Under the guard an offset outside the block kills the process with a GPU memory access fault — that
 * IS the expected outcome (tests/test_gpu_guard.py runs it in a child process); offsets inside the block return YKPRED_OK.
 * Without the guard the call returns YKPRED_E_STATE and touches nothing. */
int32_t ykpred_guard_selftest(ykpred_engine_t* e, int32_t offset);

/* The RESIDENT answer served to single callbacks. yunikorn-core walks asks, not nodes: for one ask it calls Predicates() node
 * after node (Context.IsPodFitNode, /root/reference/pkg/cache/context.go:696-716, behind scheduler_callback.go:203-205). When
 * the last evaluation is still current, every fit bit of that ask already sits in its bitmap row: ykpred_peek_row copies that
 * ONE row (row_words words; plus the ask's feasible count and bin-pack decision when the pointers are given) to the host on a
 * copy stream that waits for the evaluation's completion event — no kernel, no device-wide synchronize. The host then serves
 * the ask's callbacks from memory and needs ykpred_query only to name the failing plugin of a pair that does not fit.
 * YKPRED_E_STATE when the bitmap does not describe the current tables and these plugin lists (a node or ask changed and was not
 * re-evaluated): the caller falls back to ykpred_query_pod. ykpred_read_order: the bin-pack order of the last evaluation that
 * produced decisions (perm[i] = node at position i) — with a row, "the first k feasible nodes in bin-pack order". */
int32_t ykpred_peek_row(ykpred_engine_t* e, int32_t pod_index, uint32_t prefilter_plugins, uint32_t filter_plugins,
                        uint64_t* out_row /* [row_words] */, int32_t* out_count /* may be NULL */, int32_t* out_decision /* may be NULL */);
int32_t ykpred_read_order(ykpred_engine_t* e, int32_t* out_perm /* [N] */);
/* Building blocks of a host-side mirror of the resident answer (libykhost keeps one): YKPRED_OK iff the bitmap of the last
 * evaluation is the answer for the current tables and these plugin lists (*num_classes = classes of that evaluation); the class
 * of an ask in the engine's current class index (host-side lookup: asks that join an existing class after the evaluation are
 * answered by that class's row); the whole answer in class-compressed form, [num_classes][row_words] on the host. */
int32_t ykpred_answer_state(ykpred_engine_t* e, uint32_t prefilter_plugins, uint32_t filter_plugins, int32_t* num_classes /* may be NULL */);
int32_t ykpred_pod_class(ykpred_engine_t* e, int32_t pod_index, int32_t* out_class);
int32_t ykpred_read_class_rows(ykpred_engine_t* e, uint64_t* out /* [num_classes][row_words] */);

/* one Predicates() answer per (pod,node) pair, evaluated on the device straight from the tables */
int32_t ykpred_query(ykpred_engine_t* e, int32_t num_pairs, const int32_t* pod_index, const int32_t* node_index,
                     uint32_t prefilter_plugins, uint32_t filter_plugins, uint8_t* fit /* [num_pairs] */,
                     uint8_t* plugin_code /* [num_pairs], may be NULL */, uint32_t* reason /* [num_pairs], may be NULL */);

/* All Predicates() answers of ONE pod in one call: out arrays have one entry per node. The core tries an ask on many nodes
 * in a row (one callback per node); the Go side fetches the ask's answers once and serves those callbacks from host memory. */
int32_t ykpred_query_pod(ykpred_engine_t* e, int32_t pod_index, uint32_t prefilter_plugins, uint32_t filter_plugins,
                         uint8_t* fit /* [N] */, uint8_t* plugin_code /* [N], may be NULL */, uint32_t* reason /* [N], may be NULL */);

/* ykpred_query_pod with one 4-byte word per node and a single device → host copy: bits 0-7 plugin code, bit 8 fit, bits 9-12
 * reason bits 0-3, bits 13.. the insufficient-resource bits (reason >> YKPRED_REASON_RESOURCE_SHIFT). */
int32_t ykpred_query_pod_packed(ykpred_engine_t* e, int32_t pod_index, uint32_t prefilter_plugins, uint32_t filter_plugins, uint32_t* out /* [N] */);

/* WHY an ask fits nowhere: for every listed ask the histogram of its Predicates() verdicts over ALL nodes of the table — what the
 * default scheduler prints as "0/5000 nodes are available: 3100 Insufficient cpu, 1200 node(s) had untolerated taint, ..." and the
 * shim can put into the Message of the PodScheduled=False / Unschedulable condition (/root/reference/pkg/cache/context.go:1272-1285).
 * A reduction on the device: 32 integers per ask come back instead of 4 bytes x N per ask (ykpred_query_pod_packed + a host loop). */
#define YKPRED_EXPLAIN_BINS 32
/* per ask, int32[32], over all nodes of the table:
 *  [0..8]   nodes whose FIRST failing plugin code is 0..8 (YKPRED_CODE_*; 0 = a PreFilter plugin rejected the pod)
 *  [9]      nodes the ask fits
 *  [10]     nodes not evaluated because the ask's spec is YKPRED_SPEC_UNSUPPORTED (then [10] == N and every other bin is 0)
 *  [11]     0
 *  [12..15] nodes whose verdict carries reason bit 0..3 (TOO_MANY_PODS, PREFILTER_NODE_NOT_ELIGIBLE, PREFILTER_REJECTED,
 *           MISSING_TOPOLOGY_LABEL)
 *  [16..23] nodes whose verdict carries "insufficient resource r", r = 0..7 (reason bit YKPRED_REASON_RESOURCE_SHIFT + r)
 *  [24..31] 0
 * Invariant: [0] + ... + [10] == N. A node with several reason bits counts in each of their bins.
 * Source of the verdicts: for every listed ask and every node the contribution is exactly what ykpred_query returns for that pair
 *   (fit, code, reason) — the kernel (k_explain) calls the same per-pair routine; no plugin rule is stated a second time.
 * Evaluation state: the call reads the TABLES, not the bitmap. It needs no current evaluation and invalidates none:
 *   ykpred_answer_state, the resident answer, the last bitmap and its checksum are the same after the call as before, and the
 *   result is current right after a ykpred_update_node with no re-evaluation. With a topology plugin in both lists it prepares
 *   the PodTopologySpread / InterPodAffinity histograms exactly as ykpred_query does.
 * The listed asks are reduced to their distinct (spec, NodeName) tasks on the host; a row is copied to every ask of its task.
 * Counts as one query (ykpred_get_counters out[3]); roctx range "ykpred:explain".
 * Errors: YKPRED_E_INVALID for a bad pointer or an index out of range, YKPRED_E_STATE before the tables are uploaded; n_asks == 0
 *   returns YKPRED_OK; a table of N == 0 nodes gives all-zero rows.
 * NODE-SHARDED engines (communicator attached, world > 1): the call is COLLECTIVE — every rank passes the same asks — and every
 *   rank returns CLUSTER-WIDE bins ([0..10] sum to the cluster's node count): the [tasks][32] table is summed with one all-reduce
 *   (int32, SUM) before the copy to the host. Before it the ranks agree on (status, n_asks, the list) with one small all-gather, as
 *   ykpred_allocate_round does: a rank that cannot run, or a differing list, makes every rank return the same error instead of
 *   blocking in the reduce. */
int32_t ykpred_explain(ykpred_engine_t* e, int32_t n_asks, const int32_t* asks /* host, ask indices, any order, repeats allowed */,
                       uint32_t prefilter_plugins, uint32_t filter_plugins, int32_t* out /* host, [n_asks][YKPRED_EXPLAIN_BINS] */);

/* HOW MANY copies of an ask the cluster can still place — the question of the gang path: the shim creates minMember identical
 * placeholders per task group and then waits out placeholderTimeoutInSeconds to learn whether the gang could be placed.
 * replicas(a, n) = the largest k such that k copies of ask a, assumed one after another on node n while no other node changes, each
 * pass Predicates() under the given plugin lists at the moment it is placed:
 *   0 when the pair does not fit (exactly ykpred_query's verdict: the kernels call the same per-pair routine); otherwise
 *   k0 = min(allowed_pods[n] - pod_count[n], min over r with request_r > 0 of floor((allocatable_r[n] - requested_r[n]) / request_r))
 *   in exact int64 arithmetic, and k = min(k0, 1) when the spec requests a dictionary host port and NodePorts is in both lists (a pod
 *   conflicts with its own (ip, protocol, port)), else k = k0. k >= 1 whenever the pair fits, and k fits an int32 (the pod slots bound it).
 * The BINDER of a node with k >= 1: the host port when it cut k0 > 1 down to 1; else the lowest r whose quotient equals k0; else the
 * pod slots. */
#define YKPRED_HEADROOM_CELLS 16
/* per ask, int64[16], over all nodes of the table:
 *  [0]      sum of replicas over the nodes
 *  [1]      nodes with replicas >= 1 (== bin [9] of ykpred_explain)
 *  [2]      max of replicas over the nodes
 *  [3]      status: 0 computed; 1 the ask's spec is YKPRED_SPEC_UNSUPPORTED (every other cell 0); 2 COUPLED
 *  [4]      nodes bound by their pod slots
 *  [5]      nodes bound by the host port
 *  [6], [7] 0
 *  [8 + r]  nodes bound by resource r, r = 0..7
 * COUPLED: the spec has a topology signature and a topology plugin is enabled (PodTopologySpread in the Filter list, or
 *   InterPodAffinity in both lists) — the verdicts read the topology histograms, so copies change each other's verdicts across nodes
 *   and no per-node quotient describes them: [0] = [2] = -1, [1] is still the single-copy fit count, the binder cells are 0.
 * Invariants at status 0: [4] + [5] + [8] + ... + [15] == [1]; [1] <= [0]; [2] <= [0].
 * The figure is an upper bound while other asks compete for the same nodes.
 * Everything else is ykpred_explain's: the listed asks are reduced to their distinct (spec, NodeName) tasks; the call reads the TABLES
 *   only, needs no evaluation and invalidates none; it prepares the topology histograms as ykpred_query does; it counts as one query;
 *   roctx range "ykpred:headroom"; YKPRED_E_INVALID for a bad pointer or an index out of range, YKPRED_E_STATE before the tables are
 *   uploaded, n_asks == 0 returns YKPRED_OK, a table of N == 0 nodes gives all-zero rows. Additionally YKPRED_E_INVALID unless
 *   NodeResourcesFit is in BOTH lists: without it nothing bounds k.
 * NODE-SHARDED engines: COLLECTIVE like ykpred_explain (the same agreement all-gather first), then one all-reduce SUM (int64) of the
 *   [tasks][16] table and one all-reduce MAX (int64) of the [tasks] maxima, which the device keeps in an array of their own: every rank
 *   returns CLUSTER-WIDE cells. */
int32_t ykpred_headroom(ykpred_engine_t* e, int32_t n_asks, const int32_t* asks /* host, ask indices, any order, repeats allowed */,
                        uint32_t prefilter_plugins, uint32_t filter_plugins, int64_t* out /* host, [n_asks][YKPRED_HEADROOM_CELLS] */);
/* replicas(pod, n) for every node n of the table (thread = node, as ykpred_query_pod): which nodes take how many copies. -1 in every
 * cell for a coupled ask, 0 everywhere for a YKPRED_SPEC_UNSUPPORTED spec. On a node-sharded engine: this shard's nodes only, nothing
 * is exchanged. Errors as ykpred_query_pod, plus YKPRED_E_INVALID unless NodeResourcesFit is in both lists. */
int32_t ykpred_headroom_pod(ykpred_engine_t* e, int32_t pod_index, uint32_t prefilter_plugins, uint32_t filter_plugins, int32_t* out /* [N] */);

/* Headroom per TOPOLOGY DOMAIN — which zone, rack or host still takes the gang. node_group[n] in {-1, 0 .. num_groups-1} partitions the
 * node table (-1: the node is in no group). For a listed ask a and a group g:
 *   copies(a, g) = sum over the nodes n of group g of replicas(a, n)      (replicas: exactly ykpred_headroom's, the same device routine)
 *   nodes(a, g)  = how many of those nodes have replicas(a, n) >= 1
 * out_groups[i][g] = { copies, nodes } for g = 0 .. num_groups-1; row [num_groups] holds the same two figures for the ungrouped nodes.
 * out_summary[i], for want[i] (NULL: every want is 1):
 *  [0]      status, exactly cell [3] of ykpred_headroom: 0 computed, 1 routed, 2 coupled
 *  [1]      groups with copies >= 1
 *  [2]      groups with copies >= want
 *  [3], [4] the group with the MOST copies and its copies; ties go to the lowest id; -1, 0 when [1] == 0
 *  [5], [6] the TIGHTEST group that still holds want — the smallest copies >= want, ties to the lowest id — and its copies; -1, 0 when
 *           [2] == 0
 *  [7]      copies on ungrouped nodes
 * Status 0, same ask and plugin lists: sum over g of copies + [7] == ykpred_headroom [0]; sum of nodes over every row == ykpred_headroom
 *   [1]; [4] <= ykpred_headroom [0]. Status 2 (coupled): every copies cell and [7] are -1, [1] = [2] = [4] = 0, [3] = -1, [5], [6] = -1, 0;
 *   the nodes cells still hold the single-copy fit count per group. Status 1 (routed): every other cell is 0.
 * Everything else is ykpred_headroom's: the asks are reduced to their distinct (spec, NodeName) tasks and the summaries to the distinct
 *   (task, want); any order, repeats allowed; the call reads the TABLES only, needs no evaluation and invalidates none; it prepares the
 *   topology histograms as ykpred_query does; it counts as one query; roctx range "ykpred:headroom_groups"; n_asks == 0 returns YKPRED_OK;
 *   a table of N == 0 nodes gives zero rows with [3] = [5] = -1. YKPRED_E_INVALID for a bad pointer, an ask index out of range,
 *   num_groups < 1, a want < 1, a group id outside [-1, num_groups) (checked on the host before any launch), or NodeResourcesFit missing
 *   from either list; YKPRED_E_STATE before the tables are uploaded. out_groups may be NULL: only the summaries come back.
 * The table of all tasks can be large (num_groups == N: one group per host), so the engine works through the tasks in table chunks under
 *   a scratch budget (256 MB; YKPRED_TUNE group_scratch_mb). Up to YKPRED_GROUP_LDS_MAX_GROUPS groups a workgroup accumulates in LDS,
 *   above it straight in the global table (YKPRED_TUNE group_lds=0 forces the latter); every add is an integer add, so both give the
 *   same cells.
 * NODE-SHARDED engines: COLLECTIVE. node_group is THIS shard's column, the group ids are cluster-wide by the caller's contract. The
 *   agreement all-gather of ykpred_headroom runs first and also covers num_groups, the wants and the scratch budget (a rank that cannot
 *   run makes every rank return the same error); then one all-reduce SUM (int64) per table chunk, and the summaries are derived AFTER it:
 *   every rank returns identical cluster-wide rows and summaries. */
#define YKPRED_GROUP_CELLS 2             /* per (ask, group) int64: [0] copies, [1] nodes */
#define YKPRED_GROUP_SUMMARY 8           /* per ask int64, see above */
#define YKPRED_GROUP_LDS_MAX_GROUPS 63   /* the largest num_groups whose per-workgroup table fits the LDS budget (32 KiB) */
int32_t ykpred_headroom_groups(ykpred_engine_t* e, int32_t n_asks, const int32_t* asks /* host, ask indices, any order, repeats allowed */,
                               const int64_t* want /* host, [n_asks], NULL = all 1 */, int32_t num_groups,
                               const int32_t* node_group /* host, [N] */, uint32_t prefilter_plugins, uint32_t filter_plugins,
                               int64_t* out_summary /* host, [n_asks][YKPRED_GROUP_SUMMARY] */,
                               int64_t* out_groups /* host, [n_asks][num_groups + 1][YKPRED_GROUP_CELLS], may be NULL */);

/* Headroom for asks with ONE hard spread constraint — the asks ykpred_headroom reports as coupled (status 2) because their verdicts read the
 * topology histograms. With PodTopologySpread in the Filter list, the LIVE constraints of an ask's topology signature are those of kind
 * SPREAD, and those of the InterPodAffinity kinds when InterPodAffinity is in both lists. The ask QUALIFIES when exactly one constraint c
 * is live, it is of kind SPREAD, PodTopologySpread is in the PreFilter list too, and every node that takes a copy and carries c's key
 * COUNTS for c (a node fails to count only when c honours a node-inclusion policy whose plugin is missing from the lists). Then, with
 * cnt[d], present[d], minv = c's histogram row as ykpred_query prepares it:
 *   cap(d)   = sum over the nodes n of domain d of replicas(a, n), replicas evaluated WITHOUT PodTopologySpread in the Filter list
 *              (otherwise exactly ykpred_headroom's, the same device routine); nodes(d) = how many of them have replicas >= 1; a node
 *              without the key takes no copy
 *   self_match != 0:  M = min over present d of cnt[d] + cap(d); floor = 0 when fewer than min_domains domains are present, else M;
 *                     copies(d) = clamp(floor + max_skew - cnt[d], 0, cap(d))
 *   self_match == 0:  floor = minv; copies(d) = cap(d) if cnt[d] - minv <= max_skew, else 0
 * which is what placing copies one after another until none fits leaves in each domain, in every placement order. All int64.
 * out[i]:
 *  [0]  sum of copies          [1]  domains with copies >= 1        [2]  most copies in one domain
 *  [3]  status: 0 computed; 1 routed (YKPRED_SPEC_UNSUPPORTED); 2 still coupled (does not qualify): [0] = [2] = -1, the rest 0;
 *       3 not coupled under these lists — ykpred_headroom answers — the rest 0
 *  [4]  sum of cap             [5]  present domains                 [6]  floor
 *  [7]  the lowest domain id with cnt + cap == M; -1 under the minDomains rule, with self_match == 0, or with no present domain
 *  [8]  domains filled to capacity (copies == cap >= 1)   [9]  domains cut by the skew (0 < copies < cap)
 *  [10] domains shut by it (cap >= 1, copies == 0)        [11] the domain with the most copies, lowest id on ties, -1 if none
 *  [12] topology key index     [13] max_skew              [14] sum of nodes           [15] 0
 * Status 0: [8] + [9] + [10] == domains with cap >= 1; [0] <= [4]; [4] <= cell [0] of ykpred_headroom called without PodTopologySpread
 *   in the Filter list, equal when every fitting node carries the key.
 * Everything else is ykpred_headroom's: distinct (spec, NodeName) tasks, any order, repeats allowed; reads the TABLES only, needs no
 *   evaluation and invalidates none; prepares the topology histograms as ykpred_query does; counts as one query; roctx range
 *   "ykpred:headroom_spread"; n_asks == 0 returns YKPRED_OK; N == 0 gives status and [12], [13] with [7] = [11] = -1. The same errors, plus
 *   YKPRED_E_INVALID unless PodTopologySpread is in the Filter list. The per-task tables are ragged (a task owns the domains of its key) and
 *   are worked through in chunks under ykpred_headroom_groups' budget (YKPRED_TUNE group_scratch_mb, group_chunk_tasks); a chunk whose
 *   tasks all have at most YKPRED_GROUP_LDS_MAX_GROUPS domains accumulates in LDS, any other straight in the global table
 *   (group_lds=0 forces the latter); integer adds, the same cells either way.
 * NODE-SHARDED engines: COLLECTIVE. The agreement all-gather of ykpred_headroom also covers the chunking knobs; one all-reduce SUM (int64)
 *   per chunk over table and flags; the copies are derived AFTER it from the (already cluster-wide) histograms: identical rows on every rank.
 * ykpred_headroom_spread_pod: the rows behind ONE ask, out[d] = { cnt, cap, nodes, copies } for the *num_domains domains of its key.
 *   YKPRED_E_UNSUPPORTED for an ask at a status other than 0; YKPRED_E_INVALID when max_domains < *num_domains (which is set). Collective on
 *   a sharded engine like the first call. */
#define YKPRED_SPREAD_HEADROOM_CELLS 16
int32_t ykpred_headroom_spread(ykpred_engine_t* e, int32_t n_asks, const int32_t* asks /* host, ask indices, any order, repeats allowed */,
                               uint32_t prefilter_plugins, uint32_t filter_plugins, int64_t* out /* host, [n_asks][YKPRED_SPREAD_HEADROOM_CELLS] */);
int32_t ykpred_headroom_spread_pod(ykpred_engine_t* e, int32_t pod_index, uint32_t prefilter_plugins, uint32_t filter_plugins, int32_t max_domains,
                                   int64_t* out /* host, [max_domains][4]: cnt, cap, nodes, copies */, int32_t* num_domains);
/* Where the one live spread constraint of an ask lives in the topology histograms: out = { status as cell [3] above (from the tables
 * alone: a non-counting fitting node is not seen here), topology key index, first cell of the constraint's row in layout.spread_counts /
 * spread_present, its number of cells (domains), max_skew, min_domains, self_match, flags (YKPRED_SPREAD_HONOR_*) }; at a status other
 * than 0 the other cells are 0. What a host needs to read the row ykpred_headroom_spread fills from. Reads the tables only; valid until
 * the spec or node tables change. YKPRED_E_INVALID for a bad pointer or index, or without PodTopologySpread in the Filter list. */
#define YKPRED_SPREAD_CONSTRAINT_CELLS 8
int32_t ykpred_headroom_spread_constraint(ykpred_engine_t* e, int32_t pod_index, uint32_t prefilter_plugins, uint32_t filter_plugins,
                                          int32_t* out /* host, [YKPRED_SPREAD_CONSTRAINT_CELLS] */);

/* Headroom for asks with required pod (anti-)affinity — the other asks ykpred_headroom reports as coupled (status 2): "one executor per
 * host" and its kin. InterPodAffinity must be in both lists; the LIVE constraints of an ask's topology signature are then those of kind
 * POD_AFFINITY, POD_ANTI_AFFINITY and EXISTING_ANTI_AFFINITY, and those of kind SPREAD when PodTopologySpread is in the Filter list.
 * With w(g) = what one assumed pod of the ask's spec adds to the selector class of constraint g (ykpred_set_spec_effects; 0 for
 * selector_class == -1), the ask QUALIFIES when no SPREAD constraint is live, at least one constraint of the other kinds is, and the
 * SELF-CONTRIBUTING anti rows (kind POD_ANTI_AFFINITY or EXISTING_ANTI_AFFINITY, w > 0) all lie on ONE topology key k*. Per domain d of
 * the task's key:
 *   cap(d)   = sum over the nodes n of d of replicas(a, n) — ykpred_headroom's routine under these lists, InterPodAffinity included: the
 *              static verdict of ykpred_query against the current histograms; nodes(d) = how many of them take a copy;
 *   cnt(d)   = sum over the live anti rows on that key of their histogram cell.
 * Nodes WITHOUT the key go to an OUTSIDE row (an anti-affinity row passes them, and a copy placed there moves no cell).
 *   mode 0, static: no self-contributing anti row; key = that of the first live row; copies(d) = cap(d).
 *   mode 1, one per domain: key = k*; copies(d) = min(cap(d), 1); the outside row keeps its cap. The first copy placed in d shuts d,
 *     no placement opens a domain: every open domain ends with exactly one copy, in every placement order.
 *   mode 2, bootstrap: a POD_AFFINITY row with self_match != 0 and w > 0 while no pod matches anywhere (the sum of minv over the
 *     affinity rows is 0). The first copy lands anywhere and pins its domain: the result depends on the order. With exactly ONE affinity
 *     row and no self-contributing anti row: status 4, copies(d) = cap(d) = what the gang gets if it starts in d. Otherwise status 2.
 * out[i]:
 *  [0]  sum of copies, the outside row included    [1]  domains with copies >= 1        [2]  most copies in one domain
 *  [3]  status: 0 computed; 1 routed (YKPRED_SPEC_UNSUPPORTED): every other cell 0; 2 still coupled (a live SPREAD constraint beside the
 *       affinity ones, self-contributing anti rows on two keys, a bootstrap that does not qualify): [0] = [2] = -1, the rest 0;
 *       3 no InterPodAffinity constraint is live — ykpred_headroom or ykpred_headroom_spread answers — the rest 0;
 *       4 bootstrap: [0] = -1, [2] and [11] = the best starting domain, every other cell as computed
 *  [4]  sum of cap over the domains                [5]  domains with cnt > 0 (blocked)   [6]  copies outside
 *  [7]  nodes outside that take a copy             [8]  domains filled (copies == cap >= 1)
 *  [9]  domains cut (0 < copies < cap)             [10] 0
 *  [11] the domain with the most copies, lowest id on ties, -1 if none                   [12] topology key index
 *  [13] mode                                       [14] sum of nodes, outside included   [15] 0
 * Status 0: [8] + [9] == domains with cap >= 1; [0] <= [4] + [6]; in mode 1 [0] == [1] + [6].
 * Everything else is ykpred_headroom_spread's: tasks, tables only, one query, chunks under group_scratch_mb / group_chunk_tasks, LDS
 *   accumulation while every task of a chunk has at most YKPRED_GROUP_LDS_MAX_GROUPS domains (group_lds=0 forces the global table),
 *   integer adds; roctx range "ykpred:headroom_affinity"; N == 0 gives status, [12], [13] with [11] = -1. The same errors, with
 *   YKPRED_E_INVALID unless InterPodAffinity AND NodeResourcesFit are in both lists, and YKPRED_E_UNSUPPORTED when the spec effects are
 *   not uploaded for the current spec table (the rule of ykpred_allocate_round).
 * NODE-SHARDED engines: COLLECTIVE. The agreement all-gather covers both of those verdicts, the knobs and the effects version: no rank
 *   exits alone. One all-reduce SUM (int64) per chunk over table and flags; bootstrap and the copies are derived AFTER it from the
 *   (already cluster-wide) histograms: identical rows on every rank.
 * ykpred_headroom_affinity_pod: the rows behind ONE ask, out[d] = { cnt, cap, nodes, copies } for the *num_domains domains of its key,
 *   out[*num_domains] = the outside row. Status 0 and 4 only, else YKPRED_E_UNSUPPORTED; YKPRED_E_INVALID when max_domains <
 *   *num_domains (which is set). Collective on a sharded engine like the first call. */
#define YKPRED_AFFINITY_HEADROOM_CELLS 16
int32_t ykpred_headroom_affinity(ykpred_engine_t* e, int32_t n_asks, const int32_t* asks /* host, ask indices, any order, repeats allowed */,
                                 uint32_t prefilter_plugins, uint32_t filter_plugins, int64_t* out /* host, [n_asks][YKPRED_AFFINITY_HEADROOM_CELLS] */);
int32_t ykpred_headroom_affinity_pod(ykpred_engine_t* e, int32_t pod_index, uint32_t prefilter_plugins, uint32_t filter_plugins, int32_t max_domains,
                                     int64_t* out /* host, [max_domains + 1][4]: cnt, cap, nodes, copies */, int32_t* num_domains);

/* Where the cells behind cnt lie in the topology histograms: out = { status as cell [3] above from the tables and effects alone (bootstrap
 * is not seen here: 0 where the call may say 4 or, for a bootstrap that does not qualify, 2), topology key index, mode (0 / 1), number
 * of domains, number of live anti rows on the key, then the first cell in layout.spread_counts of each of them (the first
 * YKPRED_AFFINITY_CONSTRAINT_ROWS; each row has as many cells as the key has domains) }; at a status other than 0 the other cells are 0.
 * Reads the tables only; valid until the spec or node tables change. YKPRED_E_INVALID for a bad pointer or index, or without
 * InterPodAffinity in both lists; YKPRED_E_UNSUPPORTED without current spec effects. */
#define YKPRED_AFFINITY_CONSTRAINT_ROWS 11
#define YKPRED_AFFINITY_CONSTRAINT_CELLS 16
int32_t ykpred_headroom_affinity_constraint(ykpred_engine_t* e, int32_t pod_index, uint32_t prefilter_plugins, uint32_t filter_plugins,
                                            int32_t* out /* host, [YKPRED_AFFINITY_CONSTRAINT_CELLS] */);

/* PreemptionPredicates (predicate_manager.go:141-179): victims are described by their request vectors, in order. */
int32_t ykpred_preemption(ykpred_engine_t* e, int32_t pod_index, int32_t node_index, int32_t num_victims,
                          const int64_t* victim_requests /* [num_victims][R]; a nil victim is an all-zero row with present=0 */,
                          const uint8_t* victim_present /* [num_victims] */, int32_t start_index,
                          uint32_t prefilter_plugins, uint32_t filter_plugins, int32_t* out_index);
/* Same, for nodes whose victims hold host ports: port_bits_after[i][KP] = the node's port_bits once victims 0..i are gone. */
int32_t ykpred_preemption_ports(ykpred_engine_t* e, int32_t pod_index, int32_t node_index, int32_t num_victims,
                                const int64_t* victim_requests, const uint8_t* victim_present, const uint64_t* port_bits_after,
                                int32_t start_index, uint32_t prefilter_plugins, uint32_t filter_plugins, int32_t* out_index);

/* Batched PreemptionPredicates: query q uses victims [victim_off[q], victim_off[q+1]) of the flattened victim arrays
 * (same per-victim meaning as above) and writes out_index[q]. One launch, one thread per query. */
int32_t ykpred_preemption_batch(ykpred_engine_t* e, int32_t num_queries, const int32_t* pod_index, const int32_t* node_index,
                                const int32_t* victim_off /* [num_queries+1] */, const int64_t* victim_requests /* [total][R] */,
                                const uint8_t* victim_present /* [total] */, const uint64_t* port_bits_after /* [total][KP] or NULL */,
                                const int32_t* start_index /* [num_queries] */, uint32_t prefilter_plugins, uint32_t filter_plugins,
                                int32_t* out_index /* [num_queries] */);

/* PREEMPTION REACH — can preemption help an ask at all, and on which nodes? — answered before any victim list exists.
 *
 * The RECLAIM TABLE is resident beside the node table and shard-local on the node axis. The caller gives ascending priority bounds
 * b[0] < ... < b[T-1], 1 <= T <= YKPRED_REACH_MAX_TIERS; a resident pod's TIER is the smallest t with priority(pod) < b[t]; a pod of
 * priority >= b[T-1], a pod that opted out of preemption and a pod on no node are in no tier. Per tier and node the table holds what
 * the node's pods of that tier give back: */
#define YKPRED_REACH_MAX_TIERS 8
typedef struct ykpred_reclaim {
  int32_t tiers;               /* T */
  const int64_t* requests;     /* [T][R][N] summed request vectors per tier, not cumulative */
  const int32_t* pods;         /* [T][N] pods of the tier on the node */
  const uint64_t* ports_after; /* [T][KP][N] the node's port_bits once tiers 0..t are gone; NULL = no victim holds a dictionary port
                                  or KP == 0 */
} ykpred_reclaim_t;
/* Uploads the table for the current node table (YKPRED_E_STATE without one). NULL drops it. A ykpred_set_nodes that changes N drops it
 * as well. No other call reads the table, and setting it invalidates no evaluation. */
int32_t ykpred_set_reclaim(ykpred_engine_t* e, const ykpred_reclaim_t* table);
/* One column of every plane, in the style of ykpred_update_node: `one` describes ONE node (N == 1 in the shapes above) with the
 * resident table's tier count. ports_after must be given exactly when the resident table has that plane. */
int32_t ykpred_update_reclaim_node(ykpred_engine_t* e, int32_t node_index, const ykpred_reclaim_t* one);

/* level(a, n): 0 when Predicates(a, n) fits as the node stands; otherwise the smallest L <= limit such that the ask fits once ALL pods
 * of tiers < L are gone from n — free resources grow by the tier's request vector, len(Pods) drops by its pod count, the port words
 * become ports_after, the PreFilter state of PodTopologySpread / InterPodAffinity stays frozen: ykpred_preemption's removal with whole
 * tiers as steps; NEVER when no such L exists or a PreFilter plugin rejects the pair. With victims = the node's pods of tiers < limit
 * in ascending tier order, level == tier(victims[i]) + 1 for i = ykpred_preemption(a, n, victims, start 0), and i == -1 <=> never.
 * The limit of an ask = the number of bounds <= its priority (0 for preemptionPolicy: Never): the caller passes it. */
#define YKPRED_REACH_CELLS 16
/* per ask, int64[16], over all nodes of the table:
 *  [0]      nodes at level 0 (== bin [9] of ykpred_explain)
 *  [1..8]   nodes at level 1..8
 *  [9]      nodes never
 *  [10]     status: 0 computed; 1 the ask's spec is YKPRED_SPEC_UNSUPPORTED (every other cell 0 except [11])
 *  [11]     the limit, echoed
 *  [12]     the lowest level >= 1 that has a node, or 0
 *  [13]     the BEST node at that level: the fewest pods in tiers < level, ties to the lowest node index (a GLOBAL index on a sharded
 *           engine); -1 when there is none
 *  [14]     that node's pod count in those tiers (saturating at 2^28 - 1)
 *  [15]     0
 * Invariant at status 0: [0] + ... + [9] == N.
 * Everything else is ykpred_explain's: the listed asks are reduced to their distinct (spec, NodeName, limit) tasks; the call reads the
 *   TABLES only, needs no evaluation and invalidates none; it prepares the topology histograms as ykpred_query does; it counts as one
 *   query; roctx range "ykpred:preempt_reach"; the same errors, plus YKPRED_E_STATE without a reclaim table and YKPRED_E_INVALID for a
 *   limit outside 0..T.
 * NODE-SHARDED engines: COLLECTIVE like ykpred_explain — the agreement all-gather first (it covers the limits), then one all-reduce SUM
 *   (int64) of the cells and one all-reduce MIN (int64) of the packed best keys: every rank returns CLUSTER-WIDE cells. */
int32_t ykpred_preempt_reach(ykpred_engine_t* e, int32_t n_asks, const int32_t* asks /* host, ask indices, any order, repeats allowed */,
                             const int32_t* limits /* host, [n_asks], 0..T */, uint32_t prefilter_plugins, uint32_t filter_plugins,
                             int64_t* out /* host, [n_asks][YKPRED_REACH_CELLS] */);
/* level(pod, n) for every node n of the table (thread = node, as ykpred_headroom_pod), -1 = never: the shortlist the caller walks for
 * the real victim selection. -1 everywhere for a YKPRED_SPEC_UNSUPPORTED spec. This shard's nodes only on a sharded engine. */
int32_t ykpred_preempt_reach_pod(ykpred_engine_t* e, int32_t pod_index, int32_t limit, uint32_t prefilter_plugins, uint32_t filter_plugins,
                                 int32_t* out /* [N] */);

/* PREEMPTION EXPLAIN — WHY removing lower-priority pods opens no node: ykpred_explain's histogram on the node states of
 * ykpred_preempt_reach, what kube-scheduler prints as "preemption: 0/5000 nodes are available: 3000 Preemption is not helpful for
 * scheduling, 1500 No preemption victims found for incoming pod, 500 Insufficient memory." 
 *
 * For an ask a with limit l and a node n (limits and tiers exactly those of ykpred_preempt_reach): level(a, n) is the reach level;
 * elig(n, l) = the node's pods in tiers < l; final(n, l) = the node with ALL pods of tiers < l gone, removed as ykpred_preempt_reach
 * removes them (free resources grow by the tier requests, len(Pods) drops, the port words become ports_after of the last non-empty
 * tier, the topology PreFilter state stays frozen); V(a, n) = the (code, reason) of Predicates(a, final(n, l)). Only NEVER nodes are
 * classified, each into exactly one class:
 *   UNRESOLVABLE  the first failing code as the node stands is neither NodePorts (5) nor NodeResourcesFit (6): no removal moves it, and
 *                 V is the verdict as the node stands
 *   NO VICTIMS    the code is 5 or 6 and elig == 0
 *   NOT ENOUGH    the code is 5 or 6 and elig > 0: every eligible pod is gone and the ask still fails */
#define YKPRED_PREEMPT_EXPLAIN_CELLS 32
/* per ask, int64[32], over all nodes of the table:
 *  [0..8]   NEVER nodes whose FIRST failing plugin code in V is 0..8
 *  [9]      nodes at level 0 (== cell [0] of ykpred_preempt_reach, bin [9] of ykpred_explain)
 *  [10]     nodes not evaluated because the ask's spec is YKPRED_SPEC_UNSUPPORTED (then [10] == N and every other count cell is 0)
 *  [11]     nodes at a level 1..limit: the nodes preemption opens (== the sum of cells [1..8] of ykpred_preempt_reach)
 *  [12..15] NOT ENOUGH nodes whose V carries reason bit 0..3
 *  [16..23] NOT ENOUGH nodes whose V carries "insufficient resource r", r = 0..7
 *  [24]     NO VICTIMS nodes
 *  [25]     UNRESOLVABLE nodes
 *  [26]     NOT ENOUGH nodes
 *  [27]     NOT ENOUGH nodes whose first failure in V is NodePorts (the held triple belongs to a pod in no eligible tier)
 *  [28]     the sum of elig over the NOT ENOUGH nodes: pods whose eviction would be wasted
 *  [29]     the limit, echoed
 *  [30]     status: 0 computed; 1 the ask's spec is YKPRED_SPEC_UNSUPPORTED
 *  [31]     0
 * Invariants at status 0: [0] + ... + [11] == N; [0] + ... + [8] == [24] + [25] + [26] == cell [9] of ykpred_preempt_reach;
 *   [27] <= [26]; a node with several reason bits counts in each of their bins. At limit 0: [26] == [27] == [28] == 0, [12..23] == 0,
 *   [0..9] are ykpred_explain's bins, [24] == its [5] + [6] and [25] == its [0..4] + [7] + [8].
 * Source of the verdicts: the kernel (k_preempt_explain) calls the per-pair routine of ykpred_query on the states of
 *   ykpred_preempt_reach's tier walk; no plugin rule and no removal rule is stated a second time.
 * Everything else is ykpred_preempt_reach's: the listed asks are reduced to their distinct (spec, NodeName, limit) tasks; the call reads
 *   the TABLES only, needs no evaluation and invalidates none; it prepares the topology histograms as ykpred_query does; it counts as
 *   one query; roctx range "ykpred:preempt_explain"; the same errors (YKPRED_E_STATE without a reclaim table, YKPRED_E_INVALID for a
 *   limit outside 0..T).
 * NODE-SHARDED engines: COLLECTIVE like ykpred_preempt_reach — the agreement all-gather first (it covers the limits), then ONE
 *   all-reduce SUM (int64) of the cells: every rank returns CLUSTER-WIDE cells. */
int32_t ykpred_preempt_explain(ykpred_engine_t* e, int32_t n_asks, const int32_t* asks /* host, ask indices, any order, repeats allowed */,
                               const int32_t* limits /* host, [n_asks], 0..T */, uint32_t prefilter_plugins, uint32_t filter_plugins,
                               int64_t* out /* host, [n_asks][YKPRED_PREEMPT_EXPLAIN_CELLS] */);
/* One word per node n of the table for ONE ask (thread = node, as ykpred_preempt_reach_pod): bits 0..20 ykpred_query_pod_packed's word
 * computed on the state the verdict comes from — the node as it stands at level 0, the state at `level` when level >= 1 (fit bit
 * set), final(n, limit) when never —, bits 24..27 the level (15 = never), bit 28 elig > 0. This shard's nodes only on a sharded engine. */
int32_t ykpred_preempt_explain_pod(ykpred_engine_t* e, int32_t pod_index, int32_t limit, uint32_t prefilter_plugins, uint32_t filter_plugins,
                                   uint32_t* out /* [N] */);

/* PREEMPTION HEADROOM — how many copies of an ask the cluster takes per preemption level: can preemption up to the ask's priority place
 * the whole gang, what is the lowest level at which it can, and how many resident pods would that cost?
 *
 * For a node n and a level L in 0..limit, state_L(n) is the node with ALL pods of tiers < L gone, exactly as ykpred_preempt_reach removes
 * them: free resources grow by the summed request vectors of those tiers, len(Pods) drops by their pod counts, the port words become
 * ports_after[L-1] (where the plane exists and L >= 1), the PreFilter state of the topology plugins stays frozen.
 * rep_L(a, n) = ykpred_headroom's replicas(a, n) evaluated on state_L(n) by the same device routine: 0 when Predicates() rejects the
 * pair there, else min(free pod slots, min over r with req_r > 0 of floor(free_r / req_r)) in exact int64 arithmetic, cut to 1 when the
 * spec requests a dictionary host port and NodePorts is in both lists. Hence rep_0 == ykpred_headroom_pod, rep_L is non-decreasing in
 * L, and min{L : rep_L >= 1} == ykpred_preempt_reach_pod (-1 <=> rep_limit == 0). */
#define YKPRED_PREEMPT_HEADROOM_CELLS 32
/* per ask, int64[32], over all nodes of the table, with m(L) = min(L, limit):
 *  [0..8]   copies(L)  = sum over n of rep_m(L)(a, n), L = 0..8 (flat above the limit)
 *  [9..17]  nodes(L)   = nodes with rep_m(L) >= 1 (the prefix sums of ykpred_preempt_reach cells [0..8])
 *  [18..26] victims(L) = sum over n of gone(n, l*(n, L)): gone(n, l) = the pods of n in tiers < l, l*(n, L) = the smallest l <= m(L)
 *           with rep_l == rep_m(L) — the pods of the FEWEST whole tiers that give each node its level-L copies; a tier that frees
 *           something but adds no copy is not charged by itself. victims(0) == 0.
 *  [27]     status: 0 computed; 1 the ask's spec is YKPRED_SPEC_UNSUPPORTED (every cell but [27..29] is 0); 2 coupled, by exactly
 *           ykpred_headroom's rule: copies(.) and victims(.) are -1, nodes(.) are still the single-copy fit counts, [30] == -1
 *  [28]     the limit, echoed
 *  [29]     the want, echoed
 *  [30]     the lowest L <= limit with copies(L) >= want, or -1
 *  [31]     0
 * Invariants at status 0: copies(0) == ykpred_headroom [0]; nodes(L) <= copies(L); all three rows are non-decreasing.
 * wants == NULL means 1 for every ask. The tasks are the distinct (spec, NodeName, limit) of the list: the want multiplies no task, it
 *   is read only when the per-level table is finished on the host.
 * Everything else is ykpred_preempt_reach's: the call reads the TABLES only, needs no evaluation and invalidates none; it prepares the
 *   topology histograms as ykpred_query does; it counts as one query; roctx range "ykpred:preempt_headroom"; YKPRED_E_STATE without a
 *   reclaim table; YKPRED_E_INVALID for a limit outside 0..T, a want < 1, or NodeResourcesFit missing from either list (as
 *   ykpred_headroom). n_asks == 0 is OK; N == 0 gives zero rows with [30] == -1.
 * NODE-SHARDED engines: COLLECTIVE — the agreement all-gather first (it covers the limits and the wants), then exactly ONE all-reduce SUM
 *   (int64) of the per-level table; the prefix sums and [30] are derived after it, on every rank alike: CLUSTER-WIDE cells. */
int32_t ykpred_preempt_headroom(ykpred_engine_t* e, int32_t n_asks, const int32_t* asks /* host, ask indices, any order, repeats allowed */,
                                const int32_t* limits /* host, [n_asks], 0..T */, const int64_t* wants /* host, [n_asks], >= 1; NULL = 1 */,
                                uint32_t prefilter_plugins, uint32_t filter_plugins, int64_t* out /* host, [n_asks][YKPRED_PREEMPT_HEADROOM_CELLS] */);
/* Row L of out = rep_L(pod, n) for every node n of the table, L = 0..limit. -1 everywhere for a coupled ask, 0 for a
 * YKPRED_SPEC_UNSUPPORTED spec. This shard's nodes only on a sharded engine. */
int32_t ykpred_preempt_headroom_pod(ykpred_engine_t* e, int32_t pod_index, int32_t limit, uint32_t prefilter_plugins, uint32_t filter_plugins,
                                    int32_t* out /* [limit+1][N] */);

/* PREEMPTION VICTIMS — the shortest victim prefix on every node in one pass: what one PreemptionPredicates call per
 * candidate node answers, from resident state.
 *
 * The VICTIM TABLE is resident beside the reclaim table and shard-local on the node axis: one row per eligible pod (a pod in a tier,
 * as the reclaim table defines it), one contiguous SEGMENT per node holding order(n) = the node's eligible pods sorted by (priority
 * ascending, uid ascending bytewise). Tiers are monotone in priority, so the pods of tiers < L are a prefix of the segment for every L. */
typedef struct ykpred_victims {
  int32_t tiers;               /* T: the tier count of the resident reclaim table */
  int64_t rows;                /* P: rows of the two row planes, < 2^31; the segments lie inside 0..P */
  const int32_t* seg_base;     /* [N] first row of the node's segment */
  const int32_t* seg_cap;      /* [N] rows the segment may grow to (>= the node's victim count; the slack rows are never read) */
  const int32_t* tier_end;     /* [T][N] victims of the node in tiers <= t: non-decreasing in t, tier_end[T-1] <= seg_cap */
  const int64_t* cum;          /* [R][P] PREFIX sums of the request vectors within the segment: row p = victims 0..p of its node */
  const uint64_t* ports_after; /* [KP][P] the node's port_bits once victims 0..p are gone; NULL = no victim holds a dictionary port
                                  or KP == 0 */
} ykpred_victims_t;
/* Uploads the table for the current node table. NULL drops it; a ykpred_set_nodes that changes N drops it as well. YKPRED_E_STATE
 * without a node table or without a reclaim table of the same T; YKPRED_E_INVALID for a segment outside 0..P or a tier_end column that
 * descends or passes its capacity. No other call reads the table, and setting it invalidates no evaluation. */
int32_t ykpred_set_victims(ykpred_engine_t* e, const ykpred_victims_t* table);
/* Rewrites ONE node's segment and its tier_end column in place: `one` holds tier_end [T], cum [R][count] and ports_after [KP][count]
 * (given exactly when the resident table has that plane; seg_base, seg_cap and rows are not read). count > seg_cap[node_index] is
 * YKPRED_E_INVALID with nothing written: the caller knows the capacities and uploads the whole table instead. */
int32_t ykpred_update_victims_node(ykpred_engine_t* e, int32_t node_index, int32_t count, const ykpred_victims_t* one);

/* need(a, n): 0 when Predicates(a, n) fits as the node stands; otherwise k >= 1 with k - 1 == ykpred_preemption(a, n, victims(a, n),
 * start 0), victims(a, n) = the first tier_end[limit-1][n] rows of the segment; -1 when that call returns -1 or a PreFilter plugin
 * rejects the pair. "fits with victims 0..i gone" is monotone in i (§4.16's argument per victim), so need is found by BISECTION:
 * at most ceil(log2 len) gathers of one table row. Where need >= 1: tier(order(n)[need-1]) + 1 == ykpred_preempt_reach_pod, and need <=
 * the whole-tier pod count reach reports. */
#define YKPRED_VICTIM_CELLS 16
/* per ask, int64[16], over all nodes of the table:
 *  [0]      nodes with need 0
 *  [1]      nodes with need >= 1
 *  [2]      nodes with need -1
 *  [3]      status: 0 computed; 1 the ask's spec is YKPRED_SPEC_UNSUPPORTED (every other cell 0 except [4], [6] == -1)
 *  [4]      the limit, echoed
 *  [5]      the level of the BEST node — lowest level, then fewest victims, then lowest index —, 0 when there is none
 *  [6]      the best node (a GLOBAL index on a sharded engine), -1 when there is none
 *  [7]      the best node's need (saturating at 2^28 - 1)
 *  [8]      the sum of need over the nodes of [1]
 *  [9..15]  0
 * Invariant at status 0: [0] + [1] + [2] == N.
 * Everything else is ykpred_preempt_reach's: tasks = the distinct (spec, NodeName, limit); the call reads the TABLES only, needs no
 *   evaluation and invalidates none; it prepares the topology histograms as ykpred_query does; one query; roctx range
 *   "ykpred:preempt_victims"; YKPRED_E_STATE without a victim table (or when the reclaim table's T no longer matches);
 *   YKPRED_E_INVALID for a limit outside 0..T.
 * NODE-SHARDED engines: COLLECTIVE — the agreement all-gather first (it covers the limits), then one all-reduce SUM (int64) of the cells
 *   and one all-reduce MIN (int64) of the packed best keys (ykpred_preempt_reach's key with the exact need in the victim field). */
int32_t ykpred_preempt_victims(ykpred_engine_t* e, int32_t n_asks, const int32_t* asks /* host, ask indices, any order, repeats allowed */,
                               const int32_t* limits /* host, [n_asks], 0..T */, uint32_t prefilter_plugins, uint32_t filter_plugins,
                               int64_t* out /* host, [n_asks][YKPRED_VICTIM_CELLS] */);
/* need(pod, n) for every node n of the table (thread = node). -1 everywhere for a YKPRED_SPEC_UNSUPPORTED spec. This shard's nodes only
 * on a sharded engine. */
int32_t ykpred_preempt_victims_pod(ykpred_engine_t* e, int32_t pod_index, int32_t limit, uint32_t prefilter_plugins, uint32_t filter_plugins,
                                   int32_t* out /* [N] */);

/* PREEMPTION ROUND — conflict-resolved victim plans for a LIST of asks: the counterpart of ykpred_allocate_round for
 * preemption. The asks are processed IN LIST ORDER, each under the state the earlier asks of the list left behind, in one call with no
 * host step in between. A gang's plan is the call with the ask repeated: repeats are NOT deduplicated, each occurrence is one more
 * copy; limits may come in any order.
 *
 * ROUND STATE, per node n, zero at the start of EVERY call; nothing persists, no table is changed, no evaluation is invalidated:
 *   taken[n]          the prefix of order(n) already claimed
 *   placed_req[r][n]  the summed request vectors of the asks the round placed on n
 *   placed_pods[n]    their number
 *   placed_ports[p][n] the OR of their wanted dictionary port words
 * state(n, k), k >= taken[n] = the node as ykpred_preempt_victims sees it with victims 0..k-1 gone, and the round's pods on it: free
 *   values free + cum[k-1] - placed_req (no cum term at k == 0), the slot test on count - k + placed_pods, port words
 *   (k >= 1 ? ports_after[k-1] : ports) | placed_ports; the topology PreFilter state is frozen, as everywhere in §4.16-4.18.
 * need'(a, n), at the ask's turn: the smallest k in [taken[n], hi] whose state passes Predicates, hi = max(taken[n],
 *   tier_end[limit-1][n]) (hi = taken[n] at limit 0), reported as extra = k - taken[n]; -1 when no k of the interval passes or the
 *   failure at k == taken[n] is one no removal changes. Monotone in k by §4.18's argument (the overlay is constant in k): a bisection.
 * CHOICE: among the nodes with need' >= 0 the minimum of ykpred_preempt_reach's packed key level | extra | global node — level 0 for
 *   extra == 0, else tier(order(n)[k-1]) + 1; extra saturates at 2^28 - 1 (a table with a longer segment: YKPRED_E_UNSUPPORTED). So an
 *   ask that fits somewhere with no further victim — a node an earlier ask of the round opened counts — goes to the lowest-index such
 *   node; every other ask to the lowest level, then the fewest further victims, then the lowest index.
 * APPLY, on the chosen node: taken += extra, placed_req += req(a), placed_pods += 1, placed_ports |= wanted(a). Asks placed by the
 *   round are never victims of later asks; a skipped ask (outcome 2, 3, 4) changes nothing. */
#define YKPRED_PREEMPT_ROUND_CELLS 8
/* per ask, in list order, int64[8]:
 *  [0]  outcome: 0 placed with no further victim; 1 placed by preemption; 2 nowhere; 3 the spec is YKPRED_SPEC_UNSUPPORTED;
 *       4 COUPLED by exactly ykpred_headroom's rule (the ask's verdicts read the topology histograms under these lists)
 *  [1]  the node, a GLOBAL index on a sharded engine, or -1
 *  [2]  from = taken[node] before the ask: its victims are order(node)[from .. from + extra - 1]
 *  [3]  extra
 *  [4]  the level
 *  [5]  the limit, echoed
 *  [6]  nodes with need' >= 0 at the ask's turn
 *  [7]  the sum of extra over the nodes with extra >= 1 at its turn
 * ([6] and [7]: a wrong overlay on a node that was NOT chosen still changes an output.) At outcome 2..4: [1] == -1, [2..4] == 0, and
 * [6], [7] == 0.
 * out_summary, int64[8]: [0..4] asks per outcome, [5] victims in all (the sum of [3]), [6] distinct nodes touched, [7] 0.
 * IDENTITIES: (1) with non-increasing limits and no coupled ask the round equals, step by step, the host loop "need per node via
 *   ykpred_preempt_victims_pod → the victims removed from the node → the ask assumed on it" on fresh tables; (2) a round of W repeats of
 *   a status-0 ask places exactly min(W, ykpred_preempt_headroom copies(limit)) of them; (3) a round of ONE ask has [4], [1], [3] ==
 *   ykpred_preempt_victims cells [5], [6], [7] when cell [0] there is 0 (and [1] == the first fitting node otherwise).
 * Errors as ykpred_preempt_victims; n_asks == 0 is YKPRED_OK (the summary is zeroed); a table of N == 0 nodes gives outcome 2 for
 *   every evaluated ask. Reads the TABLES only; prepares the topology histograms as ykpred_query does; ONE query; roctx range
 *   "ykpred:preempt_round". All launches are plain launches queued on the engine's stream, with one readback at the end.
 * NODE-SHARDED engines: COLLECTIVE — the agreement all-gather first (it covers the list and the limits); per evaluated ask one
 *   all-reduce MIN of the packed key and one all-reduce SUM of the two counts, on the stream; every rank then applies the same decision,
 *   the owning shard moves its state; one all-reduce MAX of the cells at the end ([2] is the owner's). All ranks return the same cells. */
int32_t ykpred_preempt_round(ykpred_engine_t* e, int32_t n_asks, const int32_t* asks /* host, ask indices, list order, repeats = copies */,
                             const int32_t* limits /* host, [n_asks], 0..T */, uint32_t prefilter_plugins, uint32_t filter_plugins,
                             int64_t* out_cells /* host, [n_asks][YKPRED_PREEMPT_ROUND_CELLS] */, int64_t* out_summary /* host, [8] */);

/* PREEMPTION ROUND WITH LIVE TOPOLOGY HISTOGRAMS: ykpred_preempt_round for lists that hold COUPLED asks — asks whose
 * verdicts read the PodTopologySpread / InterPodAffinity histograms. ykpred_preempt_round, its kernels and its cells are unchanged.
 *
 * The VICTIM-EFFECTS PLANE is resident beside the victim table, row for row: what the victims of every prefix contributed to the
 * selector classes of the node table (ykpred_nodes_t.selector_count). A victim's contribution to class s is what the host's encoder adds
 * to selector_count[s] for that pod (a terminating pod adds nothing to a PodTopologySpread class); the contributions of ALL pods of a
 * node sum to its selector_count column. */
typedef struct ykpred_victim_effects {
  int32_t classes;          /* KS of the node table */
  int32_t columns;          /* KA <= KS: the classes some eligible pod contributes to */
  int64_t rows;             /* P of the resident victim table */
  const int32_t* class_col; /* [KS] the column of class s, or -1: no eligible pod contributes to it */
  const int32_t* cum;       /* [KA][P] PREFIX sums within the segment, like ykpred_victims_t.cum: row p = victims 0..p of its node */
} ykpred_victim_effects_t;
/* Uploads the plane for the resident victim table (YKPRED_E_STATE without one; YKPRED_E_INVALID when rows or classes differ from the
 * victim table's P / the node table's KS, or class_col leaves -1..KA-1). NULL drops it; ykpred_set_victims drops it as well.
 * THE CALLER'S DUTY: the engine checks the plane's shape (rows, KS) and that no segment was patched without its rows; it cannot see what
 * a selector class MEANS. A caller that uploads node or spec tables encoded under another selector-class dictionary must upload the
 * victim table and this plane again (the host library does: it ties the plane to a digest of its topology dictionaries). */
int32_t ykpred_set_victim_effects(ykpred_engine_t* e, const ykpred_victim_effects_t* fx);
/* Rewrites ONE node's rows: cum [KA][count], count <= seg_cap[node_index] (YKPRED_E_INVALID otherwise, nothing written). A
 * ykpred_update_victims_node marks the node's plane rows as stale until this call follows it. */
int32_t ykpred_update_victim_effects_node(ykpred_engine_t* e, int32_t node_index, int32_t count, const int32_t* cum);

/* ROUND STATE: ykpred_preempt_round's, plus a round-local copy of the histogram counts (layout.spread_counts) and of the per-constraint
 *   minima (what the Filters read as the global minimum / the domains with a match: [G], constraint order), with the running minimum over the present domains and the number of domains that sit there. The copy is
 *   taken from the engine's prepared histograms at the start of EVERY call; nothing persists; the engine's histograms and every table are
 *   unchanged after the call.
 * TURN: need' and the choice are ykpred_preempt_round's, evaluated against the round-local histograms as they stand at the START of the
 *   turn: within a turn they are frozen, the ask's own victims included (PreemptionPredicates' rule, §4.16-4.18) — a topology failure is
 *   still a failure no removal opens.
 * APPLY: ykpred_preempt_round's, and then for the chosen node n and EVERY constraint g of EVERY signature (selector class ks, key kd):
 *   delta_g = (what one pod of the ask's spec adds to class ks: ykpred_set_spec_effects) - (what the victims order(n)[from .. from+extra)
 *   contributed to ks: two cells of the plane), applied in domain domain_id[kd][n] — only where a pod on n counts for g (the node carries
 *   the key with an id inside the row; for a PodTopologySpread constraint the node carries every key of the signature's spread
 *   constraints and passes the inclusion policies the constraint honors: ykpred_allocate_round's assume test). The cell moves by delta_g,
 *   which can have either sign; a spread constraint's minimum, domains-at-minimum and minimum after the minDomains rule are recomputed; an
 *   InterPodAffinity row's minimum cell (domains with a match) moves by one when the cell crosses zero, in either direction. EVERY placed
 *   ask applies its effects, coupled or not: an uncoupled pod can match a later ask's selector.
 * OUTCOMES 0-3 as ykpred_preempt_round; outcome 4 never occurs. Cells [0..7] keep their meaning.
 * out_summary[7] = the (turn, constraint) pairs with an applied delta_g != 0; [0..6] as ykpred_preempt_round.
 * out_counts / out_minima (each may be NULL): the round-local histograms after the last turn, in the layout's cell order.
 * IDENTITIES: (1) with non-increasing limits the live round equals, step by step, the host loop "need per node via
 *   ykpred_preempt_victims_pod -> the victims removed from the node -> the ask assumed on it" on fresh tables, coupled asks included;
 *   (2) a list with no coupled ask, on specs and victims that contribute to no class, gives the cells of ykpred_preempt_round;
 *   (3) at limit 0, W repeats of an ask that ykpred_headroom_spread (ykpred_headroom_affinity) answers with status 0 place exactly
 *   min(W, its copies).
 * Errors as ykpred_preempt_round; additionally YKPRED_E_UNSUPPORTED without spec effects of the current spec table, YKPRED_E_STATE
 *   without a victim-effects plane that describes the resident victim table (none uploaded, dropped by ykpred_set_victims, or a segment
 *   patched without its plane rows). ONE query; roctx range "ykpred:preempt_round_live"; plain launches on the engine's stream: per
 *   evaluated ask the step and the apply, then k_preempt_round_effects (thread = constraint, a dense [2][G] int record zeroed on the
 *   stream first) and k_preempt_round_topo (a workgroup per constraint, at work where the record names a step).
 * NODE-SHARDED engines: COLLECTIVE; the agreement covers the new arguments; per applied turn ONE all-reduce SUM of the record between
 *   the two kernels (the owner of the node fills it, the others contribute zeros); every rank moves its cluster-wide copy. The record
 *   is dense: no cap on the constraints one turn moves. A rank whose shard holds no node takes part in every reduce. The histograms must be current (ykpred_eval) as for every sharded query. */
/* out2 = { layout.spread_cells, G = constraints of all topology signatures } for the current tables: the sizes of out_counts / out_minima.
 * Builds the signature tables when they are stale (no device pass); YKPRED_E_STATE before the node and spec tables are uploaded. */
int32_t ykpred_histogram_dims(ykpred_engine_t* e, int64_t* out2 /* [2] */);
int32_t ykpred_preempt_round_live(ykpred_engine_t* e, int32_t n_asks, const int32_t* asks /* host, ask indices, list order, repeats = copies */,
                                  const int32_t* limits /* host, [n_asks], 0..T */, uint32_t prefilter_plugins, uint32_t filter_plugins,
                                  int64_t* out_cells /* host, [n_asks][YKPRED_PREEMPT_ROUND_CELLS] */, int64_t* out_summary /* host, [8] */,
                                  int32_t* out_counts /* host, NULL or [layout.spread_cells] */, int32_t* out_minima /* host, NULL or [G] */);

/* ------------------------------------------------------------------------------------------------------------------
 * Multi-GPU: node-axis shards. One engine per GPU / process holds a contiguous shard of the node table and
 * the full ask table; every (ask, node) pair is independent, so each shard evaluates its own bitmap columns with no
 * data-path collective. The exchanges below run over RCCL (xGMI inside one box) on the stream they are given, ordered after
 * the work already queued there; librccl is loaded on first use (dlopen), so a single-GPU process never maps it.
 *
 *   ykpred_comm_unique_id   rank 0 draws the 128-byte id; the host distributes it out of band (the Go side: over whatever
 *                           already connects the shard processes; bench.py: its torch.distributed bootstrap group)
 *   ykpred_comm_init        ncclCommInitRank; node_offset = global index of this shard's node 0
 *   ykpred_gather_bitmap    all-gather of the shard bitmaps of the last ykpred_eval into the shard-major layout
 *                           [world][num_rows][row_stride] (BASELINE configs[3]) plus the shards' row_of_pod maps
 *                           [world][P]; every shard must use the same row_stride and row capacity
 *                           (ykpred_set_row_stride / ykpred_set_row_capacity) and hold the same asks in the same order
 *   ykpred_exchange_decisions  in place on the outputs of the last ykpred_eval (which must have produced decision keys):
 *                           counts → cluster-wide feasible counts (SUM); decisions → GLOBAL node index of the best
 *                           feasible node in bin-pack order, ties by global node index (MIN key, then MIN index), -1 = none
 *   PodTopologySpread / InterPodAffinity histograms: once a communicator is attached, ykpred_eval itself sums the
 *                           per-shard histograms (SUM of matches, MAX of "domain present") between its count and min
 *                           passes — the shards must share the topology-domain dictionaries (ykhost_comm_init makes
 *                           them cluster-wide; the ranks compare the histograms' shape and dictionary digest first and,
 *                           when they differ, all return the same YKPRED_E_INVALID instead of summing misaligned cells;
 *                           that check is one more small all-gather and a host sync per histogram sum) — and ykpred_query /
 *                           ykpred_preemption reuse those cluster-wide histograms instead of rebuilding shard-local ones.
 * Not sharded: PreemptionPredicates (one node, sequential victim prefix) runs on the shard that owns the node. */
#define YKPRED_COMM_ID_BYTES 128
/* Which shared library provides the collectives (ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclAllGather /
 * ncclAllReduce / ncclGetErrorString): by default librccl, loaded on the first ykpred_comm_* call. Effective only BEFORE that
 * first call of the process. The tests point it at tests/c/rccl_stub.cpp — the same entry points over shared memory between
 * processes that share one GPU, which RCCL itself refuses — so that the world > 1 branches run on a one-GPU box. */
int32_t ykpred_comm_use_library(const char* path);
int32_t ykpred_comm_unique_id(uint8_t* id /* [YKPRED_COMM_ID_BYTES] */);
int32_t ykpred_comm_init(ykpred_engine_t* e, const uint8_t* id, int32_t rank, int32_t world, int32_t node_offset);
int32_t ykpred_comm_destroy(ykpred_engine_t* e);
/* All-gather of `bytes` HOST bytes over the attached communicator: recv (host, [world][bytes]) gets every rank's `send`, in
 * rank order. Collective; every rank passes the same `bytes` (a host that ships blobs of unequal length gathers the lengths
 * first). What the hosts exchange at comm_init (ykhost_comm_init: the shards' topology-domain values) travels this way. */
int32_t ykpred_comm_allgather_bytes(ykpred_engine_t* e, const void* send, int64_t bytes, void* recv);
/* Moves the communicator (with rank, world and node offset) of `from` to `to`, an engine on the same device without one: what a
 * host does when its dictionaries change shape on a node-sharded handle and it re-creates the engine (the communicator cannot be
 * initialised twice from one id). `from` is left without a communicator. */
int32_t ykpred_comm_adopt(ykpred_engine_t* to, ykpred_engine_t* from);
/* A digest of what the topology ids stand for (the host's topology key strings, domain values in id order, selector classes).
 * Node-sharded ranks compare it, with the histogram shape, before they sum histograms or start a round: equal counts over
 * different dictionaries are refused (YKPRED_E_INVALID on every rank) instead of summed. 0 = not provided. */
int32_t ykpred_set_dictionary_digest(ykpred_engine_t* e, uint64_t digest);
/* the attached communicator's geometry (rank 0, world 1, node_offset 0 without one); any of the pointers may be NULL */
int32_t ykpred_comm_info(const ykpred_engine_t* e, int32_t* rank, int32_t* world, int32_t* node_offset);
/* Rows of the NEXT ykpred_set_nodes get this stride (64-bit words, multiple of 16, >= the shard's own need); 0 = automatic.
 * Shards of unequal size agree on the stride of the largest one so that the gathered layout is regular. */
int32_t ykpred_set_row_stride(ykpred_engine_t* e, int32_t words);
/* The bitmap is sized for at least `rows` physical rows (0 = as many as needed). Shards agree on one capacity (>= every
 * shard's layout.num_rows) so that the gathered layout [world][rows][row_stride] is regular. */
int32_t ykpred_set_row_capacity(ykpred_engine_t* e, int32_t rows);
int32_t ykpred_gather_bitmap(ykpred_engine_t* e, void* gathered /* DEVICE [world][num_rows][row_stride] u64, NULL = engine-owned */, void* stream);
int32_t ykpred_exchange_decisions(ykpred_engine_t* e, void* stream);
/* Class-compressed form of the same gather. The member rows of a pod class are identical, so a shard's bitmap IS its
 * [num_classes][row_stride] class-row table plus its pod -> class map. xGMI is per-link bound (7 links x ~50 GB/s in a ring)
 * while the local HBM takes > 5 TB/s of writes: the shards exchange class rows (MBs instead of GBs) and every GPU writes all
 * `world` slabs locally. Result: [world][num_rows][row_stride] like ykpred_gather_bitmap, with EVERY slab in the row order
 * of the receiving engine (its own row_of_pod; ykpred_read_gathered hides the difference).
 * Shards merge signatures relative to their own taint / node-name dictionaries, so their class partitions may differ:
 *   ykpred_layout_hash            64-bit digest of the class partition + row layout; a peer with MY digest is expanded with my
 *                                 writer kernels and tables (band writer + class-by-class writer), any other peer ask by ask
 *                                 row by row through its pod -> class map (k_expand_by_row)
 *   ykpred_collect_class_rows     out = DEVICE [num_classes][row_stride] u64 of the last evaluation
 *   ykpred_expand_class_rows      bitmap_out (DEVICE [num_rows][row_stride]) = the bitmap whose class rows are `class_rows`
 *                                 (indexed by this engine's classes, or by a peer's with that peer's pod -> class map), in this
 *                                 engine's row layout
 *   ykpred_gather_bitmap_compressed  header exchange (digest, class count), ncclAllGather of the class rows (and of the pod ->
 *                                 class maps when digests differ), `world` expansions; the slab of this rank is skipped when
 *                                 `gathered` + rank * slab is the bitmap the last evaluation wrote */
int32_t ykpred_layout_hash(ykpred_engine_t* e, uint64_t* out);
int32_t ykpred_collect_class_rows(ykpred_engine_t* e, void* out, void* stream);
int32_t ykpred_expand_class_rows(ykpred_engine_t* e, const void* class_rows, const int32_t* pod_class /* DEVICE int32[P]: the pod -> class map
    the table is indexed by (a peer's); NULL = this engine's own classes */, void* bitmap_out, void* stream);
int32_t ykpred_gather_bitmap_compressed(ykpred_engine_t* e, void* gathered /* DEVICE [world][num_rows][row_stride] u64, NULL = engine-owned */, void* stream);
/* readback of the engine-owned gathered bitmap: the rows of pods [first_pod, first_pod + num_pods) in shard `shard` (through
 * that shard's gathered row_of_pod map), row_stride words each */
int32_t ykpred_read_gathered(ykpred_engine_t* e, int32_t shard, int32_t first_pod, int32_t num_pods, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* YKPRED_H_ */

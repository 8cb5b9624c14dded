"""Python face of the host library: the reference's PredicateManager interface over the MI355X engine.

Method names and result conventions follow /root/reference/pkg/plugin/predicates/predicate_manager.go:47-55 so the
parity tests read like predicate_manager_test.go:

    pm = GpuPredicateManager()                       # NewPredicateManager(handle)
    pm = GpuPredicateManager.internal(ep, ep, ep, ep)  # newPredicateManagerInternal(handle, resPre, allocPre, resFilt, allocFilt)
    plugin, err = pm.predicates(pod, node, allocate)   # ("", None) when the pod fits
    index = pm.preemption_predicates(pod, node, victims, start_index)

There is no CPU evaluation path: constructing a manager without a visible GPU raises.
"""
import ctypes as C
import json

import numpy as np

from . import _ffi

PLUGIN_BITS = {
    "NodeUnschedulable": 1 << 0,
    "NodeName": 1 << 1,
    "TaintToleration": 1 << 2,
    "NodeAffinity": 1 << 3,
    "NodePorts": 1 << 4,
    "NodeResourcesFit": 1 << 5,
    "PodTopologySpread": 1 << 6,
    "InterPodAffinity": 1 << 7,
}
ALL_PLUGINS = 0xFF
OUT_BITMAP, OUT_COUNTS, OUT_DECISIONS, OUT_DECISION_KEYS = 1, 2, 4, 8
EVAL_PROFILE, EVAL_DIRECT = 1 << 8, 1 << 9
EVAL_SPREAD_COUNT_ONLY, EVAL_SPREAD_COUNTS_READY = 1 << 10, 1 << 11
# ykpred_explain: int32[EXPLAIN_BINS] per ask — [0..8] first failing plugin code, [EXPLAIN_FIT] nodes the ask fits,
# [EXPLAIN_UNSUPPORTED] nodes not evaluated (routed ask), [EXPLAIN_REASON0 + b] reason bit b, [EXPLAIN_RESOURCE0 + r] insufficient resource r
EXPLAIN_BINS = 32
EXPLAIN_FIT, EXPLAIN_UNSUPPORTED, EXPLAIN_REASON0, EXPLAIN_RESOURCE0 = 9, 10, 12, 16
# ykpred_headroom: int64[HEADROOM_CELLS] per ask — [HEADROOM_TOTAL] sum of replicas over the nodes, [HEADROOM_NODES] nodes taking at
# least one copy, [HEADROOM_MAX] the most one node takes, [HEADROOM_STATUS] 0 computed / 1 routed ask / 2 coupled (total = max = -1),
# nodes bound by [HEADROOM_BY_SLOTS] pod slots, [HEADROOM_BY_PORT] the host port, [HEADROOM_BY_RESOURCE0 + r] resource r
HEADROOM_CELLS = 16
HEADROOM_TOTAL, HEADROOM_NODES, HEADROOM_MAX, HEADROOM_STATUS, HEADROOM_BY_SLOTS, HEADROOM_BY_PORT, HEADROOM_BY_RESOURCE0 = 0, 1, 2, 3, 4, 5, 8
# ykpred_headroom_groups: per (ask, group) int64[GROUP_CELLS] = copies, nodes (row G: the ungrouped nodes); per ask int64[GROUP_SUMMARY] =
# status, groups with copies >= 1, groups with copies >= want, (most: group, copies), (tightest that holds want: group, copies), copies
# on ungrouped nodes. Up to GROUP_LDS_MAX_GROUPS groups the kernel accumulates in LDS.
GROUP_CELLS, GROUP_SUMMARY, GROUP_LDS_MAX_GROUPS = 2, 8, 63
# ykpred_headroom_spread: per ask int64[SPREAD_HEADROOM_CELLS] = copies, domains with a copy, most copies in a domain, status (0 computed,
# 1 routed, 2 still coupled, 3 not coupled: headroom answers), sum of cap, present domains, floor, the domain that pins the floor, domains
# filled / cut / shut, the domain with the most copies, topology key index, maxSkew, fitting nodes, 0; per (ask, domain)
# int64[SPREAD_ROW_CELLS] = cnt, cap, nodes, copies
SPREAD_HEADROOM_CELLS, SPREAD_ROW_CELLS = 16, 4
# ykpred_headroom_affinity: per ask int64[AFFINITY_HEADROOM_CELLS] = copies (outside included), domains with a copy, most copies in a
# domain, status (0 computed, 1 routed, 2 still coupled, 3 no InterPodAffinity constraint is live, 4 bootstrap), sum of cap, blocked
# domains, copies outside, nodes outside, domains filled / cut, 0, the domain with the most copies, topology key index, mode (0 static,
# 1 one per domain, 2 bootstrap), fitting nodes, 0; per (ask, domain) int64[SPREAD_ROW_CELLS] = cnt, cap, nodes, copies
AFFINITY_HEADROOM_CELLS = 16
# ykpred_preempt_reach: per ask int64[REACH_CELLS] = nodes at level 0, 1..8, never, status (0 computed, 1 routed), the ask's limit, the
# lowest level >= 1 with a node (0: none), the best node at it (fewest victim pods, lowest index; -1: none), its victim pods, 0
REACH_CELLS, REACH_MAX_TIERS = 16, 8
REACH_NEVER, REACH_STATUS, REACH_LIMIT, REACH_BEST_LEVEL, REACH_BEST_NODE, REACH_BEST_PODS = 9, 10, 11, 12, 13, 14
# ykpred_preempt_explain: per ask int64[PREEMPT_EXPLAIN_CELLS] = never nodes by the first failing code of their final verdict [0..8],
# nodes at level 0, nodes not evaluated, nodes at a level >= 1, reason bits and insufficient resources of the final verdict over the
# not-enough nodes [12..15] / [16..23], no-victims / unresolvable / not-enough nodes, not-enough nodes held by a port, the pods whose
# eviction would be wasted, the ask's limit, status (0 computed, 1 routed), 0. Per node (preempt_explain_nodes): query_pod_packed's word
# | level << PREEMPT_EXPLAIN_LEVEL_SHIFT (PREEMPT_EXPLAIN_LEVEL_NEVER: never) | PREEMPT_EXPLAIN_ELIGIBLE when a pod is in a tier below
# the limit
PREEMPT_EXPLAIN_CELLS = 32
(PREEMPT_EXPLAIN_FIT, PREEMPT_EXPLAIN_UNSUPPORTED, PREEMPT_EXPLAIN_OPENED, PREEMPT_EXPLAIN_REASON0, PREEMPT_EXPLAIN_RESOURCE0, PREEMPT_EXPLAIN_NO_VICTIMS,
 PREEMPT_EXPLAIN_UNRESOLVABLE, PREEMPT_EXPLAIN_NOT_ENOUGH, PREEMPT_EXPLAIN_PORTS, PREEMPT_EXPLAIN_WASTED, PREEMPT_EXPLAIN_LIMIT,
 PREEMPT_EXPLAIN_STATUS) = 9, 10, 11, 12, 16, 24, 25, 26, 27, 28, 29, 30
PREEMPT_EXPLAIN_LEVEL_SHIFT, PREEMPT_EXPLAIN_LEVEL_NEVER, PREEMPT_EXPLAIN_ELIGIBLE = 24, 15, 1 << 28
# ykpred_preempt_headroom: per ask int64[PREEMPT_HEADROOM_CELLS] = copies(L), nodes(L), victims(L) for L = 0..8 from the three row offsets,
# status (0 computed, 1 routed, 2 coupled), the ask's limit, the want, the lowest level whose copies meet the want (-1: none), 0
PREEMPT_HEADROOM_CELLS = 32
PREEMPT_HEADROOM_COPIES, PREEMPT_HEADROOM_NODES, PREEMPT_HEADROOM_VICTIMS = 0, 9, 18
PREEMPT_HEADROOM_STATUS, PREEMPT_HEADROOM_LIMIT, PREEMPT_HEADROOM_WANT, PREEMPT_HEADROOM_LEVEL = 27, 28, 29, 30
# ykpred_preempt_victims: per ask int64[VICTIM_CELLS] = nodes with need 0, need >= 1, need -1, status (0 computed, 1 routed), the ask's
# limit, the best node's level (0: none), the best node (lowest level, fewest victims, lowest index; -1: none), its need, the sum of need
# over the nodes of [1], 0 ...
VICTIM_CELLS = 16
VICTIM_FIT, VICTIM_OPEN, VICTIM_NEVER, VICTIM_STATUS, VICTIM_LIMIT, VICTIM_BEST_LEVEL, VICTIM_BEST_NODE, VICTIM_BEST_NEED, VICTIM_TOTAL = range(9)
# ykpred_preempt_round: per ask of the list int64[PREEMPT_ROUND_CELLS] = outcome (0 placed with no further victim, 1 placed by preemption,
# 2 nowhere, 3 routed, 4 coupled), node (global index, -1: none), from (the node's prefix already claimed), extra (further victims),
# level, the ask's limit, nodes that could take the ask at its turn, the sum of extra over those that need victims
PREEMPT_ROUND_CELLS = 8
(PREEMPT_ROUND_OUTCOME, PREEMPT_ROUND_NODE, PREEMPT_ROUND_FROM, PREEMPT_ROUND_EXTRA, PREEMPT_ROUND_LEVEL, PREEMPT_ROUND_LIMIT, PREEMPT_ROUND_OPEN,
 PREEMPT_ROUND_TOTAL) = range(8)


def plugin_mask(names):
    """enabledPlugins(...) of predicate_manager_test.go:2201-2207; names outside the engine's set are ignored like absent plugins."""
    if isinstance(names, int):
        return names
    m = 0
    for n in names:
        if n == "*":
            return ALL_PLUGINS
        m |= PLUGIN_BITS.get(n, 0)
    return m


class UnsupportedAsk(Exception):
    """Predicates() on an ask the engine does not evaluate (YKHOST_E_UNSUPPORTED): the CPU PredicateManager must answer it."""


class PredicateError(Exception):
    """The error value returned by Predicates(): carries the failing plugin like Context.IsPodFitNode's joined error."""

    def __init__(self, plugin, message):
        super().__init__(f"failed plugin: '{plugin}'\n{message}")
        self.plugin = plugin
        self.message = message


class GpuPredicateManager:
    def __init__(self, device=0):
        self._L = _ffi.load_ykhost()
        self._P = _ffi.load_ykpred()
        err = C.create_string_buffer(512)
        self._h = self._L.ykhost_create(device, err, 512)
        if not self._h:
            raise RuntimeError("ykhost_create failed (the engine has no CPU fallback): " + err.value.decode())
        # NewPredicateManager's phase lists (predicate_manager.go:321-373), restricted to the engine's plugins
        reserve_pre = (PLUGIN_BITS["NodeAffinity"] | PLUGIN_BITS["NodePorts"] | PLUGIN_BITS["PodTopologySpread"]
                       | PLUGIN_BITS["InterPodAffinity"])
        reserve_filt = reserve_pre | PLUGIN_BITS["NodeUnschedulable"] | PLUGIN_BITS["NodeName"] | PLUGIN_BITS["TaintToleration"]
        self._masks = (reserve_pre, ALL_PLUGINS, reserve_filt, ALL_PLUGINS)

    @classmethod
    def internal(cls, reservation_prefilters, allocation_prefilters, reservation_filters, allocation_filters, device=0):
        pm = cls(device)
        pm._masks = (plugin_mask(reservation_prefilters), plugin_mask(allocation_prefilters),
                     plugin_mask(reservation_filters), plugin_mask(allocation_filters))
        pm._L.ykhost_set_plugins(pm._h, *pm._masks)
        return pm

    def close(self):
        if getattr(self, "_h", None):
            self._L.ykhost_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc < 0:
            raise RuntimeError(self._L.ykhost_last_error(self._h).decode())
        return rc

    # ---- cluster state (SchedulerCache mirror) ------------------------------------------------------------
    def load_snapshot(self, snapshot):
        text = snapshot if isinstance(snapshot, (str, bytes)) else json.dumps(snapshot)
        self._check(self._L.ykhost_load_snapshot(self._h, text.encode() if isinstance(text, str) else text))

    def update_node(self, node):
        """SchedulerCache.UpdateNode → number of orphaned pods the node adopted."""
        return self._check(self._L.ykhost_update_node(self._h, json.dumps(node).encode()))

    def remove_node(self, name):
        """SchedulerCache.RemoveNode → number of pods orphaned (assumed pods are reverted to pending instead)."""
        return self._check(self._L.ykhost_remove_node(self._h, name.encode()))

    def update_pod(self, pod):
        """SchedulerCache.UpdatePod → False when the pod was stored as an orphan (its node is unknown)."""
        return bool(self._check(self._L.ykhost_update_pod(self._h, json.dumps(pod).encode())))

    def update_nodes_batch(self, nodes):
        """Many SchedulerCache.UpdateNode calls in one crossing: `nodes` = objects or JSON documents (bytes)."""
        text = b"\n".join(n if isinstance(n, bytes) else json.dumps(n).encode() for n in nodes)
        return self._check(self._L.ykhost_update_nodes_batch(self._h, text, len(text)))

    def update_pods_batch(self, pods):
        """Many SchedulerCache.UpdatePod calls in one crossing."""
        text = b"\n".join(p if isinstance(p, bytes) else json.dumps(p).encode() for p in pods)
        return self._check(self._L.ykhost_update_pods_batch(self._h, text, len(text)))

    def remove_pod(self, uid):
        return bool(self._check(self._L.ykhost_remove_pod(self._h, uid.encode())))

    def assume_pod(self, uid, node_name):
        self._check(self._L.ykhost_assume_pod(self._h, uid.encode(), node_name.encode()))

    def forget_pod(self, uid):
        """SchedulerCache.ForgetPod: drops the assumed mark; the pod stays accounted on its node."""
        return bool(self._check(self._L.ykhost_forget_pod(self._h, uid.encode())))

    def validate_task_groups(self, annotation):
        """GetTaskGroupsFromAnnotation: number of task groups; raises RuntimeError with the reason when rejected."""
        text = annotation if isinstance(annotation, str) else json.dumps(annotation)
        return self._check(self._L.ykhost_validate_task_groups(self._h, text.encode()))

    def add_task_groups(self, application_id, queue, namespace, annotation):
        """Creates the minMember placeholder asks of every task group (newPlaceholder); returns how many."""
        text = annotation if isinstance(annotation, str) else json.dumps(annotation)
        app = json.dumps({"applicationId": application_id, "queue": queue, "namespace": namespace})
        return self._check(self._L.ykhost_add_task_groups(self._h, app.encode(), text.encode()))

    def pod_state(self, uid):
        """Cache membership of a pod: None if not cached, else dict(node, assigned, assumed, orphan, ask)."""
        node = C.create_string_buffer(256)
        f = self._L.ykhost_pod_state(self._h, uid.encode(), node, 256)
        if not f & 1:
            return None
        return {"node": node.value.decode(), "assigned": bool(f & 2), "assumed": bool(f & 4), "orphan": bool(f & 8), "ask": bool(f & 16)}

    def node_pod_count(self, name):
        """len(NodeInfo.Pods) of a cached node; None if the node is not cached."""
        c = self._L.ykhost_node_pod_count(self._h, name.encode())
        return None if c < 0 else c

    def generate_kwok(self, seed, num_nodes, num_pods, num_templates=0, node_affinity=1, tolerations=1, unique_requests=0,
                      gang_size=0, node_index_offset=0, spread=0, total_nodes=0):
        cfg = _ffi.YkhostKwok(seed=seed, num_nodes=num_nodes, num_pods=num_pods, num_templates=num_templates,
                              node_affinity=node_affinity, tolerations=tolerations, unique_requests=unique_requests,
                              gang_size=gang_size, node_index_offset=node_index_offset, spread=spread, total_nodes=total_nodes)
        self._check(self._L.ykhost_generate_kwok(self._h, C.byref(cfg)))

    @property
    def num_nodes(self):
        return self._L.ykhost_num_nodes(self._h)

    @property
    def num_pods(self):
        return self._L.ykhost_num_pods(self._h)

    def pod_index(self, uid):
        return self._L.ykhost_pod_index(self._h, uid.encode())

    def node_index(self, name):
        return self._L.ykhost_node_index(self._h, name.encode())

    def dump_snapshot(self, pods=None, nodes=None, compact=False):
        """Snapshot JSON (text) of the selected pending pods / nodes — what the oracle is fed in parity tests. compact: runs
        of on-node pods sharing a template are written once with "replicas": k."""
        self._L.ykhost_set_dump_compact(self._h, 1 if compact else 0)
        pa = None if pods is None else np.ascontiguousarray(pods, dtype=np.int32)
        na = None if nodes is None else np.ascontiguousarray(nodes, dtype=np.int32)
        args = (pa.ctypes.data if pa is not None else None, 0 if pa is None else len(pa),
                na.ctypes.data if na is not None else None, 0 if na is None else len(na))
        need = self._L.ykhost_dump_snapshot(self._h, *args, None, 0)
        self._check(need)
        buf = C.create_string_buffer(need)
        self._check(self._L.ykhost_dump_snapshot(self._h, *args, buf, need))
        return buf.value.decode()

    def dump_documents(self, kind):
        """Newline-separated JSON documents (bytes) as the cache hooks would deliver them: 0 nodes, 1 pods on nodes, 2 asks."""
        need = self._L.ykhost_dump_documents(self._h, kind, None, 0)
        self._check(need)
        buf = C.create_string_buffer(need)
        self._check(self._L.ykhost_dump_documents(self._h, kind, buf, need))
        return buf.raw[:need - 1]

    def update_documents(self, kind, text):
        """ykhost_update_nodes_batch (kind 0) / ykhost_update_pods_batch on a buffer of documents."""
        fn = self._L.ykhost_update_nodes_batch if kind == 0 else self._L.ykhost_update_pods_batch
        return self._check(fn(self._h, text, len(text)))

    def ingest_stats(self):
        out = np.zeros(2, dtype=np.int64)
        self._L.ykhost_ingest_stats(self._h, out.ctypes.data)
        return {"template_reused": int(out[0]), "full_parse": int(out[1])}

    def ingest_timing(self):
        """Pod batches: scanning threads of the last parallel batch, ms of the parallel scan / of the ordered cache pass (summed)."""
        out = np.zeros(5, dtype=np.int64)
        self._L.ykhost_ingest_timing(self._h, out.ctypes.data)
        return {"threads": int(out[0]), "scan_ms": round(float(out[1]) / 1e3, 1), "apply_ms": round(float(out[2]) / 1e3, 1), "parallel_batches": int(out[3]), "bulk_batches": int(out[4])}

    def encoded_tables(self):
        """The structure-of-arrays tables the encoder produces (dict; masks as Python ints). Needs no device."""
        need = self._L.ykhost_encoded_tables_json(self._h, None, 0)
        self._check(need)
        buf = C.create_string_buffer(need)
        self._check(self._L.ykhost_encoded_tables_json(self._h, buf, need))
        t = json.loads(buf.value.decode())
        for k in ("taint_bits", "label_bits", "port_bits", "tolerated", "aff_terms", "pre_terms", "wanted_ports", "occupied_ports"):
            t[k] = [int(x, 16) for x in t[k]]
        return t

    def sync(self):
        self._check(self._L.ykhost_sync(self._h))

    def stats(self):
        out = np.zeros(8, dtype=np.int64)
        self._L.ykhost_stats(self._h, out.ctypes.data)
        keys = ["R", "KT", "W", "taints", "requirements", "templates", "specs", "encode_us"]
        return dict(zip(keys, out.tolist()))

    # ---- the PredicateManager interface ---------------------------------------------------------------------
    def _resolve(self, pod, node):
        p = pod if isinstance(pod, int) else self.pod_index(pod)
        n = node if isinstance(node, int) else self.node_index(node)
        if p < 0 or n < 0:
            raise KeyError("unknown pod or node")
        return p, n

    def predicates(self, pod, node, allocate):
        """Predicates(pod, node, allocate) → (plugin, err): ("", None) on fit, else (failing plugin, PredicateError)."""
        p, n = self._resolve(pod, node)
        plugin = C.create_string_buffer(64)
        msg = C.create_string_buffer(512)
        rc = self._L.ykhost_predicates(self._h, p, n, 1 if allocate else 0, plugin, 64, msg, 512)
        if rc == -13:
            raise UnsupportedAsk(msg.value.decode())
        self._check(rc)
        if rc == 1:
            return "", None
        return plugin.value.decode(), PredicateError(plugin.value.decode(), msg.value.decode())

    # ---- the scheduler-interface callbacks (by allocation key / node id) -------------------------------------
    def is_pod_fit_node(self, allocation_key, node_id, allocate):
        """Context.IsPodFitNode: None when the ask fits, else the error text the core receives (sentinel texts for an
        unknown pod / node, "failed plugin: '<name>'" + message otherwise)."""
        err = C.create_string_buffer(1200)
        rc = self._L.ykhost_is_pod_fit_node(self._h, allocation_key.encode(), node_id.encode(), 1 if allocate else 0, err, 1200)
        if rc == 1:
            return None
        if rc in (0, -10, -11):
            return err.value.decode()
        if rc == -13:
            raise UnsupportedAsk(err.value.decode())
        raise RuntimeError(err.value.decode() or self._L.ykhost_last_error(self._h).decode())

    def is_pod_fit_node_via_preemption(self, allocation_key, node_id, preempt_allocation_keys, start_index):
        """Context.IsPodFitNodeViaPreemption → (index, ok) as PreemptionPredicatesResponse{Index, Success}."""
        arr = (C.c_char_p * max(len(preempt_allocation_keys), 1))()
        for i, v in enumerate(preempt_allocation_keys):
            arr[i] = None if v is None else v.encode()
        r = self._L.ykhost_is_pod_fit_node_via_preemption(self._h, allocation_key.encode(), node_id.encode(), arr,
                                                          len(preempt_allocation_keys), start_index)
        if r < -1:
            raise RuntimeError(self._L.ykhost_last_error(self._h).decode())
        return r, r != -1

    def preemption_predicates(self, pod, node, victims, start_index):
        """PreemptionPredicates(pod, node, victims, startIndex) → index or -1. victims: UIDs (None = nil pod)."""
        p, n = self._resolve(pod, node)
        arr = (C.c_char_p * max(len(victims), 1))()
        for i, v in enumerate(victims):
            arr[i] = None if v is None else v.encode()
        r = self._L.ykhost_preemption_predicates(self._h, p, n, arr, len(victims), start_index)
        if r < -1:
            raise RuntimeError(self._L.ykhost_last_error(self._h).decode())
        return r

    def preemption_predicates_batch(self, queries):
        """queries: iterable of (pod, node, victim_uids, start_index) → list of indices; one device launch for all."""
        queries = list(queries)
        pods, nodes, off, starts, flat = [], [], [0], [], []
        for pod, node, victims, start in queries:
            p, n = self._resolve(pod, node)
            pods.append(p)
            nodes.append(n)
            flat.extend(victims)
            off.append(len(flat))
            starts.append(start)
        arr = (C.c_char_p * max(len(flat), 1))()
        for i, v in enumerate(flat):
            arr[i] = None if v is None else v.encode()
        pa, na = np.asarray(pods, dtype=np.int32), np.asarray(nodes, dtype=np.int32)
        oa, sa = np.asarray(off, dtype=np.int32), np.asarray(starts, dtype=np.int32)
        out = np.full(len(queries), -1, dtype=np.int32)
        self._check(self._L.ykhost_preemption_predicates_batch(self._h, len(queries), pa.ctypes.data, na.ctypes.data, oa.ctypes.data, arr,
                                                               sa.ctypes.data, out.ctypes.data))
        return out.tolist()

    def ask_supported(self, pod):
        """(True, "") when the engine evaluates pending pod #pod, else (False, reason): that ask goes to the CPU manager."""
        p = pod if isinstance(pod, int) else self.pod_index(pod)
        buf = C.create_string_buffer(600)
        rc = self._check(self._L.ykhost_ask_supported(self._h, p, buf, 600))
        return rc == 1, buf.value.decode()

    def candidates(self, pod, k, allocate=True):
        """The first k feasible nodes of the ask in bin-pack order, from the resident answer (needs a current evaluation
        with decisions; raises otherwise)."""
        p = pod if isinstance(pod, int) else self.pod_index(pod)
        out = np.full(max(k, 1), -1, dtype=np.int32)
        n = self._check(self._L.ykhost_candidates(self._h, p, 1 if allocate else 0, k, out.ctypes.data))
        return out[:n].copy()

    def allocate_round(self, asks=None, n=None, apply=True):
        """One scheduling round with conflict-resolved decisions (ykhost_allocate_round): ask i is decided with the earlier
        asks of the round assumed on their nodes. asks: ask indices in decision order (None: the first n asks, default all).
        → int32 array: node index, -1 = no node fits, -2 = routed to the CPU manager."""
        if asks is None:
            count = self.num_pods if n is None else int(n)
            ptr = None
        else:
            arr = np.ascontiguousarray(asks, dtype=np.int32)
            count, ptr = len(arr), arr.ctypes.data
        out = np.full(max(count, 1), -1, dtype=np.int32)
        self._check(self._L.ykhost_allocate_round(self._h, count, ptr, 1 if apply else 0, out.ctypes.data))
        return out[:count].copy()

    def device_errors(self):
        """Engine calls that failed on the device so far (each forces a full re-upload + full pass; see ykhost_device_errors)."""
        return int(self._L.ykhost_device_errors(self._h))

    def round_stats(self):
        out = np.zeros(4, dtype=np.int64)
        self._L.ykhost_round_stats(self._h, out.ctypes.data)
        return dict(zip(["rounds_on_device", "asks_on_device", "asks_one_by_one", "asks_routed"], out.tolist()))

    def resident_stats(self):
        out = np.zeros(5, dtype=np.int64)
        self._L.ykhost_resident_stats(self._h, out.ctypes.data)
        return dict(zip(["served_resident", "served_dirty_column", "served_query", "answer_fetches", "code_fetches"], out.tolist()))

    def peek_row(self, pod, allocate=True):
        """(row[row_words] uint64, count, decision) of one ask straight from the bitmap of the last evaluation (ykpred_peek_row)."""
        lay = self.layout()
        row = np.zeros(lay.row_words, dtype=np.uint64)
        cnt, dec = C.c_int32(0), C.c_int32(0)
        self._pcheck(self._P.ykpred_peek_row(self.engine, pod, self._masks[1] if allocate else self._masks[0],
                                             self._masks[3] if allocate else self._masks[2], row.ctypes.data, C.byref(cnt), C.byref(dec)))
        return row, cnt.value, dec.value

    def routing_stats(self):
        out = np.zeros(3, dtype=np.int64)
        self._L.ykhost_routing_stats(self._h, out.ctypes.data)
        return {"unsupported_asks": int(out[0]), "routed_to_cpu": int(out[1]), "dictionary_growths": int(out[2])}

    def pod_request(self, pod):
        buf = C.create_string_buffer(4096)
        self._check(self._L.ykhost_pod_request_json(self._h, pod, buf, 4096))
        return json.loads(buf.value.decode())

    # ---- batched evaluation ---------------------------------------------------------------------------------
    def evaluate(self, allocate=True, bitmap=True, counts=True, decisions=True, profile=False, direct=False):
        opts = (OUT_BITMAP if bitmap else 0) | (OUT_COUNTS if counts else 0) | (OUT_DECISIONS if decisions else 0)
        opts |= (EVAL_PROFILE if profile else 0) | (EVAL_DIRECT if direct else 0)
        self._check(self._L.ykhost_evaluate(self._h, 1 if allocate else 0, opts))

    def evaluate_dirty(self, allocate=True, counts=True, decisions=False, profile=False, spread_count_only=False, spread_counts_ready=False):
        """Patches only the node columns touched since the last evaluation (AssumePod / ForgetPod ...). Returns the
        number of columns re-evaluated, or -1 when a full evaluation had to be run instead. spread_count_only /
        spread_counts_ready: the two halves of the step on a node-sharded cluster whose host sums the topology histograms
        itself (with a communicator attached the engine does it inside one call)."""
        opts = OUT_BITMAP | (OUT_COUNTS if counts else 0) | (OUT_DECISIONS if decisions else 0) | (EVAL_PROFILE if profile else 0)
        opts |= (EVAL_SPREAD_COUNT_ONLY if spread_count_only else 0) | (EVAL_SPREAD_COUNTS_READY if spread_counts_ready else 0)
        n = C.c_int32(-1)
        self._check(self._L.ykhost_evaluate_dirty(self._h, 1 if allocate else 0, opts, C.byref(n)))
        return n.value

    def evaluate_into(self, bitmap=None, counts=None, decisions=None, keys=None, stream=None, allocate=True, profile=False,
                      direct=False, spread_count_only=False, spread_counts_ready=False):
        """ykpred_eval with caller-owned DEVICE outputs (objects exposing data_ptr(), e.g. torch tensors) on the
        caller's HIP stream — how a multi-GPU driver keeps the results where its collectives can reach them."""
        self.sync()
        a = _ffi.YkpredEvalArgs()
        a.prefilter_plugins = self._masks[1] if allocate else self._masks[0]
        a.filter_plugins = self._masks[3] if allocate else self._masks[2]
        a.options = OUT_BITMAP | OUT_COUNTS | OUT_DECISIONS | (OUT_DECISION_KEYS if keys is not None else 0)
        a.options |= (EVAL_PROFILE if profile else 0) | (EVAL_DIRECT if direct else 0)
        a.options |= (EVAL_SPREAD_COUNT_ONLY if spread_count_only else 0) | (EVAL_SPREAD_COUNTS_READY if spread_counts_ready else 0)
        a.bitmap = None if bitmap is None else bitmap.data_ptr()
        a.bitmap_rows = 0 if bitmap is None else int(bitmap.shape[0])  # a caller-owned bitmap states the rows it holds
        a.counts = None if counts is None else counts.data_ptr()
        a.decisions = None if decisions is None else decisions.data_ptr()
        a.decision_keys = None if keys is None else keys.data_ptr()
        a.stream = stream
        self._pcheck(self._P.ykpred_eval(self.engine, C.byref(a)))

    # ---- node-sharded clusters: RCCL exchanges behind the C ABI (include/ykpred.h) ---------------------------------
    @staticmethod
    def comm_unique_id():
        """ncclGetUniqueId through the C ABI: 128 bytes that rank 0 hands to the other shard processes out of band."""
        P = _ffi.load_ykpred()
        buf = (C.c_uint8 * 128)()
        if P.ykpred_comm_unique_id(buf) != 0:
            raise RuntimeError("ykpred_comm_unique_id: " + P.ykpred_last_error(None).decode())
        return bytes(buf)

    def set_row_stride(self, words):
        self._check(self._L.ykhost_set_row_stride(self._h, words))

    def set_row_capacity(self, rows):
        self._check(self._L.ykhost_set_row_capacity(self._h, rows))

    def row_map(self):
        """row_of_pod on the host: the physical bitmap row of every pending ask (rows are laid out for the writer)."""
        out = np.zeros(self.layout().num_pods, dtype=np.int32)
        self._pcheck(self._P.ykpred_read_row_map(self.engine, out.ctypes.data))
        return out

    def comm_init(self, unique_id, rank, world, node_offset):
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._check(self._L.ykhost_comm_init(self._h, buf, rank, world, node_offset))

    def topology_export(self):
        """This shard's node-side share of the topology-domain dictionaries (ykhost_topology_export): bytes. Needs no device."""
        need = self._check(self._L.ykhost_topology_export(self._h, None, 0))
        buf = C.create_string_buffer(need)
        self._check(self._L.ykhost_topology_export(self._h, buf, need))
        return buf.value

    def topology_merge(self, exports):
        """Every shard's export in rank order: the union becomes the floor of this handle's dictionaries (ykhost_topology_merge).
        ykhost_comm_init does both halves itself over the communicator."""
        blob = b"".join(x + b"\0" for x in exports)
        self._check(self._L.ykhost_topology_merge(self._h, blob, len(blob)))

    def comm_destroy(self):
        self._check(self._L.ykhost_comm_destroy(self._h))

    def comm_info(self):
        """(rank, world, node_offset) of the communicator attached to the engine — (0, 1, 0) without one (ykpred_comm_info)."""
        r, w, o = C.c_int32(0), C.c_int32(1), C.c_int32(0)
        self._pcheck(self._P.ykpred_comm_info(self.engine, C.byref(r), C.byref(w), C.byref(o)))
        return int(r.value), int(w.value), int(o.value)

    def gather_bitmap(self, gathered=None, stream=None, compressed=False):
        """All-gather of the shard bitmaps of the last evaluation into [world][rows][row_stride] (device; engine-owned when
        `gathered` is None), on `stream`. compressed=True: the shards exchange their CLASS rows and every GPU expands the
        slabs locally (same result; raises when the shards' row layouts differ — then use the plain form)."""
        fn = self._P.ykpred_gather_bitmap_compressed if compressed else self._P.ykpred_gather_bitmap
        self._pcheck(fn(self.engine, None if gathered is None else gathered.data_ptr(), stream))

    def layout_hash(self):
        """Digest of the class / row layout: shards with equal digests can expand each other's class rows."""
        out = C.c_uint64(0)
        self._pcheck(self._P.ykpred_layout_hash(self.engine, C.byref(out)))
        return int(out.value)

    def collect_class_rows(self, out, stream=None):
        """out: device int64 tensor [num_classes][row_stride] <- the class rows of the last evaluation."""
        self._pcheck(self._P.ykpred_collect_class_rows(self.engine, out.data_ptr(), stream))

    def expand_class_rows(self, class_rows, bitmap_out, pod_class=None, stream=None):
        """bitmap_out (device [num_rows][row_stride]) <- the bitmap whose class rows are `class_rows`, in this engine's row
        layout. pod_class (device int32[P]): the pod -> class map `class_rows` is indexed by when it is a PEER's table."""
        self._pcheck(self._P.ykpred_expand_class_rows(self.engine, class_rows.data_ptr(), None if pod_class is None else pod_class.data_ptr(),
                                                      bitmap_out.data_ptr(), stream))

    def exchange_decisions(self, stream=None):
        """In place on the last evaluation's outputs: cluster-wide counts and GLOBAL best node per ask."""
        self._pcheck(self._P.ykpred_exchange_decisions(self.engine, stream))

    def read_gathered(self, shard, first=0, count=None):
        lay = self.layout()
        count = lay.num_pods - first if count is None else count
        out = np.zeros((count, lay.row_stride), dtype=np.uint64)
        self._pcheck(self._P.ykpred_read_gathered(self.engine, shard, first, count, out.ctypes.data))
        return out

    def spread_tensors(self):
        """(counts, present) int32 torch tensors VIEWING the engine's PodTopologySpread histograms on the device
        (zero-copy via __cuda_array_interface__) — what a node-sharded driver all-reduces between the two halves."""
        import torch
        lay = self.layout()

        class _View:
            def __init__(self, ptr, n):
                self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i4", "data": (ptr, False), "version": 3}

        n = max(int(lay.spread_cells), 1)
        return (torch.as_tensor(_View(lay.spread_counts, n), device="cuda"),
                torch.as_tensor(_View(lay.spread_present, n), device="cuda"))

    @property
    def engine(self):
        return self._L.ykhost_engine(self._h)

    def _pcheck(self, rc):
        if rc != 0:
            raise RuntimeError("ykpred: " + self._P.ykpred_last_error(self.engine).decode())

    def layout(self):
        lay = _ffi.YkpredLayout()
        self._pcheck(self._P.ykpred_get_layout(self.engine, C.byref(lay)))
        return lay

    def synchronize(self):
        self._pcheck(self._P.ykpred_synchronize(self.engine))

    def read_bitmap(self, first=0, count=None):
        lay = self.layout()
        count = lay.num_pods - first if count is None else count
        out = np.zeros((count, lay.row_words), dtype=np.uint64)
        self._pcheck(self._P.ykpred_read_bitmap(self.engine, first, count, out.ctypes.data))
        return out

    def read_rows(self, pods):
        """Bitmap rows of the listed pods, [len(pods)][row_words] uint64 (one device gather + one copy)."""
        pa = np.ascontiguousarray(pods, dtype=np.int32)
        out = np.zeros((len(pa), self.layout().row_words), dtype=np.uint64)
        self._pcheck(self._P.ykpred_read_rows(self.engine, len(pa), pa.ctypes.data, out.ctypes.data))
        return out

    def pod_classes(self):
        """(pod_class[P], class_rep[C]): the engine's pod → class map and one representative pod per class (-1 = none)."""
        lay = self.layout()
        pc = np.zeros(lay.num_pods, dtype=np.int32)
        rep = np.zeros(lay.num_classes, dtype=np.int32)
        self._pcheck(self._P.ykpred_read_pod_classes(self.engine, pc.ctypes.data, rep.ctypes.data))
        return pc, rep

    def check_class_rows(self):
        """Number of bitmap words that differ from the row of the class representative, plus non-zero padding words."""
        v = C.c_uint64(0)
        self._pcheck(self._P.ykpred_check_class_rows(self.engine, C.byref(v)))
        return v.value

    def read_counts(self):
        out = np.zeros(self.layout().num_pods, dtype=np.int32)
        self._pcheck(self._P.ykpred_read_counts(self.engine, out.ctypes.data))
        return out

    def read_decisions(self):
        out = np.zeros(self.layout().num_pods, dtype=np.int32)
        self._pcheck(self._P.ykpred_read_decisions(self.engine, out.ctypes.data))
        return out

    def read_scores(self):
        out = np.zeros(self.layout().num_nodes, dtype=np.float64)
        self._pcheck(self._P.ykpred_read_scores(self.engine, out.ctypes.data))
        return out

    def read_order(self):
        """The bin-pack order of the last evaluation that produced decisions (ykpred_read_order): out[i] = the node at position i —
        ascending score, ties by NodeID. Raises when no such order is current."""
        out = np.zeros(self.layout().num_nodes, dtype=np.int32)
        self._pcheck(self._P.ykpred_read_order(self.engine, out.ctypes.data))
        return out

    def checksum(self):
        v = C.c_uint64(0)
        self._pcheck(self._P.ykpred_bitmap_checksum(self.engine, C.byref(v)))
        return v.value

    def query(self, pods, nodes, allocate=True, pre_mask=None, filt_mask=None):
        """Batch of Predicates() answers evaluated on the device: returns (fit, plugin_code, reason) arrays."""
        pa = np.ascontiguousarray(pods, dtype=np.int32)
        na = np.ascontiguousarray(nodes, dtype=np.int32)
        fit = np.zeros(len(pa), dtype=np.uint8)
        code = np.zeros(len(pa), dtype=np.uint8)
        reason = np.zeros(len(pa), dtype=np.uint32)
        self.sync()
        pre = ALL_PLUGINS if pre_mask is None else pre_mask
        filt = ALL_PLUGINS if filt_mask is None else filt_mask
        self._pcheck(self._P.ykpred_query(self.engine, len(pa), pa.ctypes.data, na.ctypes.data, pre, filt, fit.ctypes.data,
                                          code.ctypes.data, reason.ctypes.data))
        return fit, code, reason

    def query_pod_packed(self, pod, allocate=True, pre_mask=None, filt_mask=None):
        """Every Predicates() answer of ONE ask, one uint32 per node (ykpred_query_pod_packed): bits 0-7 plugin code, bit 8 fit,
        bits 9-12 reason bits 0-3, bits 13.. the insufficient-resource bits. Explicit masks go to the engine directly, like query."""
        p = pod if isinstance(pod, (int, np.integer)) else self.pod_index(pod)
        self.sync()
        pre, filt = self._explicit_masks(allocate, pre_mask, filt_mask)
        out = np.zeros(max(self.layout().num_nodes, 1), dtype=np.uint32)
        self._pcheck(self._P.ykpred_query_pod_packed(self.engine, int(p), pre, filt, out.ctypes.data))
        return out[:self.layout().num_nodes]

    def _explicit_masks(self, allocate, pre_mask, filt_mask):
        pre = (self._masks[1] if allocate else self._masks[0]) if pre_mask is None else pre_mask
        filt = (self._masks[3] if allocate else self._masks[2]) if filt_mask is None else filt_mask
        return pre, filt

    # ---- why an ask fits nowhere ---------------------------------------------------------------------------------
    def explain(self, pods=None, allocate=True, pre_mask=None, filt_mask=None):
        """Per ask the histogram of its Predicates() verdicts over ALL nodes, reduced on the device (ykpred_explain):
        np.int32[n, EXPLAIN_BINS]. pods: ask indices or UIDs in any order, repeats allowed; None = every ask. Needs no evaluation
        and disturbs none. An ask routed to the CPU manager gets [EXPLAIN_UNSUPPORTED] = N. Explicit masks go to ykpred_explain
        directly, like query."""
        if pods is None:
            count, ptr = self.num_pods, None
        else:
            idx = [p if isinstance(p, (int, np.integer)) else self.pod_index(p) for p in pods]
            arr = np.ascontiguousarray(idx, dtype=np.int32)
            count, ptr = len(arr), arr.ctypes.data
        out = np.zeros((max(count, 1), EXPLAIN_BINS), dtype=np.int32)
        if pre_mask is None and filt_mask is None:
            self._check(self._L.ykhost_explain(self._h, count, ptr, 1 if allocate else 0, out.ctypes.data))
        else:
            self.sync()
            pre, filt = self._explicit_masks(allocate, pre_mask, filt_mask)
            if ptr is None:
                arr = np.arange(count, dtype=np.int32)
                ptr = arr.ctypes.data
            self._pcheck(self._P.ykpred_explain(self.engine, count, ptr, pre, filt, out.ctypes.data))
        return out[:count].copy()

    def explain_format(self, bins):
        """kube-scheduler's FitError text for one row of explain(): "0/5 nodes are available: 2 Insufficient cpu, ..."
        (ykhost_explain_format; a pure function of the bins and the resource names — works without a device)."""
        b = np.ascontiguousarray(bins, dtype=np.int32)
        if b.shape != (EXPLAIN_BINS,):
            raise ValueError(f"explain_format takes one row of {EXPLAIN_BINS} bins")
        need = self._check(self._L.ykhost_explain_format(self._h, b.ctypes.data, None, 0))
        buf = C.create_string_buffer(need)
        self._check(self._L.ykhost_explain_format(self._h, b.ctypes.data, buf, need))
        return buf.value.decode()

    def explain_message(self, pod, allocate=True):
        """The Message of the PodScheduled=False / Unschedulable condition for one ask (index or UID): explain + format in one
        crossing (ykhost_explain_message). Raises UnsupportedAsk for an ask routed to the CPU manager, KeyError for an unknown pod."""
        if isinstance(pod, (int, np.integer)):  # (the host names asks by UID: an index takes the two calls)
            ok, why = self.ask_supported(int(pod))
            if not ok:
                raise UnsupportedAsk(why)
            return self.explain_format(self.explain([int(pod)], allocate)[0])
        uid = pod
        buf = C.create_string_buffer(4096)
        rc = self._L.ykhost_explain_message(self._h, uid.encode(), 1 if allocate else 0, buf, 4096)
        if rc == -13:
            raise UnsupportedAsk(buf.value.decode())
        if rc in (-10, -12):
            raise KeyError(buf.value.decode())
        self._check(rc)
        if rc > 4096:
            buf = C.create_string_buffer(rc)
            self._check(self._L.ykhost_explain_message(self._h, uid.encode(), 1 if allocate else 0, buf, rc))
        return buf.value.decode()

    # ---- how many copies of an ask still fit -----------------------------------------------------------------------
    def _headroom_list(self, name, cells, pods, pre_mask, filt_mask, before_engine):
        """What headroom, headroom_spread and headroom_affinity share: pods → indices, np.int64[n, cells], and either the host call
        (ykhost_<name>) or, with explicit masks, before_engine() and the engine call (ykpred_<name>)."""
        if pods is None:
            count, ptr = self.num_pods, None
        else:
            idx = [p if isinstance(p, (int, np.integer)) else self.pod_index(p) for p in pods]
            arr = np.ascontiguousarray(idx, dtype=np.int32)
            count, ptr = len(arr), arr.ctypes.data
        out = np.zeros((max(count, 1), cells), dtype=np.int64)
        if pre_mask is None and filt_mask is None:
            self._check(getattr(self._L, "ykhost_" + name)(self._h, count, ptr, out.ctypes.data))
        else:
            before_engine()
            pre, filt = self._explicit_masks(True, pre_mask, filt_mask)
            if ptr is None:
                arr = np.arange(count, dtype=np.int32)
                ptr = arr.ctypes.data
            self._pcheck(getattr(self._P, "ykpred_" + name)(self.engine, count, ptr, pre, filt, out.ctypes.data))
        return out[:count].copy()

    def headroom(self, pods=None, pre_mask=None, filt_mask=None):
        """Per ask how many copies of it the cluster can still place, reduced on the device (ykpred_headroom): np.int64[n,
        HEADROOM_CELLS]. pods: ask indices or UIDs in any order, repeats allowed; None = every ask. Always the allocation-phase
        lists (the reservation lists carry no NodeResourcesFit); explicit masks go to ykpred_headroom directly, like query. Needs
        no evaluation and disturbs none. A routed ask gets [HEADROOM_STATUS] = 1, a coupled one 2 with total = max = -1."""
        return self._headroom_list("headroom", HEADROOM_CELLS, pods, pre_mask, filt_mask, self.sync)

    def headroom_nodes(self, pod, pre_mask=None, filt_mask=None):
        """How many copies of ONE ask (index or UID) each node takes (ykpred_headroom_pod): np.int32[N]; -1 everywhere for a
        coupled ask. On a node-sharded manager: this shard's nodes."""
        p = pod if isinstance(pod, (int, np.integer)) else self.pod_index(pod)
        out = np.zeros(max(self.num_nodes, 1), dtype=np.int32)
        if pre_mask is None and filt_mask is None:
            self._check(self._L.ykhost_headroom_nodes(self._h, int(p), out.ctypes.data))
        else:
            self.sync()
            pre, filt = self._explicit_masks(True, pre_mask, filt_mask)
            self._pcheck(self._P.ykpred_headroom_pod(self.engine, int(p), pre, filt, out.ctypes.data))
        return out[:self.num_nodes].copy()

    # ---- preemption reach: which nodes removing lower-priority pods opens ----------------------------------------------
    def set_preemption_tiers(self, bounds):
        """Ascending priority bounds b[0] < ... < b[T-1], T <= REACH_MAX_TIERS (ykhost_set_preemption_tiers): a pod on a node is in
        tier t = the smallest t with priority < b[t]; an empty list switches the feature off and drops the device table."""
        b = np.ascontiguousarray(list(bounds), dtype=np.int32)
        self._check(self._L.ykhost_set_preemption_tiers(self._h, b.ctypes.data if len(b) else None, len(b)))

    def preempt_reach(self, pods=None, pre_mask=None, filt_mask=None):
        """Per ask the nodes by preemption LEVEL, reduced on the device (ykpred_preempt_reach): np.int64[n, REACH_CELLS] —
        [0] nodes the ask fits as they stand, [L] nodes it fits once every pod of tiers < L is gone (1 <= L <= its limit),
        [REACH_NEVER] nodes no removal opens, [REACH_STATUS] 1 for a routed ask, [REACH_LIMIT] the ask's limit,
        [REACH_BEST_LEVEL], [REACH_BEST_NODE] (global index, -1: none), [REACH_BEST_PODS]. pods: ask indices or UIDs in any order,
        repeats allowed; None = every ask. Always the allocation-phase lists; explicit masks go to the engine with the limits the
        host derives. Needs no evaluation and disturbs none."""
        if pods is None:
            count, ptr = self.num_pods, None
        else:
            idx = [p if isinstance(p, (int, np.integer)) else self.pod_index(p) for p in pods]
            arr = np.ascontiguousarray(idx, dtype=np.int32)
            count, ptr = len(arr), arr.ctypes.data
        out = np.zeros((max(count, 1), REACH_CELLS), dtype=np.int64)
        if pre_mask is None and filt_mask is None:
            self._check(self._L.ykhost_preempt_reach(self._h, count, ptr, out.ctypes.data))
        else:
            pre, filt = self._explicit_masks(True, pre_mask, filt_mask)
            limits = np.zeros(max(count, 1), dtype=np.int32)
            self._check(self._L.ykhost_preempt_limits(self._h, count, ptr, limits.ctypes.data))  # (syncs the tables and the reclaim table)
            if ptr is None:
                arr = np.arange(count, dtype=np.int32)
                ptr = arr.ctypes.data
            self._pcheck(self._P.ykpred_preempt_reach(self.engine, count, ptr, limits.ctypes.data, pre, filt, out.ctypes.data))
        return out[:count].copy()

    def preempt_reach_nodes(self, pod):
        """The level of ONE ask (index or UID) on every node (ykpred_preempt_reach_pod): np.int32[N], -1 = never — the shortlist
        to walk for the real victim selection. On a node-sharded manager: this shard's nodes."""
        p = pod if isinstance(pod, (int, np.integer)) else self.pod_index(pod)
        out = np.zeros(max(self.num_nodes, 1), dtype=np.int32)
        self._check(self._L.ykhost_preempt_reach_nodes(self._h, int(p), out.ctypes.data))
        return out[:self.num_nodes].copy()

    def preempt_reach_by_key(self, uid):
        """One ask by allocation key in one crossing (ykhost_preempt_reach_by_key) → (np.int64[REACH_CELLS], best node name or "").
        Raises UnsupportedAsk for a routed ask, KeyError for an unknown pod."""
        out = np.zeros(REACH_CELLS, dtype=np.int64)
        buf = C.create_string_buffer(512)
        rc = self._L.ykhost_preempt_reach_by_key(self._h, uid.encode(), out.ctypes.data, buf, 512)
        if rc == -13:
            raise UnsupportedAsk(self._L.ykhost_last_error(self._h).decode())
        if rc in (-10, -12):
            raise KeyError(uid)
        self._check(rc)
        return out, buf.value.decode()

    # ---- preemption explain: why removing lower-priority pods opens no node ---------------------------------------------
    def preempt_explain(self, pods=None, pre_mask=None, filt_mask=None):
        """Per ask WHY preemption opens no node, reduced on the device (ykpred_preempt_explain): np.int64[n, PREEMPT_EXPLAIN_CELLS] —
        the never nodes by the first failing plugin of their verdict with every eligible pod gone, split into
        [PREEMPT_EXPLAIN_UNRESOLVABLE] (no removal moves the failure), [PREEMPT_EXPLAIN_NO_VICTIMS] (nobody to remove) and
        [PREEMPT_EXPLAIN_NOT_ENOUGH] (everybody removed, still failing: reason bins from [PREEMPT_EXPLAIN_REASON0] and
        [PREEMPT_EXPLAIN_RESOURCE0]). pods: ask indices or UIDs in any order, repeats allowed; None = every ask. Always the
        allocation-phase lists; explicit masks go to the engine with the limits the host derives. Needs no evaluation and disturbs
        none."""
        if pods is None:
            count, ptr = self.num_pods, None
        else:
            idx = [p if isinstance(p, (int, np.integer)) else self.pod_index(p) for p in pods]
            arr = np.ascontiguousarray(idx, dtype=np.int32)
            count, ptr = len(arr), arr.ctypes.data
        out = np.zeros((max(count, 1), PREEMPT_EXPLAIN_CELLS), dtype=np.int64)
        if pre_mask is None and filt_mask is None:
            self._check(self._L.ykhost_preempt_explain(self._h, count, ptr, out.ctypes.data))
        else:
            pre, filt = self._explicit_masks(True, pre_mask, filt_mask)
            limits = np.zeros(max(count, 1), dtype=np.int32)
            self._check(self._L.ykhost_preempt_limits(self._h, count, ptr, limits.ctypes.data))  # (syncs the tables and the reclaim table)
            if ptr is None:
                arr = np.arange(count, dtype=np.int32)
                ptr = arr.ctypes.data
            self._pcheck(self._P.ykpred_preempt_explain(self.engine, count, ptr, limits.ctypes.data, pre, filt, out.ctypes.data))
        return out[:count].copy()

    def preempt_explain_nodes(self, pod):
        """The verdict word of ONE ask (index or UID) on every node (ykpred_preempt_explain_pod): np.uint32[N] — query_pod_packed's
        word on the state the verdict comes from, the level from bit PREEMPT_EXPLAIN_LEVEL_SHIFT (PREEMPT_EXPLAIN_LEVEL_NEVER: never),
        PREEMPT_EXPLAIN_ELIGIBLE when the node holds a pod below the ask's limit. On a node-sharded manager: this shard's nodes."""
        p = pod if isinstance(pod, (int, np.integer)) else self.pod_index(pod)
        out = np.zeros(max(self.num_nodes, 1), dtype=np.uint32)
        self._check(self._L.ykhost_preempt_explain_nodes(self._h, int(p), out.ctypes.data))
        return out[:self.num_nodes].copy()

    def preempt_explain_format(self, cells):
        """kube-scheduler's preemption sentence for one row of preempt_explain(): "preemption: 0/5 nodes are available: 3 Preemption is
        not helpful for scheduling, ..." (ykhost_preempt_explain_format; a pure function of the cells and the resource names — works
        without a device)."""
        c = np.ascontiguousarray(cells, dtype=np.int64)
        if c.shape != (PREEMPT_EXPLAIN_CELLS,):
            raise ValueError(f"preempt_explain_format takes one row of {PREEMPT_EXPLAIN_CELLS} cells")
        need = self._check(self._L.ykhost_preempt_explain_format(self._h, c.ctypes.data, None, 0))
        buf = C.create_string_buffer(need)
        self._check(self._L.ykhost_preempt_explain_format(self._h, c.ctypes.data, buf, need))
        return buf.value.decode()

    def preempt_explain_message(self, uid):
        """The Message of the Unschedulable condition with preemption on, for one ask by allocation key in one crossing
        (ykhost_preempt_explain_message): explain_format's sentence, a space, the preemption sentence. Raises UnsupportedAsk for an
        ask routed to the CPU manager, KeyError for an unknown pod."""
        buf = C.create_string_buffer(4096)
        rc = self._L.ykhost_preempt_explain_message(self._h, uid.encode(), buf, 4096)
        if rc == -13:
            raise UnsupportedAsk(buf.value.decode())
        if rc in (-10, -12):
            raise KeyError(buf.value.decode())
        self._check(rc)
        if rc > 4096:
            buf = C.create_string_buffer(rc)
            self._check(self._L.ykhost_preempt_explain_message(self._h, uid.encode(), buf, rc))
        return buf.value.decode()

    # ---- preemption headroom: copies of an ask per preemption level ------------------------------------------------------
    def preempt_headroom(self, pods=None, wants=None, pre_mask=None, filt_mask=None):
        """Per ask the copies the cluster takes per preemption LEVEL, reduced on the device (ykpred_preempt_headroom):
        np.int64[n, PREEMPT_HEADROOM_CELLS] — [PREEMPT_HEADROOM_COPIES + L] the copies once every pod of tiers < min(L, limit) is gone,
        [PREEMPT_HEADROOM_NODES + L] the nodes that take at least one, [PREEMPT_HEADROOM_VICTIMS + L] the pods of the fewest whole tiers
        that give each node those copies, [PREEMPT_HEADROOM_STATUS] (1 routed, 2 coupled: copies and victims -1), [PREEMPT_HEADROOM_LIMIT],
        [PREEMPT_HEADROOM_WANT], [PREEMPT_HEADROOM_LEVEL] the lowest level whose copies meet the want (-1: none). pods: ask indices or UIDs
        in any order, repeats allowed; None = every ask. wants: one int >= 1 per listed ask; None = 1 each. Always the allocation-phase
        lists; explicit masks go to the engine with the limits the host derives. Needs no evaluation and disturbs none."""
        if pods is None:
            count, ptr = self.num_pods, None
        else:
            idx = [p if isinstance(p, (int, np.integer)) else self.pod_index(p) for p in pods]
            arr = np.ascontiguousarray(idx, dtype=np.int32)
            count, ptr = len(arr), arr.ctypes.data
        wptr = None
        if wants is not None:
            warr = np.ascontiguousarray(list(wants), dtype=np.int64)
            if len(warr) != count:
                raise ValueError("preempt_headroom: one want per listed ask")
            wptr = warr.ctypes.data if count else None
        out = np.zeros((max(count, 1), PREEMPT_HEADROOM_CELLS), dtype=np.int64)
        if pre_mask is None and filt_mask is None:
            self._check(self._L.ykhost_preempt_headroom(self._h, count, ptr, wptr, out.ctypes.data))
        else:
            pre, filt = self._explicit_masks(True, pre_mask, filt_mask)
            limits = np.zeros(max(count, 1), dtype=np.int32)
            self._check(self._L.ykhost_preempt_limits(self._h, count, ptr, limits.ctypes.data))  # (syncs the tables and the reclaim table)
            if ptr is None:
                arr = np.arange(count, dtype=np.int32)
                ptr = arr.ctypes.data
            self._pcheck(self._P.ykpred_preempt_headroom(self.engine, count, ptr, limits.ctypes.data, wptr, pre, filt, out.ctypes.data))
        return out[:count].copy()

    def preempt_headroom_nodes(self, pod, pre_mask=None, filt_mask=None):
        """The copies of ONE ask (index or UID) on every node per level (ykpred_preempt_headroom_pod): np.int32[limit + 1, N], row L =
        the copies once every pod of tiers < L is gone; -1 everywhere for a coupled ask, 0 for a routed one. On a node-sharded manager:
        this shard's nodes."""
        p = int(pod if isinstance(pod, (int, np.integer)) else self.pod_index(pod))
        limit = np.zeros(1, dtype=np.int32)
        out = np.zeros((REACH_MAX_TIERS + 1) * max(self.num_nodes, 1), dtype=np.int32)
        if pre_mask is None and filt_mask is None:
            self._check(self._L.ykhost_preempt_headroom_nodes(self._h, p, out.ctypes.data, limit.ctypes.data))
        else:
            pre, filt = self._explicit_masks(True, pre_mask, filt_mask)
            arr = np.array([p], dtype=np.int32)
            self._check(self._L.ykhost_preempt_limits(self._h, 1, arr.ctypes.data, limit.ctypes.data))
            self._pcheck(self._P.ykpred_preempt_headroom_pod(self.engine, p, int(limit[0]), pre, filt, out.ctypes.data))
        rows = int(limit[0]) + 1
        return out[:rows * self.num_nodes].reshape(rows, self.num_nodes).copy()

    def preempt_headroom_by_key(self, uid, want=1):
        """One ask by allocation key and its want in one crossing (ykhost_preempt_headroom_by_key) → np.int64[PREEMPT_HEADROOM_CELLS].
        Raises UnsupportedAsk for a routed ask, KeyError for an unknown pod."""
        out = np.zeros(PREEMPT_HEADROOM_CELLS, dtype=np.int64)
        rc = self._L.ykhost_preempt_headroom_by_key(self._h, uid.encode(), int(want), out.ctypes.data)
        if rc == -13:
            raise UnsupportedAsk(self._L.ykhost_last_error(self._h).decode())
        if rc in (-10, -12):
            raise KeyError(uid)
        self._check(rc)
        return out

    # ---- preemption victims: the shortest victim prefix on every node ---------------------------------------------------
    def preempt_victims(self, pods=None, pre_mask=None, filt_mask=None):
        """Per ask the nodes by NEED, reduced on the device (ykpred_preempt_victims): np.int64[n, VICTIM_CELLS] — [VICTIM_FIT] nodes
        the ask fits as they stand, [VICTIM_OPEN] nodes it fits once the first need >= 1 pods of order(n) are gone, [VICTIM_NEVER]
        nodes no prefix opens, [VICTIM_STATUS] 1 for a routed ask, [VICTIM_LIMIT], [VICTIM_BEST_LEVEL], [VICTIM_BEST_NODE] (global
        index, -1: none), [VICTIM_BEST_NEED], [VICTIM_TOTAL] the sum of need over the open nodes. pods: ask indices or UIDs in any
        order, repeats allowed; None = every ask. Always the allocation-phase lists; explicit masks go to the engine with the limits
        the host derives. Needs no evaluation and disturbs none."""
        if pods is None:
            count, ptr = self.num_pods, None
        else:
            idx = [p if isinstance(p, (int, np.integer)) else self.pod_index(p) for p in pods]
            arr = np.ascontiguousarray(idx, dtype=np.int32)
            count, ptr = len(arr), arr.ctypes.data
        out = np.zeros((max(count, 1), VICTIM_CELLS), dtype=np.int64)
        if pre_mask is None and filt_mask is None:
            self._check(self._L.ykhost_preempt_victims(self._h, count, ptr, out.ctypes.data))
        else:
            pre, filt = self._explicit_masks(True, pre_mask, filt_mask)
            self.victim_table(planes=False)   # (syncs the tables, the reclaim and the victim table)
            limits = np.zeros(max(count, 1), dtype=np.int32)
            self._check(self._L.ykhost_preempt_limits(self._h, count, ptr, limits.ctypes.data))
            if ptr is None:
                arr = np.arange(count, dtype=np.int32)
                ptr = arr.ctypes.data
            self._pcheck(self._P.ykpred_preempt_victims(self.engine, count, ptr, limits.ctypes.data, pre, filt, out.ctypes.data))
        return out[:count].copy()

    def preempt_victims_nodes(self, pod):
        """need of ONE ask (index or UID) on every node (ykpred_preempt_victims_pod): np.int32[N] — 0 fits as it stands, k >= 1 the
        first k pods of victim_list(node) must go, -1 never. On a node-sharded manager: this shard's nodes."""
        p = pod if isinstance(pod, (int, np.integer)) else self.pod_index(pod)
        out = np.zeros(max(self.num_nodes, 1), dtype=np.int32)
        self._check(self._L.ykhost_preempt_victims_nodes(self._h, int(p), out.ctypes.data))
        return out[:self.num_nodes].copy()

    def victim_list(self, node, limit):
        """The uids of order(node) — the node's pods in a tier, by (priority, uid) ascending — in tiers < limit
        (ykhost_victim_list; works without a device): the first `need` of them are the victims."""
        n = node if isinstance(node, (int, np.integer)) else self.node_index(node)
        count = C.c_int32(0)
        size = 1 << 12
        while True:
            buf = C.create_string_buffer(size)
            self._check(self._L.ykhost_victim_list(self._h, int(n), int(limit), C.addressof(buf), size, C.addressof(count)))
            uids = [u.decode() for u in buf.raw.split(b"\0")[:count.value]]
            if all(uids) or size > (1 << 28):
                return uids
            size *= 8

    def preempt_victims_by_key(self, uid):
        """One ask by allocation key in one crossing (ykhost_preempt_victims_by_key) → (np.int64[VICTIM_CELLS], best node name or "",
        the uids of its victim prefix). Raises UnsupportedAsk for a routed ask, KeyError for an unknown pod."""
        out = np.zeros(VICTIM_CELLS, dtype=np.int64)
        name = C.create_string_buffer(512)
        uids = C.create_string_buffer(1 << 16)
        rc = self._L.ykhost_preempt_victims_by_key(self._h, uid.encode(), out.ctypes.data, name, 512, C.addressof(uids), 1 << 16)
        if rc == -13:
            raise UnsupportedAsk(self._L.ykhost_last_error(self._h).decode())
        if rc in (-10, -12):
            raise KeyError(uid)
        self._check(rc)
        victims = [u.decode() for u in uids.raw.split(b"\0")[:int(out[VICTIM_BEST_NEED])] if u] if name.value else []
        return out, name.value.decode(), victims

    # ---- preemption round: conflict-resolved victim plans for a list of asks ----------------------------------------------
    def preempt_round(self, pods=None, pre_mask=None, filt_mask=None):
        """Victim plans for a LIST of asks, each under the state the earlier asks of the list left behind (ykpred_preempt_round) →
        (np.int64[n, PREEMPT_ROUND_CELLS], np.int64[8] summary = asks per outcome 0..4, victims in all, distinct nodes touched, 0).
        pods: ask indices or UIDs IN ORDER, a repeat is one more copy; None = every ask in index order. The victims of ask i are
        victim_range(node, from, extra). Nothing in the mirror or on the device changes; two calls in a row give equal answers.
        Explicit masks go to the engine with the limits the host derives."""
        if pods is None:
            count, ptr = self.num_pods, None
        else:
            idx = [p if isinstance(p, (int, np.integer)) else self.pod_index(p) for p in pods]
            arr = np.ascontiguousarray(idx, dtype=np.int32)
            count, ptr = len(arr), arr.ctypes.data
        out = np.zeros((max(count, 1), PREEMPT_ROUND_CELLS), dtype=np.int64)
        summary = np.zeros(8, dtype=np.int64)
        if pre_mask is None and filt_mask is None:
            self._check(self._L.ykhost_preempt_round(self._h, count, ptr, out.ctypes.data, summary.ctypes.data))
        else:
            pre, filt = self._explicit_masks(True, pre_mask, filt_mask)
            self.victim_table(planes=False)   # (syncs the tables, the reclaim and the victim table)
            limits = np.zeros(max(count, 1), dtype=np.int32)
            self._check(self._L.ykhost_preempt_limits(self._h, count, ptr, limits.ctypes.data))
            if ptr is None:
                arr = np.arange(count, dtype=np.int32)
                ptr = arr.ctypes.data
            self._pcheck(self._P.ykpred_preempt_round(self.engine, count, ptr, limits.ctypes.data, pre, filt, out.ctypes.data, summary.ctypes.data))
        return out[:count].copy(), summary

    # ---- preemption round with live topology histograms: coupled asks take their turn ----------------------------------------
    def preempt_round_live(self, pods=None, pre_mask=None, filt_mask=None, histograms=False):
        """preempt_round for lists that hold asks with a hard topology spread or required pod (anti-)affinity
        (ykpred_preempt_round_live): no ask is settled as coupled, every ask takes its turn against the topology histograms as the
        earlier placements and the earlier victims left them → (cells, summary) as preempt_round, summary[7] = (turn, constraint)
        pairs that moved a histogram cell; with histograms=True also (np.int32[layout().spread_cells] counts, np.int32[G] minima): the
        round-local histograms after the last turn. Nothing in the mirror or on the device changes. Explicit masks go to the engine
        with the limits the host derives."""
        if pods is None:
            count, ptr = self.num_pods, None
        else:
            idx = [p if isinstance(p, (int, np.integer)) else self.pod_index(p) for p in pods]
            arr = np.ascontiguousarray(idx, dtype=np.int32)
            count, ptr = len(arr), arr.ctypes.data
        out = np.zeros((max(count, 1), PREEMPT_ROUND_CELLS), dtype=np.int64)
        summary = np.zeros(8, dtype=np.int64)
        dims = np.zeros(2, dtype=np.int64)
        counts, minima = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        if pre_mask is None and filt_mask is None:
            for _ in range(2):   # (the sizes come back with the first answer; the round starts from the same state each call)
                self._check(self._L.ykhost_preempt_round_live(self._h, count, ptr, out.ctypes.data, summary.ctypes.data, counts.ctypes.data, len(counts),
                                                              minima.ctypes.data, len(minima), dims.ctypes.data))
                if not histograms or (dims[0] <= len(counts) and dims[1] <= len(minima)):
                    break
                counts, minima = np.zeros(max(int(dims[0]), 1), dtype=np.int32), np.zeros(max(int(dims[1]), 1), dtype=np.int32)
        else:
            pre, filt = self._explicit_masks(True, pre_mask, filt_mask)
            self.victim_effects(planes=False)   # (syncs the tables, the reclaim table, the victim table and its effects plane)
            self._check(self._L.ykhost_preempt_round_live(self._h, 0, None, out.ctypes.data, summary.ctypes.data, None, 0, None, 0, dims.ctypes.data))
            limits = np.zeros(max(count, 1), dtype=np.int32)
            self._check(self._L.ykhost_preempt_limits(self._h, count, ptr, limits.ctypes.data))
            if ptr is None:
                arr = np.arange(count, dtype=np.int32)
                ptr = arr.ctypes.data
            self._pcheck(self._P.ykpred_histogram_dims(self.engine, dims.ctypes.data))
            counts, minima = np.zeros(max(int(dims[0]), 1), dtype=np.int32), np.zeros(max(int(dims[1]), 1), dtype=np.int32)
            self._pcheck(self._P.ykpred_preempt_round_live(self.engine, count, ptr, limits.ctypes.data, pre, filt, out.ctypes.data, summary.ctypes.data,
                                                           counts.ctypes.data, minima.ctypes.data))
        if histograms:
            return out[:count].copy(), summary, counts[:int(dims[0])].copy(), minima[:int(dims[1])].copy()
        return out[:count].copy(), summary

    def preempt_round_live_by_keys(self, uids):
        """preempt_round_by_keys over the live round, ONE crossing (ykhost_preempt_round_live_by_keys)."""
        keys = [u.encode() for u in uids]
        arr = (C.c_char_p * max(len(keys), 1))(*keys)
        return self._round_by_keys(lambda *a: self._L.ykhost_preempt_round_live_by_keys(self._h, len(keys), C.addressof(arr), *a), len(keys))

    def preempt_gang_live(self, uid, want):
        """`want` copies of one ask — a gang with a zone spread, a "one per host" rule, workers beside their driver — as a live round
        (ykhost_preempt_gang_live_by_key) → as preempt_round_by_keys."""
        return self._round_by_keys(lambda *a: self._L.ykhost_preempt_gang_live_by_key(self._h, uid.encode(), int(want), *a), int(want))

    def victim_effects(self, planes=True):
        """The victim-effects plane as the mirror keeps it (ykhost_victim_effects; works without a device) → dict(class_col
        np.int32[KS] — the column of a selector class or -1 —, cum np.int32[KA, P] — prefix sums of the victims' contributions within
        each segment of victim_table() —, derived, patches)."""
        dims = np.zeros(5, dtype=np.int32)
        self._check(self._L.ykhost_victim_effects(self._h, dims.ctypes.data, None, None))
        if not planes:
            return None
        KS, KA, P = (int(x) for x in dims[:3])
        col, cum = np.zeros(KS, dtype=np.int32), np.zeros((KA, P), dtype=np.int32)
        pad = [np.zeros(1, dtype=np.int32) if a.size == 0 else a for a in (col, cum)]
        self._check(self._L.ykhost_victim_effects(self._h, dims.ctypes.data, *(a.ctypes.data for a in pad)))
        return dict(class_col=col, cum=cum, derived=int(dims[3]), patches=int(dims[4]))

    def _round_by_keys(self, call, count):
        names_len, uids_len = 64 * count + 256, 64 * count + (1 << 12)
        while True:
            out = np.zeros((max(count, 1), PREEMPT_ROUND_CELLS), dtype=np.int64)
            summary = np.zeros(8, dtype=np.int64)
            need = np.zeros(2, dtype=np.int64)
            names, uids = C.create_string_buffer(names_len), C.create_string_buffer(uids_len)
            rc = call(out.ctypes.data, summary.ctypes.data, C.addressof(names), names_len, C.addressof(uids), uids_len, need.ctypes.data)
            if rc in (-10, -12):
                raise KeyError(self._L.ykhost_last_error(self._h).decode())
            self._check(rc)
            if need[0] <= names_len and need[1] <= uids_len:
                break
            names_len, uids_len = int(need[0]) + 1, int(need[1]) + 1   # (the round starts from zero state each call: asking again is exact)
        node = [u.decode() for u in names.raw[:int(need[0])].split(b"\0")[:count]]
        flat = [u.decode() for u in uids.raw[:int(need[1])].split(b"\0")[:-1]]
        victims, at = [], 0
        for i in range(count):
            k = int(out[i, PREEMPT_ROUND_EXTRA]) if node[i] else 0
            victims.append(flat[at:at + k])
            at += k
        return out[:count].copy(), summary, node, victims

    def preempt_round_by_keys(self, uids):
        """The round for asks named by allocation key, ONE crossing (ykhost_preempt_round_by_keys) → (cells, summary, node names — "" where
        the ask went nowhere —, per ask the uids of its victims order(node)[from .. from + extra)). KeyError for a key that names no ask."""
        keys = [u.encode() for u in uids]
        arr = (C.c_char_p * max(len(keys), 1))(*keys)
        return self._round_by_keys(lambda *a: self._L.ykhost_preempt_round_by_keys(self._h, len(keys), C.addressof(arr), *a), len(keys))

    def preempt_gang(self, uid, want):
        """`want` copies of one ask as a round (ykhost_preempt_gang_by_key): where each copy goes and at whose cost → as
        preempt_round_by_keys. summary[0] + summary[1] == min(want, preempt_headroom copies at the ask's limit)."""
        return self._round_by_keys(lambda *a: self._L.ykhost_preempt_gang_by_key(self._h, uid.encode(), int(want), *a), int(want))

    def victim_range(self, node, start, count):
        """The uids of order(node)[start .. start + count) (ykhost_victim_range; works without a device)."""
        n = node if isinstance(node, (int, np.integer)) else self.node_index(node)
        got, need = C.c_int32(0), C.c_int64(0)
        self._check(self._L.ykhost_victim_range(self._h, int(n), int(start), int(count), None, 0, C.addressof(got), C.addressof(need)))
        buf = C.create_string_buffer(need.value + 1)
        self._check(self._L.ykhost_victim_range(self._h, int(n), int(start), int(count), C.addressof(buf), need.value + 1, C.addressof(got), C.addressof(need)))
        return [u.decode() for u in buf.raw[:need.value].split(b"\0")[:got.value]]

    def victim_table(self, planes=True):
        """The victim table as the mirror keeps it — patched segment by segment, not derived afresh (ykhost_victim_table; works
        without a device) → dict(seg_base np.int32[N], seg_cap np.int32[N], tier_end np.int32[T, N], cum np.int64[R, P], ports_after
        np.uint64[KP, P], derived, patches)."""
        dims = np.zeros(5, dtype=np.int32)
        self._check(self._L.ykhost_victim_table(self._h, dims.ctypes.data, None, None, None, None, None))
        if not planes:
            return None
        T, R, KP, N, P = (int(x) for x in dims)
        arrays = [np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32), np.zeros((T, N), dtype=np.int32), np.zeros((R, P), dtype=np.int64),
                  np.zeros((KP, P), dtype=np.uint64)]
        pad = [np.zeros(1, dtype=a.dtype) if a.size == 0 else a for a in arrays]
        self._check(self._L.ykhost_victim_table(self._h, dims.ctypes.data, *(a.ctypes.data for a in pad)))
        stats = np.zeros(2, dtype=np.int64)
        self._check(self._L.ykhost_victim_stats(self._h, stats.ctypes.data))
        return dict(zip(("seg_base", "seg_cap", "tier_end", "cum", "ports_after"), arrays), derived=int(stats[0]), patches=int(stats[1]))

    def reclaim_table(self):
        """The reclaim planes the mirror derives from the pods on its nodes (ykhost_reclaim_table; works without a device) →
        (requests np.int64[T, R, N], pods np.int32[T, N], ports_after np.uint64[T, KP, N])."""
        dims = np.zeros(4, dtype=np.int32)
        self._check(self._L.ykhost_reclaim_table(self._h, dims.ctypes.data, None, None, None))
        T, R, KP, N = (int(x) for x in dims)
        req = np.zeros((T, R, N), dtype=np.int64)
        cnt = np.zeros((T, N), dtype=np.int32)
        ports = np.zeros((T, KP, N), dtype=np.uint64)
        pad = [np.zeros(1, dtype=a.dtype) if a.size == 0 else a for a in (req, cnt, ports)]
        self._check(self._L.ykhost_reclaim_table(self._h, dims.ctypes.data, *(a.ctypes.data for a in pad)))
        return req, cnt, ports

    def headroom_domains(self, pods=None, label_key=None, node_group=None, num_groups=None, want=None, groups=False, pre_mask=None,
                         filt_mask=None):
        """Headroom per topology domain (ykpred_headroom_groups): which zone, rack or host still takes `want` copies of an ask.
        Either label_key (the groups are the bytewise-sorted values of that node label in the mirror, domain_values(label_key)
        names them; allocation-phase lists) or an explicit node_group column (np.int32[N] of ids in [-1, num_groups), -1 = in no
        group), which goes straight to the engine. pods: ask indices or UIDs, any order, repeats allowed; None = every ask. want: one
        int or one per listed ask; None = 1. → np.int64[n, GROUP_SUMMARY], and with groups=True also np.int64[n, G + 1, GROUP_CELLS]
        (row G: the nodes of no group)."""
        if (label_key is None) == (node_group is None):
            raise ValueError("headroom_domains takes either label_key or node_group")
        if pods is None:
            idx = np.arange(self.num_pods, dtype=np.int32)
        else:
            idx = np.ascontiguousarray([p if isinstance(p, (int, np.integer)) else self.pod_index(p) for p in pods], dtype=np.int32)
        count = len(idx)
        if want is None:
            wants = None
        else:
            wants = np.ascontiguousarray(np.broadcast_to(np.asarray(want, dtype=np.int64), (count,)))
        wptr = None if wants is None else wants.ctypes.data
        summary = np.zeros((max(count, 1), GROUP_SUMMARY), dtype=np.int64)
        if label_key is not None:
            if pre_mask is not None or filt_mask is not None:
                raise ValueError("explicit plugin masks go with an explicit node_group")
            G = len(self.domain_values(label_key)) if groups else 0
            rows = np.zeros((max(count, 1), G + 1, GROUP_CELLS), dtype=np.int64) if groups else None
            rc = self._L.ykhost_headroom_domains(self._h, count, idx.ctypes.data, wptr, label_key.encode(), summary.ctypes.data,
                                                 rows.ctypes.data if groups else None, rows.size if groups else 0)
            if rc < 0:
                self._check(rc)
        else:
            self.sync()
            column = np.ascontiguousarray(node_group, dtype=np.int32)
            if len(column) != self.num_nodes:
                raise ValueError("node_group holds one id per node")
            G = int(num_groups if num_groups is not None else (column.max() + 1 if len(column) else 1))
            pre, filt = self._explicit_masks(True, pre_mask, filt_mask)
            rows = np.zeros((max(count, 1), max(G, 0) + 1, GROUP_CELLS), dtype=np.int64) if groups else None
            self._pcheck(self._P.ykpred_headroom_groups(self.engine, count, idx.ctypes.data, wptr, G, column.ctypes.data, pre, filt,
                                                        summary.ctypes.data, rows.ctypes.data if groups else None))
        return (summary[:count].copy(), rows[:count].copy()) if groups else summary[:count].copy()

    def domain_values(self, label_key):
        """The values of a node label key in group-id order (bytewise sorted): what the ids of headroom_domains(label_key=...) name."""
        need = self._L.ykhost_domain_values(self._h, label_key.encode(), None, 0)
        if need < 0:
            self._check(int(need))
        buf = C.create_string_buffer(int(need))
        self._L.ykhost_domain_values(self._h, label_key.encode(), buf, need)
        return json.loads(buf.value.decode())

    def headroom_spread(self, pods=None, pre_mask=None, filt_mask=None):
        """Headroom of asks with ONE hard topology spread constraint (ykpred_headroom_spread) — those headroom() reports as coupled:
        np.int64[n, SPREAD_HEADROOM_CELLS]. pods: ask indices or UIDs in any order, repeats allowed; None = every ask. Allocation-phase
        lists; explicit masks go to the engine directly, like headroom. Needs no evaluation and disturbs none. [3] is the status: 0
        computed, 1 routed, 2 still coupled (total = max = -1), 3 not coupled under these lists (headroom() answers)."""
        return self._headroom_list("headroom_spread", SPREAD_HEADROOM_CELLS, pods, pre_mask, filt_mask, self.sync)

    def headroom_spread_domains(self, pod, pre_mask=None, filt_mask=None):
        """The per-domain rows behind headroom_spread for ONE ask (index or UID): (cells np.int64[SPREAD_HEADROOM_CELLS], rows
        np.int64[D, SPREAD_ROW_CELLS] = cnt, cap, nodes, copies per domain of the constraint's key, values) — values are the domains'
        label values in id order (None with explicit masks, which go to the engine directly: one run for the cells, one for the rows,
        the table sized by headroom_spread_constraint). At a status other than 0 the rows are empty."""
        p = int(pod if isinstance(pod, (int, np.integer)) else self.pod_index(pod))
        cells = np.zeros(SPREAD_HEADROOM_CELLS, dtype=np.int64)
        if pre_mask is None and filt_mask is None:
            cap, vlen = 64, 4096
            while True:
                rows = np.zeros((cap, SPREAD_ROW_CELLS), dtype=np.int64)
                buf = C.create_string_buffer(vlen)
                rc = self._check(self._L.ykhost_headroom_spread_domains(self._h, p, cells.ctypes.data, rows.ctypes.data, cap, buf, vlen))
                if rc > cap:  # (fewer rows than domains: the size needed came back)
                    cap = rc
                elif rc > 0 and not buf.value.endswith(b"]"):  # (the value list was cut)
                    vlen *= 16
                else:
                    return cells, rows[:rc].copy(), json.loads(buf.value.decode())
        where = self.headroom_spread_constraint(p, pre_mask=pre_mask, filt_mask=filt_mask)  # (the row's size: no launch)
        pre, filt = self._explicit_masks(True, pre_mask, filt_mask)
        one = np.array([p], dtype=np.int32)
        self._pcheck(self._P.ykpred_headroom_spread(self.engine, 1, one.ctypes.data, pre, filt, cells.ctypes.data))
        if cells[3] != 0:
            return cells, np.zeros((0, SPREAD_ROW_CELLS), dtype=np.int64), None
        count = C.c_int32(0)
        rows = np.zeros((max(int(where[3]), 1), SPREAD_ROW_CELLS), dtype=np.int64)
        self._pcheck(self._P.ykpred_headroom_spread_pod(self.engine, p, pre, filt, len(rows), rows.ctypes.data, C.byref(count)))
        return cells, rows[:count.value].copy(), None

    def headroom_affinity(self, pods=None, pre_mask=None, filt_mask=None):
        """Headroom of asks with required pod (anti-)affinity (ykpred_headroom_affinity) — "one executor per host" and its kin, which
        headroom() reports as coupled: np.int64[n, AFFINITY_HEADROOM_CELLS]. pods: ask indices or UIDs in any order, repeats allowed;
        None = every ask. Allocation-phase lists; explicit masks go to the engine directly (the spec effects must then be uploaded:
        any call with the default lists does that). Needs no evaluation and disturbs none. [3] is the status: 0 computed, 1 routed,
        2 still coupled (total = max = -1), 3 no inter-pod affinity constraint is live, 4 bootstrap (total = -1, per-domain rows valid)."""
        # (an empty list: syncs and uploads the spec effects)
        upload = lambda: self._check(self._L.ykhost_headroom_affinity(self._h, 0, None, None))
        return self._headroom_list("headroom_affinity", AFFINITY_HEADROOM_CELLS, pods, pre_mask, filt_mask, upload)

    def headroom_affinity_domains(self, pod, pre_mask=None, filt_mask=None):
        """The per-domain rows behind headroom_affinity for ONE ask (index or UID): (cells np.int64[AFFINITY_HEADROOM_CELLS], rows
        np.int64[D + 1, SPREAD_ROW_CELLS] = cnt, cap, nodes, copies per domain of the ask's key with the OUTSIDE row — the nodes without
        the key — last, values) — values are the domains' label values in id order (None with explicit masks, which go to the engine
        directly). At a status other than 0 and 4 the rows are empty."""
        p = int(pod if isinstance(pod, (int, np.integer)) else self.pod_index(pod))
        cells = np.zeros(AFFINITY_HEADROOM_CELLS, dtype=np.int64)
        if pre_mask is None and filt_mask is None:
            cap, vlen = 64, 4096
            while True:
                rows = np.zeros((cap + 1, SPREAD_ROW_CELLS), dtype=np.int64)
                buf = C.create_string_buffer(vlen)
                rc = self._check(self._L.ykhost_headroom_affinity_domains(self._h, p, cells.ctypes.data, rows.ctypes.data, cap, buf, vlen))
                if rc > cap:  # (fewer rows than domains: the size needed came back)
                    cap = rc
                elif rc > 0 and not buf.value.endswith(b"]"):  # (the value list was cut)
                    vlen *= 16
                elif cells[3] not in (0, 4):
                    return cells, np.zeros((0, SPREAD_ROW_CELLS), dtype=np.int64), []
                else:
                    return cells, rows[:rc + 1].copy(), json.loads(buf.value.decode())
        self._check(self._L.ykhost_headroom_affinity(self._h, 0, None, None))  # (an empty list: syncs and uploads the spec effects)
        pre, filt = self._explicit_masks(True, pre_mask, filt_mask)
        one = np.array([p], dtype=np.int32)
        self._pcheck(self._P.ykpred_headroom_affinity(self.engine, 1, one.ctypes.data, pre, filt, cells.ctypes.data))
        if cells[3] not in (0, 4):
            return cells, np.zeros((0, SPREAD_ROW_CELLS), dtype=np.int64), None
        count = C.c_int32(0)
        rows = np.zeros((1, SPREAD_ROW_CELLS), dtype=np.int64)
        rc = self._P.ykpred_headroom_affinity_pod(self.engine, p, pre, filt, 0, rows.ctypes.data, C.byref(count))
        if rc != 0 and count.value > 0:  # (the size came back)
            rows = np.zeros((count.value + 1, SPREAD_ROW_CELLS), dtype=np.int64)
            rc = self._P.ykpred_headroom_affinity_pod(self.engine, p, pre, filt, count.value, rows.ctypes.data, C.byref(count))
        self._pcheck(rc)
        return cells, rows[:count.value + 1].copy(), None

    def headroom_affinity_constraint(self, pod, pre_mask=None, filt_mask=None):
        """Where the anti-affinity rows behind an ask's (index or UID) cnt column lie in the topology histograms
        (ykpred_headroom_affinity_constraint): np.int32[16] = status from the tables alone (bootstrap is not seen), topology key index,
        mode, domains, number of live anti rows on the key, then the first cell of each in layout().spread_counts. No device work."""
        p = int(pod if isinstance(pod, (int, np.integer)) else self.pod_index(pod))
        self._check(self._L.ykhost_headroom_affinity(self._h, 0, None, None))  # (an empty list: syncs and uploads the spec effects)
        pre, filt = self._explicit_masks(True, pre_mask, filt_mask)
        out = np.zeros(16, dtype=np.int32)
        self._pcheck(self._P.ykpred_headroom_affinity_constraint(self.engine, p, pre, filt, out.ctypes.data))
        return out

    def headroom_spread_constraint(self, pod, pre_mask=None, filt_mask=None):
        """Where the one live spread constraint of an ask (index or UID) lies in the topology histograms
        (ykpred_headroom_spread_constraint): np.int32[8] = status from the tables alone, topology key index, first cell and number of
        cells of its row in layout().spread_counts / spread_present, maxSkew, minDomains, self-match, flags. No device work."""
        p = int(pod if isinstance(pod, (int, np.integer)) else self.pod_index(pod))
        self.sync()
        pre, filt = self._explicit_masks(True, pre_mask, filt_mask)
        out = np.zeros(8, dtype=np.int32)
        self._pcheck(self._P.ykpred_headroom_spread_constraint(self.engine, p, pre, filt, out.ctypes.data))
        return out

    def round_info(self):
        """ykpred_get_round_info: how the allocation rounds so far were decided (in batches / by the sequential kernel)."""
        out = np.zeros(6, dtype=np.int64)
        self._pcheck(self._P.ykpred_get_round_info(self.engine, out.ctypes.data))
        return dict(zip(("rounds_batched", "batched_asks", "batches", "exchanges", "rounds_sequential", "sequential_asks"), (int(v) for v in out)))

    def counters(self):
        out = np.zeros(6, dtype=np.int64)
        self._pcheck(self._P.ykpred_get_counters(self.engine, out.ctypes.data))
        return dict(zip(["full_evals", "node_patches", "row_patches", "queries", "gathers", "uploads"], out.tolist()))

    def timing(self):
        t = _ffi.YkpredTiming()
        self._pcheck(self._P.ykpred_last_timing(self.engine, C.byref(t)))
        return {"total_ms": t.total_ms,
                "kernels": [(t.kernel_name[i].decode(), t.kernel_ms[i]) for i in range(t.num_kernels)]}

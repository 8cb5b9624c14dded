"""yunikorn-k8shim_amd — MI355X-native batched predicate engine for the yunikorn-k8shim hot path.

Only what the path needs lives here: csrc/engine (HIP kernels + the C ABI of include/ykpred.h), csrc/host (the
C++ stand-in for the Go shim side, include/ykhost.h) and thin ctypes bindings. See DESIGN.md.
The package name contains a hyphen; import it with importlib.import_module("yunikorn-k8shim_amd").
"""
from . import build  # noqa: F401
from .predicate_manager import (ALL_PLUGINS, EXPLAIN_BINS, EXPLAIN_FIT, EXPLAIN_REASON0, EXPLAIN_RESOURCE0,  # noqa: F401
                                EXPLAIN_UNSUPPORTED, GROUP_CELLS, GROUP_LDS_MAX_GROUPS, GROUP_SUMMARY, HEADROOM_BY_PORT, HEADROOM_BY_RESOURCE0, HEADROOM_BY_SLOTS, HEADROOM_CELLS,
                                HEADROOM_MAX, HEADROOM_NODES, HEADROOM_STATUS, HEADROOM_TOTAL, PLUGIN_BITS, SPREAD_HEADROOM_CELLS, SPREAD_ROW_CELLS,
                                AFFINITY_HEADROOM_CELLS,
                                REACH_BEST_LEVEL, REACH_BEST_NODE, REACH_BEST_PODS, REACH_CELLS, REACH_LIMIT, REACH_MAX_TIERS, REACH_NEVER, REACH_STATUS,
                                PREEMPT_HEADROOM_CELLS, PREEMPT_HEADROOM_COPIES, PREEMPT_HEADROOM_LEVEL, PREEMPT_HEADROOM_LIMIT, PREEMPT_HEADROOM_NODES,
                                PREEMPT_HEADROOM_STATUS, PREEMPT_HEADROOM_VICTIMS, PREEMPT_HEADROOM_WANT,
                                PREEMPT_EXPLAIN_CELLS, PREEMPT_EXPLAIN_ELIGIBLE, PREEMPT_EXPLAIN_FIT, PREEMPT_EXPLAIN_LEVEL_NEVER, PREEMPT_EXPLAIN_LEVEL_SHIFT,
                                PREEMPT_EXPLAIN_LIMIT, PREEMPT_EXPLAIN_NOT_ENOUGH, PREEMPT_EXPLAIN_NO_VICTIMS, PREEMPT_EXPLAIN_OPENED, PREEMPT_EXPLAIN_PORTS,
                                PREEMPT_EXPLAIN_REASON0, PREEMPT_EXPLAIN_RESOURCE0, PREEMPT_EXPLAIN_STATUS, PREEMPT_EXPLAIN_UNRESOLVABLE,
                                PREEMPT_EXPLAIN_UNSUPPORTED, PREEMPT_EXPLAIN_WASTED,
                                VICTIM_BEST_LEVEL, VICTIM_BEST_NEED, VICTIM_BEST_NODE, VICTIM_CELLS, VICTIM_FIT, VICTIM_LIMIT, VICTIM_NEVER, VICTIM_OPEN,
                                VICTIM_STATUS, VICTIM_TOTAL,
                                PREEMPT_ROUND_CELLS, PREEMPT_ROUND_EXTRA, PREEMPT_ROUND_FROM, PREEMPT_ROUND_LEVEL, PREEMPT_ROUND_LIMIT,
                                PREEMPT_ROUND_NODE, PREEMPT_ROUND_OPEN, PREEMPT_ROUND_OUTCOME, PREEMPT_ROUND_TOTAL,
                                GpuPredicateManager,
                                PredicateError, UnsupportedAsk, plugin_mask)

build_all = build.build_all

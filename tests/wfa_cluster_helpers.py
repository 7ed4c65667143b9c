"""Shared by tests/test_wfa_cluster_cases.py and tests/test_gpu_wfa_cluster_edges.py: the cases of tests/wfa_cluster_cases.py as inputs
of cluster.wfa_cluster, and the CPU oracle's answer for each, computed once per process."""
import oracle_lib as O
import wfa_cluster_cases as W
from vcfdist_amd import cluster as K

DEFINED = [c for c in W.TABLE if not c.declare.get("undefined")]
_RUNS = {}


def hap_of(case):
    return K.HapSeq([v[0] for v in case.variants], [v[1] for v in case.variants], [v[2] for v in case.variants], [v[3] for v in case.variants])


def oracle_run(case, itrs, reach_min_gap=10):
    """-> (Clusters, stats) of oracle/wfa_oracle.cpp"""
    key = (case.name, itrs, reach_min_gap)
    if key not in _RUNS:
        x, o, e = case.pen
        _RUNS[key] = K.wfa_cluster(hap_of(case), case.ctg, sub=x, open=o, extend=e, max_cluster_itrs=itrs, reach_min_gap=reach_min_gap,
                                   L=O.lib(), prefix="vco")
    return _RUNS[key]

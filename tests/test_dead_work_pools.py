"""Set-up of tests/test_gpu_dead_work_paths.py, checked on the CPU with the oracle (oracle/orc.py) at the NodeLimit the GPU test uses: every pool
branches, so that bound changes are made at all; among the pools are instances with more than 20 nodes and node-limited ones, so that stacks are deep
and are unwound (s_set_bounds_list).  The oracle's search is not the GPU's node for node; the GPU test repeats the check on its own counts.  The one pool
without a restatement here is P35 with uploaded fixings, starts and cutoffs (tests/test_gpu_history.py anchors it against HiGHS): GPU counts only."""
import pytest

import _dead_work as dw


def _check(pool, max_nodes, tag, idx=None, deep=False, limited=False):
    nodes, nlim = pool.oracle_nodes(max_nodes, idx)
    print("%s NodeLimit %d: nodes %s, node-limited %d" % (tag, max_nodes, nodes.tolist(), nlim))
    assert nodes.sum() > len(nodes), (tag, "the pool does not branch", nodes.tolist())
    if deep:
        assert nodes.max() > 20, (tag, nodes.tolist())
    if limited:
        assert nlim >= 1, (tag, nodes.tolist(), nlim)


def test_p35():
    _check(dw.p35(), dw.GENEROUS["max_nodes"], "P35", deep=True)


def test_p35_node_limit_of_three():
    _check(dw.p35(), 3, "P35", limited=True)


def test_p35_even_n():
    _check(dw.p35(N=6), dw.GENEROUS["max_nodes"], "P35 N_tilde 6")


def test_p35_quadratic_cost():
    _check(dw.p35("quadratic"), dw.GENEROUS["max_nodes"], "P35 MIQP")


def test_cfg2():
    """cfg2 x64 at NodeLimit 50 branches but stays shallow (12 nodes at most): the deep stacks are cfg3's and P35's"""
    _check(dw.medium("cfg2", 64), 50, "cfg2")


@pytest.mark.parametrize("max_nodes", (50, 800))
def test_cfg3_hard_instances(max_nodes):
    _check(dw.medium("cfg3", 64), max_nodes, "cfg3", idx=dw.CFG3_HARD, deep=True, limited=True)


def test_cfg3_multi_model():
    _check(dw.medium("cfg3", 4, 3), 30, "cfg3 three models")


def test_cfg3_quadratic_cost():
    _check(dw.medium("cfg3", 8, 1, True), 10, "cfg3 MIQP")

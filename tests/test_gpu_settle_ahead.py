"""The selection commit kernel's candidates settled AHEAD (kb_commit_sel.hip: settle(true)), against the oracle.  Needs a real MI355X: -m gpu.

While run m - 1 is being selected, the prep wave of run m settles its candidates on the assumption that run m - 1 takes every candidate of
its own: it must drop every entry it fetched whose node is one of run m - 1's candidates — none of them is in the dirty bitmap yet.  The
sessions here are built so that the fetched entries of a run BEGIN with the candidates of the run in front:

  * one queue; tiers priority + gang, then predicates + nodeorder (no drf, no proportion): a gang job whose minAvailable equals its size is
    popped to its end before the next job (allocate.go:129-193), and the jobs come in priority order — A, B, C;
  * R = 2, 128 empty nodes whose allocatable falls strictly with the node index, memory = cpu * 2^22 on every node.  Under the default
    weights (leastrequested 1, balancedresource 1) a shape's score cannot rise with the index, and equal scores go to the lower index
    (scheduler_helper.go:188-208 with the canonical tie-break): every shape's candidate list starts 0, 1, 2, ...;
  * A, B and C ask for three different requests.  A's request is an eighth of a node, so a node's score for A falls with A's first pod on
    it and A's rows take the nodes 0 .. |A| - 1, one each: they are run A's candidates, and B's list starts with exactly them.

Every case first holds its session to that description with the oracle alone (A's rows consecutive and on distinct nodes, B's first
choices at load time are A's nodes), then compares the engine with the oracle: decisions in order, bind set, float64 node state.  Under
the selection kernel a case whose A has two rows or more must have formed a multi-row run (kb_stats.select_runs_clean / _shots)."""
import importlib

import numpy as np
import pytest

kbm = importlib.import_module("kube-batch_amd")
engine = importlib.import_module("kube-batch_amd.engine")
conf, snapmod = kbm.conf, kbm.snapshot

pytestmark = pytest.mark.gpu

N_NODES = 128
CONF = """
actions: "allocate"
tiers:
- plugins:
  - name: priority
  - name: gang
- plugins:
  - name: predicates
  - name: nodeorder
"""

MEM_PER_MILLI = 1 << 22   # bytes of memory per milli-cpu of a node: 32 cores go with 128 GiB


def node_cpu(i):
    return 32000 - 10 * i   # milli-cpu, strictly falling


REQ_A = (4000, 4000 * MEM_PER_MILLI)   # an eighth of node 0, in the nodes' own proportion
REQ_B = (2000, 12 << 30)
REQ_C = (1000, 2 << 30)


def session(jobs):
    """jobs: [(name, rows, (milli-cpu, bytes))] in falling priority; every job a gang of all its rows"""
    nodes = [snapmod.Node(f"n{i:03d}", {"cpu": f"{node_cpu(i)}m", "memory": str(node_cpu(i) * MEM_PER_MILLI), "pods": "110"}) for i in range(N_NODES)]
    pods, groups = [], []
    for k, (name, rows, (cpu, mem)) in enumerate(jobs):
        groups.append(snapmod.PodGroup("default", name, min_member=rows, queue="default", priority=len(jobs) - k))
        pods += [snapmod.Pod("default", f"{name}-{i:02d}", [{"cpu": f"{cpu}m", "memory": str(mem)}], group_name=name) for i in range(rows)]
    snap = snapmod.flatten(nodes, pods, groups, [snapmod.Queue("default", 1)])
    assert snap.n_res == 2 and snap.n_nodes == N_NODES and snap.n_queues == 1
    return snap


def job_rows(snap, j):
    return range(int(snap.job_task_begin[j]), int(snap.job_task_begin[j + 1]))


_reference = {}   # case -> (snapshot, oracle decisions, binds, node state): computed once, shared by the two commit kernels' runs


def reference(oracle_mod, case, jobs, a_spreads=True):
    """the oracle's cycle, and the session held to this file's description by the oracle alone"""
    if case in _reference:
        return _reference[case]
    cfg = conf.load_scheduler_conf(CONF)
    snap = session(jobs)
    o = oracle_mod.Oracle(cfg, snap)
    rows_a, rows_b = job_rows(snap, 0), job_rows(snap, 1)
    first_b, _ = o.argmax_rows(rows_b[0], rows_b[0] + 1, 64)   # B's first choices as the session is loaded
    assert first_b[0].tolist() == list(range(64)), "every shape's list starts with nodes 0, 1, 2, ..."
    o.run(["allocate"])
    dec = o.decisions()
    tasks = dec[:, 0].tolist()
    placed_a = [t for t in tasks if t in rows_a]
    assert placed_a and tasks[:len(placed_a)] == placed_a, "A's rows are popped first, one after the other"
    nodes_a = dec[:len(placed_a), 1].tolist()
    if a_spreads:
        assert nodes_a == list(range(len(placed_a))), "A's rows take nodes 0 .. |A| - 1 in order: B's first choices are A's nodes"
    ref = (cfg, snap, dec, o.binds(), o.node_state())
    o.close()
    _reference[case] = ref
    return ref


def check_engine(ref, commit_kernel, multi_row_run):
    cfg, snap, dec, binds, state = ref
    e = engine.Engine(cfg)
    e.load(snap)
    got = e.run(["allocate"])
    assert got.shape == dec.shape and np.array_equal(got, dec), "decisions in order"
    assert np.array_equal(e.binds(), binds), "bind set"
    for a, b in zip(e.node_state(), state):
        assert a.dtype == b.dtype and np.array_equal(a, b), "node state"
    st = e.stats()
    e.close()
    if commit_kernel == "select":
        assert st["rounds_select"] > 0, st
        if multi_row_run:   # a case that never formed a multi-row run proves nothing
            assert st["select_runs_clean"] + st["select_runs_shots"] > 0, st


@pytest.mark.parametrize("b", [1, 2, 32])
@pytest.mark.parametrize("a", [1, 2, 8, 31, 32])
def test_run_behind_a_run_that_took_its_first_choices(oracle_mod, commit_kernel, a, b):
    """|A| is the number of candidates the membership test of B's run walks; C's run walks B's"""
    jobs = [("a", a, REQ_A), ("b", b, REQ_B), ("c", 4, REQ_C)]
    ref = reference(oracle_mod, ("ab", a, b), jobs)
    assert len(ref[2]) == a + b + 4, "every row is placed"
    check_engine(ref, commit_kernel, a >= 2)


def test_three_runs_of_thirty_two_rows(oracle_mod, commit_kernel):
    """r + r' + r'' = 96 entries are more than a fetch holds: the third run's walk waits for the first run and fetches r + r' (want > 64)"""
    jobs = [("a", 32, REQ_A), ("b", 32, REQ_B), ("c", 32, REQ_C)]
    ref = reference(oracle_mod, "three32", jobs)
    assert len(ref[2]) == 96
    check_engine(ref, commit_kernel, True)


def test_run_in_front_whose_last_row_finds_no_node(oracle_mod, commit_kernel):
    """A asks for nearly a whole node of the seven largest and has eight rows: the eighth finds no node (allocate.go:144-148) and A is abandoned
    behind seven placements.  B's candidates were settled ahead behind a run that did not go as assumed: they are dropped with the round, and
    settled again (settle(false)) against the bitmap as A left it when B's run comes"""
    cpu = node_cpu(6) - 5   # nodes 0 .. 6 hold one such pod each, node 7 none
    jobs = [("a", 8, (cpu, cpu * MEM_PER_MILLI)), ("b", 32, REQ_B), ("c", 4, REQ_C)]
    ref = reference(oracle_mod, "no_node", jobs)
    dec = ref[2]
    assert dec[:7, 1].tolist() == list(range(7)) and 7 not in dec[:, 0].tolist(), "seven rows of A are placed, the eighth is not"
    check_engine(ref, commit_kernel, True)


def test_run_in_front_that_keeps_to_one_node(oracle_mod, commit_kernel):
    """A's pods are so small that node 0 scores the same with them as without: every row of A goes to node 0, A leaves candidates untaken
    (spec_ok = 0) and B's candidates, settled ahead without nodes 0 .. 7, are settled again behind A with nodes 1 .. 7 back among them"""
    jobs = [("a", 8, (10, 10 * MEM_PER_MILLI)), ("b", 32, REQ_B), ("c", 4, REQ_C)]
    ref = reference(oracle_mod, "one_node", jobs, a_spreads=False)
    dec = ref[2]
    assert dec[:8, 1].tolist() == [0] * 8, "A stays on node 0"
    assert set(range(1, 8)) <= set(dec[8:40, 1].tolist()), "B takes the nodes A left"
    check_engine(ref, commit_kernel, True)

"""The start of a chained round in the commit kernels (kb_k9.hpp: k9_prologue_tables / k9_prologue_lists; kb_commit_sel.hip: the run tables built
between the two), against the oracle.  Needs a real MI355X: -m gpu.

In a launch that carries its repair workgroups the selection kernel builds its run tables — the run-start bitmap X.brk / X.stm, X.runs, K, the
compacted rinfo — from the row descriptors alone, beside the repair, and only then waits for the lists' tags.  The sessions here are the
smallest at which that table building can go wrong, run with windows of chosen length over several windows' worth of tasks, so that the
rounds are chained and the fused launch is the path under test (the run kernel goes through the same shared prologue, unfused).

Sessions as in test_gpu_settle_ahead.py: one queue; tiers priority + gang, then predicates + nodeorder; R = 2; 128 empty nodes whose
allocatable falls strictly with the index.  Every job is a gang of all its rows and the jobs come in falling priority, so the rows are popped in
the order they are listed here (allocate.go:129-193) and window k holds rows k * w .. k * w + w - 1 while nothing stops a round early.

Every case first holds its session to its description with the oracle alone (row order, every row placed — or the one row that finds no node
—, the run starts the listed requests give), then compares the engine with the oracle: decisions in order, bind set, float64 node state; and
the engine's own counters must say that the rounds were what the case is about: at least three of them, full windows (rounds = ceil(rows / w)),
no speculation break (the early stop: exactly the one it is about), under the selection kernel every round on it."""
import importlib

import numpy as np
import pytest

kbm = importlib.import_module("kube-batch_amd")
engine = importlib.import_module("kube-batch_amd.engine")
conf, snapmod = kbm.conf, kbm.snapshot

pytestmark = pytest.mark.gpu

N_NODES = 128
MAX_RUN = 32   # kb_k9.hpp: K9_SEL_MAXRUN, the selection kernel's longest run
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


def req(k):
    """request number k: distinct for distinct k, small enough that a thousand rows fit the cluster"""
    return (100 + 10 * k, (64 + 8 * k) << 20)


def session(jobs):
    """jobs: [(rows, (milli-cpu, bytes))] in falling priority; every job a gang of all its rows.  -> snapshot, the rows' requests in order"""
    nodes = [snapmod.Node(f"n{i:03d}", {"cpu": f"{node_cpu(i)}m", "memory": str(node_cpu(i) * MEM_PER_MILLI), "pods": "110"}) for i in range(N_NODES)]
    pods, groups, reqs = [], [], []
    for k, (rows, (cpu, mem)) in enumerate(jobs):
        name = f"j{k:04d}"
        groups.append(snapmod.PodGroup("default", name, min_member=rows, queue="default", priority=len(jobs) - k))
        pods += [snapmod.Pod("default", f"{name}-{i:04d}", [{"cpu": f"{cpu}m", "memory": str(mem)}], group_name=name) for i in range(rows)]
        reqs += [(cpu, mem)] * rows
    snap = snapmod.flatten(nodes, pods, groups, [snapmod.Queue("default", 1)])
    assert snap.n_res == 2 and snap.n_nodes == N_NODES and snap.n_queues == 1 and snap.n_tasks == len(reqs)
    return snap, reqs


def run_starts(reqs, w):
    """per window of w rows: the rows (window-relative) at which the selection kernel starts a run — where the request changes, and at every
    multiple of MAX_RUN inside a stretch of equal requests (kb_commit_sel.hip: X.brk, X.stm)"""
    out = []
    for w0 in range(0, len(reqs), w):
        win = reqs[w0:w0 + w]
        starts, p = [], 0
        for i in range(len(win)):
            if i == 0 or win[i] != win[i - 1]:
                p = i
            if (i - p) % MAX_RUN == 0:
                starts.append(i)
        out.append(starts)
    return out


_reference = {}   # case -> (conf, snapshot, requests, oracle decisions, binds, node state): computed once, shared by the two commit kernels' runs


def reference(oracle_mod, case, jobs, unplaced=()):
    """the oracle's cycle; the rows come in the listed order and all of them are placed, except the tasks in `unplaced` and what lies behind them in their job"""
    if case in _reference:
        return _reference[case]
    cfg = conf.load_scheduler_conf(CONF)
    snap, reqs = session(jobs)
    o = oracle_mod.Oracle(cfg, snap)
    o.run(["allocate"])
    dec = o.decisions()
    tasks = dec[:, 0].tolist()
    assert tasks == sorted(tasks), "the rows are popped in the order they are listed"
    if not unplaced:
        assert tasks == list(range(len(reqs))), "every row is placed"
    ref = (cfg, snap, reqs, dec, o.binds(), o.node_state())
    o.close()
    _reference[case] = ref
    return ref


def check_engine(ref, commit_kernel, w, rounds=None, breaks=0):
    cfg, snap, reqs, dec, binds, state = ref
    e = engine.Engine(cfg, window=w)
    e.load(snap)
    got = e.run(["allocate"])
    assert got.shape == dec.shape and np.array_equal(got, dec), "decisions in order"
    assert np.array_equal(e.binds(), binds), "bind set"
    for a, b in zip(e.node_state(), state):
        assert a.dtype == b.dtype and np.array_equal(a, b), "node state"
    st = e.stats()
    e.close()
    assert st["rounds"] >= 3, st                     # chained rounds: a case without them proves nothing about the fused launch
    assert st["spec_breaks"] == breaks, st
    if rounds is not None:
        assert st["rounds"] == rounds, st            # every window had its full length
    if commit_kernel == "select":
        assert st["rounds_select"] == st["rounds"], st


def full_windows(reqs, w):
    return -(-len(reqs) // w)


@pytest.mark.parametrize("w", [1, 3])
def test_small_windows(oracle_mod, commit_kernel, w):
    """the launch's LDS block is sized by the repair rows' tables, not by the commit layout of a window this small"""
    jobs = [(4, req(0)), (3, req(1)), (5, req(2)), (1, req(3)), (2, req(0))]
    ref = reference(oracle_mod, "small", jobs)
    reqs = ref[2]
    assert len(reqs) == 15 and len(reqs) >= 3 * w
    check_engine(ref, commit_kernel, w, rounds=full_windows(reqs, w))


@pytest.mark.parametrize("w", [31, 32, 33, 64, 65, 256])
def test_windows_at_the_mask_word_and_run_length_boundaries(oracle_mod, commit_kernel, w):
    """three windows and a few rows of jobs of 1 .. 70 rows: stretches that end at, one short of and one past the 32-row words of X.brk / X.stm and
    the 32-row run, runs that start in the last and the first bit of a word"""
    sizes = [32, 1, 31, 33, 2, 64, 1, 1, 65, 30, 3, 70, 29, 5]
    jobs, n, k = [], 0, 0
    while n < 3 * w + 5:
        rows = min(sizes[k % len(sizes)], 3 * w + 5 - n)
        jobs.append((rows, req(k % 7)))
        n += rows
        k += 1
    ref = reference(oracle_mod, ("boundaries", w), jobs)
    reqs = ref[2]
    starts = run_starts(reqs, w)
    assert len(starts) == 4 and all(len(s) >= 1 for s in starts)
    if w >= 33:
        assert any(b - a == MAX_RUN for s in starts for a, b in zip(s, s[1:])), "a run of the full 32 rows"
    check_engine(ref, commit_kernel, w, rounds=4)


def test_one_shape_for_the_whole_window(oracle_mod, commit_kernel):
    """one stretch, split at the multiples of 32: runs of 32, 32, 32 and 4 rows"""
    w = 100
    ref = reference(oracle_mod, "one_shape", [(3 * w + 10, req(0))])
    starts = run_starts(ref[2], w)
    assert starts[:3] == [[0, 32, 64, 96]] * 3 and starts[3] == [0]
    check_engine(ref, commit_kernel, w, rounds=4)


def test_second_stretch_starts_off_the_word_boundary(oracle_mod, commit_kernel):
    """5 rows of one shape, then 100 of another: the second stretch's runs start at rows 5, 37, 69 and 101 — a row of a later mask word finds the
    first row of its stretch by walking back over words without a break bit"""
    w = 105
    ref = reference(oracle_mod, "off_boundary", [(5, req(1)), (100, req(2))] * 3 + [(4, req(3))])
    starts = run_starts(ref[2], w)
    assert starts[:3] == [[0, 5, 37, 69, 101]] * 3 and starts[3] == [0]
    check_engine(ref, commit_kernel, w, rounds=4)


@pytest.mark.parametrize("shapes", [2, 64])
def test_every_row_its_own_run(oracle_mod, commit_kernel, shapes):
    """K == W: two shapes alternating, and 64 distinct requests cycling (a window of 64 rows holds at most 64 shapes: one more and it would close early —
    the engine's round count says it did not)"""
    w = 64
    jobs = [(1, req(i % shapes)) for i in range(3 * w + 2)]
    ref = reference(oracle_mod, ("single_rows", shapes), jobs)
    reqs = ref[2]
    starts = run_starts(reqs, w)
    assert starts[:3] == [list(range(w))] * 3, "every row starts a run"
    assert all(len(set(reqs[w0:w0 + w])) == shapes for w0 in range(0, 3 * w, w))
    check_engine(ref, commit_kernel, w, rounds=4)


def test_last_run_cut_by_a_row_that_finds_no_node(oracle_mod, commit_kernel):
    """windows of 16 rows.  P's 32 rows fill two windows and take nodes 0 .. 31, one each (an eighth of a node apiece: a node's score falls with its first pod).  A's 16 rows are
    the third window, one run; A asks for more than a node that holds a pod of P has left and for nearly all of nodes 32 .. 38: seven rows are placed,
    the eighth finds no node (allocate.go:144-148, KB_REASON_NO_FEASIBLE) and A is abandoned.  The window queued behind it — B's rows — skips
    itself (KB_REASON_SKIPPED; the host refuses anything else from it) and is planned again: one speculation break, the one this case is about"""
    w = 16
    cpu_a = node_cpu(38) - 5   # fits the empty nodes 32 .. 38 once each; node 39 and the nodes with a pod of P are too small
    jobs = [(32, (4000, 4000 * MEM_PER_MILLI)), (16, (cpu_a, cpu_a * MEM_PER_MILLI)), (16, (2000, 12 << 30)), (16, req(0)), (16, req(1))]
    ref = reference(oracle_mod, "early_stop", jobs, unplaced=(39,))
    dec = ref[3]
    assert dec[:32, 0].tolist() == list(range(32)) and sorted(dec[:32, 1].tolist()) == list(range(32)), "P fills two windows, a node each"
    assert dec[32:39, 0].tolist() == list(range(32, 39)) and dec[32:39, 1].tolist() == list(range(32, 39)), "seven rows of A are placed"
    assert not set(range(39, 48)) & set(dec[:, 0].tolist()), "the eighth is not, and A ends there"
    assert dec[39:, 0].tolist() == list(range(48, 96)), "everybody behind A is placed"
    check_engine(ref, commit_kernel, w, breaks=1)

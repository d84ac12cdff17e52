"""Parity of the HIP path (through the C ABI) against the CPU oracle.  Needs a real MI355X: -m gpu.

Bit-exact bar: mask bits, u16 scores, arg-max candidates, the ordered decision list, the bind set, the
final float64 node state and the drf / proportion shares must all be identical."""
import importlib

import numpy as np
import pytest

kbm = importlib.import_module("kube-batch_amd")
engine = importlib.import_module("kube-batch_amd.engine")
fixtures = importlib.import_module("kube-batch_amd.fixtures")
abi, conf, snapmod = kbm.abi, kbm.conf, kbm.snapshot

pytestmark = pytest.mark.gpu

MOST_CONF = """
actions: "allocate, backfill"
tiers:
- plugins:
  - name: priority
  - name: gang
- plugins:
  - name: drf
  - name: predicates
  - name: proportion
  - name: nodeorder
    arguments:
      leastrequested.weight: 0
      mostrequested.weight: 5
      balancedresource.weight: 1
"""


def small(idx, scale, **kw):
    p = snapmod.synth_config(idx, scale)
    for k, v in kw.items():
        setattr(p, k, v)
    return snapmod.synth(p)


def run_both(oracle_mod, cfg, snap, actions, **ekw):
    o = oracle_mod.Oracle(cfg, snap)
    o.run(actions)
    e = engine.Engine(cfg, **ekw)
    e.load(snap)
    dec = e.run(actions)
    return o, e, dec


def assert_same_outcome(o, e, dec):
    od = o.decisions()
    assert dec.shape == od.shape, (dec.shape, od.shape)
    assert np.array_equal(dec, od), f"first divergence at decision {int(np.argmax((dec != od).any(axis=1)))}"
    assert np.array_equal(e.binds(), o.binds())
    est, end = e.task_state()
    ost, ond = o.task_state()
    assert np.array_equal(est, ost) and np.array_equal(end, ond)
    for a, b in zip(e.node_state(), o.node_state()):
        assert np.array_equal(a, b)
    for a, b in zip(e.shares(), o.shares()):
        assert np.array_equal(a, b)
    st = e.stats()
    assert st["evals"] == o.evals and st["tasks_popped"] == o.popped


@pytest.mark.parametrize("case", range(2))
def test_reference_allocate_cases(oracle_mod, case):
    """actions/allocate/allocate_test.go:51-144 through the HIP path."""
    name, snap, expected = fixtures.allocate_cases()[case]
    cfg = fixtures.allocate_test_tiers()
    o, e, dec = run_both(oracle_mod, cfg, snap, ["allocate"])
    assert snap.bind_map(e.binds()) == expected, name
    assert_same_outcome(o, e, dec)


def test_example_job_config1(oracle_mod):
    cfg, snap = fixtures.example_job()
    o, e, dec = run_both(oracle_mod, cfg, snap, ["allocate"])
    assert sorted(np.bincount(e.binds(), minlength=3).tolist()) == [2, 2, 2]
    assert_same_outcome(o, e, dec)


def test_matrix_parity_config2(oracle_mod):
    """K1 over the full 10k x 1k matrix of BASELINE config 2, bit for bit on mask and score."""
    snap = snapmod.synth(snapmod.synth_config(2))
    cfg = conf.load_scheduler_conf()
    o = oracle_mod.Oracle(cfg, snap, threads=8)
    e = engine.Engine(cfg)
    e.load(snap)
    for fit in (1, 0):
        em, es = e.eval_matrix(0, snap.n_tasks, fit)
        om, os_ = o.eval_matrix(0, snap.n_tasks, fit)
        assert np.array_equal(em, om), f"mask differs (fit_mode {fit})"
        assert np.array_equal(es, os_), f"score differs (fit_mode {fit})"
    assert em.any() and es.any()
    # the same matrix through the other two launch organisations (include/kb_engine.h): every row evaluated by the matrix kernel itself,
    # with and without sharing an evaluation between adjacent equal rows — the <4 nodes, 32 rows> tile the shape-deduplicated launch never uses
    om, os_ = o.eval_matrix(0, snap.n_tasks, 1)
    for flags in (abi.MATRIX_DIRECT, abi.MATRIX_DIRECT | abi.MATRIX_NO_DEDUP):
        em, es = e.eval_matrix(0, snap.n_tasks, 1 | flags)
        assert np.array_equal(em, om) and np.array_equal(es, os_), hex(flags)


def test_matrix_parity_r16_and_after_allocate(oracle_mod):
    """16-dim resource vectors (config 4 shape, scaled) and a non-trivial live state (after an allocate pass)."""
    snap = small(4, 0.03)
    cfg = conf.load_scheduler_conf(MOST_CONF)
    o, e, dec = run_both(oracle_mod, cfg, snap, ["allocate"])
    assert_same_outcome(o, e, dec)
    em, es = e.eval_matrix(0, snap.n_tasks, 1)
    om, os_ = o.eval_matrix(0, snap.n_tasks, 1)
    assert np.array_equal(em, om) and np.array_equal(es, os_)
    for flags in (abi.MATRIX_DIRECT, abi.MATRIX_DIRECT | abi.MATRIX_NO_DEDUP):     # scalar dimensions through the direct tile's 16-byte loads
        em, es = e.eval_matrix(0, snap.n_tasks, 1 | flags)
        assert np.array_equal(em, om) and np.array_equal(es, os_), hex(flags)


@pytest.mark.parametrize("n_res,diverse", [(2, False), (2, True), (16, False)])
def test_matrix_parity_wide_direct_tiles(oracle_mod, n_res, diverse):
    """A matrix wide and tall enough (4 608 rows x 9 000 nodes) for the tiles the small configurations never launch: k_matrix_runs (runs of
    adjacent equal rows evaluated once, streamed out with 16-byte stores; rows [0, 4096) and the ragged rest), the same tile without sharing
    (KB_MATRIX_NO_DEDUP clears its row flags; k_matrix<4, 32> is the per-shape launch of tens of thousands of shapes, tests/test_gpu_kernel_edges.py),
    and the per-shape + expansion path, all bit-equal to the oracle — also in a live state after an allocate pass."""
    p = snapmod.SynthParams(n_tasks=5000, n_nodes=9000, n_queues=8, n_res=n_res, seed=snapmod.SEED_BASE + 77 + n_res)
    p.diverse_requests = diverse
    snap = snapmod.synth(p)
    cfg = conf.load_scheduler_conf(MOST_CONF) if n_res > 2 else conf.load_scheduler_conf()
    o, e, dec = run_both(oracle_mod, cfg, snap, ["allocate"])
    assert_same_outcome(o, e, dec)
    t1 = 4608
    om, os_ = o.eval_matrix(0, t1, 1)
    for flags in (0, abi.MATRIX_DIRECT, abi.MATRIX_DIRECT | abi.MATRIX_NO_DEDUP):
        em, es = e.eval_matrix(0, t1, 1 | flags)
        assert np.array_equal(em, om), hex(flags)
        assert np.array_equal(es, os_), hex(flags)
    assert om.any() and os_.any()


def test_argmax_parity(oracle_mod):
    snap = small(2, 0.5)
    cfg = conf.load_scheduler_conf()
    o = oracle_mod.Oracle(cfg, snap, threads=8)
    e = engine.Engine(cfg)
    e.load(snap)
    for k in (1, 8, 32):
        en, es = e.argmax_rows(0, 600, k)
        on, os_ = o.argmax_rows(0, 600, k)
        assert np.array_equal(en, on) and np.array_equal(es, os_), k
    # long lists: several score bands, and past the last feasible node (KB_NONE padding)
    for k in (513, snap.n_nodes + 7):
        en, es = e.argmax_rows(100, 160, k)
        on, os_ = o.argmax_rows(100, 160, k)
        assert np.array_equal(en, on) and np.array_equal(es, os_), k


@pytest.mark.parametrize("window,batch,flags", [(64, 4, 0), (1024, 16, 0), (4096, 1, 0), (512, 7, 0), (200, 2, 0),
                                                (0, 0, abi.FLAG_SYNC_ROUNDS), (96, 5, abi.FLAG_SYNC_ROUNDS), (0, 0, abi.FLAG_YIELD_WAIT), (0, 0, abi.FLAG_SPIN_WAIT)])
def test_allocate_backfill_config2(oracle_mod, window, batch, flags):
    """Full allocate + backfill on BASELINE config 2: ordered decisions, binds, state, shares identical."""
    snap = snapmod.synth(snapmod.synth_config(2))
    cfg = conf.load_scheduler_conf()
    o, e, dec = run_both(oracle_mod, cfg, snap, ["allocate", "backfill"], window=window, commit_batch=batch, flags=flags)
    assert_same_outcome(o, e, dec)
    st = e.stats()
    assert st["decisions"] == len(dec) and st["rounds"] > 0


def test_allocate_gang_drf_queues_scaled_config3(oracle_mod):
    """Config 3 shape (gang minAvailable + DRF + proportion across 128 queues), scaled to oracle-in-seconds size."""
    snap = small(3, 0.1)
    cfg = conf.load_scheduler_conf()
    o, e, dec = run_both(oracle_mod, cfg, snap, ["allocate", "backfill"])
    assert_same_outcome(o, e, dec)
    # gang semantics visible in the result: some Allocated tasks of never-ready gangs are not bound
    st, _ = e.task_state()
    assert (st == abi.TASK_BINDING).sum() == (e.binds() != abi.KB_NONE).sum()


def test_wide_cluster_more_than_64k_nodes(oracle_mod):
    """N >= 65536: the two-values-per-band variant of the candidate-list kernel, a 66k-bit dirty bitmap in the commit kernel."""
    snap = snapmod.synth(snapmod.SynthParams(n_tasks=2500, n_nodes=66_000, n_queues=4, n_res=2, seed=snapmod.SEED_BASE + 77))
    cfg = conf.load_scheduler_conf()
    o = oracle_mod.Oracle(cfg, snap, threads=8)
    e = engine.Engine(cfg)
    e.load(snap)
    en, es = e.argmax_rows(10, 40, 300)
    on, os_ = o.argmax_rows(10, 40, 300)
    assert np.array_equal(en, on) and np.array_equal(es, os_)
    o2, e2, dec = run_both(oracle_mod, cfg, snap, ["allocate", "backfill"])
    assert_same_outcome(o2, e2, dec)


def _with_affinity(snap, seed, frac=0.5):
    """Random NodeAffinity Map counts per (task class, node class); about half of the task classes have no preferred terms."""
    rng = np.random.RandomState(seed)
    a = rng.choice([0, 0, 1, 3, 10, 40], size=(snap.n_task_classes, snap.n_node_classes)).astype(np.int32)
    a[rng.uniform(size=snap.n_task_classes) < frac] = 0
    snap.class_affinity = a
    snap._check()
    return snap


def test_preferred_node_affinity(oracle_mod):
    """NodeAffinity priority (Map counts + NormalizeReduce over the feasible set + weight): matrix, candidate lists and the
    whole cycle; rows of affinity-bearing classes are committed as first rows of fresh rounds (KB_REASON_RENORM)."""
    cfg = conf.load_scheduler_conf()
    snap = _with_affinity(small(3, 0.03, zone_selector_frac=0.5), 7)
    o = oracle_mod.Oracle(cfg, snap, threads=8)
    e = engine.Engine(cfg)
    e.load(snap)
    em, es = e.eval_matrix(0, snap.n_tasks, 1)
    om, os_ = o.eval_matrix(0, snap.n_tasks, 1)
    assert np.array_equal(em, om) and np.array_equal(es, os_)
    assert int(es.max()) > 20      # the affinity term is really there (least + balanced alone stay <= 20)
    en, ek = e.argmax_rows(0, 200, 40)
    on, ok = o.argmax_rows(0, 200, 40)
    assert np.array_equal(en, on) and np.array_equal(ek, ok)
    for window, batch in ((0, 0), (64, 3), (1024, 16)):
        o2, e2, dec = run_both(oracle_mod, cfg, _with_affinity(small(3, 0.03, zone_selector_frac=0.5), 7), ["allocate", "backfill"],
                               window=window, commit_batch=batch)
        assert_same_outcome(o2, e2, dec)
    # a different plugin weight, and weight 0 (the term vanishes)
    for w in (3, 0):
        cfgw = conf.load_scheduler_conf(conf.DEFAULT_SCHEDULER_CONF.replace("  - name: nodeorder", f"  - name: nodeorder\n    arguments: {{nodeaffinity.weight: {w}}}"))
        o3, e3, dec = run_both(oracle_mod, cfgw, _with_affinity(small(2, 0.2, zone_selector_frac=0.5), 9), ["allocate", "backfill"])
        assert_same_outcome(o3, e3, dec)


def _with_ports(snap, seed):
    """Random host-port bits: ~25 % of the tasks occupy 1-2 of 6 ports, some ports collide with a wildcard sibling, ~20 % of the
    nodes already have ports in use."""
    rng = np.random.RandomState(seed)
    T, N = snap.n_tasks, snap.n_nodes
    want = np.zeros(T, np.uint64)
    has = rng.uniform(size=T) < 0.25
    want[has] = (np.uint64(1) << rng.randint(0, 6, size=int(has.sum())).astype(np.uint64))
    two = has & (rng.uniform(size=T) < 0.3)
    want[two] |= (np.uint64(1) << rng.randint(0, 6, size=int(two.sum())).astype(np.uint64))
    sibling = np.array([1, 0, 3, 2, 4, 5], np.uint64)                  # bits 0/1 and 2/3 are the same port on 0.0.0.0 / one IP
    conf = want.copy()
    for b in range(6):
        conf |= np.where((want >> np.uint64(b)) & np.uint64(1), np.uint64(1) << sibling[b], np.uint64(0)).astype(np.uint64)
    snap.task_port_want, snap.task_port_conflict = want, conf
    used = np.zeros(N, np.uint64)
    busy = rng.uniform(size=N) < 0.2
    used[busy] = rng.randint(1, 64, size=int(busy.sum())).astype(np.uint64)
    snap.node_ports = used
    snap._check()
    return snap


def test_host_ports(oracle_mod):
    """PodFitsHostPorts as a dynamic predicate: node port bits live in the dirty slots of the commit kernel."""
    cfg = conf.load_scheduler_conf()
    snap = _with_ports(small(3, 0.03), 11)
    o = oracle_mod.Oracle(cfg, snap, threads=8)
    e = engine.Engine(cfg)
    e.load(snap)
    em, es = e.eval_matrix(0, snap.n_tasks, 1)
    om, os_ = o.eval_matrix(0, snap.n_tasks, 1)
    assert np.array_equal(em, om) and np.array_equal(es, os_)
    for window, batch in ((0, 0), (64, 3), (1024, 16)):
        o2, e2, dec = run_both(oracle_mod, cfg, _with_ports(small(3, 0.03), 11), ["allocate", "backfill"], window=window, commit_batch=batch)
        assert_same_outcome(o2, e2, dec)
    # few nodes, many port-hungry pods: nodes fill up with ports, pods are turned away, jobs get abandoned
    o3, e3, dec = run_both(oracle_mod, cfg, _with_ports(small(2, 0.1, n_nodes=12), 13), ["allocate", "backfill"])
    assert_same_outcome(o3, e3, dec)


def test_reference_test_tiers_on_synthetic(oracle_mod):
    """drf+proportion only (allocate_test.go tiers): no predicates, no node order -> pure tie-break path."""
    snap = small(2, 0.2)
    o, e, dec = run_both(oracle_mod, fixtures.allocate_test_tiers(), snap, ["allocate"])
    assert_same_outcome(o, e, dec)


def test_edge_cases(oracle_mod):
    cfg = conf.load_scheduler_conf()
    # no tasks at all
    snap = snapmod.flatten([snapmod.Node("n1", {"cpu": "4", "memory": "8Gi", "pods": "10"})], [], [], [snapmod.Queue("default")])
    o, e, dec = run_both(oracle_mod, cfg, snap, ["allocate", "backfill"])
    assert len(dec) == 0
    # pod-count cap: 3 one-cpu pods, node allows 2 pods
    pods = [snapmod.Pod("ns", f"p{i}", [{"cpu": "1", "memory": "1Gi"}], group_name="g") for i in range(3)]
    snap = snapmod.flatten([snapmod.Node("n1", {"cpu": "8", "memory": "16Gi", "pods": "2"})], pods,
                           [snapmod.PodGroup("ns", "g", min_member=1)], [snapmod.Queue("default")])
    o, e, dec = run_both(oracle_mod, cfg, snap, ["allocate"])
    assert_same_outcome(o, e, dec)
    assert len(dec) == 2
    # taints / selectors / unschedulable nodes through the class table
    nodes = [snapmod.Node("a", {"cpu": "8", "memory": "16Gi", "pods": "10"}, labels={"zone": "x"}),
             snapmod.Node("b", {"cpu": "8", "memory": "16Gi", "pods": "10"}, taints=[("k", "v", "NoSchedule")]),
             snapmod.Node("c", {"cpu": "8", "memory": "16Gi", "pods": "10"}, unschedulable=True)]
    pods = [snapmod.Pod("ns", "sel", [{"cpu": "1"}], group_name="g", node_selector={"zone": "x"}),
            snapmod.Pod("ns", "tol", [{"cpu": "1"}], group_name="g", tolerations=[("k", "Equal", "v", "NoSchedule")]),
            snapmod.Pod("ns", "zzz", [{"cpu": "1"}], group_name="g", node_selector={"zone": "nowhere"})]
    snap = snapmod.flatten(nodes, pods, [snapmod.PodGroup("ns", "g", min_member=1)], [snapmod.Queue("default")])
    o, e, dec = run_both(oracle_mod, cfg, snap, ["allocate"])
    assert_same_outcome(o, e, dec)
    assert snap.bind_map(e.binds()).get("ns/sel") == "a"


def test_pipeline_init_containers_and_scalars(oracle_mod):
    """Branches of the commit kernel the synthetic configs do not reach: Pipeline onto Releasing capacity (and the host's
    re-plan after it), InitResreq > Resreq (init containers), scalar resources consumed in the commit (nvidia.com/gpu)."""
    cfg = conf.load_scheduler_conf()
    GPU = "nvidia.com/gpu"
    nodes = [snapmod.Node("n1", {"cpu": "8", "memory": "16Gi", "pods": "20", GPU: "4"}),
             snapmod.Node("n2", {"cpu": "8", "memory": "16Gi", "pods": "20", GPU: "2"}),
             snapmod.Node("n3", {"cpu": "4", "memory": "8Gi", "pods": "20"})]
    pods = []
    # a terminating pod on n3 (Releasing 3 cpu / 6Gi) and a running one: n3's Idle is tiny, its Releasing is not
    pods.append(snapmod.Pod("old", "dying", [{"cpu": "3", "memory": "6Gi"}], node_name="n3", phase="Running", deleting=True, group_name="gold"))
    pods.append(snapmod.Pod("old", "busy", [{"cpu": "900m", "memory": "1Gi"}], node_name="n3", phase="Running", group_name="gold"))
    # fill n1/n2 so that later tasks only fit n3's Releasing
    for i in range(7):
        pods.append(snapmod.Pod("a", f"fat{i}", [{"cpu": "2", "memory": "4Gi"}], group_name="ga", creation=10 + i))
    pods.append(snapmod.Pod("b", "pipe1", [{"cpu": "2", "memory": "4Gi"}], group_name="gb", creation=30))
    pods.append(snapmod.Pod("b", "pipe2", [{"cpu": "1", "memory": "2Gi"}], group_name="gb", creation=31))
    # init container raises the launch requirement above the running requirement
    pods.append(snapmod.Pod("c", "init1", [{"cpu": "500m", "memory": "512Mi"}], init_containers=[{"cpu": "1500m", "memory": "1Gi"}], group_name="gc", creation=40))
    pods.append(snapmod.Pod("c", "init2", [{"cpu": "500m", "memory": "512Mi"}], init_containers=[{"cpu": "1500m", "memory": "1Gi"}], group_name="gc", creation=41))
    # scalar resource requests: 3 gpus fit n1 only, then 2 on n2, then nothing
    for i, g in enumerate(["3", "2", "2", "1"]):
        pods.append(snapmod.Pod("d", f"gpu{i}", [{"cpu": "100m", "memory": "128Mi", GPU: g}], group_name="gd", creation=50 + i))
    pgs = [snapmod.PodGroup("old", "gold", min_member=1, creation=1), snapmod.PodGroup("a", "ga", min_member=1, creation=2),
           snapmod.PodGroup("b", "gb", min_member=1, creation=3), snapmod.PodGroup("c", "gc", min_member=2, creation=4),
           snapmod.PodGroup("d", "gd", min_member=1, creation=5)]
    snap = snapmod.flatten(nodes, pods, pgs, [snapmod.Queue("default")])
    assert snap.n_res == 3 and (snap.node_releasing[:, 2] > 0).any()
    for window in (1024, 64):
        o, e, dec = run_both(oracle_mod, cfg, snap, ["allocate", "backfill"], window=window)
        assert_same_outcome(o, e, dec)
    assert (dec[:, 2] == 1).any(), "the fixture must exercise ssn.Pipeline"
    st = e.stats()
    assert st["spec_breaks"] >= 1


def test_full_size_properties_config3():
    """Size-independent properties at BASELINE's full 100k x 10k size (the oracle would take minutes here): node accounting
    conservation, gang gating of the bind set, idempotence of a second cycle after reset, pod-count caps."""
    snap = snapmod.synth(snapmod.synth_config(3))
    cfg = conf.load_scheduler_conf()
    e = engine.Engine(cfg)
    e.load(snap)
    dec = e.run(["allocate", "backfill"])
    binds = e.binds()
    st, nd = e.task_state()
    idle, rel, nzc, nzm, cnt = e.node_state()
    # every decision placed a Pending task exactly once
    assert len(np.unique(dec[:, 0])) == len(dec) and (snap.task_status[dec[:, 0]] == abi.TASK_PENDING).all()
    # Idle + sum of placed Resreq == snapshot Idle, per node and dimension (integer-valued float64: exact)
    used = np.zeros_like(idle)
    np.add.at(used.T, dec[:, 1], snap.task_resreq[:, dec[:, 0]].T)
    assert np.array_equal(idle + used, snap.node_idle)
    assert np.array_equal(cnt, snap.node_pod_cnt + np.bincount(dec[:, 1], minlength=snap.n_nodes).astype(np.int32))
    assert (cnt <= snap.node_max_pods).all()
    # gang gating: a task is bound iff its job reached minAvailable ready tasks
    ready_status = np.isin(st, (abi.TASK_ALLOCATED, abi.TASK_BINDING, abi.TASK_BOUND, abi.TASK_RUNNING, abi.TASK_SUCCEEDED))
    ready_per_job = np.add.reduceat(ready_status.astype(np.int64), snap.job_task_begin[:-1].astype(np.int64))
    job_ready = ready_per_job >= snap.job_min_available
    placed = np.zeros(snap.n_tasks, bool)
    placed[dec[:, 0]] = True
    assert np.array_equal(binds != abi.KB_NONE, placed & job_ready[snap.task_job])
    assert (st[placed & ~job_ready[snap.task_job]] == abi.TASK_ALLOCATED).all()
    # a second cycle from the pristine state is identical
    e.reset()
    dec2 = e.run(["allocate", "backfill"])
    assert np.array_equal(dec, dec2) and np.array_equal(e.binds(), binds)


def test_the_pinned_commit_kernel_is_the_one_that_runs(oracle_mod, commit_kernel):
    """KB_COMMIT_KERNEL pins the kernel for every round (the suite's three-way axis would mean nothing otherwise), and under `select` the runs
    of two or more plain rows really go through the selection — not through the serial loop it keeps as a fall-back: kb_stats counts them."""
    snap = kbm.snapshot.synth(kbm.snapshot.synth_config(2, 1.0))
    cfg = kbm.conf.load_scheduler_conf()
    e = engine.Engine(cfg)
    e.load(snap)
    dec = e.run(["allocate", "backfill"])
    st = e.stats()
    o = oracle_mod.Oracle(cfg, snap)
    o.run(["allocate", "backfill"])
    assert np.array_equal(dec, o.decisions())
    if commit_kernel == "select":
        assert st["rounds_select"] == st["rounds"] > 10
        by_selection = st["select_runs_clean"] + st["select_runs_shots"]
        assert by_selection > 200 and st["select_runs_shots"] <= st["select_shots"] < 4 * st["select_runs_shots"] + 1, st      # every such run takes a shot, few take many
    elif commit_kernel == "run":   # (None: the emulated-device re-collection, which does not pin a kernel)
        assert st["rounds_select"] == 0 and st["select_runs_clean"] == 0 and st["select_runs_shots"] == 0 and st["select_shots"] == 0
    e.close(); o.close()

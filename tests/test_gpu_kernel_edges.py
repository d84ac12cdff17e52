"""The matrix and candidate-list kernels at their size boundaries, bit for bit against the oracle (oracle/kb_oracle.c: kbo_eval_matrix, kbo_argmax_rows).
Needs a real MI355X: -m gpu.

The launch organisation of these kernels changes at fixed sizes (kb_kernels.hip): NP pads the node count to KB_NODE_PAD = 2 048; k_expand_tiles
cuts a row into tiles of 16 384 nodes (the last one partial) and a shape's rows into chunks of 64; k_matrix picks <1,4>, <1,16>, <4,32> or
k_matrix_runs from n_mrows * NP and the workgroup count; k_argmax switches to two values per band (WIDE) from NP = 65 536 on, where the
packed 16-bit counters of one score value could carry, and takes 1 024 or 256 threads and NW = 2 or 4 words per band.  Every case here sits
on or next to one of those edges and compares every mask bit, every u16 score, and every candidate (node, score) of the requested lists.

The oracle's matrix is the high-precision reference (int64 / IEEE-double restatement).  The long candidate lists (k up to 4 096 of 66 000
nodes) are derived from it here — (score descending, node ascending) over the feasible nodes, KB_NONE / 0 behind the last one — because
kbo_argmax_rows is O(k * N) per row; the derivation itself is held to kbo_argmax_rows on a few rows of every session.

No case has a skip path: every session lies inside the engine's envelope, and a refused load or run fails the test."""
import hashlib
import importlib
import re
import time

import numpy as np
import pytest

kbm = importlib.import_module("kube-batch_amd")
engine = importlib.import_module("kube-batch_amd.engine")
abi, conf, snapmod = kbm.abi, kbm.conf, kbm.snapshot

pytestmark = pytest.mark.gpu

NONE = abi.KB_NONE
DIRECT, NO_DEDUP = abi.MATRIX_DIRECT, abi.MATRIX_NO_DEDUP
FLAG_SETS = (0, DIRECT, DIRECT | NO_DEDUP)   # per-shape + expansion, every row by the matrix kernel, and without sharing adjacent equal rows

# N -> NP: one pad block, an exact pad block, two blocks; one exact expansion tile, two tiles with a 2 048-node tail, three tiles with a tail;
# the widest row of the 16-bit-counter candidate-list kernel, the narrowest WIDE row, WIDE with a tail
NODE_COUNTS = (1, 2048, 2049, 16384, 16385, 32769, 63488, 65536, 66000)


def _nodeorder(least, most, balanced):
    return f"""
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
      leastrequested.weight: {least}
      mostrequested.weight: {most}
      balancedresource.weight: {balanced}
"""


CONFS = {
    "default": None,                                   # leastrequested 1, balancedresource 1, mostrequested 0: NW = 2
    "most": _nodeorder(0, 5, 1),                       # BASELINE's bin-packing weights: NW = 4
    # near the envelope: 10 * (sum of weights) = 32 700 <= 65 535, and (32 700 + 2) << 17 node bits still fits the commit kernel's 32-bit keys
    # at 66 000 nodes; distinct scores lie hundreds apart, so a band of 2 - 8 values holds few nodes and the band loop runs many times
    "sparse": _nodeorder(1000, 2000, 270),
    "zero": _nodeorder(0, 1, 0),                       # small pods on big empty nodes: every feasible node scores 0 (NW = 4)
}


def cfg_of(name):
    text = CONFS[name]
    return conf.load_scheduler_conf(text) if text else conf.load_scheduler_conf()


def session(n_tasks, n_nodes, seed, **kw):
    p = snapmod.SynthParams(n_tasks=n_tasks, n_nodes=n_nodes, n_queues=4, n_res=2, seed=snapmod.SEED_BASE + seed)
    for k, v in kw.items():
        setattr(p, k, v)
    return snapmod.synth(p)


def open_both(oracle_mod, cfg, snap):
    o = oracle_mod.Oracle(cfg, snap, threads=8)
    e = engine.Engine(cfg)
    e.load(snap)          # raises on any refusal: a case outside the envelope fails
    return o, e


def allocate_both(o, e):
    """one allocate pass on both sides (live node state for the matrices that follow); the decision lists must already agree"""
    o.allocate()
    dec = e.run(["allocate"])
    od = o.decisions()
    assert dec.shape == od.shape and np.array_equal(dec, od)
    for a, b in zip(e.node_state(), o.node_state()):
        assert np.array_equal(a, b)
    return len(dec)


def assert_matrix_equal(em, es, om, os_, what):
    assert em.shape == om.shape and es.shape == os_.shape, what
    if not np.array_equal(em, om):
        r = int(np.argmax((em != om).any(axis=1)))
        pytest.fail(f"{what}: mask differs, first at row {r} (bytes {np.nonzero(em[r] != om[r])[0][:8].tolist()})")
    if not np.array_equal(es, os_):
        r = int(np.argmax((es != os_).any(axis=1)))
        pytest.fail(f"{what}: score differs, first at row {r} (nodes {np.nonzero(es[r] != os_[r])[0][:8].tolist()})")


def feasible(mask, n):
    return np.unpackbits(mask, axis=1, bitorder="little")[:, :n].astype(bool)


def topk_from_matrix(mask, score, k):
    """the first k of (score descending, node ascending) over each row's feasible nodes; KB_NONE / 0 behind the last feasible one"""
    rows, n = score.shape
    feas = feasible(mask, n)
    key = np.where(feas, (65535 - score.astype(np.int64)) * n + np.arange(n, dtype=np.int64), np.int64(1) << 62)
    kk = min(k, n)
    part = np.argpartition(key, kk - 1, axis=1)[:, :kk] if kk < n else np.broadcast_to(np.arange(n), (rows, n)).copy()
    sel = np.take_along_axis(part, np.argsort(np.take_along_axis(key, part, 1), axis=1), 1)
    ok = np.take_along_axis(feas, sel, 1)
    nodes = np.full((rows, k), NONE, np.uint32)
    scores = np.zeros((rows, k), np.uint16)
    nodes[:, :kk] = np.where(ok, sel, NONE)
    scores[:, :kk] = np.where(ok, np.take_along_axis(score, sel, 1), 0)
    return nodes, scores


def k_values(n_nodes, wide_bands):
    """k around the band width VALS (2 * NW score values per band below 65 536 nodes, NW values from there on), 513 and 4 096"""
    vals = 2 * (4 if wide_bands else 2) if n_nodes <= 63488 else (4 if wide_bands else 2)
    return sorted({1, max(1, vals - 1), vals, vals + 1, 513, 4096})


_lists_cache = {}   # derived reference lists, shared by the two commit-kernel runs of a case


def check_argmax(o, e, om, os_, t0, counts, ks, what):
    """engine lists of rows [t0, t0 + c) for every c in counts and k in ks against the lists derived from the oracle's matrix rows [t0, ...);
    the derivation is held to kbo_argmax_rows on the first rows"""
    if what not in _lists_cache:
        _lists_cache.clear()
        _lists_cache[what] = topk_from_matrix(om, os_, max(ks))    # every shorter list is a prefix
    all_n, all_s = _lists_cache[what]
    for k in ks:
        ref_n, ref_s = all_n[:, :k], all_s[:, :k]
        if k <= 600:
            on, osc = o.argmax_rows(t0, t0 + 3, k)
            assert np.array_equal(on, ref_n[:3]) and np.array_equal(osc, ref_s[:3]), f"{what}: derived lists != kbo_argmax_rows (k {k})"
        for c in counts:
            en, es = e.argmax_rows(t0, t0 + c, k)
            if not (np.array_equal(en, ref_n[:c]) and np.array_equal(es, ref_s[:c])):
                r = int(np.argmax((en != ref_n[:c]).any(axis=1) | (es != ref_s[:c]).any(axis=1)))
                i = int(np.argmax((en[r] != ref_n[r]) | (es[r] != ref_s[r])))
                pytest.fail(f"{what}: {c} rows, k {k}: row {t0 + r} entry {i}: engine ({en[r, i]}, {es[r, i]}) oracle ({ref_n[r, i]}, {ref_s[r, i]})")


# ---- a. the matrix at every node-count boundary, all three launch organisations, loaded and live state ---------------------------------

@pytest.mark.parametrize("weights", ["default", "most"])
@pytest.mark.parametrize("n_nodes", NODE_COUNTS)
def test_matrix_at_node_count_boundaries(oracle_mod, n_nodes, weights):
    T = 320 if n_nodes < 32769 else 200
    snap = session(T, n_nodes, 500 + n_nodes % 997)
    cfg = cfg_of(weights)
    o, e = open_both(oracle_mod, cfg, snap)
    for state in ("loaded", "after allocate"):
        if state != "loaded":
            assert allocate_both(o, e) > 0
        for fit in (0, 1):
            om, os_ = o.eval_matrix(0, T, fit)
            if state == "loaded" and fit == 1:
                assert om.any() and os_.any(), "feasible pairs with non-zero scores"
            for flags in FLAG_SETS:
                em, es = e.eval_matrix(0, T, fit | flags)
                assert_matrix_equal(em, es, om, os_, f"N {n_nodes} {weights} {state} fit {fit} flags {hex(flags)}")
    e.close(); o.close()


@pytest.mark.parametrize("diverse", [False, True])
def test_matrix_many_rows_past_one_tile(oracle_mod, diverse):
    """2 100 rows x 16 385 nodes (two expansion tiles): enough workgroups (n_mrows * NP >= 4M, >= 1 024 blocks) for k_matrix_runs, which the
    direct launch takes with and without sharing adjacent equal rows (MATRIX_NO_DEDUP clears its row flags); the 300-row direct launches of the
    node-count cases are k_matrix<1,16> from 14 336 nodes on.  k_matrix<4,32> is the per-shape launch of ~72 000 shapes in
    test_whole_range_plan_more_than_65535_chunks."""
    T, N = 2100, 16385
    snap = session(T, N, 61 + diverse, diverse_requests=diverse)
    o, e = open_both(oracle_mod, cfg_of("most"), snap)
    assert (18432 // 1024) * ((T + 31) // 32) >= 1024
    for fit in (1, 0):
        om, os_ = o.eval_matrix(0, T, fit)
        for flags in FLAG_SETS:
            em, es = e.eval_matrix(0, T, fit | flags)
            assert_matrix_equal(em, es, om, os_, f"diverse {diverse} fit {fit} flags {hex(flags)}")
    allocate_both(o, e)
    om, os_ = o.eval_matrix(0, T, 1)
    for flags in FLAG_SETS:
        em, es = e.eval_matrix(0, T, 1 | flags)
        assert_matrix_equal(em, es, om, os_, f"diverse {diverse} after allocate flags {hex(flags)}")
    e.close(); o.close()


# ---- b. expansion chunking: shapes of 63 .. 129 rows, shape order that is not row order, ranges off the plan grid ------------------------

def _plans(capfd):
    err = capfd.readouterr().err
    return [tuple(int(x) for x in m) for m in re.findall(r"kb_eval_matrix: plan rows (\d+)\.\.(\d+) shapes (\d+) direct (\d) expansion chunks (\d+) launches (\d+)", err)]


@pytest.mark.parametrize("gang", [63, 64, 65, 128, 129, None])
def test_expansion_chunks_at_two_tiles(oracle_mod, gang, monkeypatch, capfd):
    """gang g: every job is one shape of g rows (diverse requests), so each shape ends in a chunk of g mod 64 rows (64: none); None: the stock
    request menu, a few dozen shapes interleaved across jobs (the shape order `order` is far from the identity).  Ranges that start off 0 and
    ranges across kb_eval_matrix's 4 096-row plan boundary, under the default plan size and KB_EVAL_MATRIX_ROWS (whole range; 1 000 rows)."""
    T, N = 8400, 16385
    kw = dict(diverse_requests=True, gang_sizes=(gang,), gang_probs=(1.0,)) if gang else {}
    snap = session(T, N, 70 + (gang or 0), **kw)
    o, e = open_both(oracle_mod, cfg_of("default"), snap)
    om, os_ = o.eval_matrix(0, T, 1)
    ranges = ((0, T), (37, T - 5), (4000, 8300), (4095, 4097), (1, 2))
    for a, b in ranges:
        em, es = e.eval_matrix(a, b, 1)
        assert_matrix_equal(em, es, om[a:b], os_[a:b], f"gang {gang} rows [{a}, {b})")
    for rows in (T, 1000):
        monkeypatch.setenv("KB_EVAL_MATRIX_ROWS", str(rows))
        capfd.readouterr()
        for a, b in ((0, T), (37, T - 5)):
            em, es = e.eval_matrix(a, b, 1)
            assert_matrix_equal(em, es, om[a:b], os_[a:b], f"gang {gang} rows [{a}, {b}) in plans of {rows}")
        plans = _plans(capfd)
        assert plans and all(p[3] == 0 for p in plans), "these plans take the expansion path"
        if rows == T:
            assert (plans[0][0], plans[0][1]) == (0, T) and plans[0][4] >= plans[0][2] > 0
            if gang and gang > 64:   # one chunk per started 64 rows of a shape: two or more for every g-row shape
                assert plans[0][4] >= 2 * plans[0][2] - 4
        monkeypatch.delenv("KB_EVAL_MATRIX_ROWS")
    e.close(); o.close()


# ---- c. k_argmax: all six instantiations, band widths, long lists, KB_NONE padding -----------------------------------------------------

@pytest.mark.parametrize("weights", ["default", "most", "sparse"])
@pytest.mark.parametrize("n_nodes", NODE_COUNTS)
def test_argmax_at_node_count_boundaries(oracle_mod, n_nodes, weights):
    """<= 512 rows per launch (1 024 threads) and 600 (256 threads below 65 536 nodes); k around the band width, 513 and 4 096 (longer than the
    feasible set at small N: KB_NONE padding).  kb_argmax_rows launches at most (1 << 20) / k rows at a time: k 4 096 runs 256-row launches."""
    T = 600
    snap = session(T, n_nodes, 800 + n_nodes % 991)
    cfg = cfg_of(weights)
    o, e = open_both(oracle_mod, cfg, snap)
    om, os_ = o.eval_matrix(0, T, 1)
    check_argmax(o, e, om, os_, 0, (300, 600), k_values(n_nodes, weights != "default"), f"N {n_nodes} {weights}")
    if weights == "sparse" and n_nodes > 1:
        sc = os_[feasible(om, n_nodes)]
        assert int(sc.max()) > 2000 and len(np.unique(sc)) > 8
    e.close(); o.close()


@pytest.mark.parametrize("weights", ["default", "most"])
@pytest.mark.parametrize("n_nodes", [63488, 65536])
def test_argmax_all_nodes_tied(oracle_mod, n_nodes, weights):
    """identical empty nodes, no selectors, nothing running: every row is feasible everywhere at ONE score, so one value of the band holds the
    whole node count — 63 488 in a 16-bit counter (the widest non-WIDE row), 65 536 (the narrowest WIDE row, where 16 bits would carry)"""
    T = 600
    snap = session(T, n_nodes, 90, node_cpu_cores=(32,), node_mem_gib=(128,), preload_node_frac=0.0, running_job_frac=0.0,
                   zone_selector_frac=0.0)
    o, e = open_both(oracle_mod, cfg_of(weights), snap)
    om, os_ = o.eval_matrix(0, T, 1)
    feas = feasible(om, n_nodes)
    tied = feas.all(axis=1) & (os_ == os_[:, :1]).all(axis=1)
    assert tied.mean() > 0.9, "the rows must tie across every node"
    check_argmax(o, e, om, os_, 0, (300, 600), k_values(n_nodes, weights != "default"), f"all tied N {n_nodes} {weights}")
    e.close(); o.close()


@pytest.mark.parametrize("n_nodes", [1, 2049, 16385, 63488, 65536, 66000])
def test_argmax_no_feasible_node_and_zero_scores(oracle_mod, n_nodes):
    """rows without any feasible node (a nodeSelector zone that holds no node) and rows whose feasible nodes all score 0 (mostrequested alone,
    small pods on big empty nodes): lists of KB_NONE, and lists of score-0 nodes in index order; the matrix of the same rows too"""
    T = 600
    snap = session(T, n_nodes, 95, node_cpu_cores=(32,), node_mem_gib=(128,), preload_node_frac=0.0, running_job_frac=0.0,
                   zone_selector_frac=0.4, task_cpu_milli=(100, 250), task_mem_mib=(128, 256))
    snap.node_class = (snap.node_class % 7).astype(np.uint32)     # zone 7 keeps its selector pods and loses its nodes
    snap._check()
    o, e = open_both(oracle_mod, cfg_of("zero"), snap)
    om, os_ = o.eval_matrix(0, T, 1)
    feas = feasible(om, n_nodes)
    assert (~feas.any(axis=1)).sum() >= 5 and feas.any(axis=1).sum() >= 300, "both kinds of row"
    assert int(os_.max()) == 0
    for flags in FLAG_SETS:
        em, es = e.eval_matrix(0, T, 1 | flags)
        assert_matrix_equal(em, es, om, os_, f"N {n_nodes} flags {hex(flags)}")
    check_argmax(o, e, om, os_, 0, (300, 600), k_values(n_nodes, True), f"zero scores N {n_nodes}")
    e.close(); o.close()


# ---- d. the whole-range plan kb_bench_matrix times (KB_EVAL_MATRIX_ROWS) --------------------------------------------------------------

_slice_digests = {}   # (case, first row) -> digest of the oracle's slice: the second commit-kernel run of a case does not re-run the oracle


def _digest(mask, score):
    return hashlib.sha256(mask.tobytes() + score.tobytes()).hexdigest()


def _whole_range_against_oracle(oracle_mod, case, cfg, snap, monkeypatch, capfd, slice_rows=8192):
    T = snap.n_tasks
    e = engine.Engine(cfg)
    e.load(snap)
    monkeypatch.setenv("KB_EVAL_MATRIX_ROWS", str(T))
    capfd.readouterr()
    t = time.time()
    em, es = e.eval_matrix(0, T, 1)
    t_engine = time.time() - t
    plans = _plans(capfd)
    monkeypatch.delenv("KB_EVAL_MATRIX_ROWS")
    e.close()
    assert len(plans) == 1 and plans[0][:2] == (0, T), plans
    o = None
    t = time.time()
    for a in range(0, T, slice_rows):
        b = min(T, a + slice_rows)
        ref = _slice_digests.get((case, a))
        if ref is not None and ref == _digest(em[a:b], es[a:b]):
            continue
        if o is None:
            o = oracle_mod.Oracle(cfg, snap, threads=8 if snap.n_nodes >= 4096 else 1)   # (its thread pool splits a row: slower than one thread on narrow rows)
        om, os_ = o.eval_matrix(a, b, 1)
        _slice_digests[(case, a)] = _digest(om, os_)
        assert_matrix_equal(em[a:b], es[a:b], om, os_, f"whole-range plan, rows [{a}, {b})")
    t_oracle = time.time() - t
    if o is not None:
        o.close()
    print(f"whole-range plan of {T} x {snap.n_nodes}: {plans[0]}; engine {t_engine:.1f} s, comparison {t_oracle:.1f} s")
    return plans[0]


@pytest.mark.parametrize("idx", [3, 4])
def test_whole_range_plan_full_size(oracle_mod, idx, monkeypatch, capfd):
    """BASELINE configs 3 and 4 at full size (100k x 10k; config 4: 16 resource dimensions under the bin-packing weights) as ONE plan of
    [0, T) — the plan kb_bench_matrix times — against the oracle, 8 192 rows at a time"""
    snap = snapmod.synth(snapmod.synth_config(idx))
    plan = _whole_range_against_oracle(oracle_mod, f"config {idx}", cfg_of("most" if idx == 4 else "default"), snap, monkeypatch, capfd)
    assert plan[3] == 0 and plan[4] > 0 and plan[5] == 1


def test_whole_range_plan_more_than_65535_chunks(oracle_mod, monkeypatch, capfd):
    """1.2M rows in 16-row jobs with their own requests on 2 000 nodes: ~75 000 shapes, ns * 16 <= n keeps the plan on the expansion path, and
    its chunk table (one chunk per 16-row shape, more for the shapes of colliding requests) is longer than k_expand_tiles' grid y may be
    (65 535): matrix_launch issues it in slices.  About 5 GB of scores on the device and on the host."""
    snap = session(1_200_000, 2000, 3, diverse_requests=True, gang_sizes=(16,), gang_probs=(1.0,))
    plan = _whole_range_against_oracle(oracle_mod, "1.2M rows", cfg_of("default"), snap, monkeypatch, capfd, slice_rows=65536)
    rows0, rows1, ns, direct, chunks, launches = plan
    assert direct == 0 and ns * 16 <= snap.n_tasks, plan
    assert chunks > 65535 and launches == (chunks + 65534) // 65535 >= 2, plan

"""The memory endpoint of the closed-loop network runs (csrc/model/icnt_closed.h
rule 2m; icnt_closed_loop_batch read_occupancy / write_occupancy /
write_reply_delay; icnt_closed_loop_networks occupancy / latency / mem_points;
booksim --mem-occupancy).

A memory node is one server, first come first served, with a pipelined latency
behind it, and replies leave a node in the order their requests arrived:

    start   = max(arr, busy[n])
    busy[n] = start + occ[i]
    ready   = busy[n] + lat[i]
    tinj    = ready  or  max(ready, last[n] + 1)
    last[n] = tinj

The model off is the call without it, word for word; a plain Python replay of
the recurrence recomputes every reply's creation time; hand-built lists pin the
in-order hold and a saturated server; the engines (``cpu-par``, ``gpu``) are
compared with ``cpu`` word for word.
"""
import json

import numpy as np
import pytest
import torch  # noqa: F401  (first: the process binds torch's HIP runtime before the host tests load the native module)

import test_icnt_closed_replay as crep
from accel_sim_framework_distributed_amd.icnt import booksim, capture

SIZES = crep.SIZES
MEM_KEYS = ("mem_time", "max_mem_time", "mem_wait", "mem_hold", "mem_utilisation", "max_mem_utilisation",
            "mem_nodes_used")
LIMIT = 1 << 24  # kRtClMemMax


def _mem_arrays(n, seed):
    """Per-request occupancy and latency, zero and non-zero mixed."""
    rng = np.random.default_rng(seed)
    occ = rng.choice(np.array([0, 0, 1, 3, 7, 20], np.uint32), n)
    lat = rng.choice(np.array([0, 0, 2, 5, 40, 100], np.uint32), n)
    assert (occ == 0).any() and (occ > 0).any() and (lat == 0).any() and (lat > 0).any()
    return occ, lat


def _replay_mem(r, dst, occ, lat):
    """Rule 2m from the request arrivals: per memory node in arrival order.
    Returns created, start and ready by request."""
    arr = r["request_arrivals"]
    n = len(arr)
    created, start, ready = (np.zeros(n, np.uint64) for _ in range(3))
    for node in np.unique(dst):
        idx = np.flatnonzero(dst == node)
        idx = idx[np.argsort(arr[idx], kind="stable")]
        assert (np.diff(arr[idx].astype(np.int64)) > 0).all(), node  # one ejection link: strictly increasing
        busy, last = 0, None
        for i in idx:
            s = max(int(arr[i]), busy)
            busy = s + int(occ[i])
            rd = busy + int(lat[i])
            t = rd if last is None else max(rd, last + 1)
            last = t
            created[i], start[i], ready[i] = t, s, rd
    return created, start, ready


def _check_summary(r, dst, occ, created, start, ready):
    """The summary fields against their numpy counterparts (sums of integers
    in doubles: exact)."""
    arr = r["request_arrivals"]
    n = len(arr)
    assert r["measured_requests"] == n
    mt = (created - arr).astype(np.float64)
    assert r["mem_time"] == mt.sum() / n and r["max_mem_time"] == mt.max()
    assert r["mem_wait"] == (start - arr).astype(np.float64).sum() / n
    assert r["mem_hold"] == (created - ready).astype(np.float64).sum() / n
    nodes = np.unique(dst)
    util = [float(occ[dst == node].astype(np.uint64).sum()) / float(max(r["batch_time"], 1)) for node in nodes]
    assert r["mem_nodes_used"] == len(nodes)
    assert r["mem_utilisation"] == pytest.approx(sum(util) / len(nodes), rel=1e-12)
    assert r["max_mem_utilisation"] == max(util)


# ---- 1. off is today ----

def test_off_is_today_replay(native):
    text = crep._icnt(**crep._mesh(4))
    lst = crep._list(16, 200, 7, spread=60)
    D, windows = 3, [0, 1, 3]
    ref = native.icnt_closed_loop_networks(lst, [text], windows, reply_delay=D, arrivals=True)
    assert all(r["deadlocked"] == 0 and r["batch_time"] > 0 for r in ref)
    assert all("mem" not in r and "mem_point" not in r for r in ref)
    for delay in (D, 0):  # under a memory point the point's latency answers, not reply_delay
        got = native.icnt_closed_loop_networks(lst, [text], windows, reply_delay=delay, arrivals=True,
                                               mem_points=[(0, D)])
        assert len(got) == len(ref)
        for g, r in zip(got, ref):
            assert g["deadlocked"] == 0 and (g.pop("mem_point"), g.pop("mem")) == (0, (0, D))
        crep._same(got, ref)
    for r in ref:
        assert np.array_equal(r["reply_created"], r["request_arrivals"] + np.uint64(D))
        assert (r["mem_time"], r["max_mem_time"], r["mem_wait"], r["mem_hold"]) == (D, D, 0, 0)
        assert r["mem_utilisation"] == 0 and r["mem_nodes_used"] == len(np.unique(lst[1]))


@pytest.mark.parametrize("M", [0, 1, 3])
def test_off_is_today_batch(native, M):
    text = crep._icnt(**crep._mesh(4))
    pt = dict(SIZES, batch_size=6, max_outstanding=M, seed=M + 2, reply_delay=2)
    ref = native.icnt_closed_loop_batch(text, [pt], arrivals=True)
    assert ref[0]["deadlocked"] == 0 and ref[0]["requests"] == 96
    # zero occupancies; and the model on with nothing to do (a write's latency that is reply_delay)
    for extra in (dict(read_occupancy=0, write_occupancy=0), dict(read_occupancy=0, write_occupancy=0, write_reply_delay=2),
                  dict(write_reply_delay=2)):
        got = native.icnt_closed_loop_batch(text, [dict(pt, **extra)], arrivals=True)
        assert got[0]["deadlocked"] == 0
        crep._same(got, ref)
    assert np.array_equal(ref[0]["reply_created"], ref[0]["request_arrivals"] + np.uint64(2))


# ---- 2. the rule, recomputed ----

RULE_WINDOWS = [1, 3, 0]
RULE_POINTS = ["list", (4, 6)]


def _rule_inputs(tmp):
    texts = [t for t, _ in crep._three_nets(tmp)]
    lst = crep._list(9, 120, 11, spread=40)
    assert lst[4][0] < lst[4][-1]
    occ, lat = _mem_arrays(120, 3)
    return texts, lst, occ, lat


def test_rule_recomputed(native, tmp_path):
    texts, lst, occ, lat = _rule_inputs(tmp_path)
    dst = lst[1]
    res = native.icnt_closed_loop_networks(lst, texts, RULE_WINDOWS, arrivals=True, nodes=9, occupancy=occ, latency=lat,
                                           mem_points=RULE_POINTS)
    assert [(r["network"], r["max_outstanding"], r["mem_point"], r["mem"]) for r in res] == \
        [(i, m, k, p) for i in range(3) for m in RULE_WINDOWS for k, p in enumerate(RULE_POINTS)]
    held = 0
    for r in res:
        assert r["deadlocked"] == 0 and r["requests"] == 120
        o, la = (occ, lat) if r["mem"] == "list" else (np.full(120, r["mem"][0], np.uint32), np.full(120, r["mem"][1], np.uint32))
        created, start, ready = _replay_mem(r, dst, o, la)
        assert r["reply_created"].dtype == np.uint64 and np.array_equal(r["reply_created"], created)
        assert (r["reply_arrivals"] > r["reply_created"]).all()
        assert r["batch_time"] == r["reply_arrivals"].max()
        _check_summary(r, dst, o, created, start, ready)
        if r["mem"] == "list":
            held += int((created > ready).sum())
            assert r["mem_wait"] > 0  # the servers queue
        else:
            assert r["mem_hold"] == 0  # equal latencies: nothing to hold
    assert held > 0  # the mixed latencies make the in-order return bind somewhere


# ---- 3. the hold binds, and does not ----

def _hold_inputs():
    """Four requests to node 8 of a 3x3 mesh from four nodes, 20 cycles apart:
    they arrive in list order, the last three long before the first's reply is
    ready."""
    src = np.array([0, 1, 2, 3], np.uint32)
    dst = np.full(4, 8, np.uint32)
    b = np.full(4, 32, np.uint32)
    tc = np.array([0, 20, 40, 60], np.uint64)
    occ = np.zeros(4, np.uint32)
    return crep._icnt(**crep._mesh(3)), (src, dst, b, b, tc), occ, np.array([100, 0, 0, 0], np.uint32)


def test_hold_binds_and_does_not(native):
    text, lst, occ, lat = _hold_inputs()
    call = native.icnt_closed_loop_networks
    r = call(lst, [text], [0], arrivals=True, occupancy=occ, latency=lat, mem_points=["list"])[0]
    arr = r["request_arrivals"]
    assert r["deadlocked"] == 0 and (np.diff(arr.astype(np.int64)) > 0).all() and arr[3] < arr[0] + 100
    assert r["reply_created"].tolist() == [int(arr[0]) + 100 + k for k in range(4)]
    hold = [0] + [int(arr[0]) + 100 + k - int(arr[k]) for k in (1, 2, 3)]
    assert r["mem_hold"] == sum(hold) / 4 > 0 and r["mem_wait"] == 0
    assert r["max_mem_time"] == max(100, max(hold)) and r["mem_utilisation"] == 0 and r["mem_nodes_used"] == 1
    # equal latencies: every reply leaves when it is ready
    e = call(lst, [text], [0], arrivals=True, occupancy=occ, latency=np.full(4, 100, np.uint32), mem_points=["list"])[0]
    assert e["deadlocked"] == 0 and e["mem_hold"] == 0 and e["mem_time"] == 100
    assert np.array_equal(e["reply_created"], e["request_arrivals"] + np.uint64(100))


# ---- 4. a saturated server ----

def _saturated_points(occupancies=(20,), windows=(0, 1)):
    return [dict(SIZES, batch_size=6, mem_nodes=1, max_outstanding=M, seed=4, read_occupancy=o, write_occupancy=o)
            for o in occupancies for M in windows]


def test_saturated_server(native):
    text = crep._icnt(**crep._mesh(3))
    for r in native.icnt_closed_loop_batch(text, _saturated_points(), arrivals=True):
        assert r["deadlocked"] == 0 and r["requests"] == 48 and (r["request_dst"] == 8).all()
        order = np.argsort(r["request_arrivals"], kind="stable")
        # every request reaches the node long before the server gets to it: the server never idles
        assert (np.diff(r["reply_created"][order].astype(np.int64)) == 20).all()
        assert r["reply_created"][order][0] == r["request_arrivals"][order][0] + 20
        assert r["batch_time"] >= 48 * 20 and r["max_mem_utilisation"] > 0.9 and r["mem_nodes_used"] == 1
        assert r["mem_utilisation"] == r["max_mem_utilisation"] == 48 * 20 / r["batch_time"]
        assert r["mem_hold"] == 0 and r["mem_wait"] > 0
    for M in (0, 1):
        bt = [r["batch_time"] for r in native.icnt_closed_loop_batch(text, _saturated_points((0, 5, 20), (M,)))]
        assert bt[0] <= bt[1] <= bt[2] and bt[0] < bt[2]


# ---- 5. the issue gate under the model ----

def test_gate_holds_under_the_model(native):
    src, dst, qb, pb, tc = crep._list(16, 400, 5, spread=150)
    text = crep._icnt(**crep._mesh(4))
    windows = [1, 2, 4]
    res = native.icnt_closed_loop_networks((src, dst, qb, pb, tc), [text], windows, arrivals=True, mem_points=[(6, 2)])
    for M, r in zip(windows, res):
        assert r["deadlocked"] == 0 and r["mem_wait"] > 0 and r["max_issue_stall"] > 0
        tiss, rep = r["tiss"], r["reply_arrivals"]
        for s in np.unique(src):
            idx = np.flatnonzero(src == s)
            for j, k in enumerate(idx):  # at every issue fewer than M of the node's earlier requests are outstanding
                assert int((rep[idx[:j]] > tiss[k]).sum()) < M, (M, s, k)
        assert np.array_equal(tiss, crep._replay_rule(dict(request_tinj=tc, reply_arrivals=rep, request_src=src), M))


# ---- 6. cpu-par == cpu ----

def _batch_grid():
    """Batch and rate points with per-kind occupancies and a write latency."""
    mem = dict(read_occupancy=3, write_occupancy=9, reply_delay=4, write_reply_delay=1)
    pts = [dict(SIZES, batch_size=4, max_outstanding=M, seed=2 + M, mem_nodes=mn, **mem) for M in (0, 2) for mn in (0, 3)]
    pts += [dict(SIZES, rate=0.2, cycles=300, warmup=50, max_outstanding=2, seed=9, **mem),
            dict(SIZES, batch_size=4, max_outstanding=1, seed=3, reply_delay=4)]  # one point with the model off
    return crep._icnt(**crep._mesh(4)), pts


def _engine_calls(mod, tmp, engine, **kw):
    """The inputs of tests 2, 3 and 4 and the batch grid through one engine."""
    texts, lst, occ, lat = _rule_inputs(tmp)
    out = [mod.icnt_closed_loop_networks(lst, texts, RULE_WINDOWS, engine=engine, arrivals=True, nodes=9, occupancy=occ,
                                         latency=lat, mem_points=RULE_POINTS, **kw)]
    text, lst, occ, lat = _hold_inputs()
    out.append(mod.icnt_closed_loop_networks(lst, [text], [0], engine=engine, arrivals=True, occupancy=occ, latency=lat,
                                             mem_points=["list", (0, 100)], **kw))
    out.append(mod.icnt_closed_loop_batch(crep._icnt(**crep._mesh(3)), _saturated_points((0, 5, 20)), engine=engine,
                                          arrivals=True, **kw))
    text, pts = _batch_grid()
    out.append(mod.icnt_closed_loop_batch(text, pts, engine=engine, arrivals=True, **kw))
    return out


def test_cpu_par_equals_cpu(native, tmp_path):
    ref = _engine_calls(native, tmp_path, "cpu")
    for rs in ref:
        assert all(r["deadlocked"] == 0 and "reply_created" in r for r in rs)
    grid = ref[3]
    assert grid[0]["reads"] and grid[0]["writes"] and grid[0]["mem_wait"] > 0 and grid[4]["measured_requests"] > 0
    for got, rs in zip(_engine_calls(native, tmp_path, "cpu-par"), ref):
        crep._same(got, rs)


# ---- 7. refusals and the CLI ----

def test_refusals_name_the_argument(native):
    lst = crep._list(16, 40, 3, spread=10)
    text = crep._icnt(**crep._mesh(4))
    call = native.icnt_closed_loop_networks
    occ, lat = _mem_arrays(40, 1)
    assert call(lst, [text], [1], occupancy=occ, latency=lat, mem_points=["list"])[0]["deadlocked"] == 0
    with pytest.raises(ValueError, match=r"occupancy has 39 entries, the list 40"):
        call(lst, [text], [1], occupancy=occ[:-1], latency=lat, mem_points=["list"])
    with pytest.raises(ValueError, match=r"latency has 39 entries, the list 40"):
        call(lst, [text], [1], occupancy=occ, latency=lat[:-1], mem_points=["list"])
    for name in ("occupancy", "latency"):
        big = {"occupancy": occ.copy(), "latency": lat.copy()}
        big[name][5] = LIMIT + 1
        with pytest.raises(ValueError, match=rf"{name} of request 5 is above 2\^24"):
            call(lst, [text], [1], mem_points=["list"], **big)
        big[name][5] = LIMIT  # the limit itself is taken
        assert call(lst, [text], [1], mem_points=["list"], **big)[0]["deadlocked"] == 0
        neg = {"occupancy": occ.astype(np.int64), "latency": lat.astype(np.int64)}
        neg[name][7] = -1
        with pytest.raises(ValueError, match=rf"{name} of request 7 is negative"):
            call(lst, [text], [1], mem_points=["list"], **neg)
        with pytest.raises(ValueError, match=rf"{name} is missing"):
            call(lst, [text], [1], mem_points=["list"], **{k: v for k, v in big.items() if k != name})
    with pytest.raises(ValueError, match=r"mem_points\[1\] is `list`, but the list has no occupancy and latency"):
        call(lst, [text], [1], mem_points=[(0, 2), "list"])
    for bad in ((LIMIT + 1, 0), (0, LIMIT + 1)):
        with pytest.raises(ValueError, match=r"mem_points\[0\] has an occupancy or latency above 2\^24"):
            call(lst, [text], [1], mem_points=[bad])
    for bad in ((-1, 0), (0, -3)):
        with pytest.raises(ValueError, match=r"mem_points\[1\] has a negative"):
            call(lst, [text], [1], mem_points=[(1, 1), bad])
    with pytest.raises(ValueError, match=r"mem_points\[0\]"):
        call(lst, [text], [1], mem_points=["lists"])
    pt = dict(SIZES, batch_size=2, max_outstanding=1)
    for key in ("read_occupancy", "write_occupancy", "write_reply_delay"):
        with pytest.raises(ValueError, match=rf"point 0: {key} is negative"):
            native.icnt_closed_loop_batch(text, [dict(pt, **{key: -1})])
        with pytest.raises(ValueError, match=rf"point 1: {key} \d+ is above 2\^24"):
            native.icnt_closed_loop_batch(text, [pt, dict(pt, **{key: LIMIT + 1})])
    with pytest.raises(ValueError, match=r"point 0: reply_delay \d+ is above 2\^24"):
        native.icnt_closed_loop_batch(text, [dict(pt, read_occupancy=1, reply_delay=LIMIT + 1)])
    assert native.icnt_closed_loop_batch(text, [dict(pt, reply_delay=LIMIT + 1)])[0]["deadlocked"] == 0  # as before


def test_cli(native, tmp_path, capsys):
    nets = []
    for name, kw in (("mesh", crep._mesh(3)), ("fly", dict(k=3, n=2, topology="fly"))):
        f = tmp_path / f"{name}.icnt"
        f.write_text(crep._icnt(**kw))
        nets.append(str(f))
    src, dst, qb, pb, tc = crep._list(9, 80, 13, spread=30)
    occ, lat = _mem_arrays(80, 5)
    rl = capture.RequestList(src, dst, qb, pb, tc, np.ones(80, np.uint8), 9)
    npz, bare = str(tmp_path / "mem.npz"), str(tmp_path / "bare.npz")
    capture.save_request_npz(npz, rl, occupancy=occ, latency=lat)
    capture.save_request_npz(bare, rl)
    with np.load(npz) as z, np.load(bare) as zb:
        assert np.array_equal(z["occupancy"], occ) and z["latency"].dtype == np.uint32 and "occupancy" not in zb
    with pytest.raises(ValueError, match="occupancy and latency go together"):
        capture.save_request_npz(bare, rl, occupancy=occ)
    out = tmp_path / "grid.json"
    argv = ["--closed-loop", "--replay", npz, "--networks", ",".join(nets), "--max-outstanding", "2",
            "--reply-delay", "4", "--mem-occupancy", "0,4,list", "--json", str(out)]
    assert booksim.main(argv) == 0
    printed = capsys.readouterr().out
    assert printed.count("Memory time = ") == 6 and printed.count("memory occupancy from the list") == 2
    got = json.loads(out.read_text())
    assert got["mem_points"] == [[0, 4], [4, 4], "list"]
    assert [(g["config"], g["mem_point"], g["mem"]) for g in got["grid"]] == \
        [(n, k, m) for n in nets for k, m in enumerate(([0, 4], [4, 4], "list"))]
    ref = booksim.closed_loop_replay(src, dst, qb, pb, tc, [open(n).read() for n in nets], [2], reply_delay=4, nodes=9,
                                     occupancy=occ, latency=lat, mem_points=[(0, 4), (4, 4), "list"])
    for g, r in zip(got["grid"], ref):
        assert r["deadlocked"] == 0 and g["batch_time"] == r["batch_time"]
        assert all(g[k] == r[k] for k in MEM_KEYS)
    assert ref[1]["mem_time"] > ref[0]["mem_time"] == 4
    # the word `list` needs the arrays
    assert booksim.main(argv[:2] + [bare] + argv[3:]) == 2
    assert "occupancy and latency" in capsys.readouterr().err
    # synthetic traffic: the axis, and a write's latency
    out2 = tmp_path / "batch.json"
    assert booksim.main([nets[0], "--closed-loop", "--batch-size", "4", "--mem-nodes", "2", "--max-outstanding", "2",
                         "--reply-delay", "5", "--write-reply-delay", "1", "--mem-occupancy", "0,8", "--json",
                         str(out2)]) == 0
    assert capsys.readouterr().out.count("Memory time = ") == 2
    curve = json.loads(out2.read_text())["curve"]
    assert [c["mem_occupancy"] for c in curve] == [0, 8] and all(k in c for c in curve for k in MEM_KEYS)
    assert all(c["deadlocked"] == 0 for c in curve)
    assert 1 < curve[0]["mem_time"] < 5 and curve[0]["mem_utilisation"] == 0 < curve[1]["mem_utilisation"]
    assert curve[1]["batch_time"] >= curve[0]["batch_time"] and curve[1]["mem_nodes_used"] == 2
    assert booksim.main([nets[0], "--closed-loop", "--batch-size", "4", "--mem-occupancy", "list"]) == 2
    capsys.readouterr()


# ---- the device ----

@pytest.fixture(scope="module")
def gpu_native():
    import torch  # bind torch's HIP runtime first
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    from accel_sim_framework_distributed_amd import _native
    mod = _native.load(prefer_torch_runtime=True)
    assert mod.gpu_available(), "HIP device not usable (native code must run, no silent fallback)"
    return mod


@pytest.fixture(scope="module")
def cpu_reference(gpu_native, tmp_path_factory):
    """The four calls through the defining engine, once for both placements."""
    ref = _engine_calls(gpu_native, tmp_path_factory.mktemp("icnt_mem_ref"), "cpu")
    assert all(r["deadlocked"] == 0 for rs in ref for r in rs)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("lds", [True, False])
def test_gpu_equals_cpu(gpu_native, cpu_reference, tmp_path, lds):
    """The inputs of tests 2, 3 and 4 and the batch grid, the per-(unit, VC)
    words in LDS and forced to HBM."""
    got = _engine_calls(gpu_native, tmp_path, "gpu", lds=lds)
    for g, r in zip(got, cpu_reference):
        assert all("reply_created" in x for x in g)
        crep._same(g, r)
    assert gpu_native.icnt_open_loop_batch_stats()["lds_chunks"] == (1 if lds else 0)


@pytest.mark.gpu
def test_gpu_chunk_boundary_inside_the_memory_axis(gpu_native):
    """One network and one window under four memory points and a budget that
    takes fewer than four units: every chunk boundary falls inside the
    memory-point axis, and the list's arrays go up with every chunk."""
    text = crep._icnt(**crep._mesh(4))
    lst = crep._list(16, 600, 23, spread=100)  # (a unit of this list takes over 0.4 MB)
    occ, lat = _mem_arrays(600, 8)
    points = [(0, 3), "list", (5, 0), (2, 9)]
    kw = dict(arrivals=True, occupancy=occ, latency=lat, mem_points=points)
    ref = gpu_native.icnt_closed_loop_networks(lst, [text], [2], engine="cpu", **kw)
    got = gpu_native.icnt_closed_loop_networks(lst, [text], [2], engine="gpu", mem_budget_mb=1, **kw)
    st = gpu_native.icnt_open_loop_batch_stats()
    print("chunk stats:", st)
    assert all(r["deadlocked"] == 0 for r in ref) and [r["mem"] for r in got] == points
    crep._same(got, ref)
    assert st["chunks"] >= 2 and st["max_chunk_points"] < 4 and st["max_chunk_bytes"] <= st["budget_bytes"] == 1 << 20, st

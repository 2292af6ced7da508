"""Closed-loop request-reply points with bounded windows
(icnt_closed_loop_batch, csrc/model/icnt_closed.h).

The new pass is tied to what exists: with an unlimited window a rate point is
the open-loop request-reply point, arrival for arrival; a lone issuer with a
window of one is a chain of lone-packet round trips measured by one-packet
replays; on contended runs a plain Python replay of the issue rule recomputes
every issue time from the creation times and the returned reply arrivals.  The
engines (``cpu-par``, ``gpu``) are then compared with ``cpu`` word for word.
References are computed once per module and left unchanged.
"""
import numpy as np
import pytest
import torch  # noqa: F401  (first: the process binds torch's HIP runtime before the host tests load the native module)

from accel_sim_framework_distributed_amd.models import presets

SIZES = dict(read_request_size=1, read_reply_size=3, write_request_size=3, write_reply_size=1)
ORDER_FREE = ("islip", "separable_input_first", "separable_output_first", "max_size", "loa")
ALLOCATORS = ORDER_FREE + ("wavefront", "pim")


def _icnt(**kw):
    base = dict(num_vcs="2", vc_buf_size="4", internal_speedup="1.0", flit_size="32")
    base.update(kw)
    return presets.render_icnt(presets.icnt_params(**base))


def _mesh(k):
    return dict(k=k, n=2, topology="mesh")


def _anynet_mesh(tmp, k=4):
    """The k x k mesh of test_router_anynet_network_file as an anynet file."""
    lines = []
    for y in range(k):
        for x in range(k):
            r = y * k + x
            parts = [f"router {r}", f"node {r}"]
            if x + 1 < k:
                parts.append(f"router {r + 1}")
            if y + 1 < k:
                parts.append(f"router {r + k}")
            lines.append(" ".join(parts))
    f = tmp / f"mesh{k}{k}.anynet"
    f.write_text("\n".join(lines) + "\n")
    return dict(k=k, topology="anynet", network_file=str(f))


def _same(got, ref):
    """Two result lists equal in every returned word: arrays by content and
    type, nested dicts and scalars exactly."""
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert list(g) == list(r), i
        for key, rv in r.items():
            if isinstance(rv, np.ndarray):
                assert g[key].dtype == rv.dtype and np.array_equal(g[key], rv), (i, key)
            else:
                assert g[key] == rv, (i, key)


# ---- 1. an unlimited window is the open-loop request-reply mode ----

def _open_nets(tmp):
    return {
        "mesh3": (_mesh(3), 1.0),
        "mesh4": (_mesh(4), 1.0),
        "fly22": (dict(k=2, n=2, topology="fly"), 1.0),
        "torus4": (dict(k=4, n=2, topology="torus"), 1.0),
        "anynet4": (_anynet_mesh(tmp), 1.0),
    }


def _anynet_doubled(tmp, k):
    """Two copies of the k x k anynet mesh, routers and nodes [0, k*k) and
    [k*k, 2*k*k), joined by one 10000-cycle channel that no route uses (an
    anynet graph must be connected)."""
    n = k * k
    lines = []
    for c in range(2):
        for y in range(k):
            for x in range(k):
                r = y * k + x
                parts = [f"router {c * n + r}", f"node {c * n + r}"]
                if x + 1 < k:
                    parts.append(f"router {c * n + r + 1}")
                if y + 1 < k:
                    parts.append(f"router {c * n + r + k}")
                if r == 0:
                    parts.append(f"router {(1 - c) * n} 10000")
                lines.append(" ".join(parts))
    f = tmp / f"mesh{k}{k}x2.anynet"
    f.write_text("\n".join(lines) + "\n")
    return dict(k=2 * n, topology="anynet", network_file=str(f))


@pytest.mark.parametrize("k", [3, 4])
def test_one_pass_over_two_copies_is_two_passes(native, tmp_path, k):
    """What the closed-loop pass rests on, with the replay interface alone: a
    contended request list and the replies built from its arrivals, replayed
    as 800 packets on the doubled network, arrive as in one replay per subnet
    on the single network.  Whole speedups only: a fractional speedup adds its
    passes per loop iteration, and one pass over both copies iterates through
    the union of their busy cycles, so the cycles that get the extra pass
    differ (the engines still agree with each other: test_cpu_equals_cpu_par)."""
    n = k * k
    rng = np.random.default_rng(k)
    src = rng.integers(0, n, 400).astype(np.uint32)
    dst = ((src + rng.integers(1, n, 400)) % n).astype(np.uint32)
    fl = rng.choice([1, 3], 400).astype(np.uint32)
    tinj = np.sort(rng.integers(0, 60, 400)).astype(np.uint64)
    one, two = _anynet_mesh(tmp_path, k), _anynet_doubled(tmp_path, k)
    apart = np.arange(400, dtype=np.uint64) * np.uint64(1000)  # one packet at a time: the zero-load latency
    zero = (native.icnt_replay_batch(_icnt(**one), [(src, dst, fl, apart)], arrivals=True)[0]["arrivals"] - apart).mean()
    for alloc in ORDER_FREE:
        for speedup in ("1.0", "2.0"):
            kw = dict(sw_allocator=alloc, internal_speedup=speedup, alloc_iters=2)
            req = native.icnt_replay_batch(_icnt(**one, **kw), [(src, dst, fl, tinj)], arrivals=True)[0]["arrivals"]
            assert (req - tinj).mean() >= 1.25 * zero, (alloc, speedup, (req - tinj).mean(), zero)  # contended
            o = np.argsort(req, kind="stable")
            rep = (dst[o], src[o], (4 - fl[o]).astype(np.uint32), req[o] + np.uint64(3))
            rep_arr = native.icnt_replay_batch(_icnt(**one, **kw), [rep], arrivals=True)[0]["arrivals"]
            both = (np.concatenate([src, rep[0] + n]).astype(np.uint32), np.concatenate([dst, rep[1] + n]).astype(np.uint32),
                    np.concatenate([fl, rep[2]]), np.concatenate([tinj, rep[3]]))
            got = native.icnt_replay_batch(_icnt(**two, **kw), [both], arrivals=True)[0]["arrivals"]
            assert np.array_equal(got[:400], req) and np.array_equal(got[400:], rep_arr), (alloc, speedup)


@pytest.mark.parametrize("name", ["mesh3", "mesh4", "fly22", "torus4", "anynet4"])
def test_unlimited_window_equals_open_loop(native, tmp_path, name):
    """max_outstanding = 0 against icnt_request_reply_batch on the same
    parameters: request arrivals, reply arrivals through reply_of, reads,
    writes and the activity of both subnets, for the five allocators whose
    matching does not depend on unit indices, speedups 1 and 2, 1- and 3-flit
    packets.  The rate loads the network: the open-loop request latency is at
    least 1.5 times its zero-load latency (asserted).

    switch_passes and credits are left out of the activity comparison: they
    depend on where a pass's loop runs, not on the packets alone.  One pass
    over both subnets steps through the union of their busy cycles where two
    passes each skip their own idle cycles, and a pass ends with its last
    delivery, the credits of its last flits still in flight: the request
    subnet's are returned here, while the replies travel, and not there.
    Every other count is a sum over events of the packets."""
    keys, rate = _open_nets(tmp_path)[name]
    for alloc in ORDER_FREE:
        for speedup in ("1.0", "2.0"):
            text = _icnt(**keys, sw_allocator=alloc, internal_speedup=speedup, alloc_iters=2, vc_buf_size=2)
            pts = [dict(SIZES, traffic="uniform", rate=rate, seed=3, cycles=160, warmup=20, write_fraction=0.9,
                        reply_delay=d, mem_nodes=m) for d, m in ((0, 0), (5, 0), (3, 2))]
            ref = native.icnt_request_reply_batch(text, pts, engine="cpu", arrivals=True)
            got = native.icnt_closed_loop_batch(text, [dict(p, max_outstanding=0) for p in pts], engine="cpu",
                                                arrivals=True)
            for p, r, g in zip(pts, ref, got):
                tag = (name, alloc, speedup, p["reply_delay"], p["mem_nodes"])
                assert r["request"]["packets"] > 50 and r["deadlocked"] == 0, tag
                assert r["request"]["avg_latency"] >= 1.5 * r["request"]["zero_load_latency"], tag
                assert np.array_equal(g["request_src"], r["request_src"]), tag
                assert np.array_equal(g["request_tinj"], r["request_tinj"]), tag
                assert np.array_equal(g["tiss"], r["request_tinj"]), tag
                assert np.array_equal(g["request_arrivals"], r["request_arrivals"]), tag
                assert np.array_equal(g["reply_arrivals"][r["reply_of"]], r["reply_arrivals"]), tag
                assert (g["reads"], g["writes"], g["deadlocked"]) == (r["reads"], r["writes"], 0), tag
                for k, v in g["activity"].items():
                    if k not in ("switch_passes", "credits"):
                        assert v == r["request"]["activity"][k] + r["reply"]["activity"][k], tag + (k,)
                assert g["issue_stall"] == 0 and g["batch_time"] == 0, tag


# ---- 2. one issuer, a window of one ----

@pytest.mark.parametrize("net", ["fly", "pair"])
def test_one_issuer_window_one_is_a_chain_of_round_trips(native, tmp_path, net):
    """Node 0 sends a batch of 8 to node 1 with M = 1: request k + 1 is issued
    in the cycle reply k arrives, every round trip is the lone-packet latency
    of the pair on each subnet (one-packet replays) plus reply_delay, and the
    batch time is 8 of them."""
    if net == "pair":  # two routers joined by a 5-cycle channel (1 cycle back), one node each
        g = tmp_path / "pair.anynet"
        g.write_text("router 0 node 0 router 1 5\nrouter 1 node 1\n")
        text = _icnt(k=2, topology="anynet", network_file=str(g))
    else:
        text = _icnt(k=2, n=1)
    lone = lambda s, d, fl: int(native.icnt_replay_batch(
        text, [(np.array([s], np.uint32), np.array([d], np.uint32), np.array([fl], np.uint32),
                np.array([0], np.uint64))], arrivals=True)[0]["arrivals"][0])
    for wf, (f_req, f_rep) in ((0.0, (1, 3)), (1.0, (3, 1))):
        for delay in (0, 4):
            r = native.icnt_closed_loop_batch(text, [dict(SIZES, batch_size=8, max_outstanding=1, mem_nodes=1,
                                                          write_fraction=wf, reply_delay=delay)], arrivals=True)[0]
            trip = lone(0, 1, f_req) + delay + lone(1, 0, f_rep)
            assert r["requests"] == 8 and list(r["request_src"]) == [0] * 8 and list(r["request_dst"]) == [1] * 8
            assert list(r["request_flits"]) == [f_req] * 8
            assert list(r["tiss"][1:]) == list(r["reply_arrivals"][:-1]) and r["tiss"][0] == 0
            assert list(r["reply_arrivals"] - r["tiss"]) == [trip] * 8
            assert r["batch_time"] == 8 * trip == r["last_finish"] == r["first_finish"]
            assert r["round_trip_latency"] == trip and r["deadlocked"] == 0


# ---- 3. the gate on contended runs ----

def _replay_rule(r, M):
    """Rule 1 from the creation times and the reply arrivals: per node in list
    order, the smallest t >= max(tinj, previous issue) with fewer than M of
    the node's earlier requests outstanding (a reply arriving at t frees t)."""
    tinj, rep, src = r["request_tinj"], r["reply_arrivals"], r["request_src"]
    tiss = np.zeros(len(tinj), np.uint64)
    for s in np.unique(src):
        prev, earlier = 0, []
        for k in np.flatnonzero(src == s):
            t = max(int(tinj[k]), prev)
            while M and sum(a > t for a in earlier) >= M:
                t = min(a for a in earlier if a > t)
            tiss[k] = prev = t
            earlier.append(int(rep[k]))
    return tiss


@pytest.mark.parametrize("mem_nodes", [0, 4])
def test_gate_replayed_in_python(native, mem_nodes):
    text = _icnt(**_mesh(4))
    pts = [dict(SIZES, batch_size=32, max_outstanding=M, seed=M + 1, write_fraction=wf, mem_nodes=mem_nodes,
                reply_delay=2) for M in (1, 2, 4) for wf in (0.0, 1.0, 0.5)]  # reply sizes 3, 1 and mixed
    res = native.icnt_closed_loop_batch(text, pts, arrivals=True)
    for p, r in zip(pts, res):
        M = p["max_outstanding"]
        assert r["requests"] == 32 * (16 - mem_nodes) and r["deadlocked"] == 0
        assert np.array_equal(r["tiss"], _replay_rule(r, M)), p
        assert r["max_issue_stall"] > 0 and r["batch_time"] == r["reply_arrivals"].max()
        # contended: the round trips are not all one lone-packet latency
        assert len(set((r["reply_arrivals"] - r["tiss"]).tolist())) > 4
        assert 0 < r["avg_outstanding"] <= M
    # a wider window finishes the batch sooner
    bt = {(p["max_outstanding"], p["write_fraction"]): r["batch_time"] for p, r in zip(pts, res)}
    assert bt[(1, 0.5)] > bt[(2, 0.5)] > bt[(4, 0.5)]


# ---- 4. cpu == cpu-par ----

def _engine_grid():
    """Every allocator, speedup, VC count, buffer depth, credit delay and
    window at least once on either mesh: (icnt keys, points)."""
    grid = []
    speed, vcs, buf, cred = ("1.0", "1.5", "2.0"), (1, 2, 4), (1, 4), (0, 2)
    i = 0
    for k in (6, 2):
        for alloc in ALLOCATORS:
            for M in (0, 1, 3):
                keys = dict(_mesh(k), sw_allocator=alloc, alloc_iters=2, internal_speedup=speed[i % 3],
                            num_vcs=vcs[(i // 3) % 3], vc_buf_size=buf[(i // 2) % 2], credit_delay=cred[i % 2])
                grid.append((keys, [dict(SIZES, batch_size=4, max_outstanding=M, seed=i + 1, reply_delay=i % 4)]))
                i += 1
    return grid


def test_engine_grid_covers_every_value():
    g = _engine_grid()
    for key, vals in (("sw_allocator", set(ALLOCATORS)), ("internal_speedup", {"1.0", "1.5", "2.0"}),
                      ("num_vcs", {1, 2, 4}), ("vc_buf_size", {1, 4}), ("credit_delay", {0, 2}), ("k", {6, 2})):
        assert {keys[key] for keys, _ in g} == vals
    assert {p[0]["max_outstanding"] for _, p in g} == {0, 1, 3}


def test_cpu_equals_cpu_par(native):
    for keys, pts in _engine_grid():
        text = _icnt(**keys)
        ref = native.icnt_closed_loop_batch(text, pts, engine="cpu", arrivals=True)
        assert ref[0]["requests"] == 4 * keys["k"] ** 2 and ref[0]["deadlocked"] == 0, keys
        _same(native.icnt_closed_loop_batch(text, pts, engine="cpu-par", arrivals=True), ref)
    # rate points, a loaded network
    text = _icnt(**_mesh(4))
    pts = [dict(SIZES, rate=0.8, cycles=150, warmup=20, max_outstanding=M, seed=M + 5) for M in (0, 2)]
    ref = native.icnt_closed_loop_batch(text, pts, engine="cpu", arrivals=True)
    assert ref[1]["issue_stall"] > 0 == ref[0]["issue_stall"]
    _same(native.icnt_closed_loop_batch(text, pts, engine="cpu-par", arrivals=True), ref)


# ---- 5. refusals ----

def test_refusals_name_the_key(native):
    pt = dict(SIZES, batch_size=2, max_outstanding=1)
    for rf in ("min_adapt", "valiant"):
        with pytest.raises(ValueError, match=rf):
            native.icnt_closed_loop_batch(_icnt(**_mesh(4), routing_function=rf), [pt])
    with pytest.raises(ValueError, match="batch_count"):
        native.icnt_closed_loop_batch(_icnt(**_mesh(4)), [dict(pt, batch_count=2)])
    with pytest.raises(ValueError, match="batch_count"):
        native.icnt_closed_loop_batch(_icnt(**_mesh(4), batch_count=2), [pt])
    for m in (16, 17):
        with pytest.raises(ValueError, match="mem_nodes"):
            native.icnt_closed_loop_batch(_icnt(**_mesh(4)), [dict(pt, mem_nodes=m)])
    with pytest.raises(ValueError, match="unknown field"):
        native.icnt_closed_loop_batch(_icnt(**_mesh(4)), [dict(pt, window=2)])


# ---- 6. a capped pass raises ----

@pytest.mark.parametrize("engine", ["cpu", "cpu-par"])
def test_capped_pass_raises(native, engine):
    pt = dict(SIZES, batch_size=8, max_outstanding=2)
    with pytest.raises(RuntimeError, match="loop guard"):
        native.icnt_closed_loop_batch(_icnt(**_mesh(4)), [pt], engine=engine, step_cap=5)
    assert native.icnt_closed_loop_batch(_icnt(**_mesh(4)), [pt], engine=engine)[0]["deadlocked"] == 0


# ---- the python interface ----

def test_closed_loop_sweep_and_cli(native, tmp_path, capsys):
    from accel_sim_framework_distributed_amd.icnt import booksim
    text = _icnt(**_mesh(4), sim_type="batch", batch_size=6, max_outstanding_requests=2)
    curve = booksim.closed_loop_sweep(text, max_outstanding=[1, 4, 0], batch_size=8, traffic=["uniform", "transpose"],
                                      seeds=[1, 2])
    assert [(c["traffic"], c["max_outstanding"]) for c in curve] == [
        (t, m) for t in ("uniform", "transpose") for m in (1, 4, 0)]
    for t in ("uniform", "transpose"):
        bt = [c["batch_time"] for c in curve if c["traffic"] == t]
        assert bt[0] > bt[1] >= bt[2] > 0
    assert all(c["seeds"] == 2 and c["deadlocked"] == 0 for c in curve)
    # the .icnt keys are the command line's defaults
    cfg = tmp_path / "net.icnt"
    cfg.write_text(text)
    out = tmp_path / "curve.json"
    assert booksim.main([str(cfg), "--closed-loop", "--json", str(out)]) == 0
    printed = capsys.readouterr().out
    assert "Batch received. Time used is" in printed
    import json
    got = json.loads(out.read_text())
    assert got["closed_loop"] and got["batch_size"] == 6 and [c["max_outstanding"] for c in got["curve"]] == [2]
    ref = native.icnt_closed_loop_batch(text, [dict(batch_size=6, max_outstanding=2, traffic="uniform", seed=1)])[0]
    assert got["curve"][0]["batch_time"] == ref["batch_time"]
    assert booksim.main([str(cfg), "--closed-loop", "--max-outstanding", "1,0", "--batch-size", "3"]) == 0
    assert capsys.readouterr().out.count("Batch received.") == 2


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


def _gpu_grid():
    """A cut of the engine grid: three meshes, three allocators (max_size is
    an ordered one), every window, both point kinds."""
    grid = []
    i = 0
    for k in (2, 4, 6):
        for alloc, speedup, vcs in (("islip", "1.0", 2), ("separable_input_first", "1.5", 1), ("max_size", "2.0", 4)):
            keys = dict(_mesh(k), sw_allocator=alloc, alloc_iters=2, internal_speedup=speedup, num_vcs=vcs,
                        vc_buf_size=(1, 4)[i % 2], credit_delay=(0, 2)[i % 2])
            pts = [dict(SIZES, batch_size=4, max_outstanding=M, seed=i + M + 1, reply_delay=M) for M in (0, 1, 3)]
            pts.append(dict(SIZES, rate=0.6, cycles=60, warmup=10, max_outstanding=2, seed=i + 9))
            grid.append((keys, pts))
            i += 1
    return grid


@pytest.mark.gpu
@pytest.mark.parametrize("lds", [True, False])
def test_gpu_equals_cpu(gpu_native, lds):
    for keys, pts in _gpu_grid():
        text = _icnt(**keys)
        ref = gpu_native.icnt_closed_loop_batch(text, pts, engine="cpu", arrivals=True)
        got = gpu_native.icnt_closed_loop_batch(text, pts, engine="gpu", arrivals=True, lds=lds)
        _same(got, ref)
        st = gpu_native.icnt_open_loop_batch_stats()
        assert st["chunks"] == 1 and st["lds_chunks"] == (1 if lds else 0), (keys, st)


@pytest.mark.gpu
def test_gpu_memory_budget_splits_the_grid(gpu_native):
    text = _icnt(**_mesh(4))
    pts = [dict(SIZES, batch_size=64, max_outstanding=M, seed=s) for M in (1, 4, 0) for s in (1, 2)]
    ref = gpu_native.icnt_closed_loop_batch(text, pts, engine="cpu", arrivals=True)
    _same(gpu_native.icnt_closed_loop_batch(text, pts, engine="gpu", arrivals=True, mem_budget_mb=1), ref)
    st = gpu_native.icnt_open_loop_batch_stats()
    assert st["chunks"] >= 2 and st["max_chunk_bytes"] <= st["budget_bytes"] == 1 << 20


@pytest.mark.gpu
def test_gpu_kernel_resources(gpu_native):
    info = gpu_native.icnt_cl_kernel_info()
    assert info["max_threads_per_block"] == 64 and info["lds_bytes"] == 0  # the hot words are dynamic LDS
    assert 0 < info["num_regs"] <= 512

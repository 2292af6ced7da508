"""Closed-loop replay of a request list across networks and windows
(icnt_closed_loop_networks, csrc/model/icnt_closed.h rt_cl_fill_list,
csrc/engine/icnt_cln_sweep.hip; icnt/capture.py request_list; booksim
--closed-loop --replay).

The new call is tied to what exists: a batch point of icnt_closed_loop_batch,
rebuilt as a list in bytes, comes back word for word; every network's flit
counts are those of capture.flits_for; a plain Python replay of the issue rule
recomputes every issue time of a contended list with creation times.  The
engines (``cpu-par``, ``gpu``) are then compared with ``cpu`` word for word.
"""
import json

import numpy as np
import pytest
import torch  # noqa: F401  (first: the process binds torch's HIP runtime before the host tests load the native module)

import test_router_pass_par as rpass
from accel_sim_framework_distributed_amd.icnt import booksim, capture
from accel_sim_framework_distributed_amd.models import presets

SIZES = dict(read_request_size=1, read_reply_size=3, write_request_size=3, write_reply_size=1)
ORDER_FREE = ("islip", "separable_input_first", "separable_output_first", "max_size", "loa")
MAX_PKT = 136  # kRtMaxPktBytes
MAX_REQUESTS = 25_000_000  # kReplayMaxPackets / 2
WORDS = ("tiss", "request_arrivals", "reply_arrivals", "state", "request_flit_counts", "reply_flit_counts")


def _icnt(**kw):
    base = dict(num_vcs="2", vc_buf_size="4", internal_speedup="1.0", flit_size="32")
    base.update(kw)
    return presets.render_icnt(presets.icnt_params(**base))


def _mesh(k):
    return dict(k=k, n=2, topology="mesh")


def _anynet_mesh(tmp, k):
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


def _list(nodes, n, seed, spread=0, sizes=((8, 136), (136, 8), (40, 40))):
    """n requests among `nodes` nodes, (request, reply) bytes drawn from
    `sizes`, creation times sorted over [0, spread]."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, nodes, n).astype(np.uint32)
    dst = ((src + rng.integers(1, nodes, n)) % nodes).astype(np.uint32)
    pick = rng.integers(0, len(sizes), n)
    sz = np.array(sizes, np.uint32)
    tc = np.sort(rng.integers(0, spread + 1, n)).astype(np.uint64)
    return src, dst, sz[pick, 0].copy(), sz[pick, 1].copy(), tc


# ---- 1. a batch point of the existing call, as a list in bytes ----

@pytest.mark.parametrize("M", [0, 1, 3])
def test_anchor_batch_point(native, M):
    text = _icnt(**_mesh(4))
    ref = native.icnt_closed_loop_batch(text, [dict(SIZES, batch_size=6, max_outstanding=M, seed=M + 2, reply_delay=2)],
                                        arrivals=True)[0]
    assert ref["requests"] == 6 * 16 and ref["reads"] and ref["writes"] and ref["deadlocked"] == 0
    fl = 32
    req_bytes = (ref["request_flits"] * fl).astype(np.uint32)
    reply_bytes = (np.where(ref["kind"] != 0, SIZES["write_reply_size"], SIZES["read_reply_size"]) * fl).astype(np.uint32)
    got = native.icnt_closed_loop_networks((ref["request_src"], ref["request_dst"], req_bytes, reply_bytes,
                                            ref["request_tinj"]), [text], [M], reply_delay=2, arrivals=True)
    assert len(got) == 1
    g = got[0]
    assert (g["network"], g["max_outstanding"], g["nodes"], g["requests"]) == (0, M, 16, 96)
    for k in ("tiss", "request_arrivals", "reply_arrivals", "state"):
        assert g[k].dtype == ref[k].dtype and np.array_equal(g[k], ref[k]), k
    assert g["batch_time"] == ref["batch_time"] == ref["reply_arrivals"].max()
    assert np.array_equal(g["request_flit_counts"], ref["request_flits"])
    assert g["request_flits"] == ref["request_flits"].sum() and g["measured_requests"] == 96
    for k in ("round_trip_latency", "issue_stall", "avg_outstanding", "first_finish", "last_finish", "activity"):
        assert g[k] == ref[k], k
    assert "reads" not in g and "kind" not in g


# ---- 2. every network's own flits from the bytes ----

def _three_nets(tmp):
    return [(_icnt(**_mesh(3), flit_size=16, num_vcs=1, sw_allocator="islip"), 16),
            (_icnt(k=3, n=2, topology="fly", flit_size=32, num_vcs=2, sw_allocator="separable_input_first",
                   alloc_iters=2), 32),
            (_icnt(**_anynet_mesh(tmp, 3), flit_size=40, num_vcs=4, sw_allocator="max_size"), 40)]


def test_flits_from_bytes_per_network(native, tmp_path):
    nets = _three_nets(tmp_path)
    # on, just over and far over a flit boundary of every flit size; 200 is above the largest packet
    sizes = ((16, 32), (17, 33), (32, 40), (41, 80), (128, 8), (8, 200), (200, 136))
    src, dst, qb, pb, tc = _list(9, 120, 11, spread=40, sizes=sizes)
    assert set(qb.tolist()) | set(pb.tolist()) == {s for p in sizes for s in p}
    texts = [t for t, _ in nets]
    res = native.icnt_closed_loop_networks((src, dst, qb, pb, tc), texts, [0, 2], reply_delay=1, arrivals=True, nodes=9)
    assert [(r["network"], r["max_outstanding"]) for r in res] == [(i, m) for i in range(3) for m in (0, 2)]
    counts = set()
    for i, (text, fl) in enumerate(nets):
        fq, fp = capture.flits_for(qb, fl), capture.flits_for(pb, fl)
        assert fq.max() == fp.max() == -(-MAX_PKT // fl)  # the 200-byte packets are cut to the largest packet's
        one = native.icnt_closed_loop_networks((src, dst, fq * np.uint32(fl), fp * np.uint32(fl), tc), [text], [0, 2],
                                               reply_delay=1, arrivals=True)
        for r, o in zip(res[2 * i:2 * i + 2], one):
            assert np.array_equal(r["request_flit_counts"], fq) and np.array_equal(r["reply_flit_counts"], fp)
            assert (r["request_flits"], r["reply_flits"]) == (fq.sum(), fp.sum())
            assert r["deadlocked"] == 0 and r["batch_time"] == r["reply_arrivals"].max() > 0
            _same([dict(r, network=0)], [o])
        counts.add((int(fq.sum()), int(fp.sum())))
    assert len(counts) == 3  # the three flit sizes weigh the list differently


# ---- 3. the gate, with creation times ----

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


def test_gate_replayed_in_python(native):
    src, dst, qb, pb, tc = _list(16, 400, 5, spread=150)
    assert tc[0] < tc[-1] and tc[-1] > 100
    text = _icnt(**_mesh(4))
    windows = [1, 2, 4, 0]
    res = native.icnt_closed_loop_networks((src, dst, qb, pb, tc), [text], windows, reply_delay=2, arrivals=True)
    for M, r in zip(windows, res):
        assert r["deadlocked"] == 0 and r["requests"] == 400
        rule = _replay_rule(dict(request_tinj=tc, reply_arrivals=r["reply_arrivals"], request_src=src), M)
        assert np.array_equal(r["tiss"], rule), M
        assert (r["tiss"] >= tc).all() and r["batch_time"] == r["reply_arrivals"].max()
        # contended: the round trips are not all one lone-packet latency
        assert len(set((r["reply_arrivals"] - r["tiss"]).tolist())) > 4
        if M:
            assert r["max_issue_stall"] > 0 and 0 < r["avg_outstanding"] <= M
        else:
            assert r["max_issue_stall"] == 0 and np.array_equal(r["tiss"], tc)
    bt = [r["batch_time"] for r in res]
    assert bt[0] > bt[3] and bt[0] >= bt[1] >= bt[2] >= bt[3]  # a wider window never finishes later


# ---- 4. cpu == cpu-par ----

def _engine_grid():
    """(texts, list) per call: a 2x2 mesh; a 4x4 mesh and a 4x4 torus with 2
    VCs.  Every order-free allocator on every network, speedups and buffer
    depths in turn."""
    calls = []
    speed = ("1.0", "1.5", "2.0")
    for i, alloc in enumerate(ORDER_FREE):
        kw = dict(sw_allocator=alloc, alloc_iters=2, internal_speedup=speed[i % 3], vc_buf_size=(1, 4)[i % 2],
                  credit_delay=(0, 2)[i % 2])
        calls.append(([_icnt(**_mesh(2), **kw, num_vcs=(1, 2, 4)[i % 3])], _list(4, 60, 20 + i, spread=30)))
        calls.append(([_icnt(**_mesh(4), **kw, flit_size=16), _icnt(k=4, n=2, topology="torus", **kw, num_vcs=2)],
                      _list(16, 200, 40 + i, spread=60)))
    return calls


def test_cpu_equals_cpu_par(native):
    for texts, lst in _engine_grid():
        ref = native.icnt_closed_loop_networks(lst, texts, [0, 1, 3], reply_delay=3, engine="cpu", arrivals=True)
        assert len(ref) == 3 * len(texts) and all(r["deadlocked"] == 0 and r["batch_time"] > 0 for r in ref)
        _same(native.icnt_closed_loop_networks(lst, texts, [0, 1, 3], reply_delay=3, engine="cpu-par", arrivals=True), ref)
        # without arrivals: the same figures, no arrays
        plain = native.icnt_closed_loop_networks(lst, texts, [0, 1, 3], reply_delay=3, engine="cpu-par")
        assert [p["batch_time"] for p in plain] == [r["batch_time"] for r in ref] and "tiss" not in plain[0]


# ---- 5. request lists from a capture ----

def _sub(rows):
    """(tinj, src, dst, bytes, type) rows as a capture subnet."""
    a = np.array(rows, np.int64).reshape(-1, 5)
    return capture.Subnet(a[:, 1].astype(np.uint32), a[:, 2].astype(np.uint32), a[:, 3].astype(np.uint32),
                          np.maximum((a[:, 3] + 31) // 32, 1).astype(np.uint32), a[:, 0].astype(np.uint64),
                          a[:, 4].astype(np.uint8))


def _cap(req, rep):
    q, p = _sub(req), _sub(rep)
    return capture.Capture(1, 4, 2, 2, 32, 1000, (len(q), len(p)), q, p)


def test_request_list_pairs_in_record_order():
    RD, WR, AT, RDR, WRA, ATR = 1, 2, 3, 4, 5, 6
    # two reads 0 -> 2 whose replies (72, then 40 bytes) come back in the other order in time; file order decides
    req = [(5, 0, 2, 8, RD), (3, 1, 3, 136, WR), (9, 0, 2, 8, RD), (9, 0, 2, 136, WR), (4, 1, 2, 16, AT), (2, 0, 3, 8, RD)]
    rep = [(30, 2, 0, 72, RDR), (20, 2, 0, 40, RDR), (25, 3, 1, 8, WRA), (40, 2, 0, 8, WRA), (22, 2, 1, 24, ATR),
           (21, 3, 0, 136, RDR)]
    c = _cap(req, rep)
    rl = capture.request_list(c)
    assert rl.nodes == 4 and rl.dropped == 0 and len(rl) == 6
    assert [a.dtype for a in (rl.src, rl.dst, rl.req_bytes, rl.reply_bytes, rl.tcreate, rl.type)] == \
        [np.uint32] * 4 + [np.uint64, np.uint8]
    rows = list(zip(rl.tcreate.tolist(), rl.src.tolist(), rl.dst.tolist(), rl.req_bytes.tolist(), rl.type.tolist(),
                    rl.reply_bytes.tolist()))
    # stable order of the captured time; the first read record takes the first reply record's 72 bytes
    assert rows == [(2, 0, 3, 8, RD, 136), (3, 1, 3, 136, WR, 8), (4, 1, 2, 16, AT, 24), (5, 0, 2, 8, RD, 72),
                    (9, 0, 2, 8, RD, 40), (9, 0, 2, 136, WR, 8)]
    # every group's reply count and bytes are kept
    groups = {}
    for t, s, d, b, ty, rb in rows:
        groups.setdefault((s, d, capture.ANSWER[ty]), []).append(rb)
    for (s, d, ty), got in groups.items():
        m = (c.reply.src == d) & (c.reply.dst == s) & (c.reply.type == ty)
        assert sorted(got) == sorted(c.reply.bytes[m].tolist()), (s, d, ty)
    assert sum(len(v) for v in groups.values()) == len(c.reply)
    # batch timing: zeros, in captured order
    b = capture.request_list(c, timing="batch")
    assert not b.tcreate.any() and b.tcreate.dtype == np.uint64
    for k in ("src", "dst", "req_bytes", "reply_bytes", "type"):
        assert np.array_equal(getattr(b, k), getattr(rl, k)), k
    # a missing reply: the group is named; drop leaves out the group's last request
    short = _cap(req, rep[1:])
    with pytest.raises(ValueError, match=r"P_RD from node 0 to node 2: 2 requests, 1 P_RD_REPLY"):
        capture.request_list(short)
    d = capture.request_list(short, unanswered="drop")
    assert d.dropped == 1 and len(d) == 5
    assert [(t, rb) for t, s, ds, ty, rb in zip(d.tcreate.tolist(), d.src.tolist(), d.dst.tolist(), d.type.tolist(),
                                                 d.reply_bytes.tolist()) if (s, ds, ty) == (0, 2, RD)] == [(5, 40)]
    # a reply nobody asked for
    with pytest.raises(ValueError, match=r"more replies than requests: P_WR from node 1 to node 3"):
        capture.request_list(_cap(req, rep + [(50, 3, 1, 8, WRA)]), unanswered="drop")
    with pytest.raises(ValueError, match="timing"):
        capture.request_list(c, timing="open")
    with pytest.raises(ValueError, match="unanswered"):
        capture.request_list(c, unanswered="keep")


def _small_app(root):
    """24 single-warp CTAs, 8 loads each of a line of their own, then a store:
    192 reads and 24 writes over the sub-partitions."""
    from accel_sim_framework_distributed_amd.tracegen import rodinia
    from accel_sim_framework_distributed_amd.tracegen.builder import KernelBuilder
    k = KernelBuilder("_Z5smallPf", (24, 1, 1), (32, 1, 1), nregs=32)
    for i in range(8):
        k.op("LDG.E", [8 + i], [2], base=0x7000_0000 + k.g.cta * 0x100000 + i * 128, stride=4)
    for i in range(8):
        k.op("FADD", [5], [8 + i, 5])
    k.op("STG.E", [], [2, 5], base=0x7800_0000 + k.g.cta * 0x100000, stride=4)
    k.op("EXIT")
    return rodinia.write_app(str(root / "small_app"), [k.build()], memcpy=False)


@pytest.fixture(scope="module")
def small_capture(native, tmp_path_factory):
    """A capture of the CPU engine: the small machine of test_router_pass_par
    (16 clusters, 16 sub-partitions on an 8 x 8 mesh), made once."""
    root = tmp_path_factory.mktemp("icnt_closed_replay")
    args = rpass._icnt_args(root, "small", **rpass.MESH) + ["-icnt_link_contention", "2", "-gpgpu_perf_sim_memcpy", "0"]
    path = str(root / "small.icap")
    s = native.Simulator(args + ["-icnt_capture", path, "-sim_engine", "cpu", "-trace", _small_app(root)], False)
    assert s.run() == 0 and not s.deadlock
    return path


def test_request_list_of_a_real_capture(small_capture):
    c = capture.load(small_capture)
    assert c.nodes == 64 and len(c.request) >= 200 and len(c.request) == len(c.reply)
    assert set(c.request.type.tolist()) == {1, 2}
    rl = capture.request_list(c)
    assert len(rl) == len(c.request) and rl.dropped == 0 and rl.nodes == 64
    assert int(rl.reply_bytes.sum()) == int(c.reply.bytes.sum()) and int(rl.req_bytes.sum()) == int(c.request.bytes.sum())
    assert (np.diff(rl.tcreate.astype(np.int64)) >= 0).all() and rl.tcreate[-1] > rl.tcreate[0]
    # reads are answered by lines, writes by acknowledgements
    assert set(rl.reply_bytes[rl.type == 1].tolist()) == set(c.reply.bytes[c.reply.type == 4].tolist())
    assert set(rl.reply_bytes[rl.type == 2].tolist()) == set(c.reply.bytes[c.reply.type == 5].tolist())
    assert (rl.src < c.n_clusters).all() and (rl.dst >= c.n_clusters).all()


# ---- 6. refusals ----

def test_refusals_name_the_network(native):
    src, dst, qb, pb, tc = _list(16, 40, 3, spread=10)
    ok, lst = _icnt(**_mesh(4)), (src, dst, qb, pb, tc)
    call = native.icnt_closed_loop_networks
    assert call(lst, [ok, ok], [1], nodes=16)[1]["deadlocked"] == 0
    with pytest.raises(ValueError, match=r"network 1: the network has 9 nodes, the request list is for 16"):
        call(lst, [ok, _icnt(**_mesh(3))], [1], nodes=16)
    with pytest.raises(ValueError, match=r"network 1: request \d+ has a node out of range"):
        call(lst, [ok, _icnt(**_mesh(3))], [1])
    same = dst.copy()
    same[7] = src[7]
    with pytest.raises(ValueError, match=r"network 0: request 7 has src == dst"):
        call((src, same, qb, pb, tc), [ok], [1])
    back = tc.copy()
    back[20] = back[19] - 1 if back[19] else 0
    back[19] += 1
    with pytest.raises(ValueError, match=r"network 0: request 20 has a decreasing tcreate"):
        call((src, dst, qb, pb, back), [ok], [1])
    for k in range(5):
        cut = list(lst)
        cut[k] = cut[k][:-1]
        with pytest.raises(ValueError, match=r"network 0: src, dst, req_bytes, reply_bytes and tcreate differ in length"):
            call(tuple(cut), [ok], [1])
    z32, z64 = np.zeros(MAX_REQUESTS + 1, np.uint32), np.zeros(MAX_REQUESTS + 1, np.uint64)
    with pytest.raises(ValueError, match=r"network 0: too many requests for one pass"):
        call((z32, z32, z32, z32, z64), [ok], [1])
    del z32, z64
    for rf in ("min_adapt", "valiant"):
        with pytest.raises(ValueError, match=rf"network 1: .*{rf}"):
            call(lst, [ok, _icnt(**_mesh(4), routing_function=rf)], [1])
    with pytest.raises(ValueError, match=r"network 0: .*1089 nodes, at most 1024"):
        call(lst, [_icnt(**_mesh(33))], [1])
    with pytest.raises(ValueError, match="engine"):
        call(lst, [ok], [1], engine="fpga")
    with pytest.raises(ValueError, match="expected"):
        call(lst[:4], [ok], [1])


@pytest.mark.parametrize("engine", ["cpu", "cpu-par"])
def test_capped_pass_raises(native, engine):
    lst = _list(16, 100, 8, spread=20)
    text = _icnt(**_mesh(4))
    with pytest.raises(RuntimeError, match=r"network 0: .*loop guard"):
        native.icnt_closed_loop_networks(lst, [text, text], [2], engine=engine, step_cap=5)
    assert native.icnt_closed_loop_networks(lst, [text], [2], engine=engine)[0]["deadlocked"] == 0


# ---- 7. the python interface ----

def test_cli(native, small_capture, tmp_path, capsys):
    nets = []
    for name, kw in (("mesh", dict(rpass.MESH)), ("torus16", dict(k=8, n=2, topology="torus", num_vcs=2, flit_size=16))):
        f = tmp_path / f"{name}.icnt"
        f.write_text(presets.render_icnt(presets.icnt_params(**kw)))
        nets.append(str(f))
    out = tmp_path / "grid.json"
    argv = ["--closed-loop", "--replay", small_capture, "--networks", ",".join(nets), "--max-outstanding", "1,0",
            "--reply-delay", "4", "--json", str(out)]
    assert booksim.main(argv) == 0
    printed = capsys.readouterr().out
    assert printed.count("Batch received. Time used is") == 4
    assert all(printed.count(f"on {n},") == 2 for n in nets) and "max outstanding unlimited" in printed
    got = json.loads(out.read_text())
    assert got["closed_loop"] and got["networks"] == nets and got["max_outstanding"] == [1, 0]
    assert [(g["config"], g["max_outstanding"]) for g in got["grid"]] == [(n, m) for n in nets for m in (1, 0)]
    rl = capture.request_list(capture.load(small_capture))
    ref = native.icnt_closed_loop_networks((rl.src, rl.dst, rl.req_bytes, rl.reply_bytes, rl.tcreate),
                                           [open(n).read() for n in nets], [1, 0], reply_delay=4, nodes=rl.nodes)
    assert [g["batch_time"] for g in got["grid"]] == [r["batch_time"] for r in ref]
    assert all(r["batch_time"] > 0 and r["deadlocked"] == 0 for r in ref)
    assert ref[0]["batch_time"] >= ref[1]["batch_time"]
    # the python call is the native one
    py = booksim.closed_loop_replay(rl.src, rl.dst, rl.req_bytes, rl.reply_bytes, rl.tcreate,
                                    [open(n).read() for n in nets], [1, 0], reply_delay=4, nodes=rl.nodes)
    assert [p["batch_time"] for p in py] == [r["batch_time"] for r in ref]
    # --timing batch: every request ready at cycle 0; one config in place of --networks
    assert booksim.main([nets[0], "--closed-loop", "--replay", small_capture, "--timing", "batch"]) == 0
    assert capsys.readouterr().out.count("Batch received.") == 1
    # an .npz list: with reply sizes it runs, without them it is refused
    npz = str(tmp_path / "req.npz")
    capture.save_request_npz(npz, rl)
    out2 = tmp_path / "npz.json"
    assert booksim.main(argv[:2] + [npz] + argv[3:-1] + [str(out2)]) == 0
    capsys.readouterr()
    assert [g["batch_time"] for g in json.loads(out2.read_text())["grid"]] == [r["batch_time"] for r in ref]
    bare = str(tmp_path / "bare.npz")
    capture.save_npz(bare, capture.load(small_capture), "request")
    assert booksim.main(["--closed-loop", "--replay", bare, "--networks", nets[0]]) == 2
    assert "reply_bytes" in capsys.readouterr().err


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


def _gpu_nets():
    """2x2, 4x4 and 6x6 meshes that differ in flit size, VC count and
    allocator: the workgroups of one launch carve different U * V."""
    return [_icnt(**_mesh(2), flit_size=16, num_vcs=1, sw_allocator="islip"),
            _icnt(**_mesh(4), flit_size=32, num_vcs=2, sw_allocator="separable_input_first", alloc_iters=2,
                  internal_speedup="1.5"),
            _icnt(**_mesh(6), flit_size=40, num_vcs=4, sw_allocator="max_size", internal_speedup="2.0", credit_delay=2)]


@pytest.mark.gpu
@pytest.mark.parametrize("lds", [True, False])
def test_gpu_equals_cpu(gpu_native, lds):
    texts = _gpu_nets()
    lst = _list(4, 150, 31, spread=50)  # the nodes every one of the three networks has
    assert 0 < gpu_native.icnt_closed_loop_networks_lds_bytes(texts) <= 48 * 1024
    ref = gpu_native.icnt_closed_loop_networks(lst, texts, [0, 1, 3], reply_delay=2, engine="cpu", arrivals=True)
    assert len(ref) == 9 and all(r["deadlocked"] == 0 for r in ref)
    assert len({r["request_flits"] for r in ref}) == 3 and len({len(r["state"]) for r in ref}) == 3
    got = gpu_native.icnt_closed_loop_networks(lst, texts, [0, 1, 3], reply_delay=2, engine="gpu", arrivals=True, lds=lds)
    st = gpu_native.icnt_open_loop_batch_stats()
    assert all(k in got[0] for k in WORDS)
    _same(got, ref)
    assert st["chunks"] == 1 and st["max_chunk_points"] == 9 and st["lds_chunks"] == (1 if lds else 0), st


@pytest.mark.gpu
def test_gpu_hbm_fallback(gpu_native):
    """A chunk whose largest doubled network does not fit the LDS limit keeps
    every unit's per-(unit, VC) words in HBM, the small network's too."""
    big, small = _icnt(**_mesh(8), num_vcs=4), _icnt(**_mesh(2))
    assert gpu_native.icnt_closed_loop_networks_lds_bytes([big]) > 48 * 1024
    assert gpu_native.icnt_closed_loop_networks_lds_bytes([_icnt(**_mesh(7), num_vcs=4)]) <= 48 * 1024  # the smallest that does not fit
    assert gpu_native.icnt_closed_loop_networks_lds_bytes([small]) <= 48 * 1024
    lst = _list(4, 80, 17, spread=30)
    ref = gpu_native.icnt_closed_loop_networks(lst, [big, small], [0, 2], engine="cpu", arrivals=True)
    got = gpu_native.icnt_closed_loop_networks(lst, [big, small], [0, 2], engine="gpu", arrivals=True, lds=True)
    st = gpu_native.icnt_open_loop_batch_stats()
    _same(got, ref)
    assert st["chunks"] == 1 and st["lds_chunks"] == 0, st


@pytest.mark.gpu
def test_gpu_memory_budget_splits_the_grid(gpu_native):
    texts = [_icnt(**_mesh(4), flit_size=fl) for fl in (16, 32, 40)]
    lst = _list(16, 600, 23, spread=100)
    ref = gpu_native.icnt_closed_loop_networks(lst, texts, [1, 4, 0], reply_delay=1, engine="cpu", arrivals=True)
    got = gpu_native.icnt_closed_loop_networks(lst, texts, [1, 4, 0], reply_delay=1, engine="gpu", arrivals=True,
                                               mem_budget_mb=1)
    st = gpu_native.icnt_open_loop_batch_stats()
    _same(got, ref)
    assert st["chunks"] >= 2 and st["max_chunk_bytes"] <= st["budget_bytes"] == 1 << 20, st


@pytest.mark.gpu
def test_gpu_capture_to_closed_loop_replay(gpu_native, small_capture):
    """End to end: a CPU-engine capture, its request list, and the replay on
    three networks of the capture's node count under two windows."""
    rl = capture.request_list(capture.load(small_capture))
    texts = [presets.render_icnt(presets.icnt_params(**kw)) for kw in (
        dict(rpass.MESH), dict(rpass.MESH, flit_size=16, num_vcs=2), dict(k=8, n=2, topology="torus", num_vcs=2))]
    args = (rl.src, rl.dst, rl.req_bytes, rl.reply_bytes, rl.tcreate, texts, [2, 0])
    ref = booksim.closed_loop_replay(*args, reply_delay=10, engine="cpu", arrivals=True, nodes=rl.nodes)
    got = booksim.closed_loop_replay(*args, reply_delay=10, engine="gpu", arrivals=True, nodes=rl.nodes)
    assert len(ref) == 6 and all(r["deadlocked"] == 0 and r["requests"] == len(rl) for r in ref)
    assert ref[0]["reply_flits"] != ref[2]["reply_flits"]  # the 136-byte replies weigh more in 16-byte flits
    _same(got, ref)


@pytest.mark.gpu
def test_gpu_kernel_resources(gpu_native):
    info = gpu_native.icnt_cln_kernel_info()
    assert info["max_threads_per_block"] == 64 and info["lds_bytes"] == 0  # the hot words are dynamic LDS
    assert 0 < info["num_regs"] <= 512

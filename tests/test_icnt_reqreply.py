"""Packet-list replay (icnt_replay_batch) and request-reply points over two
subnets (icnt_request_reply_batch).

The semantics are pinned on the host: the injection schedule against a plain
Python port of the generator (splitmix64), the Bernoulli loop and the
destination rule; replay against the trusted open-loop path
(icnt_open_loop_batch); and a request-reply point as a composition of two
replays around a numpy stable sort of the request arrivals.  The engines
(``cpu-par``, ``gpu``) are then compared with ``cpu`` on the full tuple: every
array, both state images, the activity counters and the whole result dicts.
Each case is one batch call; references are computed once and left unchanged.
"""
import json

import numpy as np
import pytest

from accel_sim_framework_distributed_amd.models import presets

CYC, WARM = 300, 50
M64 = (1 << 64) - 1


def _icnt(**kw):
    base = dict(num_vcs="2", vc_buf_size="2", internal_speedup="1.0", flit_size="32")
    base.update(kw)
    return presets.render_icnt(presets.icnt_params(**base))


MESH = dict(k=4, n=2, topology="mesh")  # 16 nodes; 5-flit packets wormhole through 2-flit buffers
XBAR = dict(k=8, n=1)                   # an 8-node single-stage fly: a crossbar
SIZES = dict(read_request_size=1, read_reply_size=5, write_request_size=5, write_reply_size=1)


# ---- the oracle: a plain port of the generator and the schedule ----

class Rng:
    def __init__(self, seed):
        self.s = (seed * 0x2545f4914f6cdd1d + 1) & M64

    def next(self):
        self.s = (self.s + 0x9e3779b97f4a7c15) & M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
        return z ^ (z >> 31)

    def uniform(self):
        return (self.next() >> 11) * (1.0 / 9007199254740992.0)


def _dest(traffic, s, N, k, n, r):
    if traffic == "uniform":
        while True:
            d = r.next() % N
            if d != s:
                return d
    if traffic == "transpose":
        b = N.bit_length() - 1
        h = b // 2
        return ((s & ((1 << h) - 1)) << h) | (s >> h)
    if traffic == "neighbor":
        d, pw, x = 0, 1, s
        for _ in range(n):
            d += ((x % k + 1) % k) * pw
            x //= k
            pw *= k
        return d % N
    raise AssertionError(traffic)


def oracle_open_loop(N, k, n, traffic, rate, flits, cycles, seed):
    r = Rng(seed)
    p = rate / flits
    src, dst, tinj = [], [], []
    for t in range(cycles):
        for s in range(N):
            if r.uniform() < p:
                d = _dest(traffic, s, N, k, n, r)
                if d == s:
                    continue
                src.append(s)
                dst.append(d)
                tinj.append(t)
    return (np.array(src, np.uint32), np.array(dst, np.uint32), np.full(len(src), flits, np.uint32),
            np.array(tinj, np.uint64))


def oracle_request_reply(N, k, n, pt):
    """(src, dst, flits, tinj, kind) of a request-reply point's request subnet."""
    sz = [pt.get(key, 1) for key in ("read_request_size", "read_reply_size", "write_request_size", "write_reply_size")]
    p = pt["rate"] / max(1, sum(sz) // 2)
    M = pt.get("mem_nodes", 0)
    r = Rng(pt["seed"])
    src, dst, fl, tinj, kind = [], [], [], [], []
    for t in range(pt["cycles"]):
        for s in range(N - M):
            if r.uniform() < p:
                d = N - M + r.next() % M if M else _dest(pt["traffic"], s, N, k, n, r)
                if d == s:
                    continue
                wr = 1 if r.uniform() < pt.get("write_fraction", 0.5) else 0
                src.append(s)
                dst.append(d)
                tinj.append(t)
                kind.append(wr)
                fl.append(sz[2] if wr else sz[0])
    return (np.array(src, np.uint32), np.array(dst, np.uint32), np.array(fl, np.uint32), np.array(tinj, np.uint64),
            np.array(kind, np.uint32))


# ---- the cases ----

# (traffic, rate, packet_flits, cycles, warmup, seed) of the trusted path
OPEN_POINTS = [("uniform", 0.4, 1, CYC, WARM, 1), ("transpose", 0.6, 4, CYC, WARM, 2), ("neighbor", 0.3, 4, CYC, WARM, 3)]


def _rr(traffic="uniform", rate=0.5, seed=1, **kw):
    p = dict(SIZES, traffic=traffic, rate=rate, seed=seed, cycles=CYC, warmup=WARM, write_fraction=0.3)
    p.update(kw)
    return p


# name -> (icnt keys, (N, k, n), points); a rate-0 point between two loaded ones
RR_GRID = {
    "mesh": (MESH, (16, 4, 2), [
        _rr(rate=0.6), _rr(rate=0.0, seed=2), _rr("transpose", 0.8, 3, reply_delay=7),
        _rr(rate=0.5, seed=4, write_fraction=0.0), _rr(rate=0.5, seed=5, write_fraction=1.0, reply_delay=7),
        _rr(rate=0.9, seed=6, reply_delay=7)]),
    "xbar": (XBAR, (8, 8, 1), [_rr(rate=0.5, mem_nodes=2), _rr(rate=0.7, seed=2, mem_nodes=2, reply_delay=7)]),
}
RR_ALLOC = {"alloc_" + a: (dict(MESH, sw_allocator=a, alloc_iters=2), (16, 4, 2), [_rr(rate=0.8, seed=7)])
            for a in ("wavefront", "separable_input_first")}

_ref = {}


@pytest.fixture(scope="module")
def gpu_native():
    import torch  # bind torch's HIP runtime first
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    from accel_sim_framework_distributed_amd import _native
    mod = _native.load(prefer_torch_runtime=True)
    assert mod.gpu_available(), "HIP device not usable (native code must run, no silent fallback)"
    return mod


def _same(got, ref):
    """Two results, or lists of results, equal in everything: arrays by
    content and type, nested dicts and scalars exactly."""
    if isinstance(ref, list):
        assert len(got) == len(ref)
        for i, (g, r) in enumerate(zip(got, ref)):
            try:
                _same(g, r)
            except AssertionError as e:
                raise AssertionError(f"entry {i}: {e}") from None
        return
    assert list(got) == list(ref)
    for key, r in ref.items():
        g = got[key]
        if isinstance(r, np.ndarray):
            assert g.dtype == r.dtype and np.array_equal(g, r), key
        else:
            assert g == r, key


def _replay_lists():
    """The oracle's lists of OPEN_POINTS (constant sizes 1 and 4)."""
    if "lists" not in _ref:
        _ref["lists"] = [oracle_open_loop(16, 4, 2, t, rate, fl, cyc, seed) for t, rate, fl, cyc, _, seed in OPEN_POINTS]
    return _ref["lists"]


def _replay(native, lists, engine, **kw):
    return native.icnt_replay_batch(_icnt(**MESH), lists, engine=engine, arrivals=True, cycles=CYC, warmup=WARM, **kw)


def _replay_ref(native):
    if "replay" not in _ref:
        _ref["replay"] = _replay(native, _replay_lists(), "cpu")
    return _ref["replay"]


def _rr_batch(native, name, engine, **kw):
    keys, _, points = {**RR_GRID, **RR_ALLOC}[name]
    return native.icnt_request_reply_batch(_icnt(**keys), points, engine=engine, arrivals=True, **kw)


def _rr_ref(native, name):
    if name not in _ref:
        _ref[name] = _rr_batch(native, name, "cpu")
    return _ref[name]


# ---- 1. replay is tied to the trusted path ----

def test_replay_equals_open_loop(native):
    text = _icnt(**MESH)
    trusted = native.icnt_open_loop_batch(text, OPEN_POINTS, engine="cpu", arrivals=True)
    lists = _replay_lists()
    assert [len(l[0]) for l in lists] == [t["packets"] for t in trusted] and all(len(l[0]) for l in lists)
    assert {int(l[2][0]) for l in lists} == {1, 4}
    got = _replay_ref(native)
    _same(got, trusted)  # arrivals, state, deadlocked, activity and every scalar
    # without arrivals the dict is open_loop_dict's, and the default window is [0, last injection + 1)
    plain = native.icnt_replay_batch(text, lists[:1])[0]
    assert "arrivals" not in plain and "state" not in plain
    last = int(lists[0][3].max())
    assert plain == native.icnt_replay_batch(text, lists[:1], cycles=last + 1, warmup=0)[0]
    assert plain["measured_packets"] == plain["packets"] == len(lists[0][0])


def test_replay_per_packet_sizes_in_the_summary(native):
    """Offered and accepted flits and the zero-load latency use each packet's
    own flit count: two packets far apart in time, 1 and 5 flits."""
    text = _icnt(**MESH)
    one = lambda fl: (np.array([0], np.uint32), np.array([5], np.uint32), np.array([fl], np.uint32),
                      np.array([10], np.uint64))
    both = (np.array([0, 0], np.uint32), np.array([5, 5], np.uint32), np.array([1, 5], np.uint32),
            np.array([10, 100], np.uint64))
    a, b, ab = native.icnt_replay_batch(text, [one(1), one(5), both], arrivals=True, cycles=200, warmup=0)
    assert b["zero_load_latency"] == a["zero_load_latency"] + 4 and a["avg_latency"] == a["zero_load_latency"]
    assert list(ab["arrivals"]) == [a["arrivals"][0], b["arrivals"][0] + 90]
    assert ab["zero_load_latency"] == (a["zero_load_latency"] + b["zero_load_latency"]) / 2
    assert ab["offered"] == 6 / (200 * 16) and ab["accepted"] == 6 / (200 * 16)
    assert ab["activity"]["eject_flits"] == 6


# ---- 2. request-reply is a composition ----

@pytest.mark.parametrize("name", sorted(RR_GRID))
def test_request_reply_is_a_composition(native, name):
    keys, (N, k, n), points = RR_GRID[name]
    text = _icnt(**keys)
    ref = _rr_ref(native, name)
    assert len(ref) == len(points)
    ties = disorder = 0
    for pt, res in zip(points, ref):
        src, dst, fl, tinj, kind = oracle_request_reply(N, k, n, pt)
        # the request schedule with its kind draw
        for key, want in (("request_src", src), ("request_dst", dst), ("request_flits", fl), ("request_tinj", tinj)):
            assert res[key].dtype == want.dtype and np.array_equal(res[key], want), key
        assert res["reads"] == int((kind == 0).sum()) and res["writes"] == int(kind.sum())
        if pt["rate"] == 0:
            assert len(src) == 0 and res["request"]["packets"] == 0 and res["round_trip_latency"] == 0
        else:
            assert len(src) > 50
            wf = pt["write_fraction"]
            assert (res["reads"] > 0) == (wf < 1) and (res["writes"] > 0) == (wf > 0)
        if pt.get("mem_nodes"):
            assert src.max() < N - pt["mem_nodes"] and dst.min() >= N - pt["mem_nodes"]
        # the request subnet is a replay of that list
        rq = native.icnt_replay_batch(text, [(src, dst, fl, tinj)], arrivals=True, cycles=CYC, warmup=WARM)[0]
        assert np.array_equal(res["request_arrivals"], rq["arrivals"])
        assert np.array_equal(res["request_state"], rq["state"])
        assert res["request"] == {kk: v for kk, v in rq.items() if kk not in ("arrivals", "state")}
        # the reply schedule: a stable sort of the arrivals
        arr = res["request_arrivals"]
        key_t = arr + np.uint64(pt.get("reply_delay", 0))
        order = np.argsort(key_t, kind="stable").astype(np.uint32)
        sz_rd, sz_wr = pt["read_reply_size"], pt["write_reply_size"]
        want = dict(reply_of=order, reply_src=dst[order], reply_dst=src[order],
                    reply_flits=np.where(kind[order] == 1, sz_wr, sz_rd).astype(np.uint32), reply_tinj=key_t[order])
        for key, w in want.items():
            assert res[key].dtype == w.dtype and np.array_equal(res[key], w), key
        ties += int(len(np.unique(key_t)) < len(key_t))
        disorder += int(np.any(arr[1:] < arr[:-1]))
        # the reply subnet is a replay of the reply list, on a network of its own
        rp = native.icnt_replay_batch(text, [tuple(want[kk] for kk in ("reply_src", "reply_dst", "reply_flits",
                                                                       "reply_tinj"))],
                                      arrivals=True, cycles=CYC, warmup=WARM)[0]
        assert np.array_equal(res["reply_arrivals"], rp["arrivals"])
        assert np.array_equal(res["reply_state"], rp["state"])
        assert res["reply"] == {kk: v for kk, v in rp.items() if kk not in ("arrivals", "state")}
        # the round trip by its definition: request creation to reply tail arrival
        back = np.empty(len(order), np.int64)
        back[order] = np.arange(len(order))
        rt = (res["reply_arrivals"][back] - tinj)[tinj >= WARM].astype(np.float64)
        assert res["round_trip_latency"] == (rt.sum() / len(rt) if len(rt) else 0)
        assert res["max_round_trip_latency"] == (rt.max() if len(rt) else 0)
        if len(rt):
            assert rt.min() > pt.get("reply_delay", 0)
        # these networks are deadlock free
        assert res["deadlocked"] == 0 and res["request"]["deadlocked"] == 0 and res["reply"]["deadlocked"] == 0
    assert ties >= 1, "no point has two replies created in the same cycle"
    assert disorder >= 1, "no point has arrivals out of request order"


def test_request_reply_defaults_and_plain_result(native):
    """A point's defaults (sizes 1, write_fraction 0.5, no delay, every node
    issues), and the result without arrivals."""
    text = _icnt(**MESH)
    pt = dict(traffic="uniform", rate=0.3, cycles=CYC, warmup=WARM, seed=9)
    full = dict(pt, write_fraction=0.5, read_request_size=1, read_reply_size=1, write_request_size=1,
                write_reply_size=1, reply_delay=0, mem_nodes=0)
    a, b = native.icnt_request_reply_batch(text, [pt, full])
    assert a == b
    assert sorted(a) == sorted(["request", "reply", "reads", "writes", "round_trip_latency",
                                "max_round_trip_latency", "deadlocked"])
    src, dst, fl, tinj, kind = oracle_request_reply(16, 4, 2, full)
    assert a["request"]["packets"] == a["reply"]["packets"] == len(src) == a["reads"] + a["writes"]
    # the schedule on its own: what the batch call simulates, ready to replay
    s = native.icnt_request_reply_schedule(text, [pt])[0]
    for key, want in (("src", src), ("dst", dst), ("flits", fl), ("tinj", tinj), ("kind", kind)):
        assert s[key].dtype == want.dtype and np.array_equal(s[key], want), key


# ---- 3. cpu-par equals cpu ----

def test_cpu_par_replay_equals_cpu(native):
    _same(_replay(native, _replay_lists(), "cpu-par"), _replay_ref(native))


@pytest.mark.parametrize("name", sorted({**RR_GRID, **RR_ALLOC}))
def test_cpu_par_request_reply_equals_cpu(native, name):
    ref = _rr_ref(native, name)
    assert sum(r["request"]["packets"] for r in ref) > 0
    _same(_rr_batch(native, name, "cpu-par"), ref)


# ---- 4. input checks ----

def test_replay_rejects_bad_lists(native):
    text = _icnt(**MESH)
    u32 = lambda *v: np.array(v, np.uint32)
    u64 = lambda *v: np.array(v, np.uint64)
    good = (u32(0, 1), u32(5, 6), u32(1, 5), u64(0, 3))
    assert len(native.icnt_replay_batch(text, [good])) == 1
    bad = {
        "src out of range": (u32(0, 16), u32(5, 6), u32(1, 5), u64(0, 3)),
        "dst out of range": (u32(0, 1), u32(5, 99), u32(1, 5), u64(0, 3)),
        "src == dst": (u32(0, 6), u32(5, 6), u32(1, 5), u64(0, 3)),
        "no flits": (u32(0, 1), u32(5, 6), u32(1, 0), u64(0, 3)),
        "too many flits": (u32(0, 1), u32(5, 6), u32(1, 6), u64(0, 3)),
        "unequal lengths": (u32(0, 1), u32(5, 6), u32(1, 5), u64(0)),
    }
    for why, l in bad.items():
        for engine in ("cpu", "cpu-par"):
            with pytest.raises(ValueError, match="list 1" + ("" if why == "unequal lengths" else ", packet 1")):
                native.icnt_replay_batch(text, [good, l], engine=engine)
    with pytest.raises(ValueError, match="engine"):
        native.icnt_replay_batch(text, [good], engine="tpu")


def test_replay_rejects_too_many_packets(native):
    """More than 50,000,000 packets: refused on the lengths alone, before
    anything is copied (the arrays are untouched zero pages)."""
    n = 50_000_001
    z = np.zeros(n, np.uint32)
    with pytest.raises(ValueError, match="list 0.*too many packets"):
        native.icnt_replay_batch(_icnt(**MESH), [(z, z, z, np.zeros(n, np.uint64))])


def test_request_reply_rejects_bad_points(native):
    mesh, xbar = _icnt(**MESH), _icnt(**XBAR)
    with pytest.raises(ValueError, match="point 1.*mem_nodes"):
        native.icnt_request_reply_batch(mesh, [_rr(), _rr("transpose", mem_nodes=2)])
    for m in (8, 9):
        with pytest.raises(ValueError, match="point 0.*mem_nodes"):
            native.icnt_request_reply_batch(xbar, [_rr(mem_nodes=m)])
    with pytest.raises(ValueError, match="sizes"):
        native.icnt_request_reply_batch(mesh, [_rr(read_reply_size=6)])
    with pytest.raises(ValueError, match="sizes"):
        native.icnt_request_reply_batch(mesh, [_rr(write_request_size=0)])
    with pytest.raises(ValueError, match="unknown field"):
        native.icnt_request_reply_batch(mesh, [_rr(packet_flits=2)])
    assert len(native.icnt_request_reply_batch(xbar, [_rr(mem_nodes=7)])) == 1


def test_step_cap_reports_status(native):
    """The loop guard of either subnet's pass ends the call with an error that
    names the list or point (a test-only cap far below the pass's size)."""
    with pytest.raises(RuntimeError, match="list 0.*step cap"):
        native.icnt_replay_batch(_icnt(**MESH), _replay_lists()[:1], engine="cpu-par", step_cap=5)
    with pytest.raises(RuntimeError, match="point 0.*step cap"):
        native.icnt_request_reply_batch(_icnt(**MESH), [_rr()], engine="cpu-par", step_cap=5)


# ---- 5. python layer and CLI ----

def _cli(capsys, argv):
    from accel_sim_framework_distributed_amd.icnt import booksim
    assert booksim.main(argv) == 0
    return capsys.readouterr().out


def test_python_layer_reads_the_icnt_keys(native):
    from accel_sim_framework_distributed_amd.icnt import booksim
    text = _icnt(**MESH, write_fraction="0.3", **SIZES)
    a = booksim.request_reply_sweep(text, [0.6], cycles=CYC, warmup=WARM)[0]
    want = dict(native.icnt_request_reply_batch(_icnt(**MESH), [_rr(rate=0.6)])[0], rate=0.6)
    assert a == want and a["writes"] > 0 and a["reads"] > a["writes"]
    # an argument wins over the file
    b = booksim.request_reply_sweep(text, [0.6], cycles=CYC, warmup=WARM, write_fraction=1.0, read_reply_size=2)[0]
    assert b["reads"] == 0 and b["writes"] > 0
    src, dst, fl, tinj = _replay_lists()[1]
    r = booksim.replay(_icnt(**MESH), src, dst, fl, tinj, cycles=CYC, warmup=WARM)
    assert r == {k: v for k, v in _replay_ref(native)[1].items() if k not in ("arrivals", "state")}


def test_cli_request_reply(tmp_path, capsys):
    f = tmp_path / "rw.icnt"
    f.write_text(_icnt(**MESH, use_read_write="1", write_fraction="0.3", **SIZES))
    g = tmp_path / "plain.icnt"
    g.write_text(_icnt(**MESH, write_fraction="0.3", **SIZES))
    base = ["--rates", "0.2,0.6", "--cycles", str(CYC), "--warmup", str(WARM)]
    j = tmp_path / "rr.json"
    out = _cli(capsys, [str(f), "--request-reply", "--reply-delay", "3", "--json", str(j)] + base)
    for line in ("Request average latency", "Reply average latency", "Round-trip average latency"):
        assert out.count(line) == 2
    assert out.count("Accepted rate: request") == 2 and out.count("Saturation (round trip") == 1
    doc = json.load(open(j))
    assert doc["request_reply"] is True and [c["rate"] for c in doc["curve"]] == [0.2, 0.6]
    from accel_sim_framework_distributed_amd.icnt import booksim
    want = booksim.request_reply_sweep(f.read_text(), [0.2, 0.6], cycles=CYC, warmup=WARM, reply_delay=3)
    assert doc["curve"] == want and want[1]["writes"] > 0 and want[1]["reads"] > want[1]["writes"]
    # --mem-nodes and --write-fraction reach the points
    out = _cli(capsys, [str(f), "--request-reply", "--mem-nodes", "4", "--write-fraction", "1.0"] + base)
    assert out.count("Packets = 0 reads") == 2
    # without the flag a file carrying use_read_write = 1 behaves as it always did
    j0, j1 = tmp_path / "a.json", tmp_path / "b.json"
    t0 = _cli(capsys, [str(f), "--json", str(j0)] + base)
    t1 = _cli(capsys, [str(g), "--json", str(j1)] + base)
    assert t0 == t1 and t0.count("Overall average latency") == 2 and "Round-trip" not in t0
    assert j0.read_bytes().replace(str(f).encode(), b"X") == j1.read_bytes().replace(str(g).encode(), b"X")


def test_cli_replay(tmp_path, capsys, native):
    f = tmp_path / "x.icnt"
    f.write_text(_icnt(**MESH))
    src, dst, fl, tinj = _replay_lists()[1]
    z = tmp_path / "list.npz"
    np.savez(z, src=src, dst=dst, flits=fl, tinj=tinj)
    j = tmp_path / "r.json"
    out = _cli(capsys, [str(f), "--replay", str(z), "--cycles", str(CYC), "--warmup", str(WARM), "--json", str(j)])
    assert out.count("Overall average latency") == 1 and "Replay of" in out
    want = {k: v for k, v in _replay_ref(native)[1].items() if k not in ("arrivals", "state")}
    assert json.load(open(j))["result"] == want


# ---- 6 - 8. the device ----

def _lds_ran(gpu_native, expect):
    st = gpu_native.icnt_open_loop_batch_stats()
    assert st["chunks"] >= 1 and st["lds_chunks"] == (st["chunks"] if expect else 0), st


@pytest.mark.gpu
@pytest.mark.parametrize("lds", [True, False])
def test_gpu_replay_equals_cpu(gpu_native, lds):
    ref = _replay_ref(gpu_native)  # (first: the statistics are the last batch's)
    _same(_replay(gpu_native, _replay_lists(), "gpu", lds=lds), ref)
    _lds_ran(gpu_native, lds)


@pytest.mark.gpu
@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("name", sorted(RR_GRID))
def test_gpu_request_reply_equals_cpu(gpu_native, name, lds):
    ref = _rr_ref(gpu_native, name)
    assert sum(r["request"]["packets"] for r in ref) > 0
    _same(_rr_batch(gpu_native, name, "gpu", lds=lds), ref)
    _lds_ran(gpu_native, lds)


@pytest.mark.gpu
def test_gpu_chunks_and_small_lists(gpu_native):
    """A budget that forces several launches gives the one launch's results;
    so do the rate-0 point, an empty list and a list of one packet."""
    ref = _rr_ref(gpu_native, "mesh")
    assert ref[1]["request"]["packets"] == 0  # the rate-0 point between two loaded ones
    _same(_rr_batch(gpu_native, "mesh", "gpu"), ref)
    one = gpu_native.icnt_open_loop_batch_stats()
    assert one["chunks"] == 1 and one["max_chunk_points"] == len(ref)
    _same(_rr_batch(gpu_native, "mesh", "gpu", mem_budget_mb=1), ref)
    st = gpu_native.icnt_open_loop_batch_stats()
    assert st["chunks"] >= 3 and st["max_chunk_bytes"] <= 1 << 20 and st["lds_chunks"] == st["chunks"]
    with pytest.raises(ValueError, match="memory budget"):
        gpu_native.icnt_request_reply_batch(_icnt(**MESH), [_rr(rate=1.0, cycles=3000)], engine="gpu", mem_budget_mb=1)
    e32, e64 = np.zeros(0, np.uint32), np.zeros(0, np.uint64)
    single = (np.array([3], np.uint32), np.array([12], np.uint32), np.array([5], np.uint32), np.array([7], np.uint64))
    big = _replay_lists()
    lists = [big[0], (e32, e32, e32, e64), single, big[1], big[2], big[0], big[1]]  # above 1 MB of scratch together
    want = _replay(gpu_native, lists, "cpu")
    assert len(want[1]["arrivals"]) == 0 and want[2]["packets"] == 1
    _same(_replay(gpu_native, lists, "gpu"), want)
    _same(_replay(gpu_native, lists, "gpu", mem_budget_mb=1), want)
    assert gpu_native.icnt_open_loop_batch_stats()["chunks"] >= 2


@pytest.mark.gpu
def test_gpu_replay_in_reverse_time_order(gpu_native):
    """A list given latest packet first: every packet takes the insertion path
    of the source queues (RtCtx::link_source), with per-packet sizes."""
    src, dst, _, tinj = _replay_lists()[0]
    fl = (np.arange(len(src), dtype=np.uint32) % 5) + 1
    rev = tuple(a[::-1].copy() for a in (src, dst, fl, tinj))
    # part of the list rotated as well: insertions into the middle of a queue
    h = len(src) // 2
    mid = tuple(np.concatenate([a[h:], a[:h]]) for a in (src, dst, fl, tinj))
    want = _replay(gpu_native, [rev, mid], "cpu")
    assert np.all(np.diff(rev[3].astype(np.int64)) <= 0) and want[0]["packets"] == len(src)
    # the same packets whatever the order they are listed in
    fwd = _replay(gpu_native, [(src, dst, fl, tinj)], "cpu")[0]
    assert fwd["avg_latency"] > 0 and want[0]["activity"]["eject_flits"] == int(fl.sum())
    _same(_replay(gpu_native, [rev, mid], "gpu"), want)


@pytest.mark.gpu
def test_gpu_kernel_info(gpu_native):
    info = gpu_native.icnt_rr_kernel_info()
    assert info["num_regs"] > 0 and info["max_threads_per_block"] >= 64

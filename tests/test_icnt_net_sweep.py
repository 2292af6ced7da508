"""icnt_replay_networks: one packet list, in bytes, over many networks
(csrc/driver/icnt_bench.cc; on the GPU one wavefront per network in one
launch, csrc/engine/icnt_net_sweep.hip).

The list is synthetic and fixed: 32 nodes, 16 clusters that send 8-byte read
requests and 136-byte writes to 16 memory nodes, the shape of a capture of the
small machine of tests/test_router_pass_par.py, dense enough to contend.  The
networks all have 32 nodes; they differ in topology, flit size (16 / 32 / 40
bytes: 136 bytes are 9 / 5 / 4 flits), VC count and allocator, and one of them
(a 32-node fly with 64 VCs: 5 * U * V = 20480 words, 80 KB) does not fit the
48 KB LDS limit while the others do.
"""
import numpy as np
import pytest

from accel_sim_framework_distributed_amd.icnt import booksim, capture
from accel_sim_framework_distributed_amd.models import presets

NODES = 32
NETS = {
    "line": dict(k=32, n=1, topology="mesh"),
    "ring": dict(k=32, n=1, topology="torus", num_vcs=2),
    "fly": dict(k=32, n=1, topology="fly"),
    "cmesh": dict(k=4, n=2, c=2, topology="cmesh"),
    "cmesh_flit16": dict(k=4, n=2, c=2, topology="cmesh", flit_size=16, num_vcs=2, vc_buf_size=4),
    "fly_flit32": dict(k=32, n=1, topology="fly", flit_size=32),
    "cmesh_vc4": dict(k=4, n=2, c=2, topology="cmesh", num_vcs=4),
    "cmesh_sep_if": dict(k=4, n=2, c=2, topology="cmesh", sw_allocator="separable_input_first", num_vcs=2),
    "fly_wavefront": dict(k=32, n=1, topology="fly", sw_allocator="wavefront", num_vcs=2),
    "fly_vc64": dict(k=32, n=1, topology="fly", num_vcs=64, vc_buf_size=2),  # beyond the LDS limit
}
FLIT = {n: kw.get("flit_size", 40) for n, kw in NETS.items()}  # the preset's default flit is 40 bytes
KEYS = ("packets", "measured_packets", "offered", "accepted", "drain_throughput", "avg_latency", "max_latency",
        "zero_load_latency", "deadlocked")


def _text(kw):
    return presets.render_icnt(presets.icnt_params(**kw))


@pytest.fixture(scope="module")
def plist():
    r = np.random.default_rng(7)
    n = 600
    src = r.integers(0, 16, n).astype(np.uint32)
    dst = (16 + r.integers(0, 16, n)).astype(np.uint32)
    nbytes = np.where(r.random(n) < 0.5, 8, 136).astype(np.uint32)
    tinj = np.sort(r.integers(0, 300, n)).astype(np.uint64)
    return src, dst, nbytes, tinj


@pytest.fixture(scope="module")
def texts():
    return [_text(kw) for kw in NETS.values()]


def _full(d):
    """The full result tuple of one network: summary, activity, energy,
    arrivals and state."""
    out = {k: d[k] for k in d if k not in ("arrivals", "state")}
    return out, np.asarray(d["arrivals"]).tolist(), np.asarray(d["state"]).tolist()


@pytest.fixture(scope="module")
def cpu_ref(plist, texts):
    """Engine cpu, computed once and shared.  (No `native` fixture here: a GPU
    test must load the module through its gpu_mod, after torch.)"""
    res = booksim.replay_networks(*plist, texts, engine="cpu", arrivals=True, nodes=NODES)
    assert len(res) == len(NETS)
    return [_full(d) for d in res]


# ---- CPU ---------------------------------------------------------------------
def test_cpu_equals_a_loop_of_single_replays(native, plist, texts, cpu_ref):
    """The defining form: per network, booksim.replay of the list with that
    network's flits recomputed in numpy from the bytes."""
    src, dst, nbytes, tinj = plist
    seen = set()
    for (name, kw), text, ref in zip(NETS.items(), texts, cpu_ref):
        fs = FLIT[name]
        flits = np.minimum(np.maximum((nbytes + fs - 1) // fs, 1), -(-136 // fs)).astype(np.uint32)
        assert (flits == capture.flits_for(nbytes, fs)).all()
        seen.add(int(flits.max()))
        one = booksim.replay(text, src, dst, flits, tinj, engine="cpu", arrivals=True)
        assert _full(one) == ref, name
        assert ref[0]["packets"] == len(src) and ref[0]["avg_latency"] > ref[0]["zero_load_latency"] > 0, name
    assert seen == {9, 5, 4}
    # the networks do differ
    assert len({r[0]["avg_latency"] for r in cpu_ref}) >= 6


def test_flits_come_from_the_bytes(native, plist, texts, cpu_ref):
    """A 16-byte-flit network replays 136 bytes as 9 flits, whatever flit
    count the capturing network had: its result differs from a replay with
    32-byte flits (5) on the same network."""
    src, dst, nbytes, tinj = plist
    i = list(NETS).index("cmesh_flit16")
    wrong = booksim.replay(texts[i], src, dst, capture.flits_for(nbytes, 32), tinj, engine="cpu", arrivals=True)
    assert _full(wrong) != cpu_ref[i]
    assert cpu_ref[i][0]["activity"]["buffer_writes"] > _full(wrong)[0]["activity"]["buffer_writes"]  # more flits written into buffers


def test_launch_lds_is_the_largest_networks(native, texts):
    """What a gpu launch over a set of networks asks for is the largest
    5 * U * V words among them, wherever that network stands in the list (a
    launch sized from the first network would let a larger one run past its
    LDS): a host computation, so checked without a device."""
    names = list(NETS)
    one = {n: native.icnt_replay_networks_lds_bytes([t]) for n, t in zip(names, texts)}
    print(one)
    assert one["fly_vc64"] > 48 * 1024 >= max(v for n, v in one.items() if n != "fly_vc64")
    assert one["cmesh_vc4"] == 4 * one["cmesh"] and one["fly"] < one["cmesh_vc4"]
    pick = lambda *ns: [texts[names.index(n)] for n in ns]
    for order in (("fly", "cmesh", "cmesh_vc4"), ("cmesh_vc4", "fly", "cmesh"), ("fly", "cmesh_vc4", "cmesh")):
        assert native.icnt_replay_networks_lds_bytes(pick(*order)) == one["cmesh_vc4"], order
    assert native.icnt_replay_networks_lds_bytes(texts) == one["fly_vc64"]
    assert native.icnt_replay_networks_lds_bytes(list(reversed(texts))) == one["fly_vc64"]
    assert native.icnt_replay_networks_lds_bytes([]) == 0


def test_cli_networks_take_flits_from_the_bytes(native, plist, texts, tmp_path):
    """booksim --replay FILE --networks: a list captured on a 40-byte-flit
    network (136 bytes: 4 flits) replays on a 16-byte-flit network with 9
    flits per 136-byte packet, not with the captured 4."""
    import json
    src, dst, nbytes, tinj = plist
    npz = str(tmp_path / "list.npz")
    np.savez(npz, src=src, dst=dst, flits=capture.flits_for(nbytes, 40), tinj=tinj, bytes=nbytes, nodes=np.uint32(NODES))
    files = []
    for n in ("cmesh", "cmesh_flit16"):
        f = tmp_path / f"{n}.icnt"
        f.write_text(texts[list(NETS).index(n)])
        files.append(str(f))
    out = tmp_path / "out.json"
    assert booksim.main(["--replay", npz, "--networks", ",".join(files), "--json", str(out)]) == 0
    got = json.loads(out.read_text())
    assert [g["config"] for g in got] == files
    for g, n in zip(got, ("cmesh", "cmesh_flit16")):
        want = booksim.replay(texts[list(NETS).index(n)], src, dst, capture.flits_for(nbytes, FLIT[n]), tinj)
        assert g["result"] == json.loads(json.dumps(dict(want))), n
    stale = booksim.replay(texts[list(NETS).index("cmesh_flit16")], src, dst, capture.flits_for(nbytes, 40), tinj)
    assert got[1]["result"]["avg_latency"] != stale["avg_latency"]


def test_cpu_par_equals_cpu(native, plist, texts, cpu_ref):
    res = booksim.replay_networks(*plist, texts, engine="cpu-par", arrivals=True, nodes=NODES)
    for name, d, ref in zip(NETS, res, cpu_ref):
        assert _full(d) == ref, name


def test_window_arguments(native, plist, texts):
    a = booksim.replay_networks(*plist, texts[:2], engine="cpu", cycles=400, warmup=100)
    src, dst, nbytes, tinj = plist
    for text, d in zip(texts[:2], a):
        one = booksim.replay(text, src, dst, capture.flits_for(nbytes, 40), tinj, cycles=400, warmup=100)
        assert {k: d[k] for k in KEYS} == {k: one[k] for k in KEYS}
        assert d["measured_packets"] < d["packets"]


def test_bad_input_names_the_network(native, plist, texts):
    src, dst, nbytes, tinj = plist
    mesh64 = _text(dict(k=8, n=2, topology="mesh"))
    with pytest.raises(ValueError, match=r"network 2 has 64 nodes, the packet list is for 32"):
        booksim.replay_networks(src, dst, nbytes, tinj, texts[:2] + [mesh64], nodes=NODES)
    # without a stated node count the 64-node mesh takes the list
    assert len(booksim.replay_networks(src, dst, nbytes, tinj, [mesh64])) == 1
    small = _text(dict(k=16, n=1, topology="fly"))  # 16 nodes: the memory nodes are out of range
    with pytest.raises(ValueError, match=r"network 1.*packet 0: node out of range"):
        booksim.replay_networks(src, dst, nbytes, tinj, [texts[0], small])
    loop = src.copy()
    loop[5] = dst[5]
    with pytest.raises(ValueError, match=r"network 0.*packet 5: source and destination"):
        booksim.replay_networks(loop, dst, nbytes, tinj, texts[:1])
    with pytest.raises(ValueError, match="differ in length"):
        booksim.replay_networks(src[:-1], dst, nbytes, tinj, texts[:1])
    with pytest.raises(ValueError, match="engine must be"):
        booksim.replay_networks(src, dst, nbytes, tinj, texts[:1], engine="fpga")
    assert booksim.replay_networks(src, dst, nbytes, tinj, []) == []


# ---- GPU ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_mod():
    import torch  # bind torch's HIP runtime first
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    from accel_sim_framework_distributed_amd import _native
    mod = _native.load(prefer_torch_runtime=True)
    assert mod.gpu_available(), "HIP engine cannot see the GPU (native code must run, no silent fallback)"
    return mod


@pytest.mark.gpu
def test_gpu_equals_cpu_lds_and_chunks(gpu_mod, plist, texts, cpu_ref):
    """lds=True: fly_vc64 is in the call, so the chunk that holds it keeps the
    words in HBM; a call without it runs from LDS.  A small budget splits the
    list of networks into several launches."""
    names = list(NETS)
    fit = [i for i, n in enumerate(names) if n != "fly_vc64"]
    res = booksim.replay_networks(*plist, [texts[i] for i in fit], engine="gpu", arrivals=True, nodes=NODES)
    st = gpu_mod.icnt_open_loop_batch_stats()
    print("fit:", st)
    assert st["chunks"] == 1 and st["lds_chunks"] == 1 and st["max_chunk_points"] == len(fit)
    for i, d in zip(fit, res):
        assert _full(d) == cpu_ref[i], names[i]
    # every network, the large one FIRST in its chunk and then last: the launch's LDS is the chunk's
    # largest either way, here beyond the limit, so the whole chunk runs from HBM
    for order in ([names.index("fly_vc64")] + fit, fit + [names.index("fly_vc64")]):
        res = booksim.replay_networks(*plist, [texts[i] for i in order], engine="gpu", arrivals=True, nodes=NODES)
        st = gpu_mod.icnt_open_loop_batch_stats()
        assert st["chunks"] == 1 and st["lds_chunks"] == 0
        for i, d in zip(order, res):
            assert _full(d) == cpu_ref[i], names[i]
    one_chunk = st["max_chunk_bytes"]
    # half of that (no less than the largest network's 2 MB): at least 2 chunks, the last one with
    # fly_vc64 from HBM, the others from LDS
    mb = max(2, (-(-one_chunk // (1 << 20))) // 2)
    res = booksim.replay_networks(*plist, texts, engine="gpu", arrivals=True, nodes=NODES, mem_budget_mb=mb)
    st = gpu_mod.icnt_open_loop_batch_stats()
    print("one chunk", one_chunk, "budget MB", mb, st)
    assert st["chunks"] >= 2 and 1 <= st["lds_chunks"] < st["chunks"] and st["max_chunk_bytes"] <= mb << 20
    for name, d, ref in zip(names, res, cpu_ref):
        assert _full(d) == ref, name


@pytest.mark.gpu
def test_gpu_lds_off(gpu_mod, plist, texts, cpu_ref):
    res = booksim.replay_networks(*plist, texts, engine="gpu", arrivals=True, nodes=NODES, lds=False)
    assert gpu_mod.icnt_open_loop_batch_stats()["lds_chunks"] == 0
    for name, d, ref in zip(NETS, res, cpu_ref):
        assert _full(d) == ref, name


@pytest.mark.gpu
def test_gpu_lds_is_sized_for_the_largest_network(gpu_mod, plist, texts, cpu_ref):
    """The smallest network first, the largest LDS user that fits last
    (cmesh_vc4, four VCs against the first network's one): a launch
    sized from the first network would let the last one write past its LDS."""
    names = list(NETS)
    order = [names.index("fly"), names.index("cmesh"), names.index("cmesh_vc4")]
    res = booksim.replay_networks(*plist, [texts[i] for i in order], engine="gpu", arrivals=True, nodes=NODES)
    assert gpu_mod.icnt_open_loop_batch_stats()["lds_chunks"] == 1
    for i, d in zip(order, res):
        assert _full(d) == cpu_ref[i], names[i]
    info = gpu_mod.icnt_net_kernel_info()
    print(info)
    assert info["num_regs"] > 0 and info["max_threads_per_block"] >= 64


@pytest.mark.gpu
def test_gpu_budget_too_small_names_the_network(gpu_mod, plist, texts):
    # the 32-node line's longest route is 32 links: its per-hop words alone pass 1 MB
    with pytest.raises(ValueError, match=r"network 0 needs \d+ MB, the memory budget is 1 MB"):
        booksim.replay_networks(*plist, texts, engine="gpu", mem_budget_mb=1)

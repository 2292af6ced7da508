"""The packet link model against a model-independent oracle, and the device
epoch loop (csrc/parallel/linksim_dev.hip) word for word against the host
protocol.

Three implementations of one collective are compared:

* ``oracle``: a plain-Python event simulation written from the header
  comments of csrc/parallel/linksim.h and linksim_core.h.  It imports no
  native code and simulates no epochs: one global heap of sends keyed
  (ready_ps, chan, step, slice, rank), popped in order.  It pins the schedule
  geometry and the packet rules that the host and the device share through
  linksim_core.h (and so cannot disagree about).
* ``reenact``: the distributed protocol of parallel/collectives.py
  PacketExchange.run, driven in one process over W host LinkSims through the
  LinkSim.pack_epoch / unpack_epoch bindings.  It yields every epoch's send
  words, the overflow words, the epoch count and each rank's packet count.
* the device: ``_asim_dist.dev_run_local(record=True)`` returns every rank's
  packed send buffer after each epoch kernel, the overflow exchange's sizes
  and words, and every rank's final counters.

finish_ps alone does not see the protocol words: emission times are
max(ready, link_free) and do not depend on where the epoch windows fall, so a
wrong announced next event, busy flag, earliest arrival or largest count only
changes the epoch count or the deadlock check.  The GPU tests therefore compare
all slot words (unused ones included) of every epoch, rank and destination,
and the epoch count of every rank.

The case list covers what tests/test_device_exchange.py cannot reach: more
ranks than links (several destinations per link lane), worlds above 64 (the
64-lane loops go round twice), 1 and 64 links, non-zero roots, exactly K and
K + 1 packets for one destination, overflow in consecutive epochs, starts near
10**15; ``test_case_list_keeps_its_edges`` asserts, from the host
re-enactment alone, that the list still has them.
"""
import functools
import heapq
import math
from collections import namedtuple

import numpy as np
import pytest
import torch  # noqa: F401  (first: the process binds torch's HIP runtime, which the device loop's extension needs)

K, HDR = 8, 8
SLOT = HDR + 4 * K
I64_MAX = (1 << 63) - 1
DLS_DONE = 1

BASE = dict(link_gbps=153.0, latency_ns=1000.0, links=7, slice_bytes=65536, max_channels=16, reduce_gbps=900.0)

# expect: (packets, protocol epochs, overflow epochs, largest per-destination count in one epoch), or None
Case = namedtuple("Case", "name kind starts over nbytes root expect record")


def _c(name, kind, starts, over, nbytes, root, expect, record=True):
    return Case(name, kind, [int(s) for s in starts], over, int(nbytes), root, expect, record)


CASES = [
    _c("allreduce8", "AllReduce", [0] * 8, {}, 8 << 20, 0, (1792, 25, 0, 3)),
    _c("allreduce8_slice64", "AllReduce", [0] * 8, dict(slice_bytes=64), 1 << 20, 0, (229376, 15, 14, 512)),
    _c("allreduce12_links3", "AllReduce", [0] * 12, dict(links=3), 1 << 20, 0, (792, 28, 0, 1)),
    _c("allgather12_links3_staggered", "AllGather", [0, 5, 0, 0, 10**6, 0, 0, 0, 0, 0, 0, 3],
       dict(links=3, slice_bytes=4096), 3 * 2**18 + 100, 0, (2376, 13, 10, 12)),
    _c("reducescatter12_links3", "ReduceScatter", [0] * 12, dict(links=3), 1 << 20, 0, (396, 15, 0, 1)),
    _c("allreduce5_links1", "AllReduce", [0] * 5, dict(links=1), 256 << 10, 0, (40, 12, 0, 1)),
    _c("alltoall72_links2", "AllToAll", [0] * 72, dict(links=2), 64 << 10, 0, (5112, 2, 0, 1)),
    _c("alltoall16", "AllToAll", [0] * 16, {}, 256 << 10, 0, (240, 2, 0, 1)),
    _c("alltoall16_links2_slice256", "AllToAll", [0] * 16, dict(links=2, slice_bytes=256), 36864, 0, (2160, 2, 1, 9)),
    _c("broadcast5_root3", "Broadcast", [0] * 5, {}, 4 << 20, 3, (256, 12, 0, 3)),
    _c("broadcast9_links2_root7", "Broadcast", [0, 0, 0, 7 * 10**6, 0, 0, 0, 0, 0], dict(links=2), 1 << 20, 7,
       (128, 15, 0, 3)),
    _c("reduce3_root2", "Reduce", [0, 0, 10**6], {}, 2 << 20, 2, (64, 10, 0, 3)),
    _c("reduce7_links2_root5", "Reduce", [0] * 7, dict(links=2, slice_bytes=1000), 123457, 5, (744, 7, 6, 62)),
    _c("sendrecv2", "SendRecv", [0, 2 * 10**6], {}, 1 << 20, 0, (32, 10, 0, 3)),
    _c("sendrecv3_k_plus_1", "SendRecv", [0] * 3, dict(slice_bytes=64), 576, 0, (27, 2, 1, K + 1)),
    _c("sendrecv3_k", "SendRecv", [0] * 3, dict(slice_bytes=64), 512, 0, (24, 2, 0, K)),
    _c("allreduce4_one_byte", "AllReduce", [0] * 4, {}, 1, 0, (48, 7, 0, 1)),
    _c("allreduce4_late_clock", "AllReduce", [10**15, 10**15 + 3 * 10**6, 10**15, 10**15], {}, 4 << 20, 0,
       (384, 25, 0, 3)),
    _c("allreduce6_odd_rates", "AllReduce", [0] * 6,
       dict(link_gbps=50.0, latency_ns=300.0, reduce_gbps=333.0, slice_bytes=1000), 777777, 0, (7800, 45, 43, 16)),
    _c("broadcast1", "Broadcast", [7], {}, 1 << 20, 0, (0, 1, 0, 0)),
    # every lane owns exactly one destination; expected values come from the re-enactment
    _c("alltoall65_links64", "AllToAll", [0] * 65, dict(links=64, max_channels=64), 65 * 64, 0, None),
    # heavy: final state only
    _c("allreduce67_links64", "AllReduce", [0] * 67, dict(links=64, max_channels=64), 1 << 20, 0,
       (566016, 133, 0, 1), record=False),
]
IDS = [c.name for c in CASES]


def _params(c):
    return dict(BASE, **c.over)


# ---------------------------------------------------------------------------
# a. the oracle


def _inv_mod(s, n):
    for x in range(1, n):
        if (s * x) % n == 1:
            return x
    return 1


def oracle(params, kind, nbytes, starts, root=0):
    """Finish time of every rank and the packet total, from the rules in the
    header comments of linksim.h / linksim_core.h.  No epochs."""
    N = len(starts)
    links = max(1, int(params["links"]))
    ring = kind not in ("AllToAll", "SendRecv")
    strides = []
    if N > 1:
        cap = max(1, min(int(params["links"]), int(params["max_channels"]))) if ring else 1
        for s in range(1, N):
            if len(strides) < cap and math.gcd(s, N) == 1:
                strides.append(s)
    if not strides:
        strides = [1]
    nch = len(strides)
    root = root % N
    if kind == "AllReduce":
        nsteps, chunk = 2 * (N - 1), nbytes // (nch * N)
    elif kind in ("AllGather", "ReduceScatter"):
        nsteps, chunk = N - 1, nbytes // (nch * N)
    elif kind in ("Broadcast", "Reduce"):
        nsteps, chunk = N - 1, nbytes // nch
    elif kind == "AllToAll":
        nsteps, chunk = N - 1, nbytes // N
    elif kind == "SendRecv":
        nsteps, chunk = 1, nbytes
    else:
        raise ValueError(kind)
    if N == 1:
        nsteps = 0
    chunk = max(chunk, 1)
    slice_bytes = max(int(params["slice_bytes"]), 64)
    nslices = (chunk + slice_bytes - 1) // slice_bytes
    lat = max(int(round(params["latency_ns"] * 1000)), 1000)
    link_gbps, reduce_gbps = float(params["link_gbps"]), float(params["reduce_gbps"])
    inv = [_inv_mod(s, N) for s in strides]

    def slice_len(s):
        return min(slice_bytes, chunk - s * slice_bytes)

    def chain_pos(r, ch):
        # Broadcast: the chain starts at root; Reduce: the chain ends at root
        first = root if kind == "Broadcast" else root + strides[ch]
        return ((r - first) * inv[ch]) % N

    def send_peer(r, ch, k):
        if k < 0 or k >= nsteps:
            return -1
        if kind in ("AllReduce", "AllGather", "ReduceScatter"):
            return (r + strides[ch]) % N
        if kind in ("Broadcast", "Reduce"):
            pos = chain_pos(r, ch)
            return (r + strides[ch]) % N if (k == pos and pos < N - 1) else -1
        if kind == "AllToAll":
            return (r + k + 1) % N
        return (r + 1) % N

    def depends(r, ch, k):
        """Step k of rank r waits for an arrival (of step k - 1)."""
        if not ring or k == 0:
            return False
        if kind in ("Broadcast", "Reduce"):
            return chain_pos(r, ch) == k  # the rank at position k received step k - 1
        return True

    def reduces(k):
        if kind == "AllReduce":
            return k < N - 1
        return kind in ("ReduceScatter", "Reduce")

    finish = [int(s) for s in starts]
    link_free = [[int(starts[r])] * links for r in range(N)]
    heap = []
    for r in range(N):
        for ch in range(nch):
            for k in range(nsteps):
                if send_peer(r, ch, k) >= 0 and not depends(r, ch, k):
                    for s in range(nslices):
                        heap.append((int(starts[r]), ch, k, s, r))
    heapq.heapify(heap)
    packets = 0
    while heap:
        ready, ch, k, s, r = heapq.heappop(heap)
        d = send_peer(r, ch, k)
        link = ((d - r - 1) % N) % links
        b = slice_len(s)
        start = max(ready, link_free[r][link])
        ser = math.ceil(b * 1000.0 / link_gbps)
        link_free[r][link] = start + ser
        finish[r] = max(finish[r], start + ser)
        packets += 1
        arrive = start + ser + lat
        per = 3.0 if reduces(k) else 1.0
        done = arrive + math.ceil(b * per * 1000.0 / reduce_gbps)
        finish[d] = max(finish[d], done)
        if ring and send_peer(d, ch, k + 1) >= 0:
            heapq.heappush(heap, (done, ch, k + 1, s, d))
    return finish, packets


# ---------------------------------------------------------------------------
# b. the protocol re-enactment

Enact = namedtuple("Enact", "finish_ps packets_sent epochs sends spills counts")


def reenact(mod, params, kind, nbytes, starts, root=0, keep=True):
    """PacketExchange.run's Python loop for every rank in one process.
    sends: per epoch [W][W][SLOT] (None unless keep); spills: per overflow
    epoch (epoch, extra_words [W][W], overflow words per source); counts: per
    epoch the [W][W] per-destination packet counts."""
    W = len(starts)
    ls = [mod.LinkSim(params, kind, int(nbytes), int(root), r, W, int(starts[r])) for r in range(W)]
    t = min(min(int(s) for s in starts), I64_MAX)
    E = int(ls[0].epoch_ps)
    ann = [(min(int(l.next_event()), I64_MAX), 0 if l.done() else 1) for l in ls]
    none = np.zeros(0, np.int64)
    sends, spills, counts = [], [], []
    epochs = 0
    while True:
        t_end = t + E
        send = np.zeros((W, W, SLOT), np.int64)
        extra, extra_words = [], []
        for r in range(W):
            x, xw, _, _ = ls[r].pack_epoch(t_end, K, HDR, ann[r][0], ann[r][1], send[r].reshape(-1))
            extra.append(np.asarray(x, np.int64))
            extra_words.append([int(w) for w in xw])
        counts.append(send[:, :, 0].copy())
        if keep:
            sends.append(send)
        spill = int(send[:, :, 1].max()) > K
        if spill:
            spills.append((epochs, extra_words, extra))
        res = []
        for d in range(W):
            recv = np.ascontiguousarray(send[:, d, :])
            inc = none
            if spill:
                # overflow words for d, regrouped in source order
                parts = []
                for s in range(W):
                    o = sum(extra_words[s][:d])
                    parts.append(extra[s][o:o + extra_words[s][d]])
                inc = np.concatenate(parts) if parts else none
                assert len(inc) == sum(4 * max(0, int(c) - K) for c in recv[:, 0])
            res.append(tuple(int(v) for v in ls[d].unpack_epoch(recv.reshape(-1), K, HDR, inc)))
        epochs += 1
        assert len(set(res)) == 1  # the stop and the next epoch are global decisions
        any_busy, g = res[0]
        if not any_busy:
            break
        ann = [(min(int(l.next_event()), I64_MAX), 0 if l.done() else 1) for l in ls]
        if g >= I64_MAX:
            raise RuntimeError("packet collective deadlocked (no rank has pending work)")
        t = max(t_end, g)
    return Enact([int(l.finish_ps) for l in ls], [int(l.packets_sent) for l in ls], epochs, sends, spills, counts)


@functools.lru_cache(maxsize=None)
def _oracle(i):
    c = CASES[i]
    return oracle(_params(c), c.kind, c.nbytes, c.starts, c.root)


@functools.lru_cache(maxsize=None)
def _enact(i):
    from accel_sim_framework_distributed_amd import _native
    c = CASES[i]
    return reenact(_native.load(), _params(c), c.kind, c.nbytes, c.starts, c.root, keep=c.record)


def _overflow_epochs(e):
    return [ep for ep, _, _ in e.spills]


def _longest_run(epochs):
    best = run = 0
    last = None
    for ep in epochs:
        run = run + 1 if last is not None and ep == last + 1 else 1
        best = max(best, run)
        last = ep
    return best


# ---------------------------------------------------------------------------
# c. CPU tests


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_oracle_host_and_protocol_agree(native, i):
    from accel_sim_framework_distributed_amd.parallel import collectives
    c = CASES[i]
    fin, packets = _oracle(i)
    host = collectives.emulate(_params(c), c.kind, c.nbytes, c.starts, c.root)
    e = _enact(i)
    assert [int(v) for v in host["finish_ps"]] == fin
    assert e.finish_ps == fin
    assert int(host["packets"]) == packets
    assert sum(e.packets_sent) == packets
    assert sum(int(n.sum()) for n in e.counts) == packets
    if c.expect is not None:
        largest = max(int(n.max()) for n in e.counts)
        assert (packets, e.epochs, len(e.spills), largest) == c.expect


def test_case_list_keeps_its_edges(native):
    """Computed from the host re-enactment alone: the case list still holds
    every edge the device tests are there for."""
    stats = []
    for i, c in enumerate(CASES):
        e = _enact(i)
        stats.append(dict(case=c, largest=max(int(n.max()) for n in e.counts), overflow=_overflow_epochs(e),
                          spills=e.spills))
    assert any(s["largest"] == K and not s["overflow"] for s in stats)
    assert any(s["largest"] == K + 1 for s in stats)
    assert any(_longest_run(s["overflow"]) >= 3 for s in stats)

    def shared_link_overflow(s):
        c = s["case"]
        N, links = len(c.starts), max(1, int(_params(c)["links"]))
        for _, extra_words, _ in s["spills"]:
            for src in range(N):
                on_link = {}
                for d in range(N):
                    if extra_words[src][d] > 0:
                        link = ((d - src - 1) % N) % links
                        on_link[link] = on_link.get(link, 0) + 1
                if any(n >= 2 for n in on_link.values()):
                    return True
        return False

    assert any(shared_link_overflow(s) for s in stats)
    assert any(len(c.starts) > 64 for c in CASES)
    assert any(len(c.starts) > 64 and c.record for c in CASES)
    assert any(_params(c)["links"] == 1 for c in CASES)
    assert any(_params(c)["links"] == 64 for c in CASES)
    assert any(c.kind == "Broadcast" and c.root % len(c.starts) != 0 for c in CASES)
    assert any(c.kind == "Reduce" and c.root % len(c.starts) != 0 for c in CASES)
    assert any(len(set(c.starts)) > 1 for c in CASES)
    assert any(min(c.starts) >= 10**15 for c in CASES)
    # more ranks than links + 1: a link lane carries several destinations
    assert any(len(c.starts) > _params(c)["links"] + 1 for c in CASES)


# ---------------------------------------------------------------------------
# d. GPU tests


def _ext():
    from accel_sim_framework_distributed_amd import _native
    ext = _native.load_dist()
    if ext is None:
        raise RuntimeError("_asim_dist (device epoch loop) is not built: run build_native.py")
    return ext


def _first_diff(dev, ref):
    """(epoch, rank, destination, word) of the first differing send word."""
    idx = np.argwhere(dev != ref)[0]
    return tuple(int(v) for v in idx), int(dev[tuple(idx)]), int(ref[tuple(idx)])


def _check_final(c, r, fin, e):
    W = len(c.starts)
    rk = r["ranks"]
    assert [int(v) for v in r["finish_ps"]] == fin
    assert [int(v) for v in rk["finish_ps"]] == fin
    assert [int(v) for v in rk["sent"]] == e.packets_sent
    assert [int(v) for v in rk["packets"]] == e.packets_sent
    assert [int(v) for v in rk["epochs"]] == [e.epochs] * W
    assert [int(v) for v in rk["status"]] == [DLS_DONE] * W
    assert len(set(int(v) for v in rk["channels"])) == 1
    # every launch that ran took one of the two memory paths: the first, one
    # per delivered exchange, and one more per overflow exchange
    launches = 1 + e.epochs + len(e.spills)
    assert [int(a) + int(b) for a, b in zip(rk["launches_lds"], rk["launches_hbm"])] == [launches] * W


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_device_words_match_host_protocol(native, i):
    ext = _ext()
    c = CASES[i]
    p = _params(c)
    fin, _ = _oracle(i)
    e = _enact(i)
    if c.record:
        r = ext.dev_run_local(p, c.kind, c.nbytes, c.root, c.starts, 0, record=True)
        dev = r["send"].numpy()
        ref = np.stack(e.sends)
        assert dev.shape == ref.shape, (dev.shape, ref.shape)
        if not np.array_equal(dev, ref):
            pytest.fail("first differing (epoch, rank, destination, word), device, host: %r" % (_first_diff(dev, ref),))
        assert [int(v) for v in r["spill_epochs"]] == _overflow_epochs(e)
        for (_, ew, xw), dew, dxw in zip(e.spills, r["spill_extra_words"], r["spill_extra"]):
            assert [[int(v) for v in row] for row in dew] == ew
            for s in range(len(c.starts)):
                assert [int(v) for v in dxw[s]] == [int(v) for v in xw[s]], ("overflow words of source", s)
        _check_final(c, r, fin, e)
        if c.name == "allreduce8":
            assert all(int(v) == 0 for v in r["ranks"]["launches_hbm"])
        if c.name == "allreduce8_slice64":
            # ~2048 pending sends at the start do not fit in LDS; the drained heaps at the end do
            # (measured on an MI355X: 29 launches in HBM, then 1 in LDS; allreduce8 above: 26 in LDS)
            assert all(int(v) > 0 for v in r["ranks"]["launches_hbm"])
            assert all(int(v) > 0 for v in r["ranks"]["launches_lds"])
    # the default batching: same results, same epoch count, same paths
    u = ext.dev_run_local(p, c.kind, c.nbytes, c.root, c.starts, 0)
    assert "send" not in u
    _check_final(c, u, fin, e)
    assert int(u["epochs"]) == e.epochs
    if c.record:
        assert u["ranks"]["launches_lds"] == r["ranks"]["launches_lds"]


def test_recording_rejects_a_loopback_group():
    ext = _ext()  # the arguments are refused before anything touches the device
    with pytest.raises(ValueError):
        ext.dev_run_local(BASE, "AllReduce", 1 << 20, 0, [0, 0], 0, loopback=object(), record=True)

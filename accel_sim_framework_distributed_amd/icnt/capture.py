"""Network-traffic capture files of the cycle engines (``-icnt_capture FILE``,
``simulate(..., icnt_capture=path)``): every SM-to-L2 request and L2-to-SM
reply packet the simulation injected, per subnet in epoch, mailbox cell, slot
order.  The layout is defined in ``csrc/model/icnt_capture.h``: a 64-byte
little-endian header, then the request subnet's 24-byte records, then the
reply subnet's.

    cap = capture.load("run.icap")
    cap.request.src, cap.request.bytes, cap.reply.tinj, cap.flit_size
    capture.save_npz("req.npz", cap, "request")     # booksim --replay req.npz

    rl = capture.request_list(cap)                  # booksim.closed_loop_replay(rl.src, ...)

Two ways to replay a capture.  An open-loop replay (``booksim --replay``) of
one subnet injects every packet at its recorded time, the replies whatever
the replayed network does to the requests they answer: it compares networks
under the same offered traffic.  A closed-loop replay (``booksim
--closed-loop --replay``, :func:`request_list`) takes the requests alone:
each reply is created by its request's delivery on the replayed network, and
a node keeps a bounded number of requests in flight, so the figure is the
time the application's own requests take on that network.  What remains
trace driven: the captured creation times embed the back-pressure of the
network that was simulated (a packet the injection queue held back is
recorded when it left; ``timing="batch"`` drops the times and keeps the
order), the L2's service time is one scalar per call, and the capture does
not say which reply answers which read -- :func:`request_list` pairs them in
record order within a (cluster, sub-partition, kind) group, which keeps every
group's reply count and bytes exactly but may swap the sizes of two reads of
one group that the L2 answered out of order.
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import numpy as np

MAGIC = int.from_bytes(b"ASIMICAP", "little")
VERSION = 1
SUBNETS = ("request", "reply")

HEADER = np.dtype([("magic", "<u8"), ("version", "<u4"), ("rec_bytes", "<u4"), ("nodes", "<u4"),
                   ("n_clusters", "<u4"), ("n_subpart", "<u4"), ("flit_size", "<u4"), ("per_icnt", "<u8"),
                   ("count", "<u8", (2,)), ("reserved", "<u8")])
RECORD = np.dtype([("tinj", "<u8"), ("src", "<u4"), ("dst", "<u4"), ("bytes", "<u2"), ("flits", "<u2"),
                   ("type", "u1"), ("subnet", "u1"), ("pad", "<u2")])
assert HEADER.itemsize == 64 and RECORD.itemsize == 24


@dataclasses.dataclass
class Subnet:
    src: np.ndarray    # uint32 node
    dst: np.ndarray    # uint32 node
    bytes: np.ndarray  # uint32 bytes on the wire
    flits: np.ndarray  # uint32 flits on the capturing network
    tinj: np.ndarray   # uint64 injection time, interconnect cycles
    type: np.ndarray   # uint8 packet type (csrc/model/types.h PktType)

    def __len__(self) -> int:
        return len(self.src)


@dataclasses.dataclass
class Capture:
    version: int
    nodes: int         # nodes of the capturing network
    n_clusters: int    # cluster c is node c
    n_subpart: int     # L2 sub-partition s is node n_clusters + s
    flit_size: int     # bytes per flit of the capturing network
    per_icnt_fs: int   # interconnect clock period, femtoseconds
    counts: tuple      # (request, reply) records
    request: Subnet
    reply: Subnet

    def subnet(self, name: str) -> Subnet:
        if name not in SUBNETS:
            raise ValueError(f"subnet must be request or reply, not {name!r}")
        return self.request if name == "request" else self.reply


def is_capture(path: str) -> bool:
    """Whether the file starts with the capture magic."""
    with open(path, "rb") as f:
        return f.read(8) == MAGIC.to_bytes(8, "little")


def load(path: str) -> Capture:
    """The header fields and both subnets' arrays.  ValueError: a foreign,
    truncated or otherwise inconsistent file."""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < HEADER.itemsize:
        raise ValueError(f"{path}: not a capture file (shorter than its header)")
    h = np.frombuffer(raw, HEADER, 1)[0]
    if int(h["magic"]) != MAGIC:
        raise ValueError(f"{path}: not a capture file (bad magic)")
    if int(h["version"]) != VERSION or int(h["rec_bytes"]) != RECORD.itemsize:
        raise ValueError(f"{path}: capture version {int(h['version'])} with {int(h['rec_bytes'])}-byte records, "
                         f"this reader knows version {VERSION} with {RECORD.itemsize}")
    n0, n1 = int(h["count"][0]), int(h["count"][1])
    want = HEADER.itemsize + (n0 + n1) * RECORD.itemsize
    if len(raw) != want:
        raise ValueError(f"{path}: truncated or overlong capture file ({len(raw)} bytes, the header promises {want})")
    rec = np.frombuffer(raw, RECORD, n0 + n1, HEADER.itemsize)
    if (rec["subnet"][:n0] != 0).any() or (rec["subnet"][n0:] != 1).any():
        raise ValueError(f"{path}: a record is filed under the wrong subnet")
    if n0 + n1 and max(int(rec["src"].max()), int(rec["dst"].max())) >= int(h["nodes"]):
        raise ValueError(f"{path}: a record names a node beyond the header's {int(h['nodes'])}")

    def part(r) -> Subnet:
        return Subnet(r["src"].astype(np.uint32), r["dst"].astype(np.uint32), r["bytes"].astype(np.uint32),
                      r["flits"].astype(np.uint32), r["tinj"].astype(np.uint64), r["type"].astype(np.uint8))
    return Capture(int(h["version"]), int(h["nodes"]), int(h["n_clusters"]), int(h["n_subpart"]), int(h["flit_size"]),
                   int(h["per_icnt"]), (n0, n1), part(rec[:n0]), part(rec[n0:]))


def flits_for(nbytes, flit_size: int, max_bytes: int = 136) -> np.ndarray:
    """What a network with `flit_size`-byte flits makes of packets of `nbytes`
    bytes: ceil(bytes / flit_size), at least 1, at most the largest packet's
    (icnt_router.h rt_flits, kRtMaxPktBytes)."""
    b = np.asarray(nbytes, dtype=np.uint64)
    f = np.maximum((b + flit_size - 1) // flit_size, 1)
    return np.minimum(f, max(-(-max_bytes // flit_size), 1)).astype(np.uint32)


# the one reply type that answers each request type (csrc/model/types.h PktType, mem.h)
ANSWER = {1: 4, 2: 5, 3: 6}  # P_RD: P_RD_REPLY, P_WR: P_WR_ACK, P_ATOM: P_ATOM_REPLY
TYPE_NAMES = {1: "P_RD", 2: "P_WR", 3: "P_ATOM", 4: "P_RD_REPLY", 5: "P_WR_ACK", 6: "P_ATOM_REPLY"}


@dataclasses.dataclass
class RequestList:
    src: np.ndarray          # uint32 node
    dst: np.ndarray          # uint32 node
    req_bytes: np.ndarray    # uint32 bytes of the request on the wire
    reply_bytes: np.ndarray  # uint32 bytes of its reply
    tcreate: np.ndarray      # uint64 creation time, interconnect cycles; non-decreasing
    type: np.ndarray         # uint8 request type
    nodes: int               # nodes of the capturing network
    dropped: int = 0         # unanswered requests left out (unanswered="drop")
    # optional, both or neither: uint32 cycles a request holds its memory node and the latency behind it
    # (the memory point `list` of booksim.closed_loop_replay); a capture does not record them
    occupancy: Optional[np.ndarray] = None
    latency: Optional[np.ndarray] = None

    def __len__(self) -> int:
        return len(self.src)


def request_list(cap: Capture, timing: str = "captured", unanswered: str = "error") -> RequestList:
    """The capture's requests with the sizes of their replies, the input of a
    closed-loop replay (``booksim.closed_loop_replay``), which creates each
    reply from its request's delivery.

    Pairing.  Every request type has one answering type (:data:`ANSWER`), so
    within a group -- the requests of type T from node a to node b -- the k-th
    request record takes the bytes of the k-th reply record of the answering
    type from b to a, both in file order.  This keeps every group's reply
    count and reply bytes exactly.  The capture does not say which reply
    answers which read, and this pairing may swap the sizes of two reads of
    one group that the L2 answered out of order.

    A group with more requests than replies (a run cut short) raises
    ValueError naming the group; with ``unanswered="drop"`` the group's surplus
    last requests are left out and counted in ``dropped``.  More replies than
    requests always raises: no request could have created them.

    ``timing="captured"``: ``tcreate`` is the captured injection time, which
    embeds the capturing network's back-pressure.  ``timing="batch"``: all
    zeros, every request ready at the start.  In both modes the list is in
    stable order of the captured time, so a node's requests keep their issue
    order and ``tcreate`` is non-decreasing."""
    if timing not in ("captured", "batch"):
        raise ValueError(f"timing must be captured or batch, not {timing!r}")
    if unanswered not in ("error", "drop"):
        raise ValueError(f"unanswered must be error or drop, not {unanswered!r}")
    q, p = cap.request, cap.reply
    for sub, known, name in ((q, ANSWER, "request"), (p, {v: k for k, v in ANSWER.items()}, "reply")):
        odd = ~np.isin(sub.type, list(known))
        if odd.any():
            i = int(np.flatnonzero(odd)[0])
            raise ValueError(f"{name} record {i} has type {int(sub.type[i])}, which is no {name} type")
    n = np.uint64(max(cap.nodes, 1))
    kq = (q.src.astype(np.uint64) * n + q.dst.astype(np.uint64)) * np.uint64(8) + q.type.astype(np.uint64)
    kp = (p.dst.astype(np.uint64) * n + p.src.astype(np.uint64)) * np.uint64(8) + (p.type.astype(np.uint64) - np.uint64(3))

    def group(key: int) -> str:
        t, ab = int(key) % 8, int(key) // 8
        return (f"{TYPE_NAMES[t]} from node {ab // int(n)} to node {ab % int(n)}: "
                f"{int((kq == key).sum())} requests, {int((kp == key).sum())} {TYPE_NAMES[ANSWER[t]]} records")

    oq, op = np.argsort(kq, kind="stable"), np.argsort(kp, kind="stable")
    kq_s, kp_s = kq[oq], kp[op]
    # replies nobody asked for
    extra = (np.searchsorted(kp_s, kp_s, "right") - np.searchsorted(kp_s, kp_s, "left")
             > np.searchsorted(kq_s, kp_s, "right") - np.searchsorted(kq_s, kp_s, "left"))
    if extra.any():
        raise ValueError("more replies than requests: " + group(kp_s[np.flatnonzero(extra)[0]]))
    # a request's rank within its group, in file order, and its group's first reply
    rank = np.empty(len(kq), np.int64)
    rank[oq] = np.arange(len(kq)) - np.searchsorted(kq_s, kq_s, "left")
    first = np.searchsorted(kp_s, kq, "left")
    answered = rank < np.searchsorted(kp_s, kq, "right") - first
    if not answered.all() and unanswered == "error":
        raise ValueError("more requests than replies: " + group(kq[np.flatnonzero(~answered)[0]]))
    keep = np.flatnonzero(answered)
    reply_bytes = p.bytes[op[(first + rank)[keep]]] if len(keep) else np.zeros(0, np.uint32)
    order = np.argsort(q.tinj[keep], kind="stable")
    keep = keep[order]
    tinj = q.tinj[keep].astype(np.uint64)
    return RequestList(q.src[keep].astype(np.uint32), q.dst[keep].astype(np.uint32), q.bytes[keep].astype(np.uint32),
                       reply_bytes[order].astype(np.uint32), tinj if timing == "captured" else np.zeros_like(tinj),
                       q.type[keep].astype(np.uint8), cap.nodes, int(len(kq) - len(keep)))


def save_request_npz(path: str, rl: RequestList, occupancy=None, latency=None) -> None:
    """A request list in the layout ``booksim --closed-loop --replay`` reads
    (src, dst, bytes, reply_bytes, tinj), with ``nodes`` beside them.  The
    per-request ``occupancy`` and ``latency`` of the memory endpoint (the
    arguments, else the list's own) are written when there are both."""
    occupancy = rl.occupancy if occupancy is None else occupancy
    latency = rl.latency if latency is None else latency
    if (occupancy is None) != (latency is None):
        raise ValueError("save_request_npz: occupancy and latency go together (one is missing)")
    mem = {}
    if occupancy is not None:
        for name, a in (("occupancy", occupancy), ("latency", latency)):
            a = np.asarray(a)
            if a.shape != (len(rl),):
                raise ValueError(f"save_request_npz: {name} has shape {a.shape}, the list has {len(rl)} requests")
            if len(a) and int(a.min()) < 0:
                raise ValueError(f"save_request_npz: {name} has a negative value")
            mem[name] = a.astype(np.uint32)
    np.savez(path, src=rl.src, dst=rl.dst, bytes=rl.req_bytes, reply_bytes=rl.reply_bytes, tinj=rl.tcreate,
             nodes=np.uint32(rl.nodes), **mem)


def save_npz(path: str, cap: Capture, subnet: str = "request", flit_size: Optional[int] = None) -> None:
    """One subnet in the layout ``booksim --replay`` reads (src, dst, flits,
    tinj), with ``bytes`` and ``nodes`` beside them.  `flit_size`: recompute
    the flits for a network with another flit size."""
    s = cap.subnet(subnet)
    flits = s.flits if flit_size is None else flits_for(s.bytes, flit_size)
    np.savez(path, src=s.src, dst=s.dst, flits=flits, tinj=s.tinj, bytes=s.bytes, nodes=np.uint32(cap.nodes))

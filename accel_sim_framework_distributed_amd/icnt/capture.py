"""Network-traffic capture files of the cycle engines (``-icnt_capture FILE``,
``simulate(..., icnt_capture=path)``): every SM-to-L2 request and L2-to-SM
reply packet the simulation injected, per subnet in epoch, mailbox cell, slot
order.  The layout is defined in ``csrc/model/icnt_capture.h``: a 64-byte
little-endian header, then the request subnet's 24-byte records, then the
reply subnet's.

    cap = capture.load("run.icap")
    cap.request.src, cap.request.bytes, cap.reply.tinj, cap.flit_size
    capture.save_npz("req.npz", cap, "request")     # booksim --replay req.npz

A trace-driven caveat: the captured injection times embed the back-pressure
of the network that was simulated (a packet the injection queue held back is
recorded when it left), and a replay is open loop -- the replies are injected
at their recorded times, whatever the replayed network does to the requests
they answer.  A replay therefore compares networks under the same offered
traffic; it does not predict the application's run time on them.
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


def save_npz(path: str, cap: Capture, subnet: str = "request", flit_size: Optional[int] = None) -> None:
    """One subnet in the layout ``booksim --replay`` reads (src, dst, flits,
    tinj), with ``bytes`` and ``nodes`` beside them.  `flit_size`: recompute
    the flits for a network with another flit size."""
    s = cap.subnet(subnet)
    flits = s.flits if flit_size is None else flits_for(s.bytes, flit_size)
    np.savez(path, src=s.src, dst=s.dst, flits=flits, tinj=s.tinj, bytes=s.bytes, nodes=np.uint32(cap.nodes))

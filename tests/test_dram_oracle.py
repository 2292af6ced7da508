"""The DRAM channel's command timing against a plain-Python oracle.

tests/test_memory_oracle.py is untimed: with one access in flight it can only
compare the order of RD / WR / ACT / PRE per bank.  This file pins WHEN a DRAM
command may issue.  `DramOracle` is one channel's scheduler (dram_cycle in
csrc/model/mem.h) in plain integer Python, written from the comments and rules
of mem.h: every timing gate, the single and the dual command bus, row hits
first against oldest first, FIFO, the separate write queue's watermarks and
-gpgpu_simple_dram_model.  It parses the option strings itself and never
calls native.parse_config.

The scheduler is a deterministic function of its options, of the requests
that enter its queue (DRAM cycle, read or write, bank, row; the "queues"
lines of the MEMORY_PARTITION_UNIT stream) and of how full the data return
ring is.  The oracle takes the queue entries of one channel from the run and
gives every command with its DRAM cycle; the whole list is compared, cycles
included, with the "DRAM RD / WR / ACT / PRE" lines of that channel.

Premise (the return ring): a read is picked only while the ring holds fewer
than 256 entries, and the ring hands an entry on in the first DRAM cycle at or
after its `ready` time if the L2 fill queue has room.  The run records no
event for that hand-over, so the oracle assumes that there always is room (the
cases keep -gpgpu_dram_partition_queues at 32 or more and read no faster than
the L2 takes fills) and asserts that its own ring stays far from full.  A case
that breaks the premise fills the model's ring, which holds reads back that
the oracle issues: the comparison fails, it cannot pass wrongly.  For the
same reason `ready` itself, (t + CL + burst) * per_dram (+ the MALL's miss
latency), is the oracle's word only: nothing here compares it with the run.

The run ends with its kernel.  Writes that the DRAM queues still hold then
(nobody waits for a store) stay queued, so the oracle stops at the first DRAM
cycle that begins at or after the kernel's end; the per-channel totals and the
bus use printed at the end are compared with what it issued until then.

The traffic makes the scheduler choose: several warps on two SMs issue
independent loads and stores (no register chain, no MEMBAR) over a pool of
lines that the decoder places on one or two channels, a few banks in two bank
groups and a few rows per bank, below a tiny L2 and with the L1 skipped.

Every case first asserts, on the oracle's own counters, that it reaches the
edge it is there for (see `Counters`), and only then compares.
"""
import collections
import random
import re
import time

import numpy as np
import pytest

from accel_sim_framework_distributed_amd.models import presets
from accel_sim_framework_distributed_amd.tracegen import rodinia
from accel_sim_framework_distributed_amd.tracegen.builder import KernelBuilder

from test_memory_oracle import POOL_BASE, Acc, Decoder, l2_geom, stat

K_DRAM_RET = 256        # config.h kDramRet: entries of the data return ring
K_DRAM_Q = 128          # config.h kDramQ: slots of the scheduler queue
K_MAX_BANKS = 32        # config.h kMaxBanksDram
K_MAX_BANK_GROUPS = 8   # config.h kMaxBankGroupsDram

TIMING_KEYS = ("nbk", "CCD", "RRD", "RCD", "RAS", "RP", "RC", "CL", "WL", "CDLR", "WR", "nbkgrp", "CCDL", "RTPL")
# sim_options.cc: the defaults of the options a preset may leave out
DEFAULTS = {
    "-gpgpu_dram_timing_opt": "4:2:8:12:21:13:34:9:4:5:13:1:0:0",
    "-gpgpu_dram_burst_length": "4",
    "-dram_data_command_freq_ratio": "2",
    "-dram_dual_bus_interface": "0",
    "-gpgpu_dram_scheduler": "1",
    "-dram_seperate_write_queue_enable": "0",
    "-dram_write_queue_size": "32:28:16",
    "-dram_elimnate_rw_turnaround": "0",
    "-gpgpu_simple_dram_model": "0",
    "-dram_bnkgrp_indexing_policy": "0",
    "-gpgpu_frfcfs_dram_sched_queue_size": "0",
    "-gpgpu_dram_return_queue_size": "0",
    "-sim_mall": "none",
    "-sim_mall_miss_latency": "0",
}


def period_fs(mhz):
    """femtoseconds per cycle, rounded half up (llround of a positive value)"""
    return int(1e9 / float(mhz) + 0.5)


class Counters:
    """What a case must reach, counted by the oracle alone.

    bound[rule]: cycles in which `rule` alone held back the request that would
    otherwise have issued: some queued request failed that gate and no other,
    and was older than the request that did issue (or nothing issued).  The
    column gates are RCD, CCD, CCDL, CDLR (write to read) and CL (read to
    write); the precharge gates RAS, WR (WL + burst + tWR), RTPL, HIT (the
    row still has a queued hit) and LAST_HIT (this cycle's column command
    took the row's last queued hit: the bank was one "with a queued row hit at
    the start of the cycle"); the activate gates RC, RP and RRD; SIMPLE is the
    simple model's burst gate."""

    def __init__(self):
        self.bound = collections.Counter()
        self.hit_first = 0      # column commands issued ahead of an older request that was no row hit
        self.both = 0           # cycles with a column and a row command
        self.busy = 0           # cycles with a queued request
        self.busy2 = 0          # ... with two or more
        self.drain_starts = 0   # write-drain mode entered / left
        self.drain_ends = 0
        self.tail_writes = 0    # column writes issued outside drain mode because no read was queued
        self.max_reads = 0      # most reads / writes / requests queued at once
        self.max_writes = 0
        self.max_queued = 0
        self.max_ring = 0       # most reads on their way back at once
        self.n = collections.Counter()  # commands by name

    def add(self, o):
        for k in ("bound", "n"):
            getattr(self, k).update(getattr(o, k))
        for k in ("hit_first", "both", "busy", "busy2", "drain_starts", "drain_ends", "tail_writes"):
            setattr(self, k, getattr(self, k) + getattr(o, k))
        self.max_reads = max(self.max_reads, o.max_reads)
        self.max_writes = max(self.max_writes, o.max_writes)
        self.max_queued = max(self.max_queued, o.max_queued)
        self.max_ring = max(self.max_ring, o.max_ring)


class Bank:
    __slots__ = ("open", "row", "col_ok", "pre_ras", "pre_wr", "pre_rtp", "act_rc", "act_rp")

    def __init__(self):
        self.open = False
        self.row = 0
        self.col_ok = self.pre_ras = self.pre_wr = self.pre_rtp = self.act_rc = self.act_rp = 0


class DramOracle:
    """One channel's DRAM scheduler, from the option strings."""

    def __init__(self, opts):
        def get(k):
            return str(opts.get(k, DEFAULTS[k])).strip().strip('"')
        timing = get("-gpgpu_dram_timing_opt")
        t = dict(zip(TIMING_KEYS, map(int, DEFAULTS["-gpgpu_dram_timing_opt"].split(":"))))
        if "=" in timing:
            for kv in filter(None, timing.split(":")):
                k, v = kv.split("=")
                assert k in t, k
                t[k] = int(v)
        else:
            for k, v in zip(TIMING_KEYS, timing.split(":")):
                t[k] = int(v)
        self.t = t
        self.nbk = t["nbk"]
        self.nbkgrp = t["nbkgrp"] or 1
        assert self.nbk <= K_MAX_BANKS and self.nbkgrp <= K_MAX_BANK_GROUPS
        self.grp_policy = int(get("-dram_bnkgrp_indexing_policy"))
        self.burst = max(1, int(get("-gpgpu_dram_burst_length")) // max(1, int(get("-dram_data_command_freq_ratio"))))
        self.dual = int(get("-dram_dual_bus_interface")) != 0
        self.frfcfs = int(get("-gpgpu_dram_scheduler")) != 0
        self.turnaround = int(get("-dram_elimnate_rw_turnaround")) == 0
        self.simple = int(get("-gpgpu_simple_dram_model")) != 0
        # queue sizes: 0 = the whole pool; with a write queue, reads and writes share the pool
        q = int(get("-gpgpu_frfcfs_dram_sched_queue_size"))
        self.qcap = K_DRAM_Q if q <= 0 or q > K_DRAM_Q else q
        self.wq = int(get("-dram_seperate_write_queue_enable")) != 0
        size, hi, lo = map(int, get("-dram_write_queue_size").split(":"))
        if self.wq:
            size = max(1, min(size, K_DRAM_Q // 2))
            self.qcap = min(self.qcap, K_DRAM_Q - size)
            hi = min(hi, size)
            lo = min(lo, hi)
        self.wq_size, self.wq_hi, self.wq_lo = size, hi, lo
        clocks = str(opts["-gpgpu_clock_domains"]).strip().strip('"').split(":")
        self.per_core, self.per_dram = period_fs(clocks[0]), period_fs(clocks[3])
        mall = get("-sim_mall") not in ("none", "0", "")
        self.extra_fs = int(get("-sim_mall_miss_latency")) * self.per_core if mall else 0

    def group(self, bank):
        if self.grp_policy == 1:
            return bank % self.nbkgrp                     # low bits
        return (bank // max(1, self.nbk // self.nbkgrp)) % self.nbkgrp

    def due(self, t_data):
        """first DRAM cycle at or after the data's ready time (DRAM cycle t runs at t * per_dram)"""
        return -(-(t_data * self.per_dram + self.extra_fs) // self.per_dram)

    def run(self, enq, t_end=None):
        """enq: [(DRAM cycle, write, bank, row)] in queue order; t_end: the
        first DRAM cycle the run did not simulate any more.  Gives
        ([(cycle, command, bank, row)], [(cycle, bank, row)] hand-overs of
        read data under the premise, Counters)."""
        T = self.t
        burst = self.burst
        cnt = Counters()
        cmds, handed = [], []
        banks = [Bank() for _ in range(max(1, self.nbk))]
        queue = []   # [age, write, bank, row]
        ring = collections.deque()  # (due cycle, bank, row) of reads on their way back
        seq = 0
        rrd_ok = ccd_ok = rd_ok = wr_ok = 0
        ccdl_ok = [0] * K_MAX_BANK_GROUPS
        wmode = False
        i = 0
        t = 0
        while i < len(enq) or queue or ring:
            if t_end is not None and t >= t_end:
                break
            if not queue:
                # nothing to schedule: on to the next arrival or hand-over
                nxt = [enq[i][0]] if i < len(enq) else []
                if ring:
                    nxt.append(ring[0][0])
                t = max(t, min(nxt))
            while i < len(enq) and enq[i][0] <= t:
                assert enq[i][0] == t, ("a request entered the queue in a cycle that is past", enq[i], t)
                queue.append([seq, enq[i][1], enq[i][2], enq[i][3]])
                seq += 1
                i += 1
            cnt.max_ring = max(cnt.max_ring, len(ring))
            while ring and ring[0][0] <= t:
                handed.append(ring.popleft())
            if not queue:
                t += 1
                continue
            nw = sum(1 for r in queue if r[1])
            cnt.busy += 1
            cnt.busy2 += len(queue) >= 2
            cnt.max_reads = max(cnt.max_reads, len(queue) - nw)
            cnt.max_writes = max(cnt.max_writes, nw)
            cnt.max_queued = max(cnt.max_queued, len(queue))
            if self.simple:
                # the oldest request, one column access per burst, no bank state
                r = min(queue)
                if t < ccd_ok:
                    cnt.bound["SIMPLE"] += 1
                elif r[1] or len(ring) < K_DRAM_RET:
                    if not r[1]:
                        ring.append((self.due(t + burst), r[2], r[3]))
                    cnt.n["WR" if r[1] else "RD"] += 1
                    cmds.append((t, "WR" if r[1] else "RD", r[2], r[3]))
                    ccd_ok = t + burst
                    queue.remove(r)
                t += 1
                continue
            # separate write queue: reads until the writes reach the high
            # watermark, then writes down to the low one; writes also when no
            # read is queued at all
            only = None
            if self.wq:
                if not wmode and nw >= self.wq_hi:
                    wmode = True
                    cnt.drain_starts += 1
                elif wmode and nw < self.wq_lo:
                    wmode = False
                    cnt.drain_ends += 1
                only = 1 if wmode or len(queue) == nw else 0
            served = [r for r in queue if only is None or r[1] == only]
            if not self.frfcfs:
                served = [min(served)] if served else []   # FIFO: the oldest alone, for both commands
            # ---- column command ----
            best = {}   # failed gates -> oldest request that fails exactly those

            def note(r, fails):
                k = frozenset(fails)
                if (len(k) <= 1) and (k not in best or r[0] < best[k][0]):
                    best[k] = r

            for r in served:
                b = banks[r[2]]
                if not (b.open and b.row == r[3]):
                    continue
                fails = []
                if t < b.col_ok:
                    fails.append("RCD")
                if t < ccd_ok:
                    fails.append("CCD")
                if t < ccdl_ok[self.group(r[2]) & 7]:
                    fails.append("CCDL")
                if r[1] and t < wr_ok:
                    fails.append("CL")
                if not r[1] and t < rd_ok:
                    fails.append("CDLR")
                note(r, fails)
            pick = best.pop(frozenset(), None)
            if pick is not None and not pick[1] and len(ring) >= K_DRAM_RET:
                pick = None   # (the ring is full: no column command at all this cycle)
                best = {}
            for k, r in best.items():
                if pick is None or r[0] < pick[0]:
                    cnt.bound[next(iter(k))] += 1
            col_bank = None
            if pick is not None:
                age, write, bank, row = pick
                b = banks[bank]
                if any(r[0] < age and not (banks[r[2]].open and banks[r[2]].row == r[3]) for r in served):
                    cnt.hit_first += 1
                if write:
                    b.pre_wr = max(b.pre_wr, t + T["WL"] + burst + T["WR"])
                    if self.turnaround:
                        rd_ok = max(rd_ok, t + T["WL"] + burst + T["CDLR"])
                    if self.wq and not wmode:
                        cnt.tail_writes += 1
                else:
                    ring.append((self.due(t + T["CL"] + burst), bank, row))
                    b.pre_rtp = max(b.pre_rtp, t + T["RTPL"])
                    if self.turnaround:
                        wr_ok = max(wr_ok, max(0, t + T["CL"] + burst + 2 - T["WL"]))
                ccd_ok = t + max(T["CCD"], burst)
                ccdl_ok[self.group(bank) & 7] = t + max(T["CCDL"], burst)
                cmds.append((t, "WR" if write else "RD", bank, row))
                cnt.n["WR" if write else "RD"] += 1
                queue.remove(pick)
                col_bank = bank
                if not self.dual:
                    t += 1
                    continue   # one command bus: no row command in this cycle
                if not self.frfcfs:
                    served = []   # FIFO: the oldest request has just left
                else:
                    served = [r for r in served if r is not pick]
            # ---- row command ----
            # banks with a queued row hit at the start of the cycle keep their
            # row (FR-FCFS only); the column command's bank had one
            hit = set()
            if self.frfcfs:
                hit = {r[2] for r in served if banks[r[2]].open and banks[r[2]].row == r[3]}
            held = col_bank if self.frfcfs and col_bank not in hit else None
            best = {}
            for r in served:
                b = banks[r[2]]
                fails = []
                if b.open:
                    if b.row == r[3]:
                        continue
                    if t < b.pre_ras:
                        fails.append("RAS")
                    if t < b.pre_wr:
                        fails.append("WR")
                    if t < b.pre_rtp:
                        fails.append("RTPL")
                    if r[2] in hit:
                        fails.append("HIT")
                    if r[2] == held:
                        fails.append("LAST_HIT")
                else:
                    if t < b.act_rc:
                        fails.append("RC")
                    if t < b.act_rp:
                        fails.append("RP")
                    if t < rrd_ok:
                        fails.append("RRD")
                note(r, fails)
            pick = best.pop(frozenset(), None)
            for k, r in best.items():
                if pick is None or r[0] < pick[0]:
                    cnt.bound[next(iter(k))] += 1
            if pick is not None:
                b = banks[pick[2]]
                if b.open:
                    cmds.append((t, "PRE", pick[2], b.row))
                    cnt.n["PRE"] += 1
                    b.open = False
                    b.act_rp = t + T["RP"]
                else:
                    cmds.append((t, "ACT", pick[2], pick[3]))
                    cnt.n["ACT"] += 1
                    b.open, b.row = True, pick[3]
                    b.col_ok = t + T["RCD"]
                    b.pre_ras, b.pre_wr, b.pre_rtp = t + T["RAS"], 0, 0
                    b.act_rc = t + T["RC"]
                    rrd_ok = t + T["RRD"]
                cnt.both += col_bank is not None
            t += 1
        return cmds, handed, cnt


# ---------------------------------------------------------------------------
# the oracle on hand-made queues: rules that can be stated in a line
# ---------------------------------------------------------------------------
HAND = {"-gpgpu_clock_domains": "1000:1000:1000:1000", "-gpgpu_dram_burst_length": "4",
        "-dram_data_command_freq_ratio": "2", "-dram_dual_bus_interface": "1",
        "-gpgpu_dram_timing_opt": "nbk=4:CCD=2:RRD=3:RCD=5:RAS=11:RP=4:RC=16:CL=6:WL=2:CDLR=3:WR=4:nbkgrp=2:CCDL=3:RTPL=2"}


def test_oracle_by_hand():
    """three requests, worked out on paper from the rules in mem.h"""
    # two reads of row 7 and, between them in age, one of row 9, all bank 0
    enq = [(10, 0, 0, 7), (10, 0, 0, 9), (10, 0, 0, 7)]
    cmds, handed, cnt = DramOracle(HAND).run(enq)
    assert cmds == [
        (10, "ACT", 0, 7),             # closed bank: the oldest request's row
        (15, "RD", 0, 7),              # tRCD = 5
        (18, "RD", 0, 7),              # row hit first; same group: max(CCDL = 3, burst) after the first
        (21, "PRE", 0, 7),             # no hit left; tRAS = 11 after the ACT (tRTPL = 2 is long past)
        (26, "ACT", 0, 9),             # max(tRP = 4 after the PRE, tRC = 16 after the ACT)
        (31, "RD", 0, 9),
    ]
    # data: CL + burst = 8 cycles after the command
    assert handed == [(23, 0, 7), (26, 0, 7), (39, 0, 9)]
    # tRCD alone holds the oldest read in cycles 11-14 and 27-30; tCCDL alone in 17 (16 is tCCD's too);
    # tRAS alone in 20 (15-18 are the hit's too, 19 tRTPL's); tRC alone in 25 (22-24 are tRP's too)
    assert cnt.hit_first == 1 and cnt.bound == {"RCD": 8, "CCDL": 1, "RAS": 1, "RC": 1}
    # FIFO serves the same queue strictly in order: the row is opened three times
    cmds, _, _ = DramOracle(dict(HAND, **{"-gpgpu_dram_scheduler": "0"})).run(enq)
    assert [c[1] for c in cmds] == ["ACT", "RD", "PRE", "ACT", "RD", "PRE", "ACT", "RD"]
    # one command bus: the ACT for bank 1 waits for a cycle without a column command
    two = [(10, 0, 0, 7), (10, 0, 0, 7), (15, 0, 1, 3)]
    dual, _, _ = DramOracle(HAND).run(two)
    single, _, _ = DramOracle(dict(HAND, **{"-dram_dual_bus_interface": "0"})).run(two)
    assert (15, "RD", 0, 7) in dual and (15, "ACT", 1, 3) in dual
    assert (15, "RD", 0, 7) in single and (16, "ACT", 1, 3) in single
    # a write, then a read of the same row: WL + burst + tCDLR = 7 later, or at once when told so
    wr = [(10, 1, 0, 7), (10, 0, 0, 7)]
    assert DramOracle(HAND).run(wr)[0][1:] == [(15, "WR", 0, 7), (22, "RD", 0, 7)]
    assert DramOracle(dict(HAND, **{"-dram_elimnate_rw_turnaround": "1"})).run(wr)[0][2] == (18, "RD", 0, 7)
    # a read, then a write: CL + burst + 2 - WL = 8 later
    assert DramOracle(HAND).run([(10, 0, 0, 7), (10, 1, 0, 7)])[0][1:] == [(15, "RD", 0, 7), (23, "WR", 0, 7)]
    # the simple model: the oldest, one per burst, data after `burst`
    cmds, handed, _ = DramOracle(dict(HAND, **{"-gpgpu_simple_dram_model": "1"})).run(enq)
    assert [c[0] for c in cmds] == [10, 12, 14] and [h[0] for h in handed] == [12, 14, 16]


def test_positional_timing_string_reads_like_the_named_one():
    named = DramOracle(HAND)
    pos = DramOracle(dict(HAND, **{"-gpgpu_dram_timing_opt": "4:2:3:5:11:4:16:6:2:3:4:2:3:2"}))
    assert named.t == pos.t and pos.nbkgrp == 2


def test_bank_group_policies():
    o = DramOracle(dict(HAND, **{"-gpgpu_dram_timing_opt": HAND["-gpgpu_dram_timing_opt"].replace("nbk=4", "nbk=16")
                                 .replace("nbkgrp=2", "nbkgrp=4")}))
    assert [o.group(b) for b in (0, 1, 4, 5, 15)] == [0, 0, 1, 1, 3]   # policy 0: the high bits
    o.grp_policy = 1
    assert [o.group(b) for b in (0, 1, 4, 5, 15)] == [0, 1, 0, 1, 3]   # policy 1: the low bits


def test_more_bank_groups_than_gates_are_refused(native):
    """ChanState::t_ccdl_ok has eight gates: nine bank groups would share them"""
    args = presets.args_for("QV100")
    t = presets.get_preset("QV100")["-gpgpu_dram_timing_opt"].strip('"')
    native.parse_config(args + ["-gpgpu_dram_timing_opt", t.replace("nbkgrp=4", "nbkgrp=8")])
    with pytest.raises(Exception, match="too many DRAM bank groups"):
        native.parse_config(args + ["-gpgpu_dram_timing_opt", t.replace("nbkgrp=4", "nbkgrp=9")])


# ---------------------------------------------------------------------------
# traffic
# ---------------------------------------------------------------------------
TRACE = {"-trace_enabled": "1", "-trace_sampling_core": "-1", "-gpgpu_perf_sim_memcpy": "0",
         "-trace_components": "MEMORY_PARTITION_UNIT"}
BANKS = (0, 1, 8, 9)   # of 16: two banks in each of two bank groups, whether the low or the high bits index the group


_pools = {}


def dram_pool(opts, nbk, n_ch, banks, n_rows, per_row, span):
    """lines that decode to the first n_ch channels met, to `banks` and, in
    each bank, to the first n_rows rows met; at most per_row lines of a row,
    all within 2^span lines (one search per address mapping and shape: the
    cases share the pools)"""
    key = (opts["-gpgpu_mem_addr_mapping"], opts["-gpgpu_n_mem"], opts["-gpgpu_n_sub_partition_per_mchannel"],
           opts["-gpgpu_memory_partition_indexing"], opts.get("-sim_xcd"), nbk, n_ch, banks, n_rows, per_row, span)
    if key not in _pools:
        _pools[key] = search_pool(Decoder(opts), nbk, n_ch, banks, n_rows, per_row, span)
    return _pools[key]


def search_pool(dec, nbk, n_ch, banks, n_rows, per_row, span):
    rnd = random.Random(7)
    chips, rows, pool = [], {}, {}
    want = n_ch * len(banks) * n_rows * per_row
    for _ in range(400000):
        line = POOL_BASE + (rnd.randrange(1 << span) << 7)
        d = dec.decode(line)
        bank = d["bk"] % max(1, nbk)
        if bank not in banks:
            continue
        if d["chip"] not in chips:
            if len(chips) >= n_ch:
                continue
            chips.append(d["chip"])
        seen = rows.setdefault((d["chip"], bank), [])
        if d["row"] not in seen:
            if len(seen) >= n_rows:
                continue
            seen.append(d["row"])
        lines = pool.setdefault((d["chip"], bank, d["row"]), [])
        if len(lines) < per_row and line not in lines:
            lines.append(line)
            want -= 1
            if not want:
                break
    assert not want, "the pool search ran out"
    return [l for k in sorted(pool) for l in pool[k]]


def make_streams(seed, pool, n_warps, per_warp, stores, tail_stores=0):
    """per warp a list of Acc over `pool`: mostly whole lines (four sector
    requests of one row), some single sectors; the last tail_stores of every
    warp are stores"""
    rnd = random.Random(seed)
    out = []
    for _ in range(n_warps):
        s = []
        for j in range(per_warp):
            n = rnd.choice((4, 4, 2, 1))
            s0 = rnd.randrange(0, 5 - n)
            store = rnd.random() < stores or j >= per_warp - tail_stores
            s.append(Acc(store, rnd.choice(pool), s0, n))
        out.append(s)
    return out


def build_kernel(streams, ncta, warp_size, work_ctas):
    """warp w of the working CTAs runs streams[w]: loads into eight rotating
    registers from an address register nobody writes, stores without MEMBAR,
    so every warp keeps several accesses in flight"""
    wpc = len(streams) // len(work_ctas)
    k = KernelBuilder("_Z4dramPi", (ncta, 1, 1), (warp_size * wpc, 1, 1), nregs=16, warp_size=warp_size)
    owner = np.full(k.g.nwarps, -1)
    for i, c in enumerate(work_ctas):
        owner[(k.g.cta == c)] = i * wpc + k.g.warp[k.g.cta == c]
    for j in range(len(streams[0])):
        base = np.zeros(k.g.nwarps, np.int64)
        mask = np.zeros(k.g.nwarps, np.uint64)
        store = np.zeros(k.g.nwarps, bool)
        for w in range(k.g.nwarps):
            if owner[w] >= 0:
                a = streams[owner[w]][j]
                base[w], mask[w], store[w] = a.line + 32 * a.s0, (1 << (8 * a.n)) - 1, a.store
        k.op("LDG.E", [6 + j % 8], [4], base=base, stride=4, mask=mask, present=(owner >= 0) & ~store)
        k.op("STG.E", [], [4, 5], base=base, stride=4, mask=mask, present=(owner >= 0) & store)
    k.op("EXIT")
    return k.build()


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
def timing(preset, **over):
    t = dict(kv.split("=") for kv in presets.get_preset(preset)["-gpgpu_dram_timing_opt"].strip('"').split(":"))
    t.update({k: str(v) for k, v in over.items()})
    return ":".join(f"{k}={t[k]}" for k in TIMING_KEYS)


def positional(named):
    return ":".join(kv.split("=")[1] for kv in named.split(":"))


SMALL_L2 = l2_geom("S", 2, 2, "L", "L", "P")
NOALLOC_L2 = l2_geom("S", 2, 2, "L", "N", "P")
# the FR-FCFS conditions every case with row hits to choose from has to meet
FRFCFS = dict(hit_first=10, bound={"HIT": 5})


def case(preset, over=None, rules=(), traffic=None, **need):
    return dict(preset=preset, over=over or {}, rules=tuple(rules), traffic=traffic or {}, need=need)


WQ = {"-dram_seperate_write_queue_enable": "1", "-dram_write_queue_size": "8:6:2"}
CASES = {
    # the presets as they are
    "QV100_dual_bus": case("QV100", rules=("RCD", "CCDL", "RRD"), **FRFCFS),
    "RTX2060_single_bus_burst4": case("RTX2060", rules=("CCD", "RCD"), **FRFCFS),
    "RTX2060_write_noalloc": case("RTX2060", {"-gpgpu_cache:dl2": NOALLOC_L2}, rules=("CDLR", "CL"),
                                  traffic=dict(stores=0.5), **FRFCFS),
    "MI355X_mall_xcd": case("MI355X", {"-gpgpu_perfect_inst_const_cache": "1", "-sim_l2_kernel_release": "0",
                                       "-sim_mall": "4:2"}, rules=("RCD",),
                            traffic=dict(warp_size=64, ncta=9, work_ctas=(0, 8), stores=0.5, span=17), mall=True),
    # the scheduler's modes
    "QV100_fifo": case("QV100", {"-gpgpu_dram_scheduler": "0"}, rules=("RCD", "RP")),
    "QV100_write_queue": case("QV100", dict(WQ, **{"-gpgpu_cache:dl2": NOALLOC_L2}), rules=("RCD",),
                              traffic=dict(stores=0.5, tail_stores=12), drains=3, tail_writes=5, **FRFCFS),
    "RTX2060_write_queue_fifo": case("RTX2060", dict(WQ, **{"-gpgpu_cache:dl2": NOALLOC_L2,
                                                            "-gpgpu_dram_scheduler": "0"}), rules=("RCD",),
                                     traffic=dict(stores=0.5, tail_stores=12), drains=3, tail_writes=5),
    "RTX2060_no_turnaround": case("RTX2060", {"-dram_elimnate_rw_turnaround": "1", "-gpgpu_cache:dl2": NOALLOC_L2},
                                  rules=("CCD",), traffic=dict(stores=0.5), unbound=("CDLR", "CL"), **FRFCFS),
    "QV100_simple_model": case("QV100", {"-gpgpu_simple_dram_model": "1", "-gpgpu_dram_burst_length": "8"},
                               rules=("SIMPLE",)),
    "RTX2060_simple_model_fifo": case("RTX2060", {"-gpgpu_simple_dram_model": "1", "-gpgpu_dram_scheduler": "0"},
                                      rules=("SIMPLE",)),
    # stretched timings: each term is the binding one somewhere
    "QV100_rrd": case("QV100", {"-gpgpu_dram_timing_opt": timing("QV100", RRD=23)}, rules=("RRD",), **FRFCFS),
    "QV100_ccdl_2groups_low_bits": case("QV100", {"-gpgpu_dram_timing_opt": timing("QV100", nbkgrp=2, CCDL=7),
                                                  "-dram_bnkgrp_indexing_policy": "1"}, rules=("CCDL",), **FRFCFS),
    "QV100_ccdl_2groups_high_bits": case("QV100", {"-gpgpu_dram_timing_opt": timing("QV100", nbkgrp=2, CCDL=7),
                                                   "-dram_bnkgrp_indexing_policy": "0"}, rules=("CCDL",), **FRFCFS),
    "QV100_rcd": case("QV100", {"-gpgpu_dram_timing_opt": timing("QV100", RCD=27)}, rules=("RCD",), **FRFCFS),
    "QV100_rp_rc": case("QV100", {"-gpgpu_dram_timing_opt": timing("QV100", RP=31, RC=75)}, rules=("RP", "RC"),
                        **FRFCFS),
    "QV100_ras": case("QV100", {"-gpgpu_dram_timing_opt": timing("QV100", RAS=61, RC=73)}, rules=("RAS",),
                      **FRFCFS),
    # a read's own tRTPL keeps its bank from a precharge in the same cycle; without it only the rule
    # that the column command's bank counts as hit does
    "QV100_rtpl0_last_hit": case("QV100", {"-gpgpu_dram_timing_opt": timing("QV100", RTPL=0, RAS=5)},
                                 rules=("LAST_HIT",), traffic=dict(stores=0.0), **FRFCFS),
    "QV100_rtpl": case("QV100", {"-gpgpu_dram_timing_opt": timing("QV100", RTPL=37, RAS=5)}, rules=("RTPL",),
                       **FRFCFS),
    "QV100_wr_wl": case("QV100", {"-gpgpu_dram_timing_opt": timing("QV100", WR=29, WL=9, RAS=5),
                                  "-gpgpu_cache:dl2": NOALLOC_L2}, rules=("WR",), traffic=dict(stores=0.5),
                        **FRFCFS),
    "QV100_cdlr": case("QV100", {"-gpgpu_dram_timing_opt": timing("QV100", CDLR=19),
                                 "-gpgpu_cache:dl2": NOALLOC_L2}, rules=("CDLR",), traffic=dict(stores=0.5),
                       **FRFCFS),
    "QV100_cl_read_to_write": case("QV100", {"-gpgpu_dram_timing_opt": timing("QV100", CL=33),
                                             "-gpgpu_cache:dl2": NOALLOC_L2}, rules=("CL",),
                                   traffic=dict(stores=0.5), **FRFCFS),
    "QV100_positional_timing": case("QV100", {"-gpgpu_dram_timing_opt": positional(timing("QV100", CCD=3))},
                                    rules=("CCD", "RCD"), **FRFCFS),
    # bank counts: the build's limit and a single bank
    "QV100_nbk32": case("QV100", {"-gpgpu_dram_timing_opt": timing("QV100", nbk=32, nbkgrp=8)},
                        rules=("RCD", "CCDL"), **FRFCFS),
    "QV100_nbk1": case("QV100", {"-gpgpu_dram_timing_opt": timing("QV100", nbk=1, nbkgrp=1)},
                       rules=("RCD", "RP"), traffic=dict(banks=(0,), n_rows=3, per_row=6), **FRFCFS),
}
SKIP_CASE = "QV100_dual_bus"   # run again with -sim_event_skip 0


def case_options(name):
    c = CASES[name]
    o = presets.get_preset(c["preset"])
    # every access goes below the L1, and the L2 is too small to hold the pool
    o.update({"-gpgpu_gmem_skip_L1D": "1", "-gpgpu_cache:dl2": SMALL_L2})
    o.update(c["over"])
    return o


_traffic = {}


def case_traffic(name):
    """options and kernel of a case (made once per process)"""
    if name not in _traffic:
        c = CASES[name]
        tr = dict(dict(warp_size=32, ncta=2, work_ctas=(0, 1), wpc=3, per_warp=72, stores=0.3, tail_stores=0,
                       n_ch=1, banks=BANKS, n_rows=2, per_row=4, span=15), **c["traffic"])
        opts = case_options(name)
        orc = DramOracle(opts)
        seed = sum(map(ord, name))
        pool = dram_pool(opts, orc.nbk, tr["n_ch"], tr["banks"], tr["n_rows"], tr["per_row"], tr["span"])
        streams = make_streams(seed + 1, pool, tr["wpc"] * len(tr["work_ctas"]), tr["per_warp"], tr["stores"],
                               tr["tail_stores"])
        kernel = build_kernel(streams, tr["ncta"], tr["warp_size"], tr["work_ctas"])
        _traffic[name] = (opts, kernel, sum(map(len, streams)))
    return _traffic[name]


def run_case(mod, engine, name, tmp_path, extra=None):
    from accel_sim_framework_distributed_amd.sim import build_args
    opts, kernel, n_acc = case_traffic(name)
    kl = rodinia.write_app(str(tmp_path / name), [kernel], memcpy=False)
    s = mod.Simulator(build_args(opts, kl, engine, dict(TRACE, **(extra or {}))), False)
    t0 = time.perf_counter()
    assert s.run() == 0, s.output[-2000:]
    wall = time.perf_counter() - t0
    assert s.engine == engine and not s.deadlock
    assert "trace events dropped" not in s.output
    return s.output, wall, n_acc


def parse_events(out):
    """per channel: queue entries and commands, each in trace order"""
    enq, cmd = {}, {}
    for k, w, b, r, t in re.findall(r"channel (\d+) queues (read|write) bank (\d+) row (\d+) dram_cycle (\d+)", out):
        enq.setdefault(int(k), []).append((int(t), int(w == "write"), int(b), int(r)))
    for k, c, b, r, t in re.findall(r"channel (\d+) DRAM (\w+) bank (\d+) row (\d+) dram_cycle (\d+)", out):
        cmd.setdefault(int(k), []).append((int(t), c, int(b), int(r)))
    return enq, cmd


def first_difference(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return f"entry {i}: the run has {g}, the oracle {w}"
    if len(got) != len(want):
        return f"the run has {len(got)} entries, the oracle {len(want)}"
    return None


def check_order_within_cycle(out):
    """events of one DRAM cycle stand in the order things happen: queue
    entries, then the column command, then the row command"""
    last = {}
    rank = {"queues": 0, "RD": 1, "WR": 1, "ACT": 2, "PRE": 2}
    for k, what, c, t in re.findall(r"channel (\d+) (queues|DRAM) (\w+) bank \d+ row \d+ dram_cycle (\d+)", out):
        key = (int(t), rank["queues" if what == "queues" else c])
        assert last.get(k, (0, 0)) <= key, (k, last[k], key)
        last[k] = key


def check_case(mod, engine, name, tmp_path):
    c = CASES[name]
    need = c["need"]
    out, wall, n_acc = run_case(mod, engine, name, tmp_path)
    opts = case_options(name)
    orc = DramOracle(opts)
    enq, cmd = parse_events(out)
    assert enq, "no request reached a DRAM scheduler"
    check_order_within_cycle(out)
    # ---- the oracle alone: does the case reach its edge? ----
    # the run ends with the kernel; what the DRAM queues still hold then (writes: nobody waits for
    # them) stays there, so the oracle stops at the first DRAM cycle that starts at or after the end
    t_end = -(-stat(out, "gpu_tot_sim_cycle") * orc.per_core // orc.per_dram)
    want, total = {}, Counters()
    for ch in sorted(enq):
        want[ch] = orc.run(enq[ch], t_end)
        total.add(want[ch][2])
    n_cmd = sum(total.n.values())
    print(f"{name} [{engine}]: {wall:.2f} s, {n_acc} accesses, {sum(map(len, enq.values()))} requests on "
          f"{len(enq)} channels, {n_cmd} commands, bound {dict(total.bound)}, hit-first {total.hit_first}, "
          f"both {total.both}, busy {total.busy} (two or more: {total.busy2}), drains {total.drain_starts}/"
          f"{total.drain_ends}, tail writes {total.tail_writes}, most queued {total.max_reads}r "
          f"{total.max_writes}w {total.max_queued}")
    for rule in c["rules"]:
        assert total.bound[rule] >= 5, f"vacuous: {rule} bound in {total.bound[rule]} cycles only"
    for rule, n in need.get("bound", {}).items():
        assert total.bound[rule] >= n, f"vacuous: {rule} bound in {total.bound[rule]} cycles only"
    for rule in need.get("unbound", ()):
        assert total.bound[rule] == 0, rule
    assert total.hit_first >= need.get("hit_first", 0), f"vacuous: {total.hit_first} row hits served first"
    assert 2 * total.busy2 >= total.busy, "vacuous: mostly a single request queued"
    if orc.dual and orc.frfcfs and not orc.simple and orc.nbk > 1:
        assert total.both >= 10, f"vacuous: {total.both} cycles with two commands"
    else:
        # one command bus; FIFO, whose oldest request has just left with the column command; a single
        # bank, whose row the column command holds open; the simple model, which has no row commands
        assert total.both == 0, "two commands in a cycle"
    if "drains" in need:
        assert min(total.drain_starts, total.drain_ends) >= need["drains"], (total.drain_starts, total.drain_ends)
        assert total.tail_writes >= need["tail_writes"], total.tail_writes
        assert all(w for ch in enq for _, w, _, _ in enq[ch][-8:]), "the kernel's tail is not writes alone"
    assert total.max_ring <= K_DRAM_RET // 4, "the premise: the return ring is far from full"
    if need.get("mall"):
        assert stat(out, "MALL_read_hits") >= 10 and stat(out, "MALL_writebacks") >= 10, "vacuous: the MALL idles"
    # ---- the run against the oracle ----
    for ch in sorted(set(enq) | set(cmd)):
        bad = first_difference(cmd.get(ch, []), want[ch][0] if ch in want else [])
        assert bad is None, f"channel {ch} commands, {bad}"
    # dram_room: never more queued than the queues hold (after the comparison: an oracle that serves
    # more slowly than the run also overfills its queue)
    if orc.wq:
        assert total.max_reads <= orc.qcap and total.max_writes <= orc.wq_size
    else:
        assert total.max_queued <= orc.qcap
    totals = re.findall(r"DRAM\[(\d+)\]: n_act=(\d+) n_pre=(\d+) n_rd=(\d+) n_write=(\d+) bw_util=([0-9.]+)", out)
    assert {int(t[0]) for t in totals} >= set(enq)
    for ch, act, pre, rd, wr, util in totals:
        n = want[int(ch)][2].n if int(ch) in want else {}
        assert (int(act), int(pre), int(rd), int(wr)) == tuple(n.get(k, 0) for k in ("ACT", "PRE", "RD", "WR")), ch
        # the bus-busy count, printed as a share of the t_end DRAM cycles to four places
        assert abs(float(util) - (n.get("RD", 0) + n.get("WR", 0)) * orc.burst / t_end) <= 0.51e-4, (ch, util)
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_dram_timing_matches_oracle_cpu(native, tmp_path, name):
    check_case(native, "cpu", name, tmp_path)


def trace_lines(out):
    return [l for l in out.splitlines() if l.startswith("GPGPU-Sim Cycle ")]


def test_event_skip_off_gives_the_same_events_cpu(native, tmp_path):
    a = run_case(native, "cpu", SKIP_CASE, tmp_path)[0]
    b = run_case(native, "cpu", SKIP_CASE, tmp_path, {"-sim_event_skip": "0"})[0]
    assert len(trace_lines(a)) > 1000 and trace_lines(a) == trace_lines(b)


def test_new_lines_leave_the_old_readers_alone(native, tmp_path):
    """the untimed oracle's reader still sees every command, and only those"""
    from test_memory_oracle import dram_events
    out = run_case(native, "cpu", SKIP_CASE, tmp_path)[0]
    enq, cmd = parse_events(out)
    old = dram_events(out)
    assert {k: [c[1:] for c in v] for k, v in cmd.items()} == old
    assert all(c in ("RD", "WR", "ACT", "PRE") for v in old.values() for c, _, _ in v)
    assert sum(map(len, enq.values())) > 100


# ---------------------------------------------------------------------------
# the same cases on the GPU engine (default build)
# ---------------------------------------------------------------------------
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
@pytest.mark.parametrize("name", sorted(CASES))
def test_dram_timing_matches_oracle_gpu(gpu_mod, tmp_path, name):
    check_case(gpu_mod, "gpu", name, tmp_path)


@pytest.mark.gpu
def test_event_skip_off_gives_the_same_events_gpu(gpu_mod, tmp_path):
    a = run_case(gpu_mod, "gpu", SKIP_CASE, tmp_path)[0]
    b = run_case(gpu_mod, "gpu", SKIP_CASE, tmp_path, {"-sim_event_skip": "0"})[0]
    assert len(trace_lines(a)) > 1000 and trace_lines(a) == trace_lines(b)

"""The crossbar and the link-reservation timing against a plain-Python oracle.

tests/test_core_oracle.py pins the SM pipeline, tests/test_memory_oracle.py the
caches and the address decoder (untimed) and tests/test_dram_oracle.py the DRAM
commands.  This file pins WHEN a packet travels between them.  `Oracle` is the
interconnect path of csrc/model/sm.h (sm_send's packet sizes, sm_inject,
xbar_pick, xbar_take, steps 1 and 2 of sm_receive), mem.h (gather_sorted,
mem_gather, mem_icnt_cycle, the ROP queue and its head in l2_cycle, reply_push,
the order of the clock domains in mem_window), config.h (icnt_pkt_lat_fs,
icnt_routers, core_fs) and icnt_links.h (icnt_route, icnt_reserve,
icnt_contend) in plain integer Python, in femtoseconds where the model uses
femtoseconds, written from the comments and rules of those files.  It derives
icnt_in_pkts, icnt_out_limit, flit_size, q_icnt_l2, rop_latency, eject_buf and
ldst_resp_buf from the option strings as sim_options.cc does, reads the .icnt
file itself and never calls native.parse_config.

What the run gives: every "core S injects packet to sub-partition D addr A"
line of the INTERCONNECT stream with its core cycle.  The test built the
kernel, so it knows each packet's type, sectors and size from its address (a
line belongs to one warp; per line the packets come in program order: the
store, or its two halves with -sim_l1_write_request_bytes 64, then the load).
What the oracle predicts from that: on the request subnet the L2 cycle of every
"L2 <outcome> line A" event (injection-port serialisation, arrival time and
the epoch it is gathered in, the (time, source) merge, the port grant per
interconnect cycle, the ROP intake limit, the ROP delay, one head per L2
cycle); on the reply subnet the core cycle of every "core S ejects packet type
T addr A" line (reply size, the channel's injection port, latency, the SM-side
gather, the SM port grant, the ejection-buffer gate).  The whole event list of
every memory channel and of every SM is compared, cycles included, and then
the subnets' statistics with the oracle's own counts.

Premises, asserted on every run: the run records no event for a reply created
at an L2 fill, so all traffic is answered at L2 access time.  Loads only read
sectors that full-sector stores of the same warp made valid earlier in a
write-back L2 (the oracle keeps the valid sectors per line and refuses a load
that would miss), stores are acknowledged at once, the L1 is skipped
(-gpgpu_gmem_skip_L1D 1), and the instruction cache is perfect
(-gpgpu_perfect_inst_const_cache 1): no instruction-fill packet exists, and a
packet whose address is not one of the kernel's lines fails the test.  No L2
access may be refused (Reservation_fails 0 on every bank), nothing may be lost
(no "lost to a full backlog ring", no "trace events dropped").  A case that
breaks a premise fails; nothing is skipped or trimmed.

Epochs (epoch.h): an epoch is -icnt_latency core cycles (with -network_mode 1
the smallest pair latency), aligned to multiples of it: the run starts at
cycle 0 and epoch_decide's fast-forwards add whole multiples.  Packets
injected in epoch e are gathered at the start of epoch e + 1.  A skipped epoch
is one in which nothing happens, so the oracle walks every epoch.

Documented difference S3 (sm.h header): a crossbar output port arbitrates only
in a cycle in which the HEAD of its input queue has arrived.  The queue is in
(gather epoch, arrival time, source) order, so a multi-flit packet injected in
the last cycles of an epoch (or, with -network_mode 1, one with a longer pair
latency) stands ahead of packets of the next epoch that arrive earlier: those
wait for the head.  The reference's crossbar keeps one buffer per input and
has no such wait.  The oracle was written from the stated rule first (the port
grants one of the inputs whose packet has arrived) and disagreed with the run
in seven of the fifteen cases, by up to seven cycles at the first difference;
it now follows the code (`head_gate`), and
test_head_gate_is_what_the_port_does keeps the stated rule failing.

What the trace cannot show is when sm_send queued a packet, so of sm_can_send
only the bound on packets in flight is checked by the oracle (never above
-sim_max_outstanding_pkts, and reached).  That -icnt_in_buffer_limit holds
packets back is taken from the run: serial_flit8 has one packet of injection
buffer and no bound in flight, and its gpgpu_n_stall_shd_mem must be positive.

With the L1 skipped the LD/ST unit consumes one response per core cycle, so
the cluster ejection buffer never holds a packet when step 2 looks at it: the
ejection-buffer gate cannot bind, even with both buffers at 1.  The reply
cases assert that the oracle's gate never closed instead of claiming the edge.

Every case first asserts, on the oracle's own counters (`Counters`), that it
reaches the edge it is there for, and only then compares.
"""
import collections
import random
import re

import numpy as np
import pytest

from accel_sim_framework_distributed_amd.models import presets
from accel_sim_framework_distributed_amd.tracegen import rodinia

from test_memory_oracle import POOL_BASE, TRACE_ON, Decoder, KernelBuilder, run_sim, stat

K_OUTQ = 64        # config.h kOutQ: SM injection queue
K_INQ = 128        # config.h kInQ: SM arrival queue
K_MEM_INQ = 256    # config.h kMemInQ: sub-partition arrival queue = gather sort scratch
K_ROPQ = 256       # config.h kRopQ
K_REPLYQ = 128     # config.h kReplyQ
K_EJECTQ = 32      # config.h kEjectQ
K_LDST_RESPQ = 8   # config.h kLdstRespQ
K_MAX_EPOCH = 256  # config.h kMaxEpoch
WINDOW = 64        # xbar_pick: arbitration looks at the 64 oldest arrivals
P_RD, P_WR, P_RD_REPLY, P_WR_ACK = 1, 2, 4, 5   # types.h PktType
L2_OUTCOME = ("hit", "miss")
assert {"INTERCONNECT", "MEMORY_SUBPARTITION_UNIT"} <= set(TRACE_ON["-trace_components"].split(","))
assert TRACE_ON["-trace_sampling_core"] == "-1"


def popc(x):
    return bin(x).count("1")


class PremiseError(AssertionError):
    pass


# ---------------------------------------------------------------------------
# configuration, from the option strings (sim_options.cc, icnt_config.cc)
# ---------------------------------------------------------------------------
class IcntCfg:
    def __init__(self, o, icnt_text=None):
        u = lambda k: int(str(o[k]).strip().strip('"'))
        self.cpc = max(1, u("-gpgpu_n_cores_per_cluster"))
        self.n_clusters = u("-gpgpu_n_clusters")
        self.n_sm = self.n_clusters * self.cpc
        self.n_mem = u("-gpgpu_n_mem")
        self.nsub = u("-gpgpu_n_sub_partition_per_mchannel")
        self.n_subpart = self.n_mem * self.nsub
        self.flit = max(8, u("-icnt_flit_size"))
        self.arbiter = 1 if u("-icnt_arbiter_algo") else 0
        self.grant = max(1, u("-icnt_grant_cycles"))
        # the injection buffer holds -icnt_in_buffer_limit flits; a packet is at most 136 bytes
        self.in_pkts = max(1, min(K_OUTQ, u("-icnt_in_buffer_limit") // (-(-136 // self.flit))))
        self.out_limit = min(u("-sim_max_outstanding_pkts"), K_INQ) or 1
        self.eject_buf = max(1, min(u("-gpgpu_n_cluster_ejection_buffer_size"), K_EJECTQ))
        self.resp_buf = max(1, min(u("-gpgpu_n_ldst_response_buffer_size"), K_LDST_RESPQ))
        self.rop_latency = u("-gpgpu_l2_rop_latency")
        self.q_icnt_l2 = max(1, int(str(o["-gpgpu_dram_partition_queues"]).strip().strip('"').split(":")[0]))
        f = [float(x) for x in str(o["-gpgpu_clock_domains"]).strip().strip('"').split(":")]
        self.per_core, self.per_icnt, self.per_l2 = (int(round(1e9 / x)) for x in f[:3])
        # the premises the oracle is written for
        assert u("-gpgpu_gmem_skip_L1D") == 1 and u("-gpgpu_perfect_inst_const_cache") == 1
        assert u("-sim_xcd") == 0 and str(o["-sim_mall"]) == "none"
        assert re.match(r"[SN]:\d+:128:\d+,L:B:m:L:", str(o["-gpgpu_cache:dl2"]).strip('"')), "write-back, lazy fetch"
        assert self.in_pkts < K_OUTQ          # step 3 of sm_receive never waits for the injection queue
        self.mode = u("-network_mode")
        self.contention = 0
        self.epoch = u("-icnt_latency")
        if self.mode == 1:
            kv = dict(re.findall(r"^\s*(\w+)\s*=\s*([^;]*?)\s*;", icnt_text, re.M))
            g = lambda k, d: int(float(kv[k])) if kv.get(k) else d
            self.topo, self.k, self.n = kv["topology"], g("k", 8), g("n", 2)
            assert self.topo in ("mesh", "fly") and self.k ** self.n >= self.n_clusters + self.n_subpart
            self.hop = max(1, g("routing_delay", 0) + g("vc_alloc_delay", 1) + g("sw_alloc_delay", 1) + 1)
            self.chan = max(1, g("channel_latency", 1))
            if "flit_size" in kv:
                self.flit = max(8, g("flit_size", 32))      # (after in_pkts, as in the derivation)
            self.contention = u("-icnt_link_contention")
            assert self.contention in (0, 1)
            # the lookahead: the smallest pair latency in whole core cycles, 1 .. kMaxEpoch
            self.epoch = 1
            lo = min(self.lat_fs(s, d) for s in range(0, self.n_sm, self.cpc) for d in range(self.n_subpart))
            self.epoch = max(1, min(K_MAX_EPOCH, lo // self.per_core))
        else:
            assert self.mode == 2
        assert 1 <= self.epoch <= K_MAX_EPOCH
        self.epoch_fs = self.epoch * self.per_core

    def nflits(self, size):
        return -(-size // self.flit)

    # ---- topology: the oracle's own walks -------------------------------------
    def nodes(self, sm, sub):
        return sm // self.cpc, self.n_clusters + sub     # one node per cluster, then the sub-partitions

    def digits(self, x):
        return [x // self.k ** i % self.k for i in range(self.n)]

    def route(self, a, b):
        """the directed links from node a to node b in traversal order, the last
        one ejecting into b; one link per router crossed"""
        if self.topo == "mesh":        # dimension order, lowest dimension first
            cur, dst, links = self.digits(a), self.digits(b), []
            for d in range(self.n):
                while cur[d] != dst[d]:
                    step = 1 if dst[d] > cur[d] else -1
                    links.append(("mesh", tuple(cur), d, step))
                    cur[d] += step
            return links + [("eject", b)]
        # k-ary n-fly, destination tag, most significant digit first: stage s sets digit
        # n-1-s; the router of a stage is the current address without that digit
        cur, dst, links = self.digits(a), self.digits(b), []
        for s in range(self.n):
            i = self.n - 1 - s
            links.append(("fly", s, tuple(cur[:i] + cur[i + 1:]), dst[i]))
            cur[i] = dst[i]
        return links

    def routers(self, a, b):
        if self.topo == "fly":
            return self.n
        return sum(abs(x - y) for x, y in zip(self.digits(a), self.digits(b))) + 1

    def lat_fs(self, sm, sub):
        """femtoseconds from injection complete to arrival, either direction"""
        lo = self.epoch * self.per_core
        if self.mode != 1:
            return lo
        r = self.routers(*self.nodes(sm, sub))
        return max((r * self.hop + (r + 1) * self.chan) * self.per_icnt, lo)   # never below the lookahead


class Pkt:
    __slots__ = ("src", "dst", "addr", "type", "size", "sectors", "t", "cycle", "epoch")

    def __init__(self, src, dst, addr, type, size, sectors):
        self.src, self.dst, self.addr, self.type, self.size, self.sectors = src, dst, addr, type, size, sectors
        self.t = self.cycle = self.epoch = 0


class Counters:
    """how often the oracle itself met each edge"""
    FIELDS = ("behind_multiflit", "past_epoch", "at_out_limit", "flit_exact", "flit_under", "flit_over",
              "req_conflict_cycles", "req_max_ready_srcs", "req_same_src_ready", "req_max_queued", "req_window_cycles",
              "head_gate_waits", "equal_time", "overtaken", "direct_rank", "backlog_epochs", "backlog_max",
              "rop_stall_cycles", "rop_max", "reply_port_waits", "reply_mixed", "reply_multiflit",
              "rep_conflict_cycles", "rep_max_ready_srcs", "eject_gate_closed", "link_delayed", "link_nonfinal",
              "link_reply_behind_request", "split_stores", "max_pair_latency", "min_pair_latency")

    def __init__(self):
        for f in self.FIELDS:
            setattr(self, f, 0)

    def __repr__(self):
        return " ".join(f"{f}={getattr(self, f)}" for f in self.FIELDS if getattr(self, f))


class Arbiter:
    def __init__(self):
        self.next = self.cnt = 0


def xbar_pick(cfg, q, now_fs, arb, nsrc):
    """sm.h xbar_pick: one of the inputs whose packet has arrived, among the 64
    oldest arrivals, in round-robin order from the pointer; the oldest packet
    of that input.  -> (offset, ready packets)"""
    ptr = arb.next % nsrc if cfg.arbiter else (now_fs // cfg.per_icnt) % nsrc
    ready = [i for i in range(min(len(q), WINDOW)) if q[i].t <= now_fs]
    off = min(ready, key=lambda i: ((q[i].src - ptr) % nsrc, i))
    if cfg.arbiter:      # iSLIP: the pointer moves past the granted input every icnt_grant_cycles grants
        if arb.cnt <= 1:
            arb.next = (q[off].src + 1) % nsrc
            arb.cnt = cfg.grant
        else:
            arb.cnt -= 1
    return off, ready


def port_open(q, now_fs, head_gate):
    """S3: the port arbitrates when the head of its queue has arrived (the
    rule as first stated: when any packet of the window has)"""
    if not q:
        return False
    if head_gate:
        return q[0].t <= now_fs
    return any(p.t <= now_fs for p in q[:WINDOW])


def gather(cfg, cnt, q, qcap, arrivals, backlog=None):
    """mem.h gather_sorted: the backlog first, then one epoch's arrivals in
    (time, source) order; what the queue cannot take goes to the backlog"""
    if backlog:
        m = min(len(backlog), qcap - len(q))
        q.extend(backlog[:m])
        del backlog[:m]
    if not arrivals:
        return
    keys = [(p.t, p.src) for p in arrivals]
    assert len(set(keys)) == len(keys), "one packet per source per tick"
    if len(arrivals) > qcap:
        cnt.direct_rank += 1         # more than the sort scratch: ranked against the source rows
    by_time = collections.Counter(p.t for p in arrivals)
    cnt.equal_time += sum(1 for v in by_time.values() if v > 1)
    arrivals = sorted(arrivals, key=lambda p: (p.t, p.src))
    room = 0 if backlog else qcap - len(q)      # a non-empty backlog keeps order
    q.extend(arrivals[:room])
    if len(arrivals) > room:
        assert backlog is not None, "the SM's arrival queue overflows"
        backlog.extend(arrivals[room:])


class OSub:
    """one memory sub-partition: input queue and backlog, request port, ROP
    queue, L2 access, reply queue and the reply injection port"""

    def __init__(self, orc, gsub):
        self.o, self.id = orc, gsub
        self.inq, self.ovf, self.rop, self.rep = [], [], collections.deque(), collections.deque()
        self.arb, self.port_free = Arbiter(), 0
        self.valid = {}
        self.events = []
        self.last_rep_flits = 0

    def idle(self):
        return not (self.inq or self.ovf or self.rop or self.rep)

    def l2_cycle(self, now):
        # l2_cycle: the head of the ROP queue, once its delay has passed
        if not self.rop or self.rop[0].t > now:
            return
        p = self.rop.popleft()
        have = self.valid.get(p.addr, 0)
        if p.type == P_WR:       # write-back, lazy fetch: full sectors are readable at once
            out = 0 if p.addr in self.valid and have & p.sectors == p.sectors else 1
            assert p.size - 8 == 32 * popc(p.sectors)
            self.valid[p.addr] = have | p.sectors
            r = Pkt(self.id, p.src, p.addr, P_WR_ACK, 8, p.sectors)
        else:
            if have & p.sectors != p.sectors:
                raise PremiseError(f"the load of line {p.addr:#x} misses: its reply would come from a fill")
            out = 0
            r = Pkt(self.id, p.src, p.addr, P_RD_REPLY, 8 + 32 * popc(p.sectors), p.sectors)
        if len(self.rep) >= K_REPLYQ:
            raise PremiseError("the reply queue is full: the L2 access would be refused")
        self.events.append((now // self.o.cfg.per_l2, self.id % self.o.cfg.nsub, L2_OUTCOME[out], p.addr))
        self.rep.append(r)

    def icnt_cycle(self, now, epoch):
        o, c, n = self.o, self.o.cfg, self.o.cnt
        # the request port: one ready input per interconnect cycle into the ROP queue
        limit = min(K_ROPQ, c.q_icnt_l2 + c.rop_latency)
        if self.inq:
            n.req_max_queued = max(n.req_max_queued, len(self.inq))
            if len(self.rop) >= limit:
                n.rop_stall_cycles += self.inq[0].t <= now
            elif port_open(self.inq, now, o.head_gate):
                off, ready = xbar_pick(c, self.inq, now, self.arb, c.n_sm)
                srcs = [self.inq[i].src for i in ready]
                n.req_conflict_cycles += len(ready) > 1
                n.req_max_ready_srcs = max(n.req_max_ready_srcs, len(set(srcs)))
                n.req_same_src_ready += len(set(srcs)) < len(srcs)
                n.req_window_cycles += len(self.inq) > WINDOW
                o.req_conflicts += len(ready) - 1
                p = self.inq.pop(off)
                o.req_queue_cycles += (now - p.t) // c.per_icnt
                o.req_packets += 1
                p.t = now + c.rop_latency * c.per_l2
                self.rop.append(p)
                n.rop_max = max(n.rop_max, len(self.rop))
            elif any(p.t <= now for p in self.inq[:WINDOW]):
                n.head_gate_waits += 1
        # the reply injection port
        if self.rep:
            if self.port_free > now:
                n.reply_port_waits += 1
                return
            r = self.rep.popleft()
            nfl = c.nflits(r.size)
            n.reply_multiflit += nfl > 1
            n.reply_mixed += self.last_rep_flits not in (0, nfl)
            self.last_rep_flits = nfl
            r.t = now + (nfl - 1) * c.per_icnt + c.lat_fs(r.dst, self.id)
            r.epoch = epoch
            self.port_free = now + nfl * c.per_icnt
            o.replies.setdefault(epoch, []).append(r)

    def window(self, epoch):
        """mem_window: every L2 and interconnect tick in the epoch, in time
        order; at equal times the L2 ticks first"""
        c = self.o.cfg
        t0, t1 = epoch * c.epoch_fs, (epoch + 1) * c.epoch_fs
        tl, ti = -(-t0 // c.per_l2) * c.per_l2, -(-t0 // c.per_icnt) * c.per_icnt
        while min(tl, ti) < t1 and not self.idle():
            if tl <= ti:
                self.l2_cycle(tl)
                tl += c.per_l2
            else:
                self.icnt_cycle(ti, epoch)
                ti += c.per_icnt


class OSm:
    """the reply path into one SM: arrival queue, crossbar output port,
    cluster ejection buffer, LD/ST response FIFO"""

    def __init__(self, orc, i):
        self.o, self.id = orc, i
        self.inq, self.cl, self.ld = [], collections.deque(), collections.deque()
        self.arb = Arbiter()
        self.events = []

    def idle(self):
        return not (self.inq or self.cl or self.ld)

    def run_epoch(self, epoch):
        o, c, n = self.o, self.o.cfg, self.o.cnt
        for now in range(epoch * c.epoch, (epoch + 1) * c.epoch):
            if self.idle():
                return
            now_fs = now * c.per_core
            # 1. the head of the ejection buffer moves to the response FIFO if that has room
            if self.cl and len(self.ld) < c.resp_buf:
                self.ld.append(self.cl.popleft())
            # 2. one packet that reached the port is ejected, unless the buffer is full
            if self.inq:
                if len(self.cl) >= c.eject_buf:
                    n.eject_gate_closed += self.inq[0].t <= now_fs
                elif port_open(self.inq, now_fs, o.head_gate):
                    off, ready = xbar_pick(c, self.inq, now_fs, self.arb, c.n_subpart)
                    n.rep_conflict_cycles += len(ready) > 1
                    n.rep_max_ready_srcs = max(n.rep_max_ready_srcs, len({self.inq[i].src for i in ready}))
                    o.rep_conflicts += len(ready) - 1
                    q = self.inq.pop(off)
                    o.rep_queue_cycles += (now_fs - q.t) // c.per_icnt
                    o.rep_packets += 1
                    self.events.append((now, q.type, q.addr))
                    o.ejected.setdefault(self.id, []).append(now)
                    self.cl.append(q)
                elif any(p.t <= now_fs for p in self.inq[:WINDOW]):
                    n.head_gate_waits += 1
            # 3. the LD/ST unit consumes one response (an acknowledgement or a bypassed load: never refused)
            if self.ld:
                self.ld.popleft()


class Oracle:
    def __init__(self, cfg, head_gate=True):
        self.cfg, self.head_gate = cfg, head_gate
        self.cnt = Counters()
        self.subs = [OSub(self, i) for i in range(cfg.n_subpart)]
        self.sms = [OSm(self, i) for i in range(cfg.n_sm)]
        self.replies, self.ejected = {}, {}
        self.req_conflicts = self.req_queue_cycles = self.req_packets = 0
        self.rep_conflicts = self.rep_queue_cycles = self.rep_packets = 0
        self.backlog = self.link_delayed = self.link_wait = 0
        self.link_free, self.link_owner = {}, {}

    # ---- sm_inject ------------------------------------------------------------
    def inject(self, pkts):
        """arrival times of the observed injections: the last flit leaves
        nflits - 1 cycles after the first, then the pair's latency"""
        c, n = self.cfg, self.cnt
        reqs, last = {}, {}
        for p in pkts:
            nfl = c.nflits(p.size)
            n.flit_exact += nfl > 1 and p.size % c.flit == 0
            n.flit_under += nfl > 1 and p.size % c.flit == c.flit - 8
            n.flit_over += nfl > 1 and p.size % c.flit == 8
            if p.src in last:
                free, lfl = last[p.src]
                assert p.cycle >= free, f"SM {p.src} injects at {p.cycle}: its port is busy until {free}"
                n.behind_multiflit += p.cycle == free and lfl > 1
            last[p.src] = (p.cycle + nfl, nfl)       # out_port_free
            done = p.cycle + nfl - 1
            n.past_epoch += done // c.epoch > p.cycle // c.epoch
            p.t = done * c.per_core + c.lat_fs(p.src, p.dst)
            p.epoch = p.cycle // c.epoch
            reqs.setdefault(p.epoch, []).append(p)
        lat = [c.lat_fs(s, d) for s in range(c.n_sm) for d in range(c.n_subpart)]
        n.max_pair_latency, n.min_pair_latency = max(lat) // c.per_icnt, min(lat) // c.per_icnt
        return reqs

    # ---- icnt_links.h -----------------------------------------------------------
    def reserve(self, p, a, b, is_reply, epoch):
        """icnt_reserve: the packet takes each link of its route for its flits,
        at the time its uncontended schedule (which ends at p.t) reaches that
        link, later if the link is still taken; a delay moves every later hop"""
        c, n = self.cfg, self.cnt
        links = c.route(a, b)
        assert len(links) == c.routers(a, b)
        occ = c.nflits(p.size) * c.per_icnt
        hop, last = (c.hop + c.chan) * c.per_icnt, c.chan * c.per_icnt
        delay = 0
        for h, l in enumerate(links):
            back = (len(links) - 1 - h) * hop + last
            t = max(p.t - back, 0) + delay
            f = self.link_free.get(l, 0)
            if f > t:
                delay += f - t
                t = f
                n.link_nonfinal += h < len(links) - 1
                n.link_reply_behind_request += is_reply and self.link_owner.get(l) == (False, epoch)
            self.link_free[l] = t + occ
            self.link_owner[l] = (is_reply, epoch)
        p.t += delay
        if delay:
            self.link_delayed += 1
            self.link_wait += delay // c.per_icnt
            n.link_delayed += 1

    def contend(self, reqs, reps, epoch):
        """icnt_contend, at the epoch's end: requests then replies, by
        destination, then source, then injection order"""
        c = self.cfg
        for p in sorted(reqs, key=lambda p: (p.dst, p.src)):        # (stable: injection order within a cell)
            a, b = c.nodes(p.src, p.dst)
            self.reserve(p, a, b, False, epoch)
        for p in sorted(reps, key=lambda p: (p.dst, p.src)):
            b, a = c.nodes(p.dst, p.src)
            self.reserve(p, a, b, True, epoch)

    # ---- the epoch loop -------------------------------------------------------
    def run(self, pkts):
        c, n = self.cfg, self.cnt
        reqs = self.inject(pkts)
        first = min(reqs)
        # later-injected packets that arrive before earlier-injected ones of the same port
        newest = {}
        for p in pkts:
            n.overtaken += p.t < newest.get(p.dst, 0)
            newest[p.dst] = max(newest.get(p.dst, 0), p.t)
        epoch = first
        while reqs or self.replies or not all(u.idle() for u in self.subs + self.sms):
            for s in self.subs:
                arr = [p for p in reqs.get(epoch - 1, ()) if p.dst == s.id]
                gather(c, n, s.inq, K_MEM_INQ, arr, s.ovf)
                self.backlog += len(s.ovf)
                n.backlog_epochs += bool(s.ovf)
                n.backlog_max = max(n.backlog_max, len(s.ovf))
                s.window(epoch)
            for m in self.sms:
                arr = [p for p in self.replies.get(epoch - 1, ()) if p.dst == m.id]
                gather(c, n, m.inq, K_INQ, arr)
                m.run_epoch(epoch)
            reqs.pop(epoch - 1, None)
            self.replies.pop(epoch - 1, None)
            if c.contention:
                self.contend(reqs.get(epoch, []), self.replies.get(epoch, []), epoch)
            epoch += 1
            assert epoch - first < 200000, "the oracle does not drain"
        # sm_can_send: never more in flight than -sim_max_outstanding_pkts
        for m in self.sms:
            ev = sorted([(x, 0) for x in self.ejected.get(m.id, ())] + [(p.cycle, 1) for p in pkts if p.src == m.id])
            out = 0
            for _, inj in ev:       # in a cycle sm_receive runs before sm_inject
                out += 1 if inj else -1
                assert 0 <= out <= c.out_limit, f"SM {m.id}: {out} packets in flight, the limit is {c.out_limit}"
                n.at_out_limit += inj and out == c.out_limit
        return self


# ---------------------------------------------------------------------------
# traffic
# ---------------------------------------------------------------------------
def base_options(**over):
    o = presets.get_preset("QV100")
    o.update({
        "-gpgpu_n_clusters": "4", "-gpgpu_n_cores_per_cluster": "1", "-gpgpu_n_mem": "1",
        "-gpgpu_n_sub_partition_per_mchannel": "2", "-gpgpu_clock_domains": "1000.0:1000.0:1000.0:850.0",
        "-gpgpu_gmem_skip_L1D": "1", "-gpgpu_perfect_inst_const_cache": "1", "-gpgpu_perf_sim_memcpy": "0",
        "-gpgpu_kernel_launch_latency": "0", "-gpgpu_TB_launch_latency": "0", "-gpgpu_inst_prefetch_lines": "0",
        "-gpgpu_cache:dl2": "S:32:128:24,L:B:m:L:P,A:192:4,32:0,32", "-sim_xcd": "0", "-sim_mall": "none",
        "-network_mode": "2", "-icnt_link_contention": "0", "-icnt_latency": "8", "-icnt_flit_size": "32",
        "-icnt_arbiter_algo": "1", "-icnt_grant_cycles": "1", "-icnt_in_buffer_limit": "64",
        "-sim_max_outstanding_pkts": "128", "-sim_l1_write_request_bytes": "128",
        "-gpgpu_n_cluster_ejection_buffer_size": "8", "-gpgpu_n_ldst_response_buffer_size": "2",
        "-gpgpu_l2_rop_latency": "20", "-gpgpu_dram_partition_queues": "8:8:8:8", "-sim_event_skip": "1",
    })
    o.update({k: str(v) for k, v in over.items()})
    return o


def lines_by_sub(dec, per_sub):
    """`per_sub` lines of the pool for every sub-partition, by the decoder"""
    out = collections.defaultdict(list)
    line = POOL_BASE
    while min((len(out[s]) for s in range(dec.n_mem * dec.nsub)), default=0) < per_sub:
        out[dec.decode(line)["sub"]].append(line)
        line += 128
        assert line < POOL_BASE + (1 << 26)
    return out


class Traffic:
    """A kernel of `ncta` CTAs of `wpc` warps.  Every warp stores `n_st` lines
    of its own (whole sectors) and then loads `n_ld` times sectors it stored.
    subs: the sub-partitions a warp's lines may be on; sectors: the (first
    sector, count) shapes of a store; a load reads at most max_load of a
    store's sectors, or with load_all all of them.  expect[line] is the line's packets in
    program order: (type, sectors, size)."""

    def __init__(self, opts, seed, ncta, wpc, n_st, n_ld, subs=None, sectors=((0, 4),), load_all=False, max_load=4):
        cfg_wr = int(opts["-sim_l1_write_request_bytes"])
        dec = Decoder(opts)
        rnd = random.Random(seed)
        nw = ncta * wpc
        subs = list(subs if subs is not None else range(dec.n_mem * dec.nsub))
        pool = lines_by_sub(dec, -(-nw * n_st // len(subs)) + 1)
        k = KernelBuilder("_Z4icntPi", (ncta, 1, 1), (32 * wpc, 1, 1), nregs=64, kid=1)
        assert k.g.nwarps == nw
        self.expect, self.n_packets, self.split = {}, 0, 0
        stored = [[] for _ in range(nw)]
        for j in range(n_st):
            base, mask = np.zeros(nw, np.int64), np.zeros(nw, np.uint64)
            for w in range(nw):
                sub = subs[(w + j) % len(subs)] if len(subs) > 1 else subs[0]
                line = pool[sub].pop()
                s0, n = rnd.choice(sectors)
                sec = ((1 << n) - 1) << s0
                base[w], mask[w] = line + 32 * s0, (1 << (8 * n)) - 1
                stored[w].append((line, s0, n))
                if cfg_wr == 64 and sec & 3 and sec & 12:
                    self.expect[line] = [(P_WR, sec & 3, 8 + 32 * popc(sec & 3)), (P_WR, sec & 12, 8 + 32 * popc(sec & 12))]
                    self.split += 1
                else:
                    self.expect[line] = [(P_WR, sec, 8 + 32 * n)]
            k.op("STG.E", [], [4, 5], base=base, stride=4, mask=mask)
        for j in range(n_ld):
            base, mask = np.zeros(nw, np.int64), np.zeros(nw, np.uint64)
            for w in range(nw):
                line, s0, n = stored[w][rnd.randrange(n_st)]
                if not load_all:
                    n2 = rnd.randint(1, min(n, max_load))
                    s0, n = s0 + rnd.randint(0, n - n2), n2
                base[w], mask[w] = line + 32 * s0, (1 << (8 * n)) - 1
                self.expect[line].append((P_RD, ((1 << n) - 1) << s0, 8))
            k.op("LDG.E", [8 + j % 48], [4], base=base, stride=4, mask=mask)
        k.op("EXIT")
        self.kernel = k.build()
        self.n_packets = sum(map(len, self.expect.values()))
        self.dec = dec


# ---------------------------------------------------------------------------
# the run's events
# ---------------------------------------------------------------------------
def parse_run(out):
    inj = [(int(c), int(s), int(d), int(a, 16)) for c, s, d, a in re.findall(
        r"Cycle (\d+): INTERCONNECT - core (\d+) injects packet to sub-partition (\d+) addr 0x([0-9a-f]+)", out)]
    ej, l2 = {}, {}
    for c, s, t, a in re.findall(r"Cycle (\d+): INTERCONNECT - core (\d+) ejects packet type (\d+) addr 0x([0-9a-f]+)", out):
        ej.setdefault(int(s), []).append((int(c), int(t), int(a, 16)))
    for ch, sub, what, a, c in re.findall(r"channel (\d+) sub (\d+) L2 ([\w-]+) line 0x([0-9a-f]+) l2_cycle (\d+)", out):
        l2.setdefault(int(ch), []).append((int(c), int(sub), what, int(a, 16)))
    return inj, ej, l2


def packets_of(traffic, inj):
    """type, sectors and size of every injected packet, from its address"""
    left = {a: collections.deque(v) for a, v in traffic.expect.items()}
    owner, pkts = {}, []
    for cycle, sm, sub, addr in inj:
        assert addr in left and left[addr], f"core {sm} injects a packet for {addr:#x}: not a packet of the kernel"
        assert owner.setdefault(addr, sm) == sm and traffic.dec.decode(addr)["sub"] == sub
        typ, sectors, size = left[addr].popleft()
        p = Pkt(sm, sub, addr, typ, size, sectors)
        p.cycle = cycle
        pkts.append(p)
    assert not any(left.values()), "packets of the kernel that were never injected"
    return pkts


def first_difference(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return f"entry {i}: the run has {g}, the oracle {w}"
    if len(got) != len(want):
        return f"the run has {len(got)} entries, the oracle {len(want)}"
    return None


def check_premises(out):
    fails = [int(x) for x in re.findall(r"L2_cache_bank\[\d+\]: .*Reservation_fails = (\d+)", out)]
    assert fails and not any(fails), "an L2 access was refused"
    assert stat(out, "gpu_stall_dramfull") == 0
    assert "lost to a full backlog ring" not in out and "trace events dropped" not in out


def compare(out, cfg, orc, pkts):
    """the whole event list of every unit, cycles included, then the statistics"""
    _, ej, l2 = parse_run(out)
    want_l2 = {}
    for s in orc.subs:
        want_l2.setdefault(s.id // cfg.nsub, []).extend(s.events)
    for ch in sorted(set(l2) | set(want_l2)):
        # (the host prints one channel's events of an L2 cycle in sub-partition order)
        bad = first_difference(l2.get(ch, []), sorted(want_l2.get(ch, []), key=lambda e: e[:2]))
        assert bad is None, f"channel {ch} L2 events, {bad}"
    for m in orc.sms:
        bad = first_difference(ej.get(m.id, []), m.events)
        assert bad is None, f"core {m.id} ejections, {bad}"
    assert sum(map(len, l2.values())) == sum(map(len, ej.values())) == len(pkts)
    got = {k: stat(out, k) for k in ("Req_Network_injected_packets_num", "Req_Network_conflicts",
                                      "Req_Network_queueing_cycles", "Reply_Network_injected_packets_num",
                                      "Reply_Network_conflicts", "Reply_Network_queueing_cycles",
                                      "icnt_mem_input_backlog")}
    assert got == {"Req_Network_injected_packets_num": orc.req_packets, "Req_Network_conflicts": orc.req_conflicts,
                   "Req_Network_queueing_cycles": orc.req_queue_cycles,
                   "Reply_Network_injected_packets_num": orc.rep_packets, "Reply_Network_conflicts": orc.rep_conflicts,
                   "Reply_Network_queueing_cycles": orc.rep_queue_cycles, "icnt_mem_input_backlog": orc.backlog}
    if cfg.contention:
        assert (stat(out, "Network_link_delayed_packets"), stat(out, "Network_link_wait_cycles")) == \
            (orc.link_delayed, orc.link_wait)


# ---------------------------------------------------------------------------
# the cases: options, traffic, and the edges the oracle must report (counter: at least)
# ---------------------------------------------------------------------------
MIXED = ((0, 4), (0, 1), (1, 2), (1, 3), (0, 4), (3, 1), (2, 2), (0, 3))
HALF_L2 = "1000.0:1000.0:500.0:850.0"
NONCOMMENSURATE = "2400.0:2100.0:1900.0:2000.0"     # the MI355X preset's style: three unequal clocks


def case(over=None, traffic=None, need=None, icnt=None, zero=(), run_need=None):
    return dict(over=over or {}, traffic=traffic or {}, need=need or {}, icnt=icnt, zero=tuple(zero),
                run_need=run_need or {})


SERIAL = dict(ncta=4, wpc=8, n_st=5, n_ld=6, sectors=MIXED)
SER_NEED = dict(behind_multiflit=20, at_out_limit=5, overtaken=5, reply_multiflit=20)
# (one-flit replies: the reply queue, which a reply leaves every nflits cycles, must not fill)
HOT = dict(ncta=6, wpc=16, n_st=2, n_ld=6, subs=(0,), sectors=MIXED, max_load=1)
ARB = {"-gpgpu_n_clusters": 6, "-icnt_in_buffer_limit": 200, "-icnt_flit_size": 40}
ARB_NEED = dict(req_conflict_cycles=50, req_max_ready_srcs=4, req_same_src_ready=10, req_window_cycles=20)
CONVERGE = dict(ncta=4, wpc=16, n_st=3, n_ld=6, sectors=((0, 4), (0, 4), (0, 1)), load_all=True)
REPLY = {"-gpgpu_n_mem": 2, "-gpgpu_n_cluster_ejection_buffer_size": 1, "-gpgpu_n_ldst_response_buffer_size": 1,
         "-icnt_in_buffer_limit": 300}
REPLY_NEED = dict(reply_mixed=20, reply_port_waits=20, rep_conflict_cycles=20, rep_max_ready_srcs=3)
TOPO6 = {"-gpgpu_n_clusters": 6, "-gpgpu_n_mem": 2, "-network_mode": 1, "-icnt_in_buffer_limit": 300}
LINKS = dict(ncta=6, wpc=10, n_st=4, n_ld=6, sectors=MIXED)
MESH = dict(topology="mesh", k=4, n=2, flit_size=8)
FLY = dict(topology="fly", k=4, n=2, flit_size=8)
LINK_NEED = dict(link_delayed=20, link_nonfinal=5, link_reply_behind_request=1)

CASES = {
    # 1. serialisation: multi-flit stores ahead of reads in an SM's injection queue; flit counts that cover
    #    8 + bytes exactly, one flit unit under and over; packets that end after their epoch; an injection
    #    buffer of one packet (flit8: the only thing that can refuse a packet there) or few packets in flight
    "serial_flit8": case({"-icnt_flit_size": 8, "-icnt_in_buffer_limit": 17, "-sim_max_outstanding_pkts": 128},
                         SERIAL, dict(behind_multiflit=20, overtaken=5, reply_multiflit=20, flit_exact=50, past_epoch=50,
                                      head_gate_waits=1), zero=("at_out_limit",), run_need={"gpgpu_n_stall_shd_mem": 50}),
    "serial_flit32": case({"-icnt_flit_size": 32, "-icnt_in_buffer_limit": 10, "-sim_max_outstanding_pkts": 6},
                          SERIAL, dict(SER_NEED, flit_over=50, past_epoch=20)),
    "serial_flit40_split": case({"-icnt_flit_size": 40, "-icnt_in_buffer_limit": 8, "-sim_max_outstanding_pkts": 6,
                                 "-sim_l1_write_request_bytes": 64},
                                SERIAL, dict(behind_multiflit=20, at_out_limit=5, flit_under=20, split_stores=20)),
    # 2. request port arbitration: six SMs at one sub-partition; both arbiters; more than 64 queued
    "arb_rotating": case(dict(ARB, **{"-icnt_arbiter_algo": 0}), HOT, ARB_NEED),
    "arb_islip_grant1": case(dict(ARB, **{"-icnt_arbiter_algo": 1, "-icnt_grant_cycles": 1}), HOT, ARB_NEED),
    "arb_islip_grant3": case(dict(ARB, **{"-icnt_arbiter_algo": 1, "-icnt_grant_cycles": 3}), HOT, ARB_NEED),
    # 3. gather: equal arrival times, overtaking, more arrivals in an epoch than sort scratch (8 SMs x 40
    #    cycles > 256), and a full input ring whose backlog drains in order (the wide case)
    "gather_wide": case({"-gpgpu_n_clusters": 8, "-icnt_latency": 40, "-icnt_in_buffer_limit": 200, "-icnt_flit_size": 40,
                         "-gpgpu_shader_core_pipeline": "2048:32"},
                        dict(ncta=16, wpc=30, n_st=1, n_ld=7, subs=(1,), sectors=((0, 4), (0, 1)), max_load=1),
                        dict(direct_rank=1, backlog_epochs=3, equal_time=50, overtaken=5, req_window_cycles=100)),
    # 4. ROP intake: a two-cycle ROP delay and a one-entry queue let three packets in; the L2 at half the
    #    interconnect's clock takes one every other cycle, so arrivals wait in the port
    "rop_intake": case(dict(ARB, **{"-gpgpu_l2_rop_latency": 2, "-gpgpu_dram_partition_queues": "1:8:8:8",
                                    "-gpgpu_clock_domains": HALF_L2}),
                       HOT, dict(rop_stall_cycles=50, req_conflict_cycles=20)),
    # 5. the reply side: five-flit read replies and one-flit acknowledgements on one port, every
    #    sub-partition converging on each SM, both arbiters (modulus n_subpart), both buffers at one
    "reply_rotating": case(dict(REPLY, **{"-icnt_arbiter_algo": 0}), CONVERGE, REPLY_NEED, zero=("eject_gate_closed",)),
    "reply_islip": case(dict(REPLY, **{"-icnt_arbiter_algo": 1, "-icnt_grant_cycles": 2}), CONVERGE, REPLY_NEED,
                        zero=("eject_gate_closed",)),
    # 6. clocks: (every case above has the three clocks equal) three unequal, non-commensurate clocks
    "clocks_mixed": case(dict(REPLY, **{"-gpgpu_clock_domains": NONCOMMENSURATE, "-icnt_flit_size": 8}), CONVERGE,
                         dict(reply_mixed=20, rep_conflict_cycles=5, req_conflict_cycles=5, past_epoch=20)),
    # 7. topology latency, no contention
    "topo_mesh": case(TOPO6, LINKS, dict(max_pair_latency=20, reply_multiflit=20), icnt=MESH),
    "topo_fly": case(TOPO6, LINKS, dict(max_pair_latency=9, reply_multiflit=20), icnt=FLY),
    # 8. link reservation on the same two topologies
    "links_mesh": case(dict(TOPO6, **{"-icnt_link_contention": 1}), LINKS, LINK_NEED, icnt=MESH),
    "links_fly": case(dict(TOPO6, **{"-icnt_link_contention": 1}), LINKS, LINK_NEED, icnt=FLY),
}
CLOCK_CASE = "clocks_mixed"
GATE_CASE = "serial_flit8"

_made = {}


def case_setup(name, tmp_path):
    """options, .icnt text and traffic of a case (the traffic is made once per process)"""
    c = CASES[name]
    opts = base_options(**c["over"])
    text = None
    if c["icnt"]:
        text = presets.render_icnt(presets.icnt_params(**c["icnt"]))
        p = tmp_path / f"{name}.icnt"
        p.write_text(text)
        opts["-inter_config_file"] = str(p)
    if name not in _made:
        _made[name] = Traffic(opts, sum(map(ord, name)), **c["traffic"])
    return opts, text, _made[name]


def run_case(mod, engine, name, tmp_path, extra=None):
    opts, text, traffic = case_setup(name, tmp_path)
    kl = rodinia.write_app(str(tmp_path / name), [traffic.kernel], memcpy=False)
    out, wall = run_sim(mod, opts, kl, extra or {}, engine)
    return opts, text, traffic, out, wall


def check_case(mod, engine, name, tmp_path, extra=None):
    c = CASES[name]
    opts, text, traffic, out, wall = run_case(mod, engine, name, tmp_path, extra)
    cfg = IcntCfg(opts, text)
    check_premises(out)
    inj, _, _ = parse_run(out)
    pkts = packets_of(traffic, inj)
    assert len(pkts) == traffic.n_packets
    orc = Oracle(cfg).run(pkts)
    orc.cnt.split_stores = traffic.split
    print(f"{name} [{engine}]: {wall:.2f} s, {len(pkts)} packets, epoch {cfg.epoch}, {orc.cnt}")
    # ---- the oracle alone: does the case reach its edges? ----
    for field, least in c["need"].items():
        assert getattr(orc.cnt, field) >= least, f"vacuous: {field} = {getattr(orc.cnt, field)}, wanted {least}"
    for field in c["zero"]:
        assert getattr(orc.cnt, field) == 0, field
    for key, least in c["run_need"].items():
        assert stat(out, key) >= least, f"vacuous: {key} = {stat(out, key)}, wanted {least}"
    # ---- the run against the oracle ----
    compare(out, cfg, orc, pkts)
    return out, cfg, traffic, pkts


@pytest.mark.parametrize("name", sorted(CASES))
def test_icnt_timing_matches_oracle_cpu(native, tmp_path, name):
    check_case(native, "cpu", name, tmp_path)


def trace_lines(out):
    return [l for l in out.splitlines() if l.startswith("GPGPU-Sim Cycle ")]


def check_event_skip(mod, engine, tmp_path):
    a = check_case(mod, engine, CLOCK_CASE, tmp_path, {"-sim_event_skip": "0"})[0]
    b = check_case(mod, engine, CLOCK_CASE, tmp_path, {"-sim_event_skip": "1"})[0]
    assert len(trace_lines(a)) > 1000 and trace_lines(a) == trace_lines(b)


def test_event_skip_off_gives_the_same_events_cpu(native, tmp_path):
    check_event_skip(native, "cpu", tmp_path)


def test_equal_clock_cases_have_equal_clocks():
    for name, c in CASES.items():
        cfg_clocks = base_options(**c["over"])["-gpgpu_clock_domains"].split(":")[:3]
        assert (len(set(cfg_clocks)) == 1) == (name not in (CLOCK_CASE, "rop_intake"))
    f = [float(x) for x in NONCOMMENSURATE.split(":")[:3]]
    per = [int(round(1e9 / x)) for x in f]
    assert len(set(per)) == 3 and all(a % b for a in per for b in per if a != b)


def test_head_gate_is_what_the_port_does(native, tmp_path):
    """S3: under the rule as first stated (the port arbitrates when any packet
    of its window has arrived) the oracle differs from the run"""
    out, cfg, traffic, pkts = check_case(native, "cpu", GATE_CASE, tmp_path)
    with pytest.raises(AssertionError):
        compare(out, cfg, Oracle(cfg, head_gate=False).run(packets_of(traffic, parse_run(out)[0])), pkts)


def test_oracle_refuses_a_load_that_would_miss(tmp_path):
    """a case that breaks the premise fails: it is not trimmed"""
    opts, text, traffic = case_setup("serial_flit32", tmp_path)
    cfg = IcntCfg(opts, text)
    line = next(a for a, v in traffic.expect.items() if v[0][1] != 0xf)
    p = Pkt(0, traffic.dec.decode(line)["sub"], line, P_RD, 8, 0xf)
    p.cycle = 8
    with pytest.raises(PremiseError):
        Oracle(cfg).run([p])


def test_topology_walks():
    """the oracle's own router counts: a 4 x 4 mesh in dimension order, a 4-ary 2-fly"""
    opts = base_options(**dict(TOPO6))
    mesh = IcntCfg(opts, presets.render_icnt(presets.icnt_params(**MESH)))
    fly = IcntCfg(opts, presets.render_icnt(presets.icnt_params(**FLY)))
    assert mesh.routers(0, 15) == 7 and mesh.routers(5, 6) == 2 and mesh.routers(3, 8) == 6
    assert [l[0] for l in mesh.route(4, 6)] == ["mesh", "mesh", "eject"]
    assert all(len(mesh.route(a, b)) == mesh.routers(a, b) for a in range(16) for b in range(16))
    assert all(len(fly.route(a, b)) == 2 for a in range(16) for b in range(16))
    # hop = 0 + 1 + 1 + 1 interconnect cycles per router, one per channel
    assert mesh.lat_fs(0, 0) == (mesh.routers(0, 6) * 3 + mesh.routers(0, 6) + 1) * mesh.per_icnt
    assert fly.epoch == 9 and mesh.epoch == 9
    # a request and a reply can share a link on both
    assert set(mesh.route(5, 8)) & set(mesh.route(6, 4)) and set(fly.route(0, 6)) & set(fly.route(8, 4))


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
def test_icnt_timing_matches_oracle_gpu(gpu_mod, tmp_path, name):
    check_case(gpu_mod, "gpu", name, tmp_path)


@pytest.mark.gpu
def test_event_skip_off_gives_the_same_events_gpu(gpu_mod, tmp_path):
    check_event_skip(gpu_mod, "gpu", tmp_path)

"""The memory hierarchy against an untimed plain-Python oracle.

Address decode, the L1 and L2 tag arrays with their write policies, request
routing and the DRAM row buffers are compared with a model written in plain
integer Python from the reference's rules (addrdec.cc:78-201 addrdec_tlx /
partition_address, gpu-cache.cc:80-153 set-index functions, :1229-1599
wr_hit_* / wr_miss_*) and, for what is MI355X-native, from the header comments
of csrc/model/addrdec.h, sm.h and mem.h (XCD slices, MALL, line-granular 'N'
fills, the stateless splitmix RANDOM mode).  Both engines compile the same
csrc/model/*.h, so GPU == CPU cannot see a wrong rule there; this oracle can.

What makes an untimed oracle possible: the simulated stream is serial.  One
warp issues loads in a register-dependent chain and follows every store with
MEMBAR.GL, so each access completes before the next one starts and every
outcome is a function of the address sequence alone.  The tests assert that
premise (no L1 MSHR_HIT, no L2 Pending_hits) before they compare anything.

The oracle never calls native.addr_decode / cache_set_index / ipoly_hash.
"""
import random
import re
import time

import numpy as np
import pytest

from accel_sim_framework_distributed_amd.models import presets
from accel_sim_framework_distributed_amd.tracegen import rodinia
from accel_sim_framework_distributed_amd.tracegen.builder import KernelBuilder

M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------
# oracle, part 1: hashing and address decode
# ---------------------------------------------------------------------------
# primitive polynomials (with their x^n term) and the number of address bits
# above the index that are folded in: addrdec.h ipoly_poly / ipoly_hbits; 16,
# 32 and 64 banks are the reference's IPOLY(5), IPOLY(37), IPOLY(67)
IPOLY_POLY = {1: 0x3, 2: 0x7, 3: 0xB, 4: 0x13, 5: 0x25, 6: 0x43, 7: 0x83, 8: 0x11D, 9: 0x211, 10: 0x409}
IPOLY_HBITS = {4: 13, 5: 15, 6: 19}


def gf2_mod(v, poly):
    """v(x) mod poly(x) over GF(2): bit-serial long division, one quotient bit
    per step from the top."""
    n = poly.bit_length() - 1
    for bit in range(v.bit_length() - 1, n - 1, -1):
        if v >> bit & 1:
            v ^= poly << (bit - n)
    return v


def o_ipoly(higher, index, nbanks):
    n = nbanks.bit_length() - 1
    if n == 0:
        return 0
    h = higher & ((1 << IPOLY_HBITS.get(n, 3 * n + 1)) - 1)
    return (index ^ gf2_mod(h << n, IPOLY_POLY[n])) & (nbanks - 1)


def o_bitwise(higher, index, nbanks):
    return (index ^ (higher & (nbanks - 1))) & (nbanks - 1)


def o_splitmix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def o_gather(mask, val):
    """the bits of val selected by mask, packed towards bit 0 (addrdec_packbits
    over the mask's own limits)"""
    r = pos = 0
    for i in range(64):
        if mask >> i & 1:
            r |= (val >> i & 1) << pos
            pos += 1
    return r


def _log2_floor(x):
    return x.bit_length() - 1


class Decoder:
    """linear_to_raw_address_translation, from the option strings."""

    FIELDS = ("chip", "bk", "row", "col", "burst")

    def __init__(self, opts):
        self.n_mem = int(opts["-gpgpu_n_mem"])
        self.nsub = int(opts["-gpgpu_n_sub_partition_per_mchannel"])
        self.pidx = int(opts["-gpgpu_memory_partition_indexing"])
        mapping = opts["-gpgpu_mem_addr_mapping"].strip().strip('"')
        m = re.match(r"dramid@(\d+)", mapping)
        chip_s = int(m.group(1)) if m else -1
        text = mapping.split(";", 1)[1] if ";" in mapping else mapping
        mask = dict.fromkeys(self.FIELDS, 0)
        ofs = 63
        for ch in text:
            c = ch.upper()
            if c in "| .":
                continue
            if c == "D":
                assert chip_s < 0
                mask["chip"] |= 1 << ofs
            elif c == "B":
                mask["bk"] |= 1 << ofs
            elif c == "R":
                mask["row"] |= 1 << ofs
            elif c == "C":
                mask["col"] |= 1 << ofs
            elif c == "S":
                mask["burst"] |= 1 << ofs
                mask["col"] |= 1 << ofs
            else:
                assert c == "0", ch
            ofs -= 1
        assert ofs == -1, mapping
        nbits = _log2_floor(self.n_mem)
        self.log2ch = nbits
        self.log2sub = _log2_floor(self.nsub)
        self.gap = self.n_mem != 1 << nbits
        if self.gap:
            nbits += 1
        self.n_ch_pow2 = 1 << nbits
        if chip_s >= 0 and not self.gap:
            # a power-of-two channel count: the channel bits are inserted at chip_s
            low = (1 << chip_s) - 1
            for f in ("bk", "row", "col"):
                mask[f] = ((mask[f] & ~low) << nbits) | (mask[f] & low)
            for i in range(chip_s, chip_s + nbits):
                mask["chip"] |= 1 << i
        self.chip_s = max(chip_s, 0)
        self.mask = mask
        # the lowest log2(nsub) bank bits select the sub-partition
        self.sub_id_mask = 0
        pos = 0
        for i in range(64):
            if pos >= self.log2sub:
                break
            if mask["bk"] >> i & 1:
                self.sub_id_mask |= 1 << i
                pos += 1
        # MI355X: private L2 slices per XCD (addrdec.h l2_slice_of)
        self.n_xcd = int(opts.get("-sim_xcd", "0"))
        self.log2_spx = 0
        if self.n_xcd:
            self.log2_spx = _log2_floor(self.n_mem * self.nsub // self.n_xcd)

    def _squeeze(self, addr):
        """gap (non-power-of-two) channel counts: the bits from chip_s upwards
        divide into channel (remainder) and the rest (quotient)"""
        hi = addr >> self.chip_s
        rest = ((hi // self.n_mem) << self.chip_s) | (addr & ((1 << self.chip_s) - 1))
        return hi % self.n_mem, rest, hi // self.n_mem

    def decode(self, addr):
        k = self.mask
        if not self.gap:
            chip = o_gather(k["chip"], addr)
            rest = addr
            high = addr >> (self.chip_s + self.log2ch + self.log2sub)
        else:
            chip, rest, high = self._squeeze(addr)
        t = {f: o_gather(k[f], rest) for f in ("bk", "row", "col", "burst")}
        total = self.n_mem * self.nsub
        if self.pidx == 1:
            assert not self.gap
            chip = o_bitwise(high, chip, self.n_mem)
        elif self.pidx in (2, 3):
            # 3 (PAE) has no decoder case in the reference; addrdec.h documents
            # that it decodes as IPOLY (defect D11)
            sp = chip * self.nsub + (t["bk"] & (self.nsub - 1))
            sp = o_ipoly(high, sp, self.n_ch_pow2 * self.nsub)
            if self.gap:
                sp %= total
            t.update(chip=sp // self.nsub, sub=sp)
            return t
        elif self.pidx == 4:
            # addrdec.h: the reference's rand()-filled map is a stateless
            # splitmix hash of the same key here
            sp = o_splitmix(addr >> (self.chip_s - self.log2sub)) % total
            t.update(chip=sp // self.nsub, sub=sp)
            return t
        t.update(chip=chip, sub=chip * self.nsub + (t["bk"] & (self.nsub - 1)))
        return t

    def partition_address(self, addr):
        if not self.gap:
            return o_gather(~(self.mask["chip"] | self.sub_id_mask) & M64, addr)
        return o_gather(~self.sub_id_mask & M64, self._squeeze(addr)[1])

    # XCD-private L2 (addrdec.h): the slice of the requesting SM's own XCD, and
    # the set address with the slice-select bits squeezed out of the channel field
    def l2_slice_of(self, sm, gsub):
        if not self.n_xcd:
            return gsub
        return ((sm % self.n_xcd) << self.log2_spx) | (gsub & ((1 << self.log2_spx) - 1))

    def l2_set_address(self, line):
        if not self.n_xcd:
            return self.partition_address(line)
        lo, k = self.chip_s, self.log2_spx
        return ((line >> (lo + k)) << lo) | (line & ((1 << lo) - 1))

    def boundaries(self):
        """bit positions where any field's mask starts or stops"""
        b = {self.chip_s, self.chip_s + self.log2ch + self.log2sub}
        for m in self.mask.values():
            for i in range(64):
                if (m >> i & 1) != ((m >> (i - 1) & 1) if i else 0):
                    b.add(i)
        return sorted(x for x in b if 0 < x <= 47)


def o_set_index(fn, nsets, addr, line_log2=7):
    """cache_config::hash_function"""
    sb = nsets.bit_length() - 1
    idx = (addr >> line_log2) & (nsets - 1)
    if fn == "H":
        if nsets not in (32, 64):
            return idx  # (the reference asserts; addrdec.h falls back to linear)
        upper = (addr & 0xE000) >> 13 | (addr & 0x20000) >> 14 | (addr & 0x80000) >> 15
        s = ((addr >> line_log2) & 0x1F) ^ upper
        if nsets == 64:
            s |= (addr & 0x1000) >> 7
        return s & (nsets - 1)
    if fn == "X":
        return o_bitwise(addr >> (line_log2 + sb), idx, nsets)
    if fn == "P":
        return o_ipoly(addr >> (line_log2 + sb), idx, nsets)
    return idx


# a row field of 9 and a column field of 10 separate runs: make_runs gives up
# (0xff) and addr_decode gathers those fields bit by bit (pack_bits)
MANY_RUNS = "dramid@8;00000000.00000000.00000000.00000000.RCRCRCRC.RCRCRCRC.RBBBCCCB.CCCSSSSS"
# explicit channel bits, no dramid@
D_BITS = "00000.00000000.00000000.0000000R.RRRRRRRR.RRRRRRRB.BBCCCBDD.DDDCCCSS.SSS".replace(".", "")


def decode_configs():
    cfgs = {name: presets.get_preset(name) for name in presets.PRESETS}
    cfgs["QV100_bitwise"] = {**presets.get_preset("QV100"), "-gpgpu_memory_partition_indexing": "1"}
    cfgs["QV100_many_runs"] = {**presets.get_preset("QV100"), "-gpgpu_mem_addr_mapping": MANY_RUNS}
    cfgs["TITANV_many_runs"] = {**presets.get_preset("TITANV"), "-gpgpu_mem_addr_mapping": MANY_RUNS}
    cfgs["QV100_D_bits"] = {**presets.get_preset("QV100"), "-gpgpu_mem_addr_mapping": D_BITS,
                            "-gpgpu_memory_partition_indexing": "0"}
    cfgs["QV100_D_bits_ipoly"] = {**presets.get_preset("QV100"), "-gpgpu_mem_addr_mapping": D_BITS}
    return cfgs


DECODE_CONFIGS = decode_configs()


def decode_addresses(dec, seed):
    rnd = random.Random(seed)
    a = [0] + [1 << b for b in range(48)] + [(1 << b) - 1 for b in dec.boundaries()]
    for bits in (20, 32, 40, 47):
        a += [rnd.getrandbits(bits) for _ in range(500)]  # 2000 in all
    return a


def test_mapping_strings_are_what_they_claim():
    assert len(D_BITS) == 64 and "D" in D_BITS and "dramid" not in D_BITS
    runs = lambda m: sum(1 for i in range(64) if (m >> i & 1) and not (m >> (i + 1) & 1))
    d = Decoder(DECODE_CONFIGS["QV100_many_runs"])
    assert runs(d.mask["row"]) > 8 and runs(d.mask["col"]) > 8
    # (partition_address gathers the complement of the channel and
    # sub-partition bits: with dramid@ that mask has at most three runs, so only
    # addr_decode's fields can reach the bit-by-bit path)
    assert {Decoder(c).pidx for c in DECODE_CONFIGS.values()} >= {0, 1, 2, 4}
    assert any(Decoder(c).gap and Decoder(c).pidx == 2 for c in DECODE_CONFIGS.values())
    mi = Decoder(DECODE_CONFIGS["MI355X"])
    assert mi.n_ch_pow2 * mi.nsub == 128


@pytest.mark.parametrize("name", sorted(DECODE_CONFIGS))
def test_addr_decode_matches_oracle(native, name):
    opts = DECODE_CONFIGS[name]
    dec = Decoder(opts)
    args = presets.args_for(opts)
    addrs = decode_addresses(dec, 7)
    want = [dec.decode(a) for a in addrs]
    # vacuity: every channel and every sub-partition is produced (oracle alone)
    assert {t["chip"] for t in want} == set(range(dec.n_mem))
    assert {t["sub"] for t in want} == set(range(dec.n_mem * dec.nsub))
    for a, w in zip(addrs, want):
        got = native.addr_decode(args, a)
        assert {k: got[k] for k in w} == w, (name, hex(a))


def test_ipoly_matches_long_division(native):
    """test_addrdec's 16-bank row check, as a property over 2..1024 banks: the
    hash is index ^ (h(x) * x^n mod P(x)), by polynomial long division"""
    rnd = random.Random(1)
    for n in range(1, 11):
        nb = 1 << n
        for _ in range(400):
            a = rnd.getrandbits(rnd.choice((8, 20, 40, 57)))
            b = rnd.getrandbits(n)
            assert native.ipoly_hash(a, b, nb) == o_ipoly(a, b, nb), (nb, hex(a), b)
        # linear in the high bits: one bit at a time covers every row
        for j in range(3 * n + 3):
            assert native.ipoly_hash(1 << j, 0, nb) == o_ipoly(1 << j, 0, nb), (nb, j)


@pytest.mark.parametrize("fn,nsets,assoc", [
    ("L", 4, 4), ("L", 1, 1), ("L", 64, 16), ("X", 8, 2), ("X", 1, 4), ("X", 128, 1), ("P", 4, 4), ("P", 1, 1),
    ("P", 16, 4), ("P", 32, 24), ("P", 64, 16), ("P", 128, 16), ("P", 1024, 1), ("H", 32, 4), ("H", 64, 4),
    ("H", 16, 4), ("H", 1, 1)])
def test_cache_set_index_matches_oracle(native, fn, nsets, assoc):
    geom = f"S:{nsets}:128:{assoc},L:B:m:L:{fn},A:192:4,32:0,32"
    rnd = random.Random(nsets * 131 + ord(fn))
    addrs = [0] + [1 << b for b in range(48)] + [i << 7 for i in range(nsets)]
    addrs += [rnd.getrandbits(w) for w in (20, 32, 47) for _ in range(500)]
    want = [o_set_index(fn, nsets, a) for a in addrs]
    assert set(want) == set(range(nsets))
    for a, w in zip(addrs, want):
        assert native.cache_set_index(geom, a) == w, (geom, hex(a))


# ---------------------------------------------------------------------------
# serial access streams and their traces
# ---------------------------------------------------------------------------
TRACE_ON = {"-trace_enabled": "1", "-trace_sampling_core": "-1", "-gpgpu_perf_sim_memcpy": "0",
            "-trace_components": "MEMORY_PARTITION_UNIT,MEMORY_SUBPARTITION_UNIT,INTERCONNECT"}
POOL_BASE = 0x7000_0000


def popc(x):
    return bin(x).count("1")


class Acc:
    """one warp instruction = one coalesced access: `n` whole sectors from
    sector `s0` of `line` (8 lanes of 4 bytes each), or half of each of them
    for a partial (2-byte) store"""

    def __init__(self, store, line, s0=0, n=4, partial=False, local=False):
        self.store, self.line, self.s0, self.n, self.partial, self.local = store, line, s0, n, partial, local
        self.sectors = ((1 << n) - 1) << s0
        self.bytes = (2 if partial else 4) * 8 * n

    def mnemonic(self):
        if self.local:
            return "STL" if self.store else "LDL"
        return ("STG.E.U16" if self.partial else "STG.E") if self.store else "LDG.E"


def make_stream(seed, pool, n_acc, stores=0.0, partial=0.0, local=0.0, follow=False, small_stores=False,
                veto=None):
    """seeded mix of full-line, one- and two-sector accesses over `pool`, as a
    generator.  follow: every store is followed by a full-line load of its
    line (a store that starts a fetch nobody waits for: the load waits for it);
    veto(store) drops a store whose follow-up load would ask for nothing new
    and so merge into the store's fetch instead of waiting behind it."""
    rnd = random.Random(seed)
    made = 0
    while made < n_acc:
        line = rnd.choice(pool)
        n = rnd.choice((4, 4, 1, 1, 2, 2, 3))
        s0 = rnd.randrange(0, 5 - n)
        loc = rnd.random() < local
        if rnd.random() < stores:
            if small_stores and n > 2:
                n = rnd.choice((1, 2))
                s0 = rnd.randrange(0, 5 - n)
            st = Acc(True, line, s0, n, partial=(not loc and rnd.random() < partial), local=loc)
            if veto and veto(st):
                continue
            yield st
            made += 1
            if follow:
                yield Acc(False, line, 0, 4, local=loc)
                made += 1
        else:
            yield Acc(False, line, s0, n, local=loc)
            made += 1


def build_kernel(stream, kid=1, ncta=1, work_cta=0, warp_size=32):
    """the serial warp program of `stream`, run by CTA `work_cta` alone: each
    load's address register is the previous load's destination, each store is
    followed by MEMBAR.GL"""
    k = KernelBuilder(f"_Z3mo{kid}Pi", (ncta, 1, 1), (warp_size, 1, 1), nregs=16, kid=kid, warp_size=warp_size)
    work = k.g.cta == work_cta
    ra, rb = 4, 6
    for a in stream:
        base = np.full(k.g.nwarps, a.line + 32 * a.s0, np.int64)
        mask = (1 << (8 * a.n)) - 1
        if a.store:
            k.op(a.mnemonic(), [], [ra, 5], base=base, stride=4, mask=mask, present=work)
            k.op("MEMBAR.GL", present=work)
        else:
            k.op(a.mnemonic(), [rb], [ra], base=base, stride=4, mask=mask, present=work)
            ra, rb = rb, ra
    k.op("EXIT")
    return k.build()


def run_sim(mod, config, kl, extra, engine="cpu"):
    from accel_sim_framework_distributed_amd.sim import build_args
    s = mod.Simulator(build_args(config, kl, engine, dict(TRACE_ON, **extra)), False)
    t0 = time.perf_counter()
    assert s.run() == 0, s.output[-2000:]
    assert s.engine == engine
    assert "trace events dropped" not in s.output
    return s.output, time.perf_counter() - t0


def stat(out, key):
    m = re.findall(rf"{re.escape(key)} = ([0-9]+)", out)
    assert m, key
    return int(m[-1])


def injected(out):
    """[(core, sub-partition, line)] of the INTERCONNECT inject lines, in order"""
    return [(int(c), int(s), int(a, 16)) for c, s, a in
            re.findall(r"INTERCONNECT - core (\d+) injects packet to sub-partition (\d+) addr 0x([0-9a-f]+)", out)]


L1_TYPES = ("GLOBAL_ACC_R", "GLOBAL_ACC_W", "LOCAL_ACC_R", "LOCAL_ACC_W")


def assert_serial(out, n_banks):
    """the premise of every comparison below: no access met another in flight"""
    for t in L1_TYPES:
        assert stat(out, f"Total_core_cache_stats_breakdown[{t}][MSHR_HIT]") == 0, \
            f"the trace was not serial (L1 {t} MSHR_HIT): not a model failure"
    pend = [int(x) for x in re.findall(r"L2_cache_bank\[\d+\]: .*Pending_hits = (\d+)", out)[-n_banks:]]
    assert len(pend) == n_banks and not any(pend), "the trace was not serial (L2 Pending_hits): not a model failure"


# ---------------------------------------------------------------------------
# oracle, part 2: the L1 data cache
# ---------------------------------------------------------------------------
class Way:
    __slots__ = ("tag", "valid", "dirty", "stamp")

    def __init__(self):
        self.tag = self.valid = self.dirty = self.stamp = 0


class TagArray:
    """sets of ways with tag, valid-sector mask, dirty-sector mask and stamp.
    Victim: the lowest invalid way, else the smallest stamp; the stamp moves on
    a hit only under LRU (FIFO keeps the allocation stamp).

    One rule here is the model's and not the reference's, documented as
    difference M1 in the headers of csrc/model/mem.h and sm.h: `valid` holds
    readable sectors only, and a way left with dirty sectors but no readable
    one (a part-sector store under lazy write-allocate) is not found by its tag
    and counts as invalid.  The next access to its line misses and allocates
    again; the way's dirty sectors are written back when it is taken.  The
    reference would keep the line MODIFIED (gpu-cache.cc:269-297)."""

    def __init__(self, nsets, assoc, lru, index_fn):
        self.sets = [[Way() for _ in range(assoc)] for _ in range(nsets)]
        self.lru, self.index_fn, self.clock = lru, index_fn, 0
        self.evictions = self.dirty_victims = self.max_way = 0

    def tick(self):
        self.clock += 1
        return self.clock

    def find(self, line):
        ways = self.sets[self.index_fn(line)]
        for i, w in enumerate(ways):
            if w.valid and w.tag == line:  # readable lines only (M1)
                self.max_way = max(self.max_way, i)
                return w
        return None

    def touch(self, w):
        if self.lru:
            w.stamp = self.tick()

    def allocate(self, line, on_dirty):
        """replace the victim by `line` (no sector valid yet); on_dirty(tag,
        dirty mask) sees a victim that holds dirty sectors"""
        ways = self.sets[self.index_fn(line)]
        inval = [i for i, w in enumerate(ways) if not w.valid]  # dirty-only ways too (M1)
        i = inval[0] if inval else min(range(len(ways)), key=lambda j: ways[j].stamp)
        w = ways[i]
        self.max_way = max(self.max_way, i)
        if w.valid or w.dirty:
            self.evictions += 1
            if w.dirty:
                self.dirty_victims += 1
                on_dirty(w.tag, w.dirty)
        w.tag, w.valid, w.dirty, w.stamp = line, 0, 0, self.tick()
        return w


class L1Oracle:
    """sm.h sm_ldst / l1_fill, i.e. the reference's data_cache with
    allocate-on-fill reads and the wr_hit_* / wr_miss_* write policies."""

    def __init__(self, dec, nsets, assoc, repl, wpolicy, walloc, index, sectored):
        self.dec = dec
        self.tags = TagArray(nsets, assoc, repl == "L", lambda a: o_set_index(index, nsets, a))
        self.wpolicy, self.walloc, self.sectored = wpolicy, walloc, sectored
        self.stats = {(t, o): 0 for t in L1_TYPES for o in ("HIT", "MISS")}
        self.packets = []        # (destination sub-partition, line)
        self.writebacks = 0
        self.sector_misses = 0   # the tag is there, a sector is not
        self.pending = 0         # sectors of a store's own fetch still on their way

    def send(self, line):
        self.packets.append((self.dec.decode(line)["sub"], line))

    def _writeback(self, tag, dirty):
        self.writebacks += 1
        self.send(tag)

    def fill(self, line, sectors):
        w = self.tags.find(line) or self.tags.allocate(line, self._writeback)
        w.valid |= sectors
        self.tags.touch(w)

    def follow_up_would_merge(self, st):
        w = self.tags.find(st.line)
        have = w.valid if w else 0
        return have & st.sectors != st.sectors and have | st.sectors == 0xF

    def access(self, a):
        key = ("LOCAL" if a.local else "GLOBAL") + ("_ACC_W" if a.store else "_ACC_R")
        hit = self.store(a) if a.store else self.load(a)
        self.stats[key, "HIT" if hit else "MISS"] += 1

    def load(self, a):
        w = self.tags.find(a.line)
        have = w.valid if w else 0
        miss = a.sectors & ~have
        if not miss:
            self.tags.touch(w)
            return True
        self.sector_misses += w is not None
        # a sectored cache fetches the sectors the access misses, a
        # line-granular one ('N') the whole line it does not hold
        fetch = miss if self.sectored else 0xF & ~have
        self.send(a.line)
        pending, self.pending = self.pending, 0
        assert not (pending and not fetch & ~pending), "stream error: this load would merge into the store's fetch"
        if pending:
            self.fill(a.line, pending)
        self.fill(a.line, fetch & ~pending)
        return False

    def store(self, a):
        t = self.tags
        pol = self.wpolicy
        if pol == "L":  # write-back for local, write-evict for global data
            pol = "B" if a.local else "E"
        w = t.find(a.line)
        have = w.valid if w else 0
        hit = w is not None and have & a.sectors == a.sectors
        full = a.bytes >= 32 * popc(a.sectors) if self.sectored else a.bytes >= 128
        wb = pol == "B"
        if hit:
            if wb:  # the line absorbs the store
                w.dirty |= a.sectors
                t.touch(w)
            else:
                self.send(a.line)
                if pol == "E":
                    w.valid &= ~a.sectors
                else:
                    t.touch(w)
            return True
        self.sector_misses += w is not None
        if self.walloc == "N" or pol == "E":  # no write-allocate: straight below
            self.send(a.line)
            if w and pol == "E":
                w.valid &= ~a.sectors
            return False
        # write-allocate: lazy fetch on read (L), fetch-on-write of partial
        # sectors (F), write and read the line (W)
        fetch = self.walloc == "W" or (self.walloc == "F" and not full)
        if not wb or self.walloc == "W":
            self.send(a.line)
        if w is None:
            w = t.allocate(a.line, self._writeback)
        if full and not fetch:
            w.valid |= a.sectors
        if wb:
            w.dirty |= a.sectors
        t.touch(w)
        if fetch:
            want = a.sectors & ~w.valid
            if want:
                # nobody waits for this read: the stream's next access is a
                # full-line load of the same line, which does
                self.send(a.line)
                self.pending = want
        return False


def l1_geom(nsets, assoc, repl, wpolicy, walloc, index, sect):
    return f"{sect}:{nsets}:128:{assoc},{repl}:{wpolicy}:m:{walloc}:{index},A:512:8,16:0,32"


def sparse_pool(seed, n):
    """lines whose high bits differ too, for the hashed set-index functions"""
    rnd = random.Random(seed)
    return sorted(POOL_BASE + (i << 7) for i in rnd.sample(range(1 << 14), n))


DENSE40 = [POOL_BASE + (i << 7) for i in range(40)]
# (nsets, assoc, repl, wpolicy, walloc, index, sectored 'S' / line 'N', pool, stream options)
L1_CASES = {
    "4x4_lru_wt_lazy": (4, 4, "L", "T", "L", "L", "S", DENSE40, dict(stores=0.35, partial=0.3)),
    "4x4_fifo_wb_lazy": (4, 4, "F", "B", "L", "L", "S", DENSE40, dict(stores=0.4)),
    # part-sector stores on a write-back lazy L1: dirty-only ways (M1) meet l1_evict
    "4x4_lru_wb_lazy_partial": (4, 4, "L", "B", "L", "L", "S", DENSE40, dict(stores=0.45, partial=0.5)),
    "8x2_lru_xor_wb_lazy": (8, 2, "L", "B", "L", "X", "S", sparse_pool(1, 40), dict(stores=0.4)),
    "8x2_fifo_ipoly_wb_noalloc": (8, 2, "F", "B", "N", "P", "S", sparse_pool(2, 40), dict(stores=0.4, partial=0.3)),
    "1x4_lru_wb_fetch_on_write": (1, 4, "L", "B", "F", "L", "S", DENSE40[:12],
                                  dict(stores=0.4, partial=0.5, follow=True, small_stores=True)),
    "4x1_lru_wb_naive": (4, 1, "L", "B", "W", "L", "S", DENSE40[:16], dict(stores=0.4, follow=True, small_stores=True)),
    "4x4_lru_ipoly_line_wb_lazy": (4, 4, "L", "B", "L", "P", "N", sparse_pool(3, 40), dict(stores=0.4)),
    "32x1_lru_fermi_wb_lazy": (32, 1, "L", "B", "L", "H", "S", sparse_pool(4, 64), dict(stores=0.4)),
    "1x96_lru_wb_lazy": (1, 96, "L", "B", "L", "L", "S", DENSE40 + sparse_pool(5, 90), dict(stores=0.4)),
    "1x96_fifo_wt_lazy": (1, 96, "F", "T", "L", "L", "S", DENSE40 + sparse_pool(6, 90), dict(stores=0.3)),
    "4x4_lru_we_noalloc": (4, 4, "L", "E", "N", "L", "S", DENSE40, dict(stores=0.3)),
    "4x4_fifo_xor_we_lazy": (4, 4, "F", "E", "L", "X", "S", sparse_pool(7, 40), dict(stores=0.3)),
    "4x4_lru_we_naive": (4, 4, "L", "E", "W", "L", "S", DENSE40, dict(stores=0.3, partial=0.3)),
    "8x2_fifo_we_fetch_on_write": (8, 2, "F", "E", "F", "L", "S", DENSE40, dict(stores=0.3, partial=0.5)),
    "4x4_lru_localwb_lazy": (4, 4, "L", "L", "L", "L", "S", DENSE40, dict(stores=0.4, local=0.6)),
    "4x4_lru_localwb_noalloc": (4, 4, "L", "L", "N", "L", "S", DENSE40[:24], dict(stores=0.5, local=0.7)),
    "4x4_lru_localwb_fetch_on_write": (4, 4, "L", "L", "F", "L", "S", DENSE40,
                                       dict(stores=0.4, local=0.6, partial=0.5, follow=True, small_stores=True)),
    "8x2_lru_localwb_naive": (8, 2, "L", "L", "W", "L", "S", DENSE40,
                              dict(stores=0.4, local=0.6, follow=True, small_stores=True)),
    "4x4_lru_wt_noalloc": (4, 4, "L", "T", "N", "L", "S", DENSE40, dict(stores=0.35, partial=0.3)),
    "4x4_lru_wt_fetch_on_write": (4, 4, "L", "T", "F", "L", "S", DENSE40,
                                  dict(stores=0.35, partial=0.5, follow=True, small_stores=True)),
    "4x1_fifo_line_wt_naive": (4, 1, "F", "T", "W", "L", "N", DENSE40[:16],
                               dict(stores=0.35, follow=True, small_stores=True)),
}
L1_ACCESSES = 360


def l1_expect(name):
    nsets, assoc, repl, wp, wa, index, sect, pool, opt = L1_CASES[name]
    o = L1Oracle(Decoder(presets.get_preset("QV100")), nsets, assoc, repl, wp, wa, index, sect == "S")
    stream = []
    for a in make_stream(sum(map(ord, name)), pool, L1_ACCESSES, veto=o.follow_up_would_merge if opt.get("follow") else None,
                         **opt):
        o.access(a)
        stream.append(a)
    assert not o.pending
    # vacuity guards, from the oracle alone
    hits = sum(v for (t, oc), v in o.stats.items() if oc == "HIT")
    misses = sum(v for (t, oc), v in o.stats.items() if oc == "MISS")
    assert hits >= 20 and misses >= 20 and o.tags.evictions >= 20, (name, hits, misses, o.tags.evictions)
    if wp in "BL":
        assert o.tags.dirty_victims >= 10, (name, o.tags.dirty_victims)
    if sect == "S":
        assert o.sector_misses >= 10, (name, o.sector_misses)
    if assoc > 64:
        assert o.tags.max_way >= 64, (name, o.tags.max_way)
    return stream, o


def check_l1(mod, engine, name, tmp_path):
    stream, o = l1_expect(name)
    geom = L1_CASES[name][:7]
    kl = rodinia.write_app(str(tmp_path / name), [build_kernel(stream)], memcpy=False)
    out, wall = run_sim(mod, "QV100", kl, {"-gpgpu_adaptive_cache_config": "0", "-gpgpu_cache:dl1": l1_geom(*geom)},
                        engine)
    assert_serial(out, 64)
    assert "L1 write-backs lost" not in out
    got = {(t, oc): stat(out, f"Total_core_cache_stats_breakdown[{t}][{oc}]") for (t, oc) in o.stats}
    print(f"{name} [{engine}]: {wall:.2f} s, {len(stream)} accesses, oracle {o.stats}, "
          f"write-backs {o.writebacks}, packets {len(o.packets)}")
    assert got == o.stats
    assert stat(out, "gpgpu_n_l1_writebacks") == o.writebacks
    assert len({c for c, _, _ in injected(out)}) == 1  # one warp on one SM
    inj = [(s, a) for _, s, a in injected(out)]
    bad = next((i for i, (g, w) in enumerate(zip(inj, o.packets)) if g != w), None)
    assert bad is None, (bad, inj[bad], o.packets[bad])
    assert len(inj) == len(o.packets)
    return wall


@pytest.mark.parametrize("name", sorted(L1_CASES))
def test_l1_matches_oracle_cpu(native, tmp_path, name):
    check_l1(native, "cpu", name, tmp_path)


# ---------------------------------------------------------------------------
# oracle, part 3: L2 slices, routing, MALL and the DRAM row buffers
# ---------------------------------------------------------------------------
class MemOracle:
    """mem.h l2_access / l2_fill / dram_cycle for one access at a time: one tag
    array per sub-partition indexed by cache_set_index(partition_address(line))
    (xcd_partition_address with XCDs), a read miss allocated when its first
    sector returns, a write-back L2 with lazy ('L') or no ('N') write-allocate,
    and below it one MALL and one open row per bank for every channel."""

    def __init__(self, opts):
        self.dec = dec = Decoder(opts)
        g = re.match(r"(\w):(\d+):128:(\d+),(\w):(\w):\w:(\w):(\w),", opts["-gpgpu_cache:dl2"].strip('"'))
        self.sectored = g.group(1) == "S"
        nsets, assoc = int(g.group(2)), int(g.group(3))
        assert g.group(5) == "B" and g.group(6) in "LN"
        self.walloc = g.group(6)
        self.nsets, self.assoc, self.lru, self.index = nsets, assoc, g.group(4) == "L", g.group(7)
        self.nbk = int(re.search(r"nbk=(\d+)", opts["-gpgpu_dram_timing_opt"]).group(1))
        self.tags = {}
        mall = opts.get("-sim_mall", "none")
        self.mall_geom = tuple(int(x) for x in mall.split(":")) if mall != "none" else None
        self.mall = {}
        self.open_row = {}
        self.l2_events = []   # (sub-partition, "hit" / "miss", line)
        self.dram = {}        # channel -> [(command, bank, row)]
        self.stats = {}
        self.sector_misses = 0

    def bump(self, key, n=1):
        self.stats[key] = self.stats.get(key, 0) + n

    def slice_tags(self, sub):
        if sub not in self.tags:
            self.tags[sub] = TagArray(self.nsets, self.assoc, self.lru,
                                      lambda a: o_set_index(self.index, self.nsets, self.dec.l2_set_address(a)))
        return self.tags[sub]

    # ---- DRAM: open-page banks; a command to another row precharges, then activates
    def dram_cmd(self, ch, write, line, sector):
        t = self.dec.decode(line + 32 * sector)
        bank, row = t["bk"] % self.nbk, t["row"]
        log = self.dram.setdefault(ch, [])
        cur = self.open_row.get((ch, bank))
        if cur != row:
            if cur is not None:
                log.append(("PRE", bank, cur))
                self.bump(("n_pre", ch))
            log.append(("ACT", bank, row))
            self.bump(("n_act", ch))
            self.open_row[ch, bank] = row
        log.append(("WR" if write else "RD", bank, row))
        self.bump(("n_write" if write else "n_rd", ch))

    # ---- MALL: per channel, sectored, LRU, allocated when the DRAM read returns
    def mall_ways(self, ch, line):
        sets, assoc = self.mall_geom
        key = ch, (self.dec.l2_set_address(line) >> 7) & (sets - 1)
        if key not in self.mall:
            self.mall[key] = [Way() for _ in range(assoc)]
        return self.mall[key]

    def below_read(self, ch, line, sectors):
        """sectors leave the L2 for memory, lowest first"""
        todo = [s for s in range(4) if sectors >> s & 1]
        if self.mall_geom:
            ways = self.mall_ways(ch, line)
            clock = self.mall.setdefault(("clock", ch), [0])
            miss = []
            for s in todo:
                w = next((w for w in ways if w.valid and w.tag == line), None)
                if w and w.valid >> s & 1:
                    clock[0] += 1
                    w.stamp = clock[0]
                    self.bump("MALL_read_hits")
                else:
                    miss.append(s)
                    self.bump("MALL_read_misses")
            todo = miss
        for s in todo:
            self.dram_cmd(ch, False, line, s)
        if self.mall_geom:
            for s in todo:
                w = next((w for w in ways if w.valid and w.tag == line), None)
                if w is None:
                    inval = [w for w in ways if not w.valid]
                    w = inval[0] if inval else min(ways, key=lambda x: x.stamp)
                    assert not w.dirty, "read-only streams only: the MALL write path is not modelled here"
                    w.tag, w.valid = line, 0
                w.valid |= 1 << s
                clock[0] += 1
                w.stamp = clock[0]

    def _evict(self, sub):
        ch = sub // self.dec.nsub

        def on_dirty(tag, dirty):
            assert not self.mall_geom, "read-only streams only with a MALL"
            self.bump("dirty_evictions")
            for s in range(4):
                if dirty >> s & 1:
                    self.dram_cmd(ch, True, tag, s)
        return on_dirty

    def access(self, a, core):
        sub = self.dec.l2_slice_of(core, self.dec.decode(a.line)["sub"])
        ch = sub // self.dec.nsub
        t = self.slice_tags(sub)
        w = t.find(a.line)
        have = w.valid if w else 0
        self.bump(("Access", sub))
        if a.store:
            hit = w is not None and have & a.sectors == a.sectors
            self.sector_misses += w is not None and not hit
            self.l2_events.append((sub, "hit" if hit else "miss", a.line))
            if not hit:
                self.bump(("Miss", sub))
                if self.walloc == "N":  # the miss goes to DRAM without allocating
                    for s in range(4):
                        if a.sectors >> s & 1:
                            self.dram_cmd(ch, True, a.line, s)
                    return
            if w is None:
                w = t.allocate(a.line, self._evict(sub))
            # only whole-sector writes are readable at once (lazy fetch on read)
            if a.bytes >= 32 * popc(a.sectors):
                w.valid |= a.sectors
            w.dirty |= a.sectors
            t.touch(w)
            return
        miss = a.sectors & ~have
        if not miss:
            t.touch(w)
            self.l2_events.append((sub, "hit", a.line))
            return
        self.sector_misses += w is not None
        self.bump(("Miss", sub))
        self.l2_events.append((sub, "miss", a.line))
        fetch = miss if self.sectored else 0xF & ~have
        self.below_read(ch, a.line, fetch)
        for s in range(4):  # every returning sector fills; the first allocates
            if fetch >> s & 1:
                w = t.find(a.line) or t.allocate(a.line, self._evict(sub))
                w.valid |= 1 << s
                t.touch(w)


def l2_geom(sect, nsets, assoc, repl, walloc, index):
    return f"{sect}:{nsets}:128:{assoc},{repl}:B:m:{walloc}:{index},A:192:4,32:0,32"


def l2_options(name):
    base, over, _ = L2_CASES[name]
    o = presets.get_preset(base)
    # every access goes below the L1; the L2 is small enough for 40 lines to fight over
    o.update({"-gpgpu_gmem_skip_L1D": "1"}, **over)
    return o


def l2_pool(dec, seed, n_lines, n_subs):
    """lines that decode to the first n_subs sub-partitions met, so that they
    collide in those slices' sets"""
    rnd = random.Random(seed)
    subs, pool = [], []
    while len(pool) < n_lines:
        line = POOL_BASE + (rnd.randrange(1 << 16) << 7)
        s = dec.decode(line)["sub"]
        if s not in subs and len(subs) < n_subs:
            subs.append(s)
        if s in subs and line not in pool:
            pool.append(line)
    return pool


# preset, option overrides, stream options
L2_CASES = {
    "QV100_ipoly_sectored_lazy": ("QV100", {"-gpgpu_cache:dl2": l2_geom("S", 4, 4, "L", "L", "P")},
                                  dict(stores=0.4, partial=0.2)),
    "TITANV_gap_ipoly_line_lazy": ("TITANV", {"-gpgpu_cache:dl2": l2_geom("N", 4, 2, "L", "L", "P")},
                                   dict(stores=0.4)),
    "RTX2060_consecutive_noalloc": ("RTX2060", {"-gpgpu_cache:dl2": l2_geom("S", 2, 4, "L", "N", "L")},
                                    dict(stores=0.4, partial=0.2)),
    "TITANX_random_fifo_lazy": ("TITANX", {"-gpgpu_cache:dl2": l2_geom("S", 4, 2, "F", "L", "X")},
                                dict(stores=0.4)),
    "QV100_many_runs_lazy": ("QV100", {"-gpgpu_mem_addr_mapping": MANY_RUNS,
                                       "-gpgpu_cache:dl2": l2_geom("S", 8, 2, "L", "L", "L")}, dict(stores=0.4)),
    "TITANV_many_runs_gap_lazy": ("TITANV", {"-gpgpu_mem_addr_mapping": MANY_RUNS,
                                             "-gpgpu_cache:dl2": l2_geom("S", 8, 2, "L", "L", "L")}, dict(stores=0.4)),
}
L2_ACCESSES = 360


def l2_expect(name):
    opts = l2_options(name)
    o = MemOracle(opts)
    pool = l2_pool(o.dec, sum(map(ord, name)), 40, 3)
    stream = list(make_stream(sum(map(ord, name)) + 1, pool, L2_ACCESSES, **L2_CASES[name][2]))
    for a in stream:
        o.access(a, 0)
    hits = sum(1 for e in o.l2_events if e[1] == "hit")
    ev = sum(t.evictions for t in o.tags.values())
    dirty = sum(t.dirty_victims for t in o.tags.values())
    assert hits >= 20 and len(o.l2_events) - hits >= 20 and ev >= 20 and dirty >= 10, (name, hits, ev, dirty)
    if o.sectored:
        assert o.sector_misses >= 10, (name, o.sector_misses)
    return opts, stream, o


def l2_events(out):
    return [(int(k), int(j), oc, int(a, 16)) for k, j, oc, a in
            re.findall(r"channel (\d+) sub (\d+) L2 ([\w-]+) line 0x([0-9a-f]+)", out)]


def dram_events(out):
    ev = {}
    for k, cmd, b, r in re.findall(r"channel (\d+) DRAM (\w+) bank (\d+) row (\d+)", out):
        ev.setdefault(int(k), []).append((cmd, int(b), int(r)))
    return ev


def check_below(out, o, n_sub_total):
    """the L2 and DRAM side of a run against the oracle `o`"""
    nsub = o.dec.nsub
    got = [(k * nsub + j, oc, a) for k, j, oc, a in l2_events(out)]
    bad = next((i for i, (g, w) in enumerate(zip(got, o.l2_events)) if g != w), None)
    assert bad is None, (bad, got[bad], o.l2_events[bad])
    assert len(got) == len(o.l2_events)
    bank = {int(b): (int(a), int(m)) for b, a, m in
            re.findall(r"L2_cache_bank\[(\d+)\]: Access = (\d+), Miss = (\d+)", out)[-n_sub_total:]}
    assert bank == {s: (o.stats.get(("Access", s), 0), o.stats.get(("Miss", s), 0)) for s in range(n_sub_total)}
    assert stat(out, "L2_cache_dirty_evictions") == o.stats.get("dirty_evictions", 0)
    # DRAM: dram_cycle issues ACT and PRE only for a queued request whose row
    # is not the bank's open one (no refresh, no close-page timer), so with one
    # access in flight they are a function of the address sequence
    # too.  Banks work side by side, so the order is compared bank by bank.
    dram = dram_events(out)
    for ch in sorted(set(dram) | set(o.dram)):
        for bk in range(o.nbk):
            g = [e for e in dram.get(ch, []) if e[1] == bk]
            w = [e for e in o.dram.get(ch, []) if e[1] == bk]
            bad = next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), None)
            assert bad is None, (ch, bk, bad, g[bad], w[bad])
            assert len(g) == len(w), (ch, bk)
    n_ch = n_sub_total // nsub
    totals = re.findall(r"DRAM\[(\d+)\]: n_act=(\d+) n_pre=(\d+) n_rd=(\d+) n_write=(\d+)", out)[-n_ch:]
    for ch, act, pre, rd, wr in totals:
        want = tuple(o.stats.get((k, int(ch)), 0) for k in ("n_act", "n_pre", "n_rd", "n_write"))
        assert (int(act), int(pre), int(rd), int(wr)) == want, ch


def check_l2(mod, engine, name, tmp_path):
    opts, stream, o = l2_expect(name)
    kl = rodinia.write_app(str(tmp_path / name), [build_kernel(stream)], memcpy=False)
    out, wall = run_sim(mod, opts, kl, {}, engine)
    n_sub_total = o.dec.n_mem * o.dec.nsub
    assert_serial(out, n_sub_total)
    print(f"{name} [{engine}]: {wall:.2f} s, {len(stream)} accesses, {len(o.l2_events)} L2 events, "
          f"{sum(len(v) for v in o.dram.values())} DRAM commands")
    # routing: every request goes to the sub-partition its line decodes to
    assert [(s, a) for _, s, a in injected(out)] == [(s, a) for s, _, a in o.l2_events]
    check_below(out, o, n_sub_total)
    return wall


@pytest.mark.parametrize("name", sorted(L2_CASES))
def test_l2_dram_matches_oracle_cpu(native, tmp_path, name):
    check_l2(native, "cpu", name, tmp_path)


def test_kernel_release_writes_every_dirty_sector_back(native, tmp_path):
    """-sim_l2_kernel_release: at the kernel's end every dirty sector left in
    the L2s goes to memory, those of dirty-only lines (M1) included."""
    name = "QV100_ipoly_sectored_lazy"
    opts, stream, o = l2_expect(name)
    # the stream ends with part-sector stores to six lines the L2 does not hold
    tail = [Acc(True, POOL_BASE + (1 << 24) + (i << 7), i % 4, 1, partial=True) for i in range(6)]
    for a in tail:
        o.access(a, 0)
    stream = stream + tail
    left = [w for t in o.tags.values() for ways in t.sets for w in ways if w.dirty]
    assert sum(1 for w in left if not w.valid) >= 3, "vacuous: no dirty-only line is left at the end"
    kl = rodinia.write_app(str(tmp_path / "rel"), [build_kernel(stream)], memcpy=False)
    out, _ = run_sim(native, opts, kl, {"-sim_l2_kernel_release": "1"})
    assert_serial(out, o.dec.n_mem * o.dec.nsub)
    during = sum(1 for log in o.dram.values() for e in log if e[0] == "WR")
    assert stat(out, "L2_to_mem_write_sectors") == during + sum(popc(w.dirty) for w in left)
    assert stat(out, "L2_cache_dirty_evictions") == o.stats["dirty_evictions"] + len(left)


# ---- MI355X: XCD-private L2 slices and the MALL ---------------------------
# three kernels of eight CTAs; one CTA of each does the work, so the working
# warp sits in another XCD every time (config.h: CTA i runs on an SM of XCD
# i % n_xcd, SM s belongs to XCD s % n_xcd).  The L2s keep their lines from
# kernel to kernel (-sim_l2_kernel_release is another test's subject).
XCD_WORK_CTAS = (0, 3, 5)
XCD_CTAS = 8
# (nor are the instruction and scalar caches: their fetches would mix with the stream)
MI355X_OVER = {"-gpgpu_gmem_skip_L1D": "1", "-sim_l2_kernel_release": "0", "-gpgpu_perfect_inst_const_cache": "1",
               "-gpgpu_cache:dl2": l2_geom("N", 4, 2, "L", "L", "P")}


def xcd_expect():
    opts = presets.get_preset("MI355X")
    assert opts["-sim_xcd"] == "8" and opts["-sim_mall"] == "1024:16"  # as the preset sets them
    opts.update(MI355X_OVER)
    o = MemOracle(opts)
    pool = l2_pool(o.dec, 11, 40, 3)
    stream = list(make_stream(12, pool, L2_ACCESSES))  # read-only: the MALL's write path is not modelled
    per = len(stream) // len(XCD_WORK_CTAS)
    parts = [stream[i * per:(i + 1) * per] for i in range(len(XCD_WORK_CTAS))]
    for cta, part in zip(XCD_WORK_CTAS, parts):
        for a in part:
            o.access(a, cta % o.dec.n_xcd)
    hits = sum(1 for e in o.l2_events if e[1] == "hit")
    ev = sum(t.evictions for t in o.tags.values())
    assert hits >= 20 and len(o.l2_events) - hits >= 20 and ev >= 20, (hits, ev)
    assert o.stats["MALL_read_hits"] >= 20 and o.stats["MALL_read_misses"] >= 20, o.stats
    assert len({s >> o.dec.log2_spx for s, _, _ in o.l2_events}) >= 2, "vacuous: one XCD only"
    return opts, parts, o


def check_xcd(mod, engine, tmp_path):
    opts, parts, o = xcd_expect()
    kernels = [build_kernel(p, kid=i + 1, ncta=XCD_CTAS, work_cta=c, warp_size=64)
               for i, (c, p) in enumerate(zip(XCD_WORK_CTAS, parts))]
    kl = rodinia.write_app(str(tmp_path / "xcd"), kernels, memcpy=False)
    out, wall = run_sim(mod, opts, kl, {}, engine)
    n_sub_total = o.dec.n_mem * o.dec.nsub
    assert_serial(out, n_sub_total)
    print(f"MI355X_xcd_mall [{engine}]: {wall:.2f} s, {sum(map(len, parts))} accesses, MALL hits "
          f"{o.stats['MALL_read_hits']} misses {o.stats['MALL_read_misses']}")
    inj = injected(out)
    # the destination is the slice of the requesting SM's own XCD
    xcds = [c % o.dec.n_xcd for c, _, _ in inj]
    assert xcds == [c % o.dec.n_xcd for c, p in zip(XCD_WORK_CTAS, parts) for _ in p]
    assert len(set(xcds)) >= 2
    assert [(o.dec.l2_slice_of(c, o.dec.decode(a)["sub"]), a) for c, _, a in inj] == [(s, a) for _, s, a in inj]
    assert [(s, a) for _, s, a in inj] == [(s, a) for s, _, a in o.l2_events]
    check_below(out, o, n_sub_total)
    assert stat(out, "MALL_read_hits") == o.stats["MALL_read_hits"]
    assert stat(out, "MALL_read_misses") == o.stats["MALL_read_misses"]
    return wall


def test_mi355x_xcd_slices_and_mall_match_oracle_cpu(native, tmp_path):
    check_xcd(native, "cpu", tmp_path)


# ---------------------------------------------------------------------------
# the same traces on the GPU engine (default build), against the oracle itself
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
@pytest.mark.parametrize("name", sorted(L1_CASES))
def test_l1_matches_oracle_gpu(gpu_mod, tmp_path, name):
    check_l1(gpu_mod, "gpu", name, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(L2_CASES))
def test_l2_dram_matches_oracle_gpu(gpu_mod, tmp_path, name):
    check_l2(gpu_mod, "gpu", name, tmp_path)


@pytest.mark.gpu
def test_mi355x_xcd_slices_and_mall_match_oracle_gpu(gpu_mod, tmp_path):
    check_xcd(gpu_mod, "gpu", tmp_path)

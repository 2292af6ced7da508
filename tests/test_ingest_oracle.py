"""Trace ingest against a plain-Python oracle.

The host coalescer (csrc/trace/trace.cc: smem_conflict_degree, coalesce_lanes,
lds_groups_for) and its MI355X twin on the matrix cores
(csrc/engine/ingest_mfma.hip) are compared value by value with an oracle
written here from the contracts in the header comment of ingest_mfma.hip and in
trace.h, with arbitrary-precision ints, sets and dicts.  The oracle never calls
the native coalescer, and the CDNA4 lane-group tables below are written out
from the LDS table of the MI355X micro-architecture guide, not read back from
lds_groups_for.

  no marker: host == oracle for every instruction
  gpu:       device == host == oracle, and the placement (matrix cores or
             host fallback) of every instruction == the documented windows
"""
import random
from collections import defaultdict

import pytest

M64 = (1 << 64) - 1
K_MAX_ACCESS = 64  # kMaxAccess: accesses kept per instruction (the lowest lines)
L1_BANKS = 4       # passed explicitly so that TAcc::bank is not trivially 0


# ----------------------------------------------------------------------------
# CDNA4 LDS table (MI355X_MICROARCH, section LDS): lane groups, one LDS cycle
# each, and the bank count of every ds_* form
def _lanes(*runs):
    return frozenset(l for lo, hi in runs for l in range(lo, hi + 1))


_LO, _HI = _lanes((0, 31)), _lanes((32, 63))
_HALVES = [_LO, _HI]
_Q16 = [_lanes((16 * i, 16 * i + 15)) for i in range(4)]  # 4 x 16 contiguous
_O8 = [_lanes((8 * i, 8 * i + 7)) for i in range(8)]      # 8 x 8 contiguous
_B128 = [_lanes((0, 3), (12, 15), (20, 27)), _lanes((4, 11), (16, 19), (28, 31)),
         _lanes((32, 35), (44, 47), (52, 59)), _lanes((36, 43), (48, 51), (60, 63))]
_B96 = [_lanes((0, 3), (20, 23)), _lanes((4, 7), (16, 19)), _lanes((8, 11), (28, 31)), _lanes((12, 15), (24, 27)),
        _lanes((32, 35), (52, 55)), _lanes((36, 39), (48, 51)), _lanes((40, 43), (60, 63)),
        _lanes((44, 47), (56, 59))]

LDS_TABLE = {
    # opcode: (banks, lane groups)
    "ds_read_b32": (32, _HALVES),
    "ds_read_b64": (64, _HALVES),
    "ds_read_b96": (32, _B96),
    "ds_read_b128": (64, _B128),
    "ds_read_b64_tr_b16": (64, _HALVES),
    # the table has no row of its own for sub-dword reads and LDS atomics: they
    # are 4-byte-class accesses, banked like ds_read_b32 (trace.cc: "32 for the rest")
    "ds_read_u8": (32, _HALVES),
    "ds_read_u16": (32, _HALVES),
    "ds_add_u32": (32, _HALVES),
    "ds_read2_b32": (32, _HALVES + _HALVES),  # as two ds_read_b32
    "ds_read2_b64": (32, _Q16 + _Q16),        # two accesses, each 4 x 16 contiguous
    "ds_write_b32": (32, _HALVES),
    "ds_write_b64": (32, _Q16),
    "ds_write_b96": (32, _O8),
    "ds_write_b128": (32, _O8),
    # the guide's table is silent on ds_write2: pinned to trace.cc's comment (one store of the
    # combined size: write2_b32 banks like ds_write_b64, write2_b64 like ds_write_b128; the
    # guide's prose pairs them the same way by their source dwords)
    "ds_write2_b32": (32, _Q16),
    "ds_write2_b64": (32, _O8),
    # the ds_load_* / ds_store_* spellings of the same instructions
    "ds_load_b128": (64, _B128),
    "ds_store_b64": (32, _Q16),
    "ds_load_2addr_b32": (32, _HALVES + _HALVES),
    "ds_store_2addr_b64": (32, _O8),
}


# ----------------------------------------------------------------------------
# configurations: (preset, extra options) and what the oracle needs of them,
# stated here and not read from the native config
class Cfg:
    def __init__(self, preset, extra, ws, nb, parts=1, groups=False, lbcast=False):
        self.preset, self.extra = preset, dict(extra, **{"-gpgpu_l1_banks": str(L1_BANKS)})
        self.ws, self.nb, self.parts, self.groups, self.lbcast = ws, nb, parts, groups, lbcast

    def args(self):
        from accel_sim_framework_distributed_amd.models import presets
        return presets.args_for(self.preset, self.extra)

    def table(self, op):
        """(banks, lane groups) of one shared instruction under this configuration"""
        if self.groups:
            return LDS_TABLE[op]
        per = -(-self.ws // self.parts)
        return self.nb, [frozenset(range(p * per, min((p + 1) * per, self.ws))) for p in range(self.parts)]


CONFIGS = {
    "qv100": Cfg("QV100", {}, 32, 32),
    "qv100_parts2": Cfg("QV100", {"-gpgpu_shmem_warp_parts": "2"}, 32, 32, parts=2),
    "qv100_nb64": Cfg("QV100", {"-gpgpu_shmem_num_banks": "64"}, 32, 64),
    "mi355x": Cfg("MI355X", {}, 64, 64, groups=True),
    "mi355x_nogroups": Cfg("MI355X", {"-gpgpu_shmem_cdna_lane_groups": "0"}, 64, 64),
    "qv100_nb16": Cfg("QV100", {"-gpgpu_shmem_num_banks": "16"}, 32, 16),
    "qv100_lbcast": Cfg("QV100", {"-gpgpu_shmem_limited_broadcast": "1"}, 32, 32, lbcast=True),
}


# ----------------------------------------------------------------------------
# the oracle.  An instruction is (space, width, mask, addresses, opcode) with
# addresses a list (one per active lane) or a (base, stride) tuple.
def lane_addresses(cfg, inst):
    """{lane: address} of the active lanes: addr = list[rank] or base + stride * rank (mod 2^64)"""
    _, _, mask, addrs, _ = inst
    out, rank = {}, 0
    for l in range(cfg.ws):  # only lanes below the warp size are active
        if mask >> l & 1:
            out[l] = (addrs[0] + addrs[1] * rank) & M64 if isinstance(addrs, tuple) else addrs[rank]
            rank += 1
    return out


def _words(a, width):
    return range(a >> 2, ((a + width - 1) >> 2) + 1)


def _group_degree(la, lanes, width, nb):
    """distinct 4-byte words on the busiest of nb banks over the active lanes in `lanes` (0: none active)"""
    banks = defaultdict(set)
    for l, a in la.items():
        if l in lanes:
            for w in _words(a, width):
                banks[w % nb].add(w)
    return max((len(s) for s in banks.values()), default=0)


def oracle_shared(cfg, inst):
    _, width, _, _, op = inst
    la = lane_addresses(cfg, inst)
    nb, groups = cfg.table(op)
    degs = [_group_degree(la, g, width, nb) for g in groups]
    if cfg.groups:
        deg = 1 + sum(max(0, d - 1) for d in degs)
    else:
        deg = max(1, sum(d if d else (1 if p == 0 else 0) for p, d in enumerate(degs)))
    return ("shared", min(deg, 255), [])


def _pieces(a, width):
    """(line, sector mask, bytes) of [a, a + width) split at 128 B lines"""
    end = a + width
    while a < end:
        line = a & ~127
        pend = min(end, line + 128)
        sec = 0
        for s in range(a >> 5, ((pend - 1) >> 5) + 1):
            sec |= 1 << (s & 3)
        yield line, sec, pend - a
        a = pend


def oracle_global(cfg, inst):
    _, width, _, _, _ = inst
    secs, nbytes = defaultdict(int), defaultdict(int)
    for a in lane_addresses(cfg, inst).values():
        for line, sec, n in _pieces(a, width):
            secs[line] |= sec
            nbytes[line] += n  # summed over the lanes, no deduplication
    lines = sorted(secs)[:K_MAX_ACCESS]
    if not lines:
        return ("shared", 1, [])  # completes as a 1-cycle shared access
    return ("global", len(lines), [(l, secs[l], min(nbytes[l], 128), (l >> 7) % L1_BANKS) for l in lines])


def oracle(cfg, inst):
    return oracle_shared(cfg, inst) if inst[0] == "shared" else oracle_global(cfg, inst)


def on_device(cfg, inst):
    """the documented windows of the matrix-core path"""
    space, width, _, _, op = inst
    la = lane_addresses(cfg, inst)
    if space == "global":
        if not la:
            return True
        if max(((a + width - 1) >> 7) - (a >> 7) + 1 for a in la.values()) > 2:
            return False
        return (max(a + width - 1 for a in la.values()) >> 7) - (min(la.values()) >> 7) + 1 <= 64
    nb, groups = cfg.table(op)
    if nb not in (32, 64) or cfg.lbcast:
        return False
    for g in groups:
        ws = [_words(a, width) for l, a in la.items() if l in g]
        if not ws:
            continue
        if max(len(w) for w in ws) > 8:
            return False
        if max(w[-1] // nb for w in ws) - min(w[0] // nb for w in ws) > 255:
            return False
    return True


# ----------------------------------------------------------------------------
# cases: (name, instruction)
def _mask(lanes):
    m = 0
    for l in lanes:
        m |= 1 << l
    return m


GBASE = 0x7F1234560000  # 128 B aligned


def shared_cases(cfg, op):
    ws = cfg.ws
    nb, groups = cfg.table(op)
    distinct = list(dict.fromkeys(groups))  # read2 tables list their groups twice
    g0 = sorted(distinct[0])
    la, lb = g0[0], g0[-1]  # two lanes of one group
    full = (1 << ws) - 1
    row = nb * 4            # bytes of one bank row
    out = []

    def sh(name, width, lanes_or_mask, addrs):
        m = lanes_or_mask if isinstance(lanes_or_mask, int) else _mask(lanes_or_mask)
        if isinstance(addrs, dict):
            addrs = [addrs[l] for l in sorted(addrs)]
        out.append((f"{op or 'generic'}:{name}", ("shared", width, m, addrs, op)))

    # row window: max(w1 / nb) - min(w0 / nb) <= 255 per lane group / warp part
    r0 = 1000
    for d in (255, 256):
        sh(f"rows differ by {d}", 4, [la, lb], {la: r0 * row + 8, lb: (r0 + d) * row + 20})
        sh(f"rows differ by {d}, far lane first", 4, [la, lb], {la: (r0 + d) * row, lb: r0 * row + 4})
        # the far row is reached only by the last word of an 8-byte access
        sh(f"last word in row +{d}", 8, [la, lb], {la: r0 * row, lb: (r0 + d) * row - 4})
    if len(distinct) > 1:
        lc = sorted(distinct[1])[0]
        sh("1 MiB apart, different groups", 4, [la, lc], {la: 64, lc: 64 + (1 << 20)})
    sh("1 MiB apart, one group", 4, [la, lb], {la: 64, lb: 64 + (1 << 20)})
    # row tiles and accumulator halves (rows 0-3 / 4-7 of a 32x32 tile sit on different halves of the wave)
    g8 = g0[:8]
    for bank in (0, 31, 32, 63):
        if bank < nb:
            sh(f"bank {bank} rows 0..7", 4, g8, {l: (r * nb + bank) * 4 for r, l in enumerate(g8)})
            # the maximum (3 words) on this bank, 2 words on its neighbour
            other = (bank + 1) % nb
            five = g0[:5]
            rows = [(0, bank), (5, bank), (37, bank), (2, other), (40, other)]
            sh(f"maximum in bank {bank}", 4, five, {l: (r * nb + b) * 4 for l, (r, b) in zip(five, rows)})
    sh("rows 31, 32", 4, [la, lb], {la: (31 * nb + 3) * 4, lb: (32 * nb + 3) * 4})
    sh("rows 0, 255", 4, [la, lb], {la: 3 * 4, lb: (255 * nb + 3) * 4})
    sh("rows 4, 7 only", 4, [la, lb], {la: (4 * nb + 9) * 4, lb: (7 * nb + 9) * 4})
    sh("every lane its own row, one bank", 4, full, (5 * 4, row))
    sh("every lane its own row, one bank (list)", 4, full, [5 * 4 + l * row for l in range(ws)])
    # words per lane (device: at most 8)
    for name, width, off in (("w1 at 3", 1, 3), ("w2 at 3", 2, 3), ("w12 at 2", 12, 2), ("w32 aligned", 32, 0),
                             ("w29 at 3", 29, 3), ("w32 at 1", 32, 1), ("w16 aligned", 16, 0), ("w8 at 2", 8, 2)):
        sh(f"words per lane: {name}", width, full, [l * 32 + off for l in range(ws)])
        sh(f"words per lane, conflicting: {name}", width, full, [l * row + off for l in range(ws)])
        sh(f"words per lane, one lane: {name}", width, [lb], [4096 + off])
    # deduplication
    sh("one word from every lane", 4, full, [128] * ws)
    sh("one word from every lane, unaligned bytes", 1, full, [128 + l % 4 for l in range(ws)])
    lm = g0[1]
    sh("A's first word is B's last", 8, [la, lm, lb], {la: 16, lm: 12, lb: (4 + nb) * 4})
    sh("four words shared pairwise", 16, g0[:4], {l: 8 * i for i, l in enumerate(g0[:4])})
    # masks
    sh("empty mask", 4, 0, [])
    for l in (0, 31, 32, 63):
        if l < ws:
            sh(f"only lane {l}", 4, [l], [l * 4])
            sh(f"only lane {l}, two rows", 8, [l], [row - 4])
    for i, g in enumerate(distinct):
        gl = sorted(g)
        sh(f"only group {i}, one bank", 4, gl, [7 * 4 + k * row for k in range(len(gl))])
        sh(f"only group {i}, linear", 4, gl, [k * 4 for k in range(len(gl))])
    firsts = sorted(sorted(g)[0] for g in distinct)
    sh("one lane of every group, one bank", 4, firsts, [11 * 4 + k * row for k in range(len(firsts))])
    lasts = sorted(sorted(g)[-1] for g in distinct)
    sh("last lane of every group, one word", 4, lasts, [44] * len(lasts))
    # address forms: base + stride * rank, rank = active lanes below the lane
    half = int("01" * 32, 2) & full
    for name, base in (("low", 4096), ("1 << 63", 1 << 63), ("below 1 << 48", (1 << 48) - 65536)):
        sh(f"stride 0 at {name}", 4, full, (base, 0))
        sh(f"stride 4 at {name}", 4, full, (base, 4))
        sh(f"stride 8 at {name}, width 8", 8, full, (base + 4, 8))
        sh(f"stride of one row at {name}, partial mask", 4, half, (base, row))
        sh(f"stride 36 at {name}, partial mask", 4, 0x6DB6DB6DB6DB6DB6 & full, (base, 36))
        sh(f"negative stride from {name}", 4, full, (base + 65536, -4))
        sh(f"negative stride of one row from {name}, partial mask", 4, half, (base + 65536, -row))
        sh(f"negative stride of 9 rows from {name}", 4, full, (base + (1 << 20), -9 * row))
    return out


def global_cases(cfg):
    ws = cfg.ws
    full = (1 << ws) - 1
    B = GBASE
    out = []

    def gl(name, width, lanes_or_mask, addrs):
        m = lanes_or_mask if isinstance(lanes_or_mask, int) else _mask(lanes_or_mask)
        out.append((f"global:{name}", ("global", width, m, addrs, "")))

    last = ws - 1
    # line window: at most 64 spanned lines
    gl("lines 0, 63", 4, [0, last], [B, B + 63 * 128])
    gl("lines 0, 64", 4, [0, last], [B, B + 64 * 128])
    gl("lines 63, 0 (far lane first)", 4, [0, last], [B + 63 * 128 + 124, B])
    gl("line 62 spilling into 63", 8, [0, last], [B, B + 62 * 128 + 124])
    gl("line 63 spilling into 64", 8, [0, last], [B, B + 63 * 128 + 124])
    if ws == 64:
        gl("all 64 lines", 4, full, (B, 128))
        gl("65 lines: 64 lanes of 16 bytes at offset 120", 16, full, (B + 120, 128))
    else:
        gl("all 64 lines from 32 lanes", 16, full, (B + 120, 256))
        gl("65 lines from 32 lanes", 16, full, [B + 120 + 256 * l + (128 if l == last else 0) for l in range(ws)])
    gl("96 lines, three per lane: the lowest 64 kept", 200, full & 0xFFFFFFFF, (B + 100, 384))
    gl("descending lanes, 3 lines each", 255, full, (B + 127 + 63 * 256, -256))
    # tile boundary of the two 32-line tiles
    gl("only lines 31, 32", 4, [0, last], [B + 31 * 128 + 40, B + 32 * 128 + 100])
    gl("lines 0, 31, 32, 63", 4, [0, 1, 2, last], [B + 96, B + 31 * 128 + 64, B + 32 * 128 + 32, B + 63 * 128])
    gl("lines 0, 32", 4, [0, 1], [B, B + 32 * 128])
    gl("lines 0, 31", 4, [0, 1], [B, B + 31 * 128])
    gl("lines 32, 0, 33, 1 (unsorted lanes)", 4, [0, 1, 2, 3], [B + 32 * 128, B, B + 33 * 128 + 64, B + 128 + 96])
    rng = random.Random(1234 + ws)
    for k in range(6):
        lines = [rng.randrange(64) for _ in range(ws)]
        gl(f"random subset of the 64 lines #{k}", rng.choice((1, 2, 4)), full,
           [B + 128 * ln + rng.randrange(0, 125) for ln in lines])
    # lines per lane (device: at most 2)
    gl("width 128 at offset 1", 128, [0], [B + 1])
    gl("width 129 aligned", 129, [0], [B])
    gl("width 128 aligned", 128, [0], [B])
    gl("width 255 aligned", 255, [0], [B])
    gl("width 130 at offset 127", 130, [0], [B + 127])
    gl("width 255 at offset 127", 255, [0], [B + 127])
    gl("width 130 at offset 127 on one lane of many", 130, full, [B + (127 if l == 5 else 0) for l in range(ws)])
    # bytes: summed over the lanes, clamped to 128
    gl("every lane on one 4-byte address", 4, full, [B + 64] * ws)
    gl("every lane on one 8-byte address", 8, full, (B + 32, 0))
    gl("every lane 128 bytes of one line", 128, full, [B] * ws)
    gl("31 lanes of 4 bytes: 124", 4, _mask(range(31)), (B, 4))
    gl("one byte in each sector", 1, [0, 1, 2, 3], [B, B + 32 + 5, B + 64 + 31, B + 127])
    gl("sectors 1 and 2 only", 2, [0], [B + 63])
    gl("sector 3 and the next line's sector 0", 2, [0], [B + 127])
    # address forms and masks
    gl("empty mask", 4, 0, [])
    gl("empty mask, stride form", 4, 0, (B, 4))
    for l in (0, 31, 32, 63):
        if l < ws:
            gl(f"only lane {l}", 4, [l], [B + 4 * l])
    half = int("10" * 32, 2) & full
    gl("stride 4", 4, full, (B, 4))
    gl("stride 4, partial mask", 4, half, (B, 4))
    gl("stride 16 from an unaligned base", 16, full, (B + 1, 16))
    gl("stride 132", 4, full, (B + 1, 132))
    gl("negative stride", 4, full, (B + 63 * 128, -128))
    gl("negative stride, partial mask", 8, half, (B + 4096, -136))
    gl("stride 0", 4, half, (B + 1, 0))
    gl("base 1 << 63", 8, full, ((1 << 63) + 124, 8))
    gl("base just below 1 << 48", 4, full, ((1 << 48) - 8192 + 2, 128))
    if ws == 32:
        # mask bits at and above the warp size carry addresses but are not active
        gl("mask bits above the warp size", 4, (1 << 40) | 0x80000001, [B, B + 128, B + 64 * 128])
    return out


def _random_shared(cfg, rng, ops):
    op = rng.choice(ops)
    nb, groups = cfg.table(op)
    ws = cfg.ws
    mask = rng.choice(((1 << ws) - 1, rng.getrandbits(ws), rng.getrandbits(ws) & rng.getrandbits(ws))) or 1
    active = [l for l in range(ws) if mask >> l & 1]
    width = rng.choice((1, 2, 4, 4, 8, 8, 12, 16, 16, 28, 29, 32, 33))
    # the row span of one group / part from the window's edges or a small range
    span = rng.choice((254, 255, 255, 256, 256, 257, rng.randrange(0, 9), rng.randrange(0, 9)))
    g = sorted(set(rng.choice(groups)) & set(active))
    r0 = rng.randrange(0, 1 << 30)
    rows = {l: r0 + rng.randrange(0, min(span, 255) + 1) for l in active}
    if len(g) >= 2:
        lo, hi = rng.sample(g, 2)
        rows[lo], rows[hi] = r0, r0 + span
    nbanks = rng.choice((nb, nb, 4, 1))
    addrs = [(rows[l] * nb + rng.randrange(nbanks)) * 4 + rng.randrange(4) for l in active]
    return ("shared", width, mask, addrs, op)


def _random_global(cfg, rng):
    ws = cfg.ws
    mask = rng.choice(((1 << ws) - 1, rng.getrandbits(ws), rng.getrandbits(ws) & rng.getrandbits(ws))) or 1
    active = [l for l in range(ws) if mask >> l & 1]
    width = rng.choice((1, 2, 4, 4, 4, 8, 8, 16, 16, 32, 64, 128, 129, 200))
    span = rng.choice((62, 63, 63, 64, 64, 65, rng.randrange(0, 9), rng.randrange(0, 9)))
    base = (rng.randrange(1, 1 << 40) << 7)
    lines = {l: rng.randrange(0, span + 1) for l in active}
    if len(active) >= 2:
        lo, hi = rng.sample(active, 2)
        lines[lo], lines[hi] = 0, span
    offs = rng.choice((0, 0, 127))  # aligned lanes, or lanes that may spill into the next line
    addrs = [base + 128 * lines[l] + rng.randrange(0, offs + 1) for l in active]
    return ("global", width, mask, addrs, "")


N_RANDOM = 1500


def random_cases(cfg, name):
    rng = random.Random(f"ingest-oracle-{name}")
    ops = sorted(LDS_TABLE) if cfg.groups else [""]
    out = []
    # every second instruction is a shared one; every fourth where all of them go to the host, so
    # that the device side of the set stays populated
    every = 2 if cfg.nb in (32, 64) and not cfg.lbcast else 4
    for i in range(N_RANDOM):
        inst = _random_shared(cfg, rng, ops) if i % every == 1 else _random_global(cfg, rng)
        out.append((f"random #{i} {inst[4]}", inst))
    return out


_CASES = {}


def cases(name):
    """the explicit and the random cases of one configuration with their oracle results, computed once"""
    if name not in _CASES:
        cfg = CONFIGS[name]
        ex = []
        for op in (sorted(LDS_TABLE) if cfg.groups else [""]):
            ex += shared_cases(cfg, op)
        ex += global_cases(cfg)
        rnd = random_cases(cfg, name)
        both = ex + rnd
        _CASES[name] = dict(names=[n for n, _ in both], insts=[i for _, i in both], n_explicit=len(ex),
                            want=[oracle(cfg, i) for _, i in both], place=[on_device(cfg, i) for _, i in both])
    return _CASES[name]


# ----------------------------------------------------------------------------
# comparison: a failure names the instruction, its pattern and the field
FIELDS = ("line", "sectors", "bytes", "bank")


def first_difference(got, want):
    """None, or (field, got, want) of the first differing field of one instruction's result"""
    if got[0] != want[0]:
        return ("space", got[0], want[0])
    if got[1] != want[1]:
        return ("width", got[1], want[1])
    ga, wa = [tuple(a) for a in got[2]], [tuple(a) for a in want[2]]
    for q, (g, w) in enumerate(zip(ga, wa)):
        for f, gv, wv in zip(FIELDS, g, w):
            if gv != wv:
                return (f"access {q} {f}", hex(gv), hex(wv))
    if len(ga) != len(wa):
        return ("accesses", len(ga), len(wa))
    return None


def assert_results(who, got, want, names, insts, skip=lambda inst: False):
    assert len(got) == len(want), (who, len(got), len(want))
    bad = []
    for i, (g, w) in enumerate(zip(got, want)):
        if skip(insts[i]):
            continue
        d = first_difference(g, w)
        if d:
            bad.append(f"instruction {i} [{names[i]}] {d[0]}: {who} {d[1]}, expected {d[2]}")
    assert not bad, f"{len(bad)} of {len(want)} differ:\n" + "\n".join(bad[:20])


def _lbcast_shared(cfg):
    # limited broadcast is outside the oracle's contract: device == host and placement only
    return (lambda inst: inst[0] == "shared") if cfg.lbcast else (lambda inst: False)


# ----------------------------------------------------------------------------
# CPU: host == oracle
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_host_equals_oracle(native, name):
    cfg, c = CONFIGS[name], cases(name)
    r = native.ingest_lanes_result(c["insts"], cfg.args(), -1)
    assert r["ran"] is False and "device" not in r
    assert_results("host", r["host"], c["want"], c["names"], c["insts"], skip=_lbcast_shared(cfg))


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_cases_populate_both_sides_of_the_windows(name):
    """a condition on the inputs: the oracle's placement predicate puts at least a quarter of the
    random set on the device and a quarter on the host (so an edge that moved shows)"""
    cfg, c = CONFIGS[name], cases(name)
    n0 = c["n_explicit"]
    place, insts = c["place"][n0:], c["insts"][n0:]
    assert len(place) == N_RANDOM
    dev = sum(place)
    assert dev >= N_RANDOM // 4 and N_RANDOM - dev >= N_RANDOM // 4, (dev, N_RANDOM)
    for space in ("shared", "global"):
        p = [x for x, i in zip(place, insts) if i[0] == space]
        if space == "shared" and (cfg.nb not in (32, 64) or cfg.lbcast):
            assert not any(p)  # every shared instruction goes to the host
            assert not any(x for x, i in zip(c["place"][:n0], c["insts"][:n0]) if i[0] == "shared")
        else:
            assert sum(p) >= len(p) // 4 and len(p) - sum(p) >= len(p) // 4, (space, sum(p), len(p))


def test_explicit_window_edges_are_where_the_contract_puts_them():
    """the predicate itself on the edges the header comment of ingest_mfma.hip names"""
    c = cases("mi355x")
    where = dict(zip(c["names"], c["place"]))
    for op in ("ds_read_b32", "ds_read_b128", "ds_write_b96"):
        assert where[f"{op}:rows differ by 255"] and not where[f"{op}:rows differ by 256"]
        assert where[f"{op}:last word in row +255"] and not where[f"{op}:last word in row +256"]
        assert where[f"{op}:1 MiB apart, different groups"] and not where[f"{op}:1 MiB apart, one group"]
        assert where[f"{op}:words per lane: w29 at 3"] and not where[f"{op}:words per lane: w32 at 1"]
    assert where["global:lines 0, 63"] and not where["global:lines 0, 64"]
    assert where["global:line 62 spilling into 63"] and not where["global:line 63 spilling into 64"]
    assert where["global:all 64 lines"] and not where["global:65 lines: 64 lanes of 16 bytes at offset 120"]
    assert where["global:width 129 aligned"] and not where["global:width 130 at offset 127"]
    want = dict(zip(c["names"], c["want"]))
    assert want["global:all 64 lines"][1] == K_MAX_ACCESS
    kept = want["global:65 lines: 64 lanes of 16 bytes at offset 120"]
    assert kept[1] == K_MAX_ACCESS and [a[0] for a in kept[2]] == [GBASE + 128 * i for i in range(64)]
    assert want["global:every lane 128 bytes of one line"][2] == [(GBASE, 0xF, 128, (GBASE >> 7) % L1_BANKS)]
    assert want["ds_read_b32:bank 0 rows 0..7"][1] == 8 and want["ds_read_b128:bank 63 rows 0..7"][1] == 8


def test_bad_input(native):
    args = CONFIGS["qv100"].args()
    with pytest.raises(ValueError):  # three active lanes, two addresses
        native.ingest_lanes_result([("shared", 4, 0x7, [0, 4], "")], args, -1)
    with pytest.raises(ValueError):
        native.ingest_lanes_result([("global", 4, 0x1, [], "")], args, -1)
    for stride in (1 << 31, -(1 << 31) - 1, 1 << 70):
        with pytest.raises(ValueError):
            native.ingest_lanes_result([("global", 4, 0xF, (4096, stride), "")], args, -1)
    with pytest.raises(ValueError):
        native.ingest_lanes_result([("global", 256, 0xF, (4096, 4), "")], args, -1)
    with pytest.raises(ValueError):
        native.ingest_lanes_result([("texture", 4, 0xF, (4096, 4), "")], args, -1)
    # the int32 limits themselves are accepted
    lim = [("global", 4, 0x3, (1 << 40, (1 << 31) - 1), ""), ("global", 4, 0x3, (1 << 40, -(1 << 31)), "")]
    r = native.ingest_lanes_result(lim, args, -1)
    assert_results("host", r["host"], [oracle(CONFIGS["qv100"], i) for i in lim], ["stride max", "stride min"], lim)
    assert r["host"][1][2][0][0] == (1 << 40) - (1 << 31)


# ----------------------------------------------------------------------------
# the 65,536-job batch loop: one- and two-lane instructions, line-crossing
# global ones on both sides of the batch boundary
K_BATCH = 1 << 16


def batch_insts():
    out = []
    for i in range(K_BATCH + 70):
        k = i % 4
        if k == 0:    # two lanes, the second one crossing into the next line: 3 accesses
            out.append(("global", 8, 0x5, [GBASE + 256 * i, GBASE + 256 * i + 1148], ""))
        elif k == 1:  # one lane crossing a line: 2 accesses
            out.append(("global", 16, 0x2, (GBASE + 128 * i + 120, 0), ""))
        elif k == 2:  # two lanes, one bank, two rows
            out.append(("shared", 4, 0x3, [(i % 32) * 4, (i % 32) * 4 + 128 * (1 + i % 7)], ""))
        else:         # one lane
            out.append(("shared", 8, 0x1, (i * 4 % 4096, 0), ""))
    return out


SMALL3 = [("global", 4, 0x3, [GBASE, GBASE + 4096], ""), ("shared", 4, 0x3, [0, 128], ""),
          ("global", 8, 0x1, [GBASE + 124], "")]

_BATCH = {}


def batch_case():
    if not _BATCH:
        cfg = CONFIGS["qv100"]
        insts = batch_insts()
        _BATCH.update(insts=insts, names=[f"batch #{i}" for i in range(len(insts))],
                      want=[oracle(cfg, i) for i in insts], small=[oracle(cfg, i) for i in SMALL3])
    return _BATCH


def test_batch_host_equals_oracle(native):
    b = batch_case()
    # both sides of the batch boundary hold line-crossing global instructions
    assert b["want"][K_BATCH - 4][1] == 3 and b["want"][K_BATCH][1] == 3 and b["want"][K_BATCH + 1][1] == 2
    r = native.ingest_lanes_result(b["insts"], CONFIGS["qv100"].args(), -1)
    assert_results("host", r["host"], b["want"], b["names"], b["insts"])


# ----------------------------------------------------------------------------
# GPU: device == host == oracle, placement == the documented windows
@pytest.fixture(scope="module")
def gpu_native():
    import torch  # bind torch's HIP runtime first
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    from accel_sim_framework_distributed_amd import _native
    mod = _native.load(prefer_torch_runtime=True)
    assert mod.gpu_available(), "HIP device not usable (native code must run, no silent fallback)"
    return mod


def assert_placement(got, want, names):
    bad = [f"instruction {i} [{names[i]}] ran on the {'device' if g else 'host'}, the windows say "
           f"{'device' if w else 'host'}" for i, (g, w) in enumerate(zip(got, want)) if bool(g) != bool(w)]
    assert len(got) == len(want) and not bad, f"{len(bad)} misplaced:\n" + "\n".join(bad[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_device_equals_oracle(gpu_native, name):
    cfg, c = CONFIGS[name], cases(name)
    r = gpu_native.ingest_lanes_result(c["insts"], cfg.args(), 0)
    assert r["ran"], "the device coalescer did not run"
    assert_results("host", r["host"], c["want"], c["names"], c["insts"], skip=_lbcast_shared(cfg))
    assert_results("device", r["device"], c["want"], c["names"], c["insts"], skip=_lbcast_shared(cfg))
    assert_results("device", r["device"], r["host"], c["names"], c["insts"])
    assert_placement(r["on_device"], c["place"], c["names"])
    # the counters agree with the per-instruction flags
    dev = sum(r["on_device"])
    assert r["smem_device"] + r["gmem_device"] == dev
    assert r["smem_host"] + r["gmem_host"] == len(c["insts"]) - dev
    assert r["mfma"] > 0


@pytest.mark.gpu
def test_batch_loop_and_buffer_reuse(gpu_native):
    """65,536 + 70 jobs: the second batch's access offsets are rebased; a 3-instruction call before
    and after grows the thread's device buffers and then reuses them with a reset cursor"""
    b = batch_case()
    args = CONFIGS["qv100"].args()
    small_names = ["small #0", "small #1", "small #2"]
    for when in ("before", "after"):
        r = gpu_native.ingest_lanes_result(SMALL3, args, 0)
        assert r["ran"]
        assert_results(f"device ({when} the large call)", r["device"], b["small"], small_names, SMALL3)
        assert r["on_device"] == [1, 1, 1]
        if when == "before":
            big = gpu_native.ingest_lanes_result(b["insts"], args, 0)
            assert big["ran"]
            assert_results("device", big["device"], b["want"], b["names"], b["insts"])
            assert_results("host", big["host"], b["want"], b["names"], b["insts"])
            assert all(big["on_device"]) and len(big["on_device"]) == K_BATCH + 70

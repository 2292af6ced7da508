"""Seeded random kernels and model configurations for differential tests.

``kernel(seed)`` is a random straight-line warp program on ``KernelBuilder``;
``config(seed)`` is a random set of QV100 option overrides.  A *case* is two
kernels (``seed`` and ``seed + 500``) in one application, simulated under
``config(seed)``.  ``CASES`` pins the cases the suite runs (tests/
test_fuzz_engines.py: CPU engine self-consistency, GPU engine == CPU engine;
tests/test_engine_builds.py: every engine kernel build).

Everything is a pure function of the seed (numpy ``default_rng``), so a case
names the same trace and options everywhere; tests/test_fuzz_engines.py holds
a golden hash of one case's arrays.
"""
from __future__ import annotations

import hashlib
from typing import Dict, List, NamedTuple, Tuple

import numpy as np

from .builder import KernelBuilder
from .format import KernelArrays

SCHEDULERS = ("lrr", "gto", "old", "rrr", "two_level_active:4:0:1", "warp_limiting:2:2")
DL1 = {
    "write_through": "S:4:128:64,L:T:m:L:L,A:512:8,16:0,32",
    "write_back": "S:4:128:64,L:B:m:L:L,A:512:8,16:0,32",
    "fetch_on_write": "S:4:128:64,L:T:m:F:L,A:512:8,16:0,32",
    "small_unsectored": "N:8:128:4,L:T:m:L:L,A:64:8,16:0,32",
}
DL2 = {
    "default": "S:32:128:24,L:B:m:L:P,A:192:4,32:0,32",
    "no_write_alloc": "S:32:128:24,L:B:m:N:P,A:192:4,32:0,32",
    "tiny_4x4": "S:4:128:4,L:B:m:L:P,A:192:4,32:0,32",
}
STRIDES_GLOBAL = (0, 4, 8, 32, 64, 128, 132)
STRIDES_SHARED = (4, 8, 128)
BLOCKS = (32, 48, 64, 96, 100, 128, 160, 192, 250, 256, 320, 384, 500, 512)

# mnemonic per role: SASS (warp 32, binary_version 70) and CDNA4 (wave64, 950)
_SASS = dict(sp="FFMA", int="IMAD", dp="DFMA", sfu="MUFU.RCP", tensor="HMMA.1688.F32", ldg="LDG.E", stg="STG.E",
             lds="LDS", sts="STS", ldl="LDL", ldc="LDC", atom="ATOMG.E.ADD.STRONG.GPU", bar="BAR.SYNC",
             membar="MEMBAR.GL", exit="EXIT")
_CDNA = dict(sp="v_fma_f32", int="s_add_u32", dp="v_fma_f64", sfu="v_sqrt_f32", tensor="v_mfma_f32_32x32x16_bf16",
             ldg="global_load_dword", stg="global_store_dword", lds="ds_read_b32", sts="ds_write_b32",
             ldl="global_load_dwordx2", ldc="s_load_dwordx2", atom="global_atomic_add", bar="s_barrier",
             membar="s_waitcnt", exit="s_endpgm")
_ALU = ("sp", "int", "dp", "sfu", "tensor")
_KINDS = _ALU + ("ldg", "ldg", "ldg_list", "stg", "lds", "sts", "ldl", "ldc", "atom", "bar", "membar")


def kernel(seed: int, wave64: bool = False, ctas: int | None = None) -> KernelArrays:
    """Random straight-line program: 12-40 ops of every unit class and memory
    space, random per-warp active masks (~30 % of the ops) and per-warp
    ``present`` (~20 %, never on a barrier), 3-40 CTAs of 32-512 threads."""
    rng = np.random.default_rng(int(seed))
    isa = _CDNA if wave64 else _SASS
    lanes = 64 if wave64 else 32
    ncta = int(rng.integers(3, 41)) if ctas is None else int(ctas)
    threads = int(BLOCKS[int(rng.integers(0, len(BLOCKS)))])
    k = KernelBuilder(f"fuzz_{seed}", (ncta, 1, 1), (threads, 1, 1), shmem=16384, nregs=int(rng.choice((16, 32, 64))),
                      binary_version=950 if wave64 else 70, warp_size=lanes)
    g = k.g
    n = g.nwarps
    nops = int(rng.integers(12, 41))
    kinds = list(_ALU) + [_KINDS[int(i)] for i in rng.integers(0, len(_KINDS), nops - len(_ALU))]
    kinds = [kinds[int(i)] for i in rng.permutation(len(kinds))]
    gtid = g.gtid0.astype(np.int64)
    lane_ix = np.arange(lanes, dtype=np.int64)[None, :]
    for kind in kinds:
        reg = lambda: int(rng.integers(2, 14))
        mask = present = None
        if rng.random() < 0.3:
            mask = rng.integers(0, 1 << 63, n, dtype=np.uint64) | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))
        if rng.random() < 0.2:
            present = rng.random(n) < 0.8
        kw = dict(mask=mask, present=present)
        if kind in _ALU or kind == "ldc":
            k.op(isa[kind], [reg()], [reg(), reg()], **kw)
        elif kind in ("ldg", "stg"):
            stride = int(STRIDES_GLOBAL[int(rng.integers(0, len(STRIDES_GLOBAL)))])
            region = 0x7000_0000 + 0x0100_0000 * int(rng.integers(0, 4))
            base = region + gtid * max(stride, 4)
            if kind == "ldg":
                k.op(isa["ldg"], [reg()], [reg()], base=base, stride=stride, **kw)
            else:
                k.op(isa["stg"], [], [reg(), reg()], base=base, stride=stride, **kw)
        elif kind == "ldg_list":
            addrs = 0x7800_0000 + 4 * rng.integers(0, 1 << 16, (n, lanes), dtype=np.int64)
            k.op(isa["ldg"], [reg()], [reg()], addrs=addrs.astype(np.uint64), **kw)
        elif kind in ("lds", "sts"):
            stride = int(STRIDES_SHARED[int(rng.integers(0, len(STRIDES_SHARED)))])
            base = (g.warp.astype(np.int64) * 128) % 4096
            if kind == "lds":
                k.op(isa["lds"], [reg()], [reg()], base=base, stride=stride, **kw)
            else:
                k.op(isa["sts"], [], [reg()], base=base, stride=stride, **kw)
        elif kind == "ldl":
            # per-thread private words (the wave64 table has no local space: a
            # second global load shape stands in)
            base = (k.header["local_base"] if not wave64 else 0x7C00_0000) + gtid * 8
            k.op(isa["ldl"], [reg()], [reg()], base=base, stride=8 if wave64 else 4, **kw)
        elif kind == "atom":
            nlines = int(rng.integers(1, 5))
            addrs = 0x7F00_0000 + 128 * rng.integers(0, nlines, (n, lanes), dtype=np.int64) + 4 * (lane_ix % 32)
            k.op(isa["atom"], [reg()], [reg(), reg()], addrs=addrs.astype(np.uint64), **kw)
        elif kind == "bar":
            k.op(isa["bar"])  # every warp of the CTA, or the CTA would never leave it
        else:
            k.op(isa["membar"], present=present)
    k.op(isa["exit"])
    return k.build()


def config(seed: int) -> Dict[str, str]:
    """Random QV100 ``extra`` options (scheduler, topology, caches, DRAM, core)."""
    rng = np.random.default_rng(100_003 + int(seed))
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]
    return {
        "-gpgpu_n_clusters": str(int(rng.integers(2, 9))),
        "-gpgpu_n_cores_per_cluster": str(int(rng.integers(1, 3))),
        "-gpgpu_n_mem": str(int(rng.integers(1, 9))),
        "-gpgpu_n_sub_partition_per_mchannel": str(int(rng.integers(1, 3))),
        "-gpgpu_scheduler": pick(SCHEDULERS),
        "-gpgpu_max_insn_issue_per_warp": str(int(rng.integers(1, 3))),
        "-gpgpu_memory_partition_indexing": str(int(rng.integers(0, 5))),
        "-gpgpu_cache:dl1": DL1[pick(sorted(DL1))],
        "-gpgpu_cache:dl2": DL2[pick(sorted(DL2))],
        "-gpgpu_dram_scheduler": str(int(rng.integers(0, 2))),
        "-gpgpu_perfect_inst_const_cache": str(int(rng.integers(0, 2))),
        "-gpgpu_operand_collector_num_units_gen": pick(("2", "8")),
        "-gpgpu_num_reg_banks": pick(("4", "16")),
        "-gpgpu_perf_sim_memcpy": "0",
    }


class Case(NamedTuple):
    seed: int
    preset: str = "QV100"

    @property
    def id(self) -> str:
        return f"{self.preset.lower()}_{self.seed}"


def case_kernels(case: Case) -> List[KernelArrays]:
    if case.preset == "MI355X":  # the whole 256-CU preset: wave64 kernels of 64 workgroups
        return [kernel(case.seed, wave64=True, ctas=64), kernel(case.seed + 500, wave64=True, ctas=64)]
    return [kernel(case.seed), kernel(case.seed + 500)]


def case_config(case: Case) -> Tuple[str, Dict[str, str]]:
    """(preset name, extra options) of a case."""
    if case.preset == "MI355X":
        return "MI355X", {"-gpgpu_perf_sim_memcpy": "0"}
    return "QV100", config(case.seed)


def write_case(out_dir: str, case: Case) -> str:
    """Write the case's application; returns its kernelslist.g."""
    from . import rodinia
    return rodinia.write_app(out_dir, case_kernels(case), memcpy=False)


def arrays_sha256(kernels: List[KernelArrays]) -> str:
    h = hashlib.sha256()
    for k in kernels:
        for a in (k.insts, k.mems, k.addrs, k.streams):
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# Pinned cases: chosen so that every option value of config() is drawn at least
# once and every case finishes in <= 60,000 simulated cycles on the CPU engine
# (both asserted by tests/test_fuzz_engines.py).
CASES: List[Case] = [Case(s) for s in (0, 2, 9, 16, 20, 22, 23, 24, 30, 35, 36, 43, 47)] + [Case(2, "MI355X")]
# the two cases every engine build is run on (tests/test_engine_builds.py):
# two cores per cluster with a sector-less L1, and gto with partition hash 4
BUILD_CASES: List[Case] = [Case(2), Case(23)]

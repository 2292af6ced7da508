"""Recorded results of the router model (tests/golden/router_pins.json).

The serial pass (rt_simulate) and the lane-parallel pass (rt_simulate_par)
share their routing, VC, allocator and traversal code, so comparing one with
the other does not check that code.  These pins do: every digest was recorded
from the build of the commit the fixture names, and both passes must still
give it.

  open loop   every case of tests/test_icnt_sweep.py (CASES, the two anynet
              networks, MECH_POINTS): per point a SHA-256 over the arrivals,
              the final state words, deadlocked, the seven activity counters
              and the rest of the result dict; engines cpu and cpu-par
  epoch pass  every case of tests/test_router_pass_par.py on the CPU engine:
              cycles, the five link / injection / deadlock statistics and the
              SHA-256 of the state image; -sim_router_pass serial and par

Three epoch-pass cases pin no more than `mesh` does: `mesh_min_adapt`,
`mesh_sep_input_first` and `mesh_sep_output_first` end with the statistics and
the state image of `mesh`: with this kernel's traffic the options make no
difference.  Adaptive routing and the separable allocators are pinned by the
open-loop cases `min_adapt`, `alloc_separable_input_first` and
`alloc_separable_output_first` only.

The device is pinned through these: the gpu tests of those two modules compare
it with the CPU result of the same run.

    python tests/test_router_pins.py --record     # rewrite the fixture from the current build
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_icnt_sweep as sweep
import test_router_pass_par as rpass

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "router_pins.json")


def _digest(r):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(r["arrivals"], dtype=np.uint64).tobytes())
    h.update(np.ascontiguousarray(r["state"], dtype=np.uint64).tobytes())
    act = r["activity"]
    assert len(act) == 7
    rest = {k: v for k, v in r.items() if k not in ("arrivals", "state", "deadlocked", "activity")}
    h.update(json.dumps([r["deadlocked"], sorted(dict(act).items()), rest], sort_keys=True).encode())
    return h.hexdigest()


def _open_loop_cases(tmp_path):
    """name -> (.icnt text, points)"""
    cases = {name: (sweep._icnt(**keys), points) for name, (keys, points) in sweep.CASES.items()}
    for i, (text, points) in enumerate(sweep._anynet(tmp_path)):
        cases[f"anynet{i}"] = (text, points)
    cases["mech"] = (sweep._icnt(**sweep.MECH_KEYS), sweep.MECH_POINTS)
    return cases


def _open_loop(native, text, points, engine):
    res = sweep._batch(native, text, points, engine)
    return [dict(sha256=_digest(r), packets=r["packets"], deadlocked=r["deadlocked"]) for r in res]


def _epoch(native, work, case, mode):
    res, snap, _ = work.run(native, case, "cpu", mode)
    return dict(cycles=res[0], stats=dict(zip(rpass.STAT_KEYS, res[1:])), state_sha256=hashlib.sha256(snap).hexdigest())


def _check_not_empty(pins):
    """A pin must not hide an empty run."""
    for name, pts in pins["open_loop"].items():
        for i, p in enumerate(pts):
            if name == "mech" and i == 1:  # the deliberate rate-0 point
                assert p["packets"] == 0
            else:
                assert p["packets"] > 0, (name, i)
    assert pins["open_loop"]["deadlock"][0]["deadlocked"] > 0
    for name, e in pins["epoch"].items():
        s = e["stats"]
        assert s["Network_link_delayed_packets"] > 0 or s["Network_link_wait_cycles"] > 0, name


@pytest.fixture(scope="module")
def pins():
    with open(PINS) as f:
        p = json.load(f)
    _check_not_empty(p)
    return p


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return rpass._Work(tmp_path_factory.mktemp("router_pins"))


@pytest.fixture(scope="module")
def open_loop_cases(tmp_path_factory):
    return _open_loop_cases(tmp_path_factory.mktemp("router_pins_anynet"))


def test_pins_cover_every_case(pins, open_loop_cases):
    assert sorted(pins["open_loop"]) == sorted(open_loop_cases)
    assert len(sweep.CASES) == 19 and len(pins["open_loop"]) == 22
    for name, (_, points) in open_loop_cases.items():
        assert len(pins["open_loop"][name]) == len(points), name
    assert sorted(pins["epoch"]) == sorted(rpass.CASES)


@pytest.mark.parametrize("engine", ["cpu", "cpu-par"])
@pytest.mark.parametrize("name", sorted(sweep.CASES) + ["anynet0", "anynet1", "mech"])
def test_open_loop_pin(native, pins, open_loop_cases, name, engine):
    text, points = open_loop_cases[name]
    assert _open_loop(native, text, points, engine) == pins["open_loop"][name]


@pytest.mark.parametrize("mode", ["serial", "par"])
@pytest.mark.parametrize("case", list(rpass.CASES))
def test_epoch_pass_pin(native, pins, work, case, mode):
    assert _epoch(native, work, case, mode) == pins["epoch"][case]


def _record():
    import pathlib
    import subprocess
    import tempfile
    from accel_sim_framework_distributed_amd import _native
    native = _native.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    commit = subprocess.run(["git", "-C", root, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    with tempfile.TemporaryDirectory(prefix="router_pins_") as tmp:
        tmp = pathlib.Path(tmp)
        work = rpass._Work(tmp)
        rec = dict(recorded_from=commit,
                   open_loop={name: _open_loop(native, text, points, "cpu")
                              for name, (text, points) in _open_loop_cases(tmp).items()},
                   epoch={case: _epoch(native, work, case, "serial") for case in rpass.CASES})
    _check_not_empty(rec)
    with open(PINS, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", PINS, "from", commit)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_router_pins.py --record")
    _record()

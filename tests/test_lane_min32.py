"""The lane policy's order-free minimum (SeqPar::min32 / WavePar::min32):
value i is folded into slot m[i] of 64 words; both policies must leave every
slot at the minimum of its values (0xffffffff where none landed)."""
import random

import pytest

EMPTY = 0xFFFFFFFF


def _cases():
    rnd = random.Random(7)
    out = []
    # nothing, one lane, a full wave on one slot, more than one stride, ties, every slot
    shapes = [(0, 1), (1, 1), (64, 1), (65, 3), (200, 7), (4096, 64), (300, 64)]
    for n, slots in shapes:
        vals = [rnd.choice([rnd.getrandbits(32), rnd.randrange(8), EMPTY, 0]) for _ in range(n)]
        idx = [rnd.randrange(slots) for _ in range(n)]
        want = [EMPTY] * 64
        for v, s in zip(vals, idx):
            want[s] = min(want[s], v)
        out.append((n, vals, idx, want))
    return out


def test_seqpar_min32(native):
    for n, vals, idx, want in _cases():
        assert list(native.lane_policy_check("min32", n, vals, idx)["seq"]) == want


def test_min32_validates(native):
    with pytest.raises(ValueError):
        native.lane_policy_check("min32", 2, [1, 2], [0, 64])
    with pytest.raises(ValueError):
        native.lane_policy_check("min32", 2, [1, 2], [0])


@pytest.mark.gpu
def test_wavepar_min32():
    import torch  # bind torch's HIP runtime first
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    from accel_sim_framework_distributed_amd import _native
    native = _native.load(prefer_torch_runtime=True)
    for n, vals, idx, want in _cases():
        r = native.lane_policy_check("min32", n, vals, idx)
        assert r["ran"], "no device: the WavePar kernel did not run"
        assert list(r["seq"]) == want and list(r["wave"]) == want

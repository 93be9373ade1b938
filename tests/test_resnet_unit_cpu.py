"""Pins tests/resnet_unit.py (no GPU): the recorded noise floors r0 are what the oracle measures, and the bound 2 r0 that
tests/test_resnet_gpu.py::test_bottleneck_unit_matches_the_oracle holds the device to is one a wrong shortcut gradient exceeds."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet_unit as RU  # noqa: E402

CASES = [(k, t) for k in RU.UNITS for t in (False, True)]


@pytest.mark.parametrize("kind,training", CASES, ids=["%s-%s" % (k, "train" if t else "infer") for k, t in CASES])
def test_bound_is_twice_the_measured_floor_and_a_wrong_shortcut_gradient_exceeds_it(kind, training):
    """r0: float64 against 16-bit storage emulation, worst tensor over five seeds (recorded to four digits; re-measured here within a tenth,
    the room another CPU's summation order may take).  Then, per seed, the float64 unit with the shortcut's gradient dropped and doubled: the
    input gradient and the projection kernel's gradient must each be further from the true ones than the bound."""
    r0 = 0.0
    sk = RU.shortcut_kernel(kind)
    far = []
    for seed in RU.SEEDS:
        P, x, dy = RU.make_case(kind, seed)
        ref = RU.oracle_unit(kind, training, P, x, dy)
        assert len(ref) == 2 + len(RU.trainable(P)) == 2 + (12 if sk else 9)
        assert all(float(v.abs().sum()) > 0 for v in ref.values())
        r0 = max(r0, max(RU.errors(RU.oracle_unit(kind, training, P, x, dy, emulate=True), ref).values()))
        same = RU.oracle_unit(kind, training, P, x, dy, shortcut_scale=1.0)
        assert all(torch.equal(same[n], ref[n]) for n in ref), "the restated unit is not the oracle unit"
        for scale in (0.0, 2.0):
            e = RU.errors(RU.oracle_unit(kind, training, P, x, dy, shortcut_scale=scale), ref)
            far.append(e["dx"])
            assert e["dx"] > RU.bound(kind, training), (seed, scale, e["dx"])
            if sk:
                assert e[sk] > RU.bound(kind, training), (seed, scale, e[sk])
            assert e["out"] == 0.0
    print(kind, training, "r0 %.5f recorded %.5f bound %.5f; wrong shortcut gradient: dx off by >= %.3f" % (r0, RU.R0[(kind, training)], RU.bound(kind, training), min(far)))
    assert abs(r0 - RU.R0[(kind, training)]) <= 0.1 * RU.R0[(kind, training)], (r0, RU.R0[(kind, training)])

"""Pins tests/deform_exact.py itself (no GPU): every case's references meet the exactness limits the equality tests of
tests/test_deform_exact_gpu.py rest on, every case samples each knife-edge class, and the oracle gives the same numbers in float64 and
float32 on these inputs (which the exactness argument implies, and which guards the oracle's own dtype handling)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deform_exact as DE  # noqa: E402
from oracle import deform as OD  # noqa: E402

F64 = torch.float64
NAMES = [c.name for c in DE.CASES]


def test_case_table_covers_the_shapes_each_kernel_can_go_wrong_at():
    shapes = {(c.H, c.W) for c in DE.CASES if c.C // c.dg == 64 and c.dil == 1}
    assert shapes == {(5, 5), (8, 16), (9, 17), (17, 33)}
    for hw in shapes:
        assert {(c.C, c.dg) for c in DE.CASES if (c.H, c.W) == hw and c.C // c.dg == 64 and c.dil == 1} == {(64, 1), (128, 2), (256, 4)}
    assert {(c.C, c.dg) for c in DE.CASES if c.C // c.dg != 64} == {(128, 4), (256, 2)}
    assert any(c.dil == 2 and c.C // c.dg == 64 for c in DE.CASES)
    assert all(c.N == 2 for c in DE.CASES)
    assert set(DE.CONV_CASES) <= set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_references_meet_the_exactness_limits(name):
    """A condition, not a measurement: seeds and densities of the case table are chosen so that these hold."""
    c = DE.CASE_BY_NAME[name]
    d = DE.check_case(c)
    fc = DE.fwd_conv_data(name)
    print(name, "max |16 y| %d" % (16 * fc.y).abs().max().item())
    print(name, "max |16 col| %d  |4 dOffset| %d  |16 dX| %d  |16 (dX + dx0)| %d" % (
        (16 * d.col).abs().max().item(), (4 * d.doff).abs().max().item(), (16 * d.dx).abs().max().item(), (16 * (d.dx + d.dx0)).abs().max().item()))
    assert d.x.abs().max().item() <= 3 and d.off.abs().max().item() <= 8
    assert set(d.dS.unique().tolist()) == {-1.0, 0.0, 1.0}
    # the gradients are not trivially zero: a kernel that wrote nothing would not pass
    assert (d.dx != 0).float().mean().item() > 0.3 and (d.doff != 0).float().mean().item() > 0.3 and (d.col != 0).float().mean().item() > 0.3


@pytest.mark.parametrize("name", NAMES)
def test_every_knife_edge_class_is_sampled(name):
    c = DE.CASE_BY_NAME[name]
    cen = DE.census(c)
    print(name, dict(cen))
    low = {k: v for k, v in cen.items() if v < DE.MIN_PER_CLASS}
    assert not low, low
    pairs = c.N * c.H * c.W * c.dg * 9
    assert cen["far1"] >= cen["far2"] and cen["far1"] < pairs


def test_census_counts_a_hand_made_map():
    """3 x 4 map, one group: offsets all zero but four planted pairs."""
    H, W = 3, 4
    off = torch.zeros((1, H, W, 18), dtype=F64)
    # output pixel (0, 0), tap 0: nominal (-1, -1)
    off[0, 0, 0, 0], off[0, 0, 0, 1] = 1.0, 1.0          # -> (0, 0): h=0 and w=0
    # output pixel (2, 3), tap 8: nominal (3, 4)
    off[0, 2, 3, 16], off[0, 2, 3, 17] = -0.25, -1.0     # -> (2.75, 3): h=L-0.25, w=L-1, both clamped
    # output pixel (1, 1), tap 4: nominal (1, 1)
    off[0, 1, 1, 8], off[0, 1, 1, 9] = 2.0, -2.0         # -> (3, -1): h=L but w outside: counted by neither edge class
    off[0, 1, 2, 8], off[0, 1, 2, 9] = -0.75, 0.0        # tap 4 of (1, 2) -> (0.25, 2): relative coordinate 1 - 0.75 >= 0
    cen = DE.census_of(off, H, W, 1, 1)
    # the expected counts come from a plain loop over the coordinates (zero offsets put many taps on integer edges too)
    nh, nw = DE.nominal(H, W, 1)
    ch = nh.view(H, 1, 9).expand(H, W, 9).clone()
    cw = nw.view(1, W, 9).expand(H, W, 9).clone()
    ch[0, 0, 0], cw[0, 0, 0] = 0.0, 0.0
    ch[2, 3, 8], cw[2, 3, 8] = 2.75, 3.0
    ch[1, 1, 4], cw[1, 1, 4] = 3.0, -1.0
    ch[1, 2, 4] = 0.25
    want_h0 = sum(1 for h in range(H) for w in range(W) for t in range(9) if ch[h, w, t] == 0 and 0 <= cw[h, w, t] < W)
    want_wl = sum(1 for h in range(H) for w in range(W) for t in range(9) if cw[h, w, t] == W and 0 <= ch[h, w, t] < H)
    assert cen["h=0"] == want_h0 and cen["w=L"] == want_wl
    assert cen["h=L-0.25"] == 1 and cen["h=L"] == sum(1 for h in range(H) for w in range(W) for t in range(9) if ch[h, w, t] == H and 0 <= cw[h, w, t] < W)
    assert cen["off=2"] == 1 and cen["off=-2"] == 1 and cen["off=1"] == 1 and cen["off=-1"] == 1 and cen["off=-0.75"] == 1 and cen["off=0.75"] == 0
    assert (cen["far2"], cen["far1"]) == (1, 2)          # (2, -2) leaves both windows; (1, 1) leaves [-1, 1) only
    both = sum(1 for h in range(H) for w in range(W) for t in range(9) if H - 1 <= ch[h, w, t] < H and W - 1 <= cw[h, w, t] < W)
    assert cen["clamp_hw"] == both and both >= 2
    assert cen["floor!=trunc"] == 0
    off[0, 1, 2, 9] = -0.25                              # tap 4 of (1, 2): relative column 1 - 0.25 >= 0 still
    off[0, 1, 2, 0] = -0.5                               # tap 0 of (1, 2): nominal (0, 1), relative row -0.5, absolute -0.5: outside
    assert DE.census_of(off, H, W, 1, 1)["floor!=trunc"] == 0
    off[0, 2, 2, 0] = -0.5                               # tap 0 of (2, 2): nominal (1, 1) -> (0.5, 1): inside, relative row -0.5
    assert DE.census_of(off, H, W, 1, 1)["floor!=trunc"] == 1


@pytest.mark.parametrize("name", NAMES)
def test_oracle_in_float64_and_float32_agree_exactly(name):
    c = DE.CASE_BY_NAME[name]
    d = DE.data(name)
    col32 = DE.col_ref(d.x, d.off, c.dg, c.dil, torch.float32)
    dx32, doff32 = DE.sample_bwd_ref(d.x, d.off, d.dS, c.dg, c.dil, torch.float32)
    assert col32.dtype == dx32.dtype == doff32.dtype == torch.float32
    assert torch.equal(col32.double(), d.col) and torch.equal(dx32.double(), d.dx) and torch.equal(doff32.double(), d.doff)


@pytest.mark.parametrize("name", DE.CONV_CASES)
def test_convolution_references_meet_the_exactness_limits(name):
    c = DE.CASE_BY_NAME[name]
    cv = DE.check_conv(name)
    print(name, "max |16 y| %d  |dS| %d  |4 dOffset| %d  |16 dX| %d  |16 dW| %d" % (
        (16 * cv.y).abs().max().item(), cv.dS.abs().max().item(), (4 * cv.doff).abs().max().item(), (16 * cv.dx).abs().max().item(),
        (16 * cv.dw).abs().max().item()))
    assert (cv.w != 0).sum(dim=(1, 2, 3)).tolist() == [5] * c.C
    d = DE.data(name)
    # delivery: times (x > 0), on top of dx0
    DE.check_exact(cv.dx * (d.x > 0) + d.dx0, 1.0 / 16, True)
    # float32 oracle, whole op
    xr, offr = d.x.float().permute(0, 3, 1, 2), d.off.float().permute(0, 3, 1, 2)
    y32 = OD.deform_conv_forward(xr, cv.w.float(), offr, 1, c.dil, c.dg).permute(0, 2, 3, 1) + cv.bias.float()
    assert torch.equal(y32.double(), cv.y)


def test_sample_backward_helper_is_the_oracle_backward_with_an_identity_filter():
    """deform_sample_backward was split out of deform_conv_backward: with the filter = identity on k (Cout = 9 C) dS equals dY."""
    c = DE.CASE_BY_NAME["generic_5x5_c128_dg4"]
    d = DE.data(c.name)
    K = 9 * c.C
    w = torch.eye(K, dtype=F64).reshape(K, 9, c.C).permute(0, 2, 1).reshape(K, c.C, 3, 3)         # output channel k = tap * C + ch
    dy = d.dS.reshape(c.N, c.H, c.W, K)
    dx, dw, doff, dS = DE.conv_bwd_ref(d.x, w, d.off, dy, c.dg, c.dil)
    assert torch.equal(dS, d.dS) and torch.equal(dx, d.dx) and torch.equal(doff, d.doff)


def test_planted_offsets_move_the_statistic_by_exactly_the_count():
    N, H, W, dg = 2, 8, 16, 1
    assert DE.far_counts(DE.bulk_offsets(N, H, W, dg, 5)) == (0, 0)
    assert DE.far_counts(DE.planted_offsets(N, H, W, dg, 5, 19, 1.25)) == (0, 19)
    assert DE.far_counts(DE.planted_offsets(N, H, W, dg, 5, 346, 2.25)) == (346, 346)
    assert DE.far_counts(DE.planted_offsets(N, H, W, dg, 5, 7, 2.0)) == (7, 7) and DE.far_counts(DE.planted_offsets(N, H, W, dg, 5, 7, -2.0)) == (0, 7)
    assert DE.far_counts(DE.planted_offsets(N, H, W, dg, 5, 7, 1.0)) == (0, 7) and DE.far_counts(DE.planted_offsets(N, H, W, dg, 5, 7, -1.0)) == (0, 0)

"""The kernels of dan_amd/csrc/loss.hip through the C ABI against the float64 references of tests/train_tail.py, at sizes where every
grid-stride loop takes a second (partial) trip: hard-negative scores and selection, the detection loss and its gradient (B A = 546 000 and
A = 8192 + 1), the head split just past its launch cap, the fused momentum-SGD step on every path of its paired loop (segment tables of
300+ variables with unique coefficients, so an element updated with a neighbour's coefficients differs), its range form, its L2 sum, and
the dynamic loss scale (torch.cuda.amp.GradScaler's rule: a step is skipped only when some gradient element is not finite).

Selection decisions are compared exactly - the threshold with torch.topk of the device's own scores, the selection codes with the codes
recomputed from the device's scores and thresholds - and arithmetic against float64 with bounds counted in float32 roundings, so a 1-ulp
score difference neither flips a decision nor hides one.

Measured on an MI355X (worst over the cases; every test prints its figures before it asserts):
  score |err| 9.2e-08 (bound 2^-20 = 9.5e-07); ce_sum / loc_sum relative 3.8e-07 / 1.8e-07 (bound 1e-5);
  dcls |err| 0.36 of 8 u kc, dloc |err| 0.21 of 4 u kl; v' 0.39 of 8 u S, w' 0.495 of its bound; l2 relative 2.3e-06 (bound 2.5e-04).
With the float4-sum term still in grad_nonfinite_kernel the large-finite-gradient test fails: the step is skipped and the state moves to
[128, 0, 1000, 0] instead of [256, 4, 1000, 0]."""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_tail as TT  # noqa: E402

pytestmark = pytest.mark.gpu

U = TT.U
LR, MOMENTUM, SCALE = TT.f32(0.1), TT.f32(0.9), 256.0
INF, NAN = float("inf"), float("nan")


def _api():
    from dan_amd import _lib
    return _lib.call, _lib.ptr, _lib.stream


def _at(t, elems):
    return ctypes.c_void_p(t.data_ptr() + t.element_size() * elems)


# ---------------------------------------------------------------------------------------------------------------- mining and loss
@functools.lru_cache(maxsize=None)
def _mining(B, A):
    return TT.mining_inputs(B, A)


@pytest.mark.parametrize("at_least_one", [False, True])
@pytest.mark.parametrize("B,A", [(16, 34125), (3, 8192 + 1)])
def test_mining_and_detection_loss_against_float64(B, A, at_least_one, dev):
    call, ptr, stream = _api()
    cls, loc, loc_t, labels = _mining(B, A)
    ce_scale, loc_scale = TT.f32(4.0 / 3.0), 0.625
    d_cls, d_loc, d_loc_t, d_labels = cls.to(dev), loc.to(dev), loc_t.to(dev), labels.to(dev)
    score = torch.full((B, A), NAN, device=dev)
    counts = torch.full((B, 2), -7, dtype=torch.int32, device=dev)
    thr = torch.full((B,), NAN, device=dev)
    k = torch.full((B,), -7, dtype=torch.int32, device=dev)
    sel = torch.full((B, A), 9, dtype=torch.uint8, device=dev)
    acc = torch.full((4,), NAN, device=dev)
    dcls = torch.full((B, A, 2), NAN, device=dev)
    dloc = torch.full((B, A, 4), NAN, device=dev)
    call("danhip_hard_neg_select", ptr(d_cls), ptr(d_labels), ptr(score), ptr(counts), ptr(thr), ptr(k), B, A, 3.0, int(at_least_one), stream())
    call("danhip_detection_loss_fwd", ptr(d_cls), ptr(d_loc), ptr(d_labels), ptr(d_loc_t), ptr(score), ptr(thr), ptr(sel), ptr(acc), B, A, stream())
    call("danhip_detection_loss_bwd", ptr(d_cls), ptr(d_loc), ptr(d_loc_t), ptr(sel), ptr(acc), ptr(dcls), ptr(dloc), ce_scale, loc_scale, B, A, stream())
    torch.cuda.synchronize()
    score_d, thr_d = score, thr
    score, counts, thr, k, sel, acc, dcls, dloc = (t.cpu() for t in (score, counts, thr, k, sel, acc, dcls, dloc))

    score_ref, n_pos, n_neg = TT.scores_ref(cls, labels)
    err = (score.double() - score_ref).abs().max().item()
    print("score: max |err| = %.3g (bound %.3g)" % (err, 2.0 ** -20))
    assert err <= 2.0 ** -20
    assert torch.equal(counts.long(), torch.stack([n_pos, n_neg], -1))
    k_ref = TT.k_ref(n_pos, n_neg, 3.0, at_least_one)
    assert torch.equal(k.long(), k_ref)
    for b in range(B):
        want = torch.topk(score_d[b], int(k_ref[b])).values[-1].item() if int(k_ref[b]) > 0 else INF
        assert thr_d[b].item() == want, (b, int(k_ref[b]), thr_d[b].item(), want)
    assert thr[1].item() == -1.0 and int(k_ref[2]) == int(at_least_one)
    sel_ref = TT.select_codes(score, thr, labels)
    assert torch.equal(sel, sel_ref)
    ce_sum, n_sel, loc_sum, npos = TT.loss_sums_ref(cls, loc, labels, loc_t, sel)
    assert acc[1].item() == n_sel == int((sel > 0).sum()) and acc[3].item() == npos == int((sel == 2).sum())
    print("ce_sum: rel err %.3g, loc_sum: rel err %.3g (bound 1e-5)" % (abs(acc[0].item() - ce_sum) / ce_sum, abs(acc[2].item() - loc_sum) / loc_sum))
    assert abs(acc[0].item() - ce_sum) <= 1e-5 * ce_sum and abs(acc[2].item() - loc_sum) <= 1e-5 * loc_sum

    dcls_ref, dloc_ref = TT.loss_grads_ref(cls, loc, loc_t, sel, n_sel, npos, ce_scale, loc_scale)
    kc, kl = ce_scale / n_sel, loc_scale / npos
    assert not torch.isnan(dcls).any() and not torch.isnan(dloc).any()                      # every element written, second trip included
    assert dcls[sel == 0].abs().max().item() == 0 and dloc[sel != 2].abs().max().item() == 0
    ec, el = (dcls.double() - dcls_ref).abs().max().item(), (dloc.double() - dloc_ref).abs().max().item()
    print("dcls: max |err| = %.3g (bound %.3g), dloc: max |err| = %.3g (bound %.3g)" % (ec, 8 * U * kc, el, 4 * U * kl))
    assert ec <= 8 * U * kc and el <= 4 * U * kl


# ---------------------------------------------------------------------------------------------------------------- head split
def test_head_split_past_the_launch_cap(dev):
    call, ptr, stream = _api()
    B, HW, nneg, npos, off = 41, 25600, 3, 1, 7
    A, Ch = HW + 12, 4 + nneg + npos
    h = TT.head_inputs(B, HW, nneg, npos)
    g = torch.Generator().manual_seed(11)
    dloc_in, dcls_in = torch.randn((B, A, 4), generator=g), torch.randn((B, A, 2), generator=g)
    d_h = h.to(dev)
    loc = torch.full((B, A, 4), -77.0, device=dev)
    cls = torch.full((B, A, 2), -77.0, device=dev)
    dy = torch.full((B * HW, Ch), NAN, device=dev)
    call("danhip_head_split_fwd", ptr(d_h), ptr(loc), ptr(cls), B, HW, Ch, nneg, npos, A, off, stream())
    d_dloc, d_dcls = dloc_in.to(dev), dcls_in.to(dev)
    call("danhip_head_split_bwd", ptr(d_h), ptr(d_dloc), ptr(d_dcls), ptr(dy), B, HW, Ch, nneg, npos, A, off, stream())
    torch.cuda.synchronize()
    loc, cls, dy = loc.cpu(), cls.cpu(), dy.cpu()
    loc_ref, cls_ref = TT.head_split_ref(h.view(B, HW, Ch), nneg, npos)
    assert torch.equal(loc[:, off:off + HW].double(), loc_ref) and torch.equal(cls[:, off:off + HW].double(), cls_ref)
    for t in (loc, cls):                                         # anchors of the other heads: untouched
        assert bool((t[:, :off] == -77.0).all()) and bool((t[:, off + HW:] == -77.0).all())
    dy_ref, divided = TT.head_split_bwd_ref(h.view(B, HW, Ch), dloc_in[:, off:off + HW], dcls_in[:, off:off + HW], nneg, npos)
    dy_ref, divided = dy_ref.view(B * HW, Ch), divided.view(B * HW, Ch)
    assert not torch.isnan(dy).any()
    assert torch.equal(dy.double()[~divided], dy_ref[~divided])
    assert bool(((dy.double() - dy_ref).abs()[divided] <= 2.0 ** -23 * dy_ref.abs()[divided]).all())     # one float32 ulp


# ---------------------------------------------------------------------------------------------------------------- optimizer
def _sgd_ref(name):
    w, g, v, seg, gm, wdc = TT.sgd_inputs(name)
    return TT.sgd_ref(w, g, v, seg, gm, wdc, LR, MOMENTUM, 1.0 / SCALE)


def _check_sgd(what, w_got, v_got, w0, ref):
    w2, v2, _, S = ref
    bv = 8 * U * S
    ev = (v_got.cpu().double() - v2).abs()
    bw = 2 * U * w0.double().abs() + LR * bv + U * LR * v2.abs()
    ew = (w_got.cpu().double() - w2).abs()
    print("%s: max err / bound: v' %.3g, w' %.3g" % (what, (ev / bv.clamp(min=1e-300)).max().item(), (ew / bw.clamp(min=1e-300)).max().item()))
    bad_v, bad_w = (ev > bv).nonzero().reshape(-1), (ew > bw).nonzero().reshape(-1)
    assert bad_v.numel() == 0, (what, "v'", bad_v.numel(), bad_v[:8].tolist())
    assert bad_w.numel() == 0, (what, "w'", bad_w.numel(), bad_w[:8].tolist())


@pytest.mark.parametrize("name", list(TT.SGD_CASES))
def test_sgd_step_and_l2_sum_against_float64(name, dev):
    call, ptr, stream = _api()
    w0, g, v0, seg, gm, wdc = TT.sgd_inputs(name)
    nseg, total = seg.numel() - 1, w0.numel()
    ref = _sgd_ref(name)
    d_g, d_seg, d_gm, d_wdc = g.to(dev), seg.to(dev), gm.to(dev), wdc.to(dev)
    prior = 0.25 * ref[2]
    w, v, l2 = w0.to(dev), v0.to(dev), torch.tensor([prior], dtype=torch.float32, device=dev)
    call("danhip_sgd_momentum_flat", ptr(w), ptr(d_g), ptr(v), ptr(d_seg), ptr(d_gm), ptr(d_wdc), nseg, total, LR, MOMENTUM, 1.0 / SCALE, ptr(l2), stream())
    wn, vn = w0.to(dev), v0.to(dev)                              # without the L2 output: the same update
    call("danhip_sgd_momentum_flat", ptr(wn), ptr(d_g), ptr(vn), ptr(d_seg), ptr(d_gm), ptr(d_wdc), nseg, total, LR, MOMENTUM, 1.0 / SCALE, None, stream())
    torch.cuda.synchronize()
    _check_sgd(name, w, v, w0, ref)
    assert torch.equal(w, wn) and torch.equal(v, vn)
    blocks = min((total // 4 + 255) // 256, TT.SGD_BLOCKS)
    want = float(l2.new_tensor(prior).item()) + ref[2]
    print("%s: l2 rel err %.3g (bound %.3g)" % (name, abs(l2.item() - want) / want, (blocks + 32) * U))
    assert abs(l2.item() - want) <= (blocks + 32) * U * want


def test_sgd_range_form_updates_only_its_range(dev):
    """FlatParams.sgd_range: pointers offset into the buffers, a segment table relative to the range, offset coefficient tables."""
    call, ptr, stream = _api()
    w0, g, v0, seg, gm, wdc = TT.sgd_inputs("pair-then-tail")
    nseg = seg.numel() - 1
    k0, k1 = nseg // 8, 7 * nseg // 8
    s, e = int(seg[k0]), int(seg[k1])
    assert TT.SGD_STRIDE * 4 < e - s < 2 * TT.SGD_STRIDE * 4
    rel = (seg[k0:k1 + 1] - s).contiguous()
    ref = TT.sgd_ref(w0[s:e], g[s:e], v0[s:e], rel, gm[k0:k1], wdc[k0:k1], LR, MOMENTUM, 1.0 / SCALE)
    d_g, d_rel, d_gm, d_wdc = g.to(dev), rel.to(dev), gm.to(dev), wdc.to(dev)
    w, v, l2 = w0.to(dev), v0.to(dev), torch.tensor([3.0], device=dev)
    call("danhip_sgd_momentum_flat", _at(w, s), _at(d_g, s), _at(v, s), ptr(d_rel), _at(d_gm, k0), _at(d_wdc, k0), k1 - k0, e - s, LR, MOMENTUM,
         1.0 / SCALE, ptr(l2), stream())
    torch.cuda.synchronize()
    w, v = w.cpu(), v.cpu()
    _check_sgd("range", w[s:e], v[s:e], w0[s:e], ref)
    for got, before in ((w, w0), (v, v0)):
        assert torch.equal(got[:s], before[:s]) and torch.equal(got[e:], before[e:])
    blocks = min(((e - s) // 4 + 255) // 256, TT.SGD_BLOCKS)
    assert abs(l2.item() - (3.0 + ref[2])) <= (blocks + 32) * U * (3.0 + ref[2])


def _padding_element(name):
    raw, starts = TT.sgd_layout(name)
    return next(starts[i] + n for i, n in enumerate(raw) if n % 64 and i > 3)


def test_dynamic_loss_scale_skips_exactly_the_steps_with_a_nonfinite_gradient(dev):
    call, ptr, stream = _api()
    name = "pair-then-tail"
    w0, g, v0, seg, gm, wdc = TT.sgd_inputs(name)
    nseg, total = seg.numel() - 1, w0.numel()
    d_w0, d_v0, d_g, d_seg, d_gm, d_wdc = w0.to(dev), v0.to(dev), (g * 1.0).to(dev), seg.to(dev), gm.to(dev), wdc.to(dev)

    def dyn(w, v, grad, state):
        st = torch.tensor(state, dtype=torch.float32, device=dev)
        call("danhip_sgd_momentum_flat_dynamic", ptr(w), ptr(grad), ptr(v), ptr(d_seg), ptr(d_gm), ptr(d_wdc), nseg, total, LR, MOMENTUM, ptr(st), None, stream())
        torch.cuda.synchronize()
        return st.tolist()

    # one non-finite element anywhere: first float4 (every component), last float4, the check's second trip, the last lane of a wave, padding
    places = [0, 1, 2, 3, total - 2, TT.NONFINITE_TRIP + 4 * 1000 + 1, 63 * 4 + 2, _padding_element(name)]
    assert places[5] < total and places[4] // 4 == total // 4 - 1
    w, v = d_w0.clone(), d_v0.clone()
    for at in places:
        keep = d_g[at].item()
        for bad in (INF, -INF, NAN):
            d_g[at] = bad
            state = dyn(w, v, d_g, [SCALE, 3.0, 1000.0, 0.0])
            assert torch.equal(w, d_w0) and torch.equal(v, d_v0), (at, bad)
            assert state == TT.loss_scale_ref([SCALE, 3.0, 1000.0, 0.0], True) == [SCALE / 2, 0.0, 1000.0, 0.0], (at, bad, state)
        d_g[at] = keep
    # the floor: a bad step at scale 1 leaves it at 1
    d_g[places[5]] = INF
    assert dyn(w, v, d_g, [1.0, 5.0, 1000.0, 0.0]) == TT.loss_scale_ref([1.0, 5.0, 1000.0, 0.0], True) == [1.0, 0.0, 1000.0, 0.0]
    assert torch.equal(w, d_w0) and torch.equal(v, d_v0)
    d_g[places[5]] = g[places[5]]
    assert torch.equal(d_g.cpu(), g)
    # the ceiling: the interval reached at 2^24 leaves it at 2^24 (a clean step: w and v move)
    top = [2.0 ** 24, 1.0, 2.0, 0.0]
    assert dyn(w, v, d_g, top) == TT.loss_scale_ref(top, False) == [2.0 ** 24, 0.0, 2.0, 0.0]
    assert not torch.equal(w, d_w0)


def test_dynamic_loss_scale_takes_a_step_whose_finite_gradients_sum_past_float32(dev):
    """GradScaler skips a step only when some gradient ELEMENT is inf or NaN.  Two elements of 2e38 in one float4 are finite, their float32
    sum is not: the step is taken, with g / scale.  (grad_nonfinite_kernel used to test the float4's sum as well and skipped this step.)"""
    call, ptr, stream = _api()
    name = "pair-then-tail"
    w0, g, v0, seg, gm, wdc = TT.sgd_inputs(name)
    nseg, total = seg.numel() - 1, w0.numel()
    at = TT.NONFINITE_TRIP + 4 * 12345
    g = g.clone()
    g[at:at + 4] = torch.tensor([2e38, 2e38, 0.0, 0.0])
    assert bool(torch.isfinite(g).all()) and not bool(torch.isfinite(g[at] + g[at + 1]))
    ref = TT.sgd_ref(w0, g, v0, seg, gm, wdc, LR, MOMENTUM, 1.0 / SCALE)
    w, v, st = w0.to(dev), v0.to(dev), torch.tensor([SCALE, 3.0, 1000.0, 0.0], device=dev)
    d_g, d_seg, d_gm, d_wdc = g.to(dev), seg.to(dev), gm.to(dev), wdc.to(dev)
    call("danhip_sgd_momentum_flat_dynamic", ptr(w), ptr(d_g), ptr(v), ptr(d_seg), ptr(d_gm), ptr(d_wdc), nseg, total, LR, MOMENTUM, ptr(st), None, stream())
    torch.cuda.synchronize()
    assert st.tolist() == TT.loss_scale_ref([SCALE, 3.0, 1000.0, 0.0], False) == [SCALE, 4.0, 1000.0, 0.0], st.tolist()
    _check_sgd("large finite gradients", w, v, w0, ref)

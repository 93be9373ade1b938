"""Pins tests/train_tail.py itself (no GPU): each float64 reference against the project's float32 oracle (oracle/train.py, oracle/tf_ops.py)
at the tolerances the oracle tests of these quantities use, the edges the input generators must produce, and the loop-trip conditions of the
sizes that tests/test_train_tail_gpu.py runs."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_tail as TT  # noqa: E402
from oracle import tf_ops as T  # noqa: E402
from oracle import train as OT  # noqa: E402

# the shapes of test_train_tail_gpu.py
MINING_SHAPES = [(16, 34125), (3, 8192 + 1)]
HEAD_SHAPE = (41, 25600, 3, 1)


@pytest.mark.parametrize("at_least_one", [False, True])
def test_mining_and_loss_references_are_the_oracle(at_least_one):
    B, A = 4, 2500
    cls, loc, loc_t, labels = TT.mining_inputs(B, A, seed=1)
    final, pos, score32, k = OT.hard_neg_mask(cls, labels.long(), 3.0, at_least_one)
    score, n_pos, n_neg = TT.scores_ref(cls, labels)
    assert (score - score32.double()).abs().max().item() <= 1e-6
    assert torch.equal(n_pos, pos.sum(-1)) and torch.equal(n_neg, (labels == 0).sum(-1))
    assert torch.equal(TT.k_ref(n_pos, n_neg, 3.0, at_least_one), k.long())
    thr = torch.stack([torch.topk(score32[b], int(k[b])).values[-1] if int(k[b]) > 0 else torch.tensor(float("inf")) for b in range(B)])
    sel = TT.select_codes(score32, thr, labels)
    assert torch.equal(sel > 0, final) and torch.equal(sel == 2, pos)
    assert int((sel[2] > 0).sum()) == (1 if at_least_one else 0)                  # the row without positives
    # losses and gradients: the oracle's means, through autograd
    clsr, locr = cls.clone().requires_grad_(True), loc.clone().requires_grad_(True)
    ce, ll, _ = OT.detection_loss(clsr, locr, labels.long(), loc_t, 3.0, at_least_one)
    (ce + ll).backward()
    ce_sum, n_sel, loc_sum, npos = TT.loss_sums_ref(cls, loc, labels, loc_t, sel)
    assert n_sel == int(final.sum()) and npos == int(pos.sum())
    assert abs(4.0 * ce_sum / n_sel - ce.item()) <= 1e-4 * abs(ce.item())
    assert abs(loc_sum / npos - ll.item()) <= 1e-4 * abs(ll.item())
    dcls, dloc = TT.loss_grads_ref(cls, loc, loc_t, sel, n_sel, npos, 4.0, 1.0)
    assert torch.allclose(dcls.float(), clsr.grad, rtol=1e-4, atol=1e-7)
    assert torch.allclose(dloc.float(), locr.grad, rtol=1e-4, atol=1e-7)
    assert dcls[sel == 0].abs().max().item() == 0 and dloc[sel != 2].abs().max().item() == 0
    # the scales are factors of the gradient
    d2, l2 = TT.loss_grads_ref(cls, loc, loc_t, sel, n_sel, npos, 2.0, 0.25)
    assert torch.allclose(d2 * 2.0, dcls, rtol=1e-14, atol=0) and torch.allclose(l2 * 4.0, dloc, rtol=1e-14, atol=0)


@pytest.mark.parametrize("B,A", MINING_SHAPES)
def test_mining_inputs_hold_the_edges_of_the_selection_rule(B, A):
    cls, loc, loc_t, labels = TT.mining_inputs(B, A)
    score, n_pos, n_neg = TT.scores_ref(cls, labels)
    score32 = torch.where(labels == 0, -torch.softmax(cls, -1)[..., 0], torch.tensor(-1.0))
    assert bool((3 * n_pos[0] < n_neg[0]) and (3 * n_pos[3 % B] < n_neg[3 % B]))
    assert 3 * int(n_pos[1]) > int(n_neg[1]) and int(n_pos[2]) == 0
    assert all(int((labels[b] == -1).sum()) > 0 for b in range(B))
    assert int((labels[:, A - 1] == 0).sum()) == B                                # the anchor on the last trip of a row carries a real score
    # row 0: a run of equal scores across the threshold
    k = TT.k_ref(n_pos, n_neg, 3.0, False)
    thr0 = torch.topk(score32[0], int(k[0])).values[-1]
    neg0 = labels[0] == 0
    above, equal = int((neg0 & (score32[0] > thr0)).sum()), int((neg0 & (score32[0] == thr0)).sum())
    assert equal >= 50 and above + 20 <= int(k[0]) <= above + equal - 20
    # row 1: k = n_neg, and at least 100 negatives whose float32 background probability is exactly 1
    sat = (labels[1] == 0) & (cls[1, :, 0] - cls[1, :, 1] >= 20)
    assert int(k[1]) == int(n_neg[1]) and int(sat.sum()) >= 100
    assert bool((score32[1][sat] == -1.0).all()) and torch.topk(score32[1], int(k[1])).values[-1].item() == -1.0
    sel = TT.select_codes(score32, torch.stack([thr0] + [torch.tensor(-1.0)] * (B - 1)), labels)
    assert bool((sel[1][sat] == 1).all()) and bool((sel[1][labels[1] == -1] == 0).all())
    # the row without positives: its hardest negative is the last anchor
    assert int(score32[2].argmax()) == A - 1
    # localisation differences below, above and exactly 1, among the positives
    d = (loc - loc_t)[labels > 0].abs()
    assert int((d == 1).sum()) >= 10 and int((d < 1).sum()) >= 10 and int((d > 1).sum()) >= 10
    # the loops repeat, and the looped part holds a visible share of what the sums add
    if B * A > TT.LOSS_BWD_TRIP:
        assert B * A % TT.LOSS_BWD_TRIP != 0 and B * A < 2 * TT.LOSS_BWD_TRIP and B * A % TT.LOSS_FWD_TRIP != 0
        assert A > TT.SCORE_ROW_TRIP and A % 64 != 0
        thr = torch.stack([torch.topk(score32[b], int(k[b])).values[-1] if int(k[b]) > 0 else torch.tensor(float("inf")) for b in range(B)])
        sel = TT.select_codes(score32, thr, labels).reshape(-1)
        for code in (1, 2):
            assert int((sel[TT.LOSS_FWD_TRIP:] == code).sum()) >= 0.01 * int((sel == code).sum()) > 0
        assert int((sel[TT.LOSS_BWD_TRIP:] > 0).sum()) > 0
    else:
        assert A == TT.SCORE_ROW_TRIP + 1


def test_head_split_reference_is_the_oracle_max_out():
    g = torch.Generator().manual_seed(5)
    B, H, W = 2, 5, 4
    for nneg, npos in ((3, 1), (1, 1), (1, 3)):
        h = torch.randn((B, H, W, 4 + nneg + npos), generator=g)
        h[0, 0, 0, 4:4 + nneg] = 1.5
        h[1, 2, 3, 4 + nneg:] = -0.25
        hr = h.clone().requires_grad_(True)
        cls_o = T.maxout_cls(hr[..., 4:], 1, nneg, npos)
        loc, cls = TT.head_split_ref(h, nneg, npos)
        assert torch.equal(loc.float(), h[..., :4]) and torch.equal(cls.float(), cls_o.detach())
        dl, dc = torch.randn((B, H, W, 4), generator=g), torch.randn((B, H, W, 2), generator=g)
        ((hr[..., :4] * dl).sum() + (cls_o * dc).sum()).backward()
        dy, divided = TT.head_split_bwd_ref(h, dl, dc, nneg, npos)
        assert torch.allclose(dy.float(), hr.grad, rtol=1e-6, atol=1e-7)
        assert int(divided.sum()) == (nneg if nneg > 1 else 0) + (npos if npos > 1 else 0)
    # the shape of the GPU test: just past the launch cap, ties on both trips
    B, HW, nneg, npos = HEAD_SHAPE
    assert TT.HEAD_TRIP < B * HW < TT.HEAD_TRIP + 256 * 8
    h = TT.head_inputs(B, HW, nneg, npos)
    cnt = (h[:, 4:4 + nneg] == h[:, 4:4 + nneg].amax(-1, keepdim=True)).sum(-1)
    assert int((cnt == 2).sum()) > 1000 and int((cnt == 3).sum()) > 1000
    assert int(cnt[TT.HEAD_TRIP]) == 2 and int(cnt[-1]) == 3 and int((cnt[TT.HEAD_TRIP:] == 1).sum()) > 900


def test_sgd_reference_is_the_oracle_momentum_step_and_l2_term():
    g = torch.Generator().manual_seed(6)
    shapes = {"conv1/kernel": (3, 3, 4, 5), "conv1/bias": (5,), "bn1/gamma": (7,), "l2_norm_layer/weight": (70,), "conv2/kernel": (1, 1, 5, 130), "conv2/bias": (130,)}
    params = {k: torch.randn(s, generator=g) for k, s in shapes.items()}
    grads = {k: torch.randn(s, generator=g) for k, s in shapes.items()}
    momenta = {k: torch.randn(s, generator=g) for k, s in shapes.items()}
    wd, lr, mom, gscale = 5e-4, TT.f32(0.1), TT.f32(0.9), 1.0 / 8
    starts, w, gr, v, gm, wdc = [0], [], [], [], [], []
    for k in shapes:                                              # the flat layout and the per-variable coefficients of FlatParams
        n = params[k].numel()
        for flat, src in ((w, params), (gr, grads), (v, momenta)):
            flat.append(torch.cat([src[k].reshape(-1), torch.zeros(TT.pad64(n) - n)]))
        starts.append(starts[-1] + TT.pad64(n))
        gm.append(2.0 if "/bias" in k else 1.0)
        wdc.append(0.0 if "bn" in k or "/bias" in k else (0.2 * wd if "l2_norm_layer" in k else wd))
    w, gr, v = torch.cat(w), torch.cat(gr), torch.cat(v)
    w2, v2, l2, S = TT.sgd_ref(w, gr / gscale, v, torch.tensor(starts), torch.tensor(gm), torch.tensor(wdc), lr, mom, gscale)
    # oracle: the L2 term is part of the loss, its gradient reaches the optimizer with the loss gradient
    pr = {k: p.clone().requires_grad_(True) for k, p in params.items()}
    reg = OT.l2_regularizer(pr, wd)
    reg.backward()
    total = {k: grads[k] + (pr[k].grad if pr[k].grad is not None else 0.0) for k in shapes}    # (bias and batch-norm variables are not regularised)
    po, mo = {k: p.clone() for k, p in params.items()}, {k: m.clone() for k, m in momenta.items()}
    OT.momentum_sgd_step(po, total, mo, lr, mom)
    assert abs(l2 - reg.item()) <= 1e-5 * reg.item()
    wmax = w.abs().max().item()
    for i, k in enumerate(shapes):
        n = params[k].numel()
        assert (w2[starts[i]:starts[i] + n].float() - po[k].reshape(-1)).abs().max().item() <= 1e-5 * wmax, k
        assert (v2[starts[i]:starts[i] + n].float() - mo[k].reshape(-1)).abs().max().item() <= 1e-5 * wmax, k
    assert bool((S >= v2.abs() - 1e-12).all())                   # S bounds every partial result of v'


def test_loss_scale_reference_is_the_grad_scaler_rule_with_clamps():
    assert TT.loss_scale_ref([256.0, 3.0, 1000.0, 0.0], True) == [128.0, 0.0, 1000.0, 0.0]
    assert TT.loss_scale_ref([256.0, 3.0, 1000.0, 1.0], False) == [256.0, 4.0, 1000.0, 0.0]
    assert TT.loss_scale_ref([256.0, 1.0, 2.0, 0.0], False) == [512.0, 0.0, 2.0, 0.0]
    assert TT.loss_scale_ref([1.0, 5.0, 1000.0, 0.0], True) == [1.0, 0.0, 1000.0, 0.0]
    assert TT.loss_scale_ref([1.5, 0.0, 1000.0, 0.0], True) == [1.0, 0.0, 1000.0, 0.0]
    assert TT.loss_scale_ref([2.0 ** 24, 1.0, 2.0, 0.0], False) == [2.0 ** 24, 0.0, 2.0, 0.0]


def test_sgd_layouts_put_segment_boundaries_on_every_path_of_the_kernel():
    regions = {}
    for name in TT.SGD_CASES:
        raw, starts = TT.sgd_layout(name)
        assert raw[-1] == 64 and all(s % 64 == 0 for s in starts) and starts[-1] == TT.SGD_CASES[name][0]
        regions[name] = TT.sgd_regions(starts)
        if name != "tail-only":
            assert len(raw) >= 300, (name, len(raw))
            assert {64, 128, 576, 36864}.issubset(raw) and any(n % 64 for n in raw)
        w, g, v, seg, gm, wdc = TT.sgd_inputs(name)
        assert len(set(gm.tolist())) == len(raw) and len(set(wdc.tolist())) == len(raw)     # unique in float32
        assert 0.9 < w.std().item() < 1.1 and 0.9 < g.std().item() < 1.1 and 0.9 < v.std().item() < 1.1
    count = lambda name, kind, trip=None: sum(1 for k, t in regions[name] if k == kind and (trip is None or t == trip))
    n4 = lambda name: TT.SGD_CASES[name][0] // 4
    # 2.5 strides: a pair then a tail, or a pair only
    assert 2 * TT.SGD_STRIDE < n4("pair-then-tail") < 3 * TT.SGD_STRIDE and TT.SGD_CASES["pair-then-tail"][0] >= 10485760
    assert 589824 in TT.sgd_layout("pair-then-tail")[0]
    assert count("pair-then-tail", "first") + count("pair-then-tail", "second") >= 250
    assert count("pair-then-tail", "first") >= 20 and count("pair-then-tail", "second") >= 20 and count("pair-then-tail", "tail") >= 20
    # 1.5 strides: a pair, or a tail only (the tail of a thread that never paired)
    assert TT.SGD_STRIDE < n4("pair-or-tail") < 2 * TT.SGD_STRIDE
    assert count("pair-or-tail", "second") >= 20 and count("pair-or-tail", "tail", 0) >= 20 and count("pair-or-tail", "first") >= 20
    # 3.25 strides: boundaries at the first float4 of a second paired trip, where the first scan has to move
    assert 3 * TT.SGD_STRIDE < n4("two-pairs") < 4 * TT.SGD_STRIDE
    assert count("two-pairs", "first", 1) >= 20 and count("two-pairs", "second", 1) >= 20 and count("two-pairs", "tail", 1) >= 20
    # one block, one trip
    assert n4("tail-only") <= 256 * 3 and len(TT.sgd_layout("tail-only")[0]) == 5
    assert all(k == "tail" for k, _ in regions["tail-only"])
    assert TT.SGD_CASES["pair-then-tail"][0] > 2 * TT.NONFINITE_TRIP


def test_constants_mirror_the_source():
    """The launch caps are read back from loss.hip, so a changed cap fails here and not silently in the shape conditions."""
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dan_amd", "csrc")
    src = open(os.path.join(root, "loss.hip")).read()
    assert src.count("dim3(dh_grid_for((long)B * HW, 256, %d)), dim3(256)" % (TT.HEAD_TRIP // 256)) == 2      # (no default cap: each launch states its own)
    assert "grid_for(A, 1024, %d)" % (TT.SCORE_ROW_TRIP // 1024) in src
    assert "grid_for(total, 1024, %d)), dim3(1024)" % (TT.LOSS_FWD_TRIP // 1024) in src
    assert "grid_for(total, 256, %d)), dim3(256)" % (TT.LOSS_BWD_TRIP // 256) in src
    assert src.count("sgd_momentum_flat_kernel, dim3(dh_grid_for(total / 4, 256, %d)), dim3(256)" % TT.SGD_BLOCKS) == 2
    assert "grad_nonfinite_kernel, dim3(dh_grid_for(total / 4, 256, %d)), dim3(256)" % (TT.NONFINITE_TRIP // 1024) in src
    assert "fmaxf(dyn[0] * 0.5f, 1.f)" in src and "fminf(dyn[0] * 2.f, 16777216.f)" in src

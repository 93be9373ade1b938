"""float64 references, input generators and launch geometry for the kernels of dan_amd/csrc/loss.hip: hard-negative scoring and selection,
the detection loss and its gradient, the head split, the fused momentum-SGD step and its dynamic loss scale.  No GPU dependency: every
reference restates its operation from the definition in plain torch float64 (tests/test_train_tail_cpu.py pins them to oracle/train.py and
oracle/tf_ops.py); tests/test_train_tail_gpu.py runs the kernels against them at sizes where their grid-stride loops repeat."""
import functools

import torch

from oracle import train as OT

U = 2.0 ** -24                         # unit roundoff of float32

# items per grid-stride trip of each kernel (blocks x threads of the capped launch); test_train_tail_cpu.py reads the caps back from loss.hip
HEAD_TRIP = 4096 * 256                 # head_split_{fwd,bwd}: rows of h
SCORE_ROW_TRIP = 8 * 1024              # hard_neg_scores: anchors of one row
LOSS_FWD_TRIP = 128 * 1024             # detection_loss_fwd: anchors
LOSS_BWD_TRIP = 2048 * 256             # detection_loss_bwd: anchors
SGD_BLOCKS = 4096
SGD_STRIDE = SGD_BLOCKS * 256          # sgd_momentum_flat: float4s
NONFINITE_TRIP = 2048 * 256 * 4        # grad_nonfinite: elements
SCALE_FLOOR, SCALE_CEILING = 1.0, 2.0 ** 24


def f32(x):
    """The float32 value a C `float` argument receives."""
    return torch.tensor(x, dtype=torch.float32).item()


# ---------------------------------------------------------------------------------------------------------------- mining and loss
def scores_ref(cls, labels):
    """score = -softmax(cls)[..., 0] where the label is 0, -1 elsewhere; per-row (n_pos, n_neg)."""
    p_bg = torch.softmax(cls.double(), -1)[..., 0]
    neg = labels == 0
    return torch.where(neg, -p_bg, torch.full_like(p_bg, -1.0)), (labels > 0).sum(-1), neg.sum(-1)


def k_ref(n_pos, n_neg, ratio, at_least_one):
    """k = min(int(ratio * n_pos), n_neg) with the product in float32, at least 1 for DAN."""
    k = torch.minimum((torch.tensor(ratio, dtype=torch.float32) * n_pos.to(torch.float32)).to(torch.int64), n_neg.to(torch.int64))
    return torch.clamp(k, min=1) if at_least_one else k


def select_codes(score, thr, labels):
    """0 not selected, 1 selected negative (label 0 and score >= the row's threshold), 2 positive."""
    neg = (labels == 0) & (score >= thr[:, None])
    return torch.where(labels > 0, 2, torch.where(neg, 1, 0)).to(torch.uint8)


def loss_sums_ref(cls, loc, labels, loc_t, sel):
    """(ce_sum, n_sel, loc_sum, n_pos): cross entropy logsumexp - logit[target] over the selected anchors, smooth L1 over the positives."""
    c = cls.double()
    s, pos = sel > 0, sel == 2
    ce = torch.logsumexp(c, -1) - torch.where(labels > 0, c[..., 1], c[..., 0])
    sl1 = OT.modified_smooth_l1(loc.double(), loc_t.double(), 1.0).sum(-1)
    return ce[s].sum().item(), int(s.sum()), sl1[pos].sum().item(), int(pos.sum())


def loss_grads_ref(cls, loc, loc_t, sel, n_sel, n_pos, ce_scale, loc_scale):
    """d(ce_scale * ce_sum / n_sel) / dcls and d(loc_scale * loc_sum / n_pos) / dloc; zero on every anchor that is not selected."""
    p = torch.softmax(cls.double(), -1)
    onehot = torch.stack([sel == 1, sel == 2], -1).double()
    kc = ce_scale / n_sel if n_sel > 0 else 0.0
    kl = loc_scale / n_pos if n_pos > 0 else 0.0
    dcls = torch.where((sel > 0)[..., None], (p - onehot) * kc, torch.zeros_like(p))
    d = loc.double() - loc_t.double()
    dl = torch.where(d.abs() < 1.0, d, torch.sign(d)) * kl
    return dcls, torch.where((sel == 2)[..., None], dl, torch.zeros_like(dl))


def mining_inputs(B, A, seed=0):
    """Logits, boxes, targets and labels with the edges of the selection rule (rows: 0 exact ties across the threshold, 1 k = n_neg with
    saturated background scores, 2 no positive, the rest 3 n_pos < n_neg) and of the smooth L1 (|d| below, above and exactly 1)."""
    assert B >= 3 and A >= 2000
    g = torch.Generator().manual_seed(1000 + seed)
    cls = torch.randn((B, A, 2), generator=g) * 2
    loc_t = torch.round(torch.randn((B, A, 4), generator=g) * 4) / 4
    loc = loc_t + torch.randn((B, A, 4), generator=g) * 1.2
    labels = torch.zeros((B, A), dtype=torch.int32)
    for b in range(B):
        perm = torch.randperm(A - 1, generator=g)                # (the last anchor of a row stays a negative: set below)
        if b == 1:
            labels[b, ::3] = 1                                   # 3 n_pos > n_neg: k = n_neg
            free = perm[perm % 3 != 0]
            labels[b, free[:A // 100]] = -1
            sat = free[A // 100:A // 100 + 150]                  # background probability exactly 1 in float32: the score ties with the sentinel
            cls[b, sat, 0], cls[b, sat, 1] = 12.0, -12.0
            continue
        n_pos = 0 if b == 2 else max(3, A // (60 + 23 * b))
        labels[b, perm[:n_pos]] = 1
        labels[b, perm[n_pos:n_pos + A // 100]] = -1
    labels[1, A - 1] = 0
    cls[2, A - 1, 0], cls[2, A - 1, 1] = -9.0, 9.0               # the hardest negative of the row without positives
    # row 0: 60 negatives around the k-th largest score take the k-th one's logits
    k = 3 * int((labels[0] > 0).sum())
    score = torch.where(labels[0] == 0, -torch.softmax(cls[0], -1)[:, 0], torch.tensor(-1.0))
    order = torch.argsort(score, descending=True)
    cls[0, order[k - 30:k + 30]] = cls[0, order[k - 1]].clone()
    # positives with a localisation difference of exactly +1 / -1 in one or all coordinates
    pos = (labels > 0).nonzero()
    for j, (b, a) in enumerate(pos[::7].tolist()):
        if j % 3 == 0:
            loc[b, a] = loc_t[b, a] + 1.0
        elif j % 3 == 1:
            loc[b, a, 1] = loc_t[b, a, 1] - 1.0
        else:
            loc[b, a, 3] = loc_t[b, a, 3] + 1.0
    return cls, loc, loc_t, labels


# ---------------------------------------------------------------------------------------------------------------- head split
def head_split_ref(h, nneg, npos):
    """h [..., 4 + nneg + npos] -> loc [..., 4], cls [..., 2] = (max of the nneg background logits, max of the npos face logits)."""
    h = h.double()
    return h[..., :4], torch.stack([h[..., 4:4 + nneg].amax(-1), h[..., 4 + nneg:].amax(-1)], -1)


def head_split_bwd_ref(h, dloc, dcls, nneg, npos):
    """Gradient of head_split_ref; a max-out gradient is shared equally between tied maxima.  Also returns where a tie divided."""
    h = h.double()
    dy = torch.zeros_like(h)
    divided = torch.zeros(h.shape, dtype=torch.bool)
    dy[..., :4] = dloc.double()
    for grp, (s, n) in enumerate(((4, nneg), (4 + nneg, npos))):
        x = h[..., s:s + n]
        top = x == x.amax(-1, keepdim=True)
        cnt = top.sum(-1, keepdim=True)
        dy[..., s:s + n] = torch.where(top, dcls.double()[..., grp:grp + 1] / cnt, torch.zeros_like(x))
        divided[..., s:s + n] = top & (cnt > 1)
    return dy, divided


def head_inputs(B, HW, nneg, npos, seed=0):
    """Random h with two- and three-way ties inside the background group, the last row and the first row of the second trip included."""
    g = torch.Generator().manual_seed(2000 + seed)
    h = torch.randn((B * HW, 4 + nneg + npos), generator=g)
    rows = torch.arange(B * HW)
    two = (rows % 97 == 0) | (rows == HEAD_TRIP)
    three = (rows % 89 == 1) | (rows == B * HW - 1)
    if nneg >= 2:
        h[two, 4] = h[two, 5] = h[two, 4:4 + nneg].amax(-1) + 1.0
    if nneg >= 3:
        h[three, 4:4 + nneg] = h[three, 4:5]
    return h


# ---------------------------------------------------------------------------------------------------------------- optimizer
def sgd_ref(w, g, v, seg, gmult, wdc, lr, momentum, gscale):
    """v' = m v + (g gscale + c w) gm, w' = w - lr v', l2 = sum c w^2 / 2 with c, gm of the element's segment [seg[s], seg[s + 1]).
    Also the per-element magnitude sum S = |m v| + (|g gscale| + |c w|) gm that bounds the rounding of v'."""
    w, g, v = w.double(), g.double(), v.double()
    sizes = seg[1:] - seg[:-1]
    assert int(seg[0]) == 0 and int(seg[-1]) == w.numel() and bool((sizes >= 0).all())
    idx = torch.repeat_interleave(torch.arange(sizes.numel()), sizes)
    c, gm = wdc.double()[idx], gmult.double()[idx]
    mv, gs, cw = momentum * v, g * gscale, c * w
    v2 = mv + (gs + cw) * gm
    return w - lr * v2, v2, (0.5 * c * w * w).sum().item(), mv.abs() + (gs.abs() + cw.abs()) * gm


def loss_scale_ref(state, any_nonfinite):
    """torch.cuda.amp.GradScaler's rule on {scale, clean steps, growth interval, flag}: halve after a step with a non-finite gradient, double
    after `interval` clean ones; the scale stays within [1, 2^24] and the flag is cleared."""
    scale, good, interval, _ = state
    if any_nonfinite:
        return [max(scale * 0.5, SCALE_FLOOR), 0.0, interval, 0.0]
    good += 1.0
    if good >= interval:
        return [min(scale * 2.0, SCALE_CEILING), 0.0, interval, 0.0]
    return [scale, good, interval, 0.0]


SGD_PATTERN = [589824, 64, 128, 576, 16, 36864, 64, 1000, 128, 576, 64, 36864, 21, 128, 64, 576, 36864, 64, 128, 576, 3, 36864, 64, 128, 576, 64]
# name -> (total elements, one 589 824-element variable every `big_every` cycles of the pattern)
SGD_CASES = {
    "tail-only": (64 * 40, 0),
    "pair-or-tail": (3 * SGD_STRIDE * 2 + 64 * 11, 4),            # 1.5 strides: a pair, or a tail only
    "two-pairs": (13 * SGD_STRIDE + 64 * 5, 1),                   # 3.25 strides: the paired loop's first scan moves on its second trip
    "pair-then-tail": (5 * SGD_STRIDE * 2 + 64 * 37, 1),          # 2.5 strides: threads do a pair and a tail, or a pair only
}


def pad64(n):
    return (n + 63) // 64 * 64


def sgd_layout(name):
    """(raw sizes, starts) of a flat parameter buffer as FlatParams lays it out: every variable starts on a 64-element boundary; the last one
    has 64 elements and the padded sizes add up to the case's total."""
    total, big_every = SGD_CASES[name]
    if big_every == 0:
        raw = [640, 64, 1000, 768, 64]
    else:
        raw, used, cycle, done = [], 0, 0, False
        while not done:
            for j, n in enumerate(SGD_PATTERN):
                if j == 0 and cycle % big_every != 0:
                    continue
                if used + pad64(n) > total - 64:
                    done = True
                    break
                raw.append(n)
                used += pad64(n)
            cycle += 1
        if total - 64 - used > 0:
            raw.append(total - 64 - used)
        raw.append(64)
    starts = [0]
    for n in raw:
        starts.append(starts[-1] + pad64(n))
    assert starts[-1] == total, (name, starts[-1], total)
    return raw, starts


def sgd_regions(starts):
    """How sgd_momentum_flat_kernel reaches the float4 at each inner segment boundary: 'first' / 'second' float4 of a paired trip (with the
    trip number) or the single-trip 'tail'.  Thread q0 pairs (q0 + 2 j S, q0 + (2 j + 1) S) while the second lies inside the buffer."""
    n4 = starts[-1] // 4
    stride = min((n4 + 255) // 256, SGD_BLOCKS) * 256
    out = []
    for b in starts[1:-1]:
        q = b // 4
        t = q // stride
        if t % 2 == 1:
            out.append(("second", t // 2))
        elif q + stride < n4:
            out.append(("first", t // 2))
        else:
            out.append(("tail", t // 2))
    return out


@functools.lru_cache(maxsize=1)                                   # (the cases are listed so that the one several tests share comes last)
def sgd_inputs(name):
    """w, g, v of order 1 (padding included: the kernel treats it as part of the variable), segment table, per-segment multipliers
    that are unique, so an element updated with a neighbour's values differs."""
    raw, starts = sgd_layout(name)
    nseg, total = len(raw), starts[-1]
    g = torch.Generator().manual_seed(3000 + total % 9973)
    w, gr, v = (torch.randn(total, generator=g) for _ in range(3))
    s = torch.arange(nseg, dtype=torch.float64)
    return w, gr, v, torch.tensor(starts, dtype=torch.int64), (1.0 + s / nseg).float(), (1e-4 * (1.0 + s)).float()

"""DynamicAnchorRouting (train mode) and greedy NMS of csrc/routing_exact.hip on the paths test_routing_gpu.py never reaches, against the CPU
oracle (oracle.extra_lib.dynamic_anchor_routing / uniform_stream, oracle.anchors.nms_tf):

  train mode, B > 1, counter_dev   stream position counter0 + *counter_dev + b*N + i, the b*N offsets of the seven workspace arrays,
                                   route_scan_kernel with one block per image (the form train_dan.py runs every step)
  route_train_cell_kernel          buckets of several hundred sources: the insertion sort that restores index order after the atomic-ordered
                                   scatter, and the reservoir replay (accept probability 1 / (m + 1), first 1/2 on a pass-1 positive cell)
  route_scan_kernel                N = 25 600 (160 x 160 x 1, stride 4): 25 counts per thread
  nms_kernel                       B = 3 through the C ABI (bbox_util passes B = 1), K at the 1024-thread stride, max_out binding, swapped
                                   corners, and the declared maximum K = 65 536 = 64 KB of dynamic LDS

Every case asserts from oracle-side data that it reaches its path before it compares.  Masks, indices and counts are equal; train-mode
decode_out (device logf) keeps rtol = 3e-7, atol = 1e-6 and eval-mode decode_out (device expf) rtol = 3e-7, atol = 1e-5 of the
neighbouring tests."""
import functools

import numpy as np
import pytest
import torch

from oracle import anchors as OA
from oracle import extra_lib as OX

pytestmark = pytest.mark.gpu

F32 = np.float32
THRES, IGNORE_THRES = 0.5, 0.35


def _spread_case(seed, fh, fw, depth, stride):
    """Sources all over the map, some degenerate, some outside, absolute gt boxes near the stage-1 boxes (the generator of
    test_routing_train_matches_oracle)."""
    rng = np.random.RandomState(seed)
    N = fh * fw * depth
    cy, cx = (rng.rand(N) * fh * stride).astype(F32), (rng.rand(N) * fw * stride).astype(F32)
    h, w = (rng.rand(N) * 6 * stride).astype(F32), (rng.rand(N) * 6 * stride).astype(F32)
    h[rng.rand(N) < 0.05] = 0.3
    anchors = np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], -1).astype(F32)
    anchors[rng.rand(N) < 0.03] += F32(3 * fh * stride)
    mask_in = (rng.rand(N) < 0.6).astype(np.int32)
    gt = (anchors + (rng.randn(N, 4) * stride * 0.5).astype(F32)).astype(F32)
    labels = (rng.rand(N) < 0.4).astype(F32)
    return anchors, gt, labels, mask_in


def _centre_cell(boxes, fh, fw, depth, stride):
    """NumPy restatement of route_cell (dynamic_anchor_routing.cc:262-279) for boxes whose centre coordinate / stride is not within rounding
    of k + 0.5 (the generators here keep away from it): (cell, routed)."""
    ymin, xmin, ymax, xmax = [boxes[:, i].astype(np.float64) for i in range(4)]
    cx = np.clip(np.floor((xmin + xmax) / (2. * stride) + 0.5), 0, fw - 1).astype(np.int64)
    cy = np.clip(np.floor((ymin + ymax) / (2. * stride) + 0.5), 0, fh - 1).astype(np.int64)
    ok = ~((xmin / stride < -1) | (xmax / stride > fw) | (ymin / stride < -1) | (ymax / stride > fh))
    return (cy * fw + cx) * depth + np.arange(boxes.shape[0]) % depth, ok


def _buckets(anchors, gt, labels, mask_in, fh, fw, depth, stride):
    """Per cell: the number of reservoir candidates (pass 2, :245-305) and the pass-1 positive flag (:205-243), restated in float64; used for
    path preconditions only (the sizes asserted below are far from any rounding question)."""
    N = labels.shape[0]
    a, g = anchors.astype(np.float64), gt.astype(np.float64)
    cell, ok = _centre_cell(anchors, fh, fw, depth, stride)
    ih = np.maximum(np.minimum(a[:, 2], g[:, 2]) - np.maximum(a[:, 0], g[:, 0]) + 1., 0.)
    iw = np.maximum(np.minimum(a[:, 3], g[:, 3]) - np.maximum(a[:, 1], g[:, 1]) + 1., 0.)
    inter = ih * iw
    uni = (g[:, 2] - g[:, 0] + 1.) * (g[:, 3] - g[:, 1] + 1.) + (a[:, 2] - a[:, 0] + 1.) * (a[:, 3] - a[:, 1] + 1.) - inter
    valid = (mask_in >= 1) & ~((a[:, 3] - a[:, 1] < 1) | (a[:, 2] - a[:, 0] < 1)) & ok & (labels > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        cand = valid & (np.abs(uni) > 1.) & (inter / uni > IGNORE_THRES)
    count = np.bincount(cell[cand], minlength=N)
    gcell, _ = _centre_cell(gt, fh, fw, depth, stride)
    p1 = (labels > 0) & ~((g[:, 3] - g[:, 1] < 1) | (g[:, 2] - g[:, 0] < 1))
    matched = np.zeros(N, np.int64)
    matched[gcell[p1]] = 1
    return count, matched


def _route_train(dev, case, fh, fw, depth, stride, seed, counter0, counter_dev=None):
    from dan_amd.utility import custom_op
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    mo, do = custom_op.dynamic_anchor_routing(t(case[0]), t(case[1]), t(case[2]), t(case[3]), fh, fw, depth, stride, 0, 0, True, THRES, IGNORE_THRES,
                                              seed=seed, counter0=counter0, counter_dev=counter_dev)
    return mo.cpu().numpy(), do.cpu().numpy()


def _assert_train(mo, do, mo_ref, do_ref, what=None):
    assert np.array_equal(mo, mo_ref), what
    assert np.allclose(do, do_ref, rtol=3e-7, atol=1e-6), (what, np.abs(do - do_ref).max())      # log() from the device libm


def test_routing_train_batched_with_a_device_counter(dev):
    """B = 3 images with different inputs, counter0 = 1000 on the host and 555 in a device tensor: image b replays
    uniform_stream(seed, counter0 + 555 + b*N, N)."""
    fh, fw, depth, stride = 20, 16, 2, 8
    N, B, seed, counter0, c = fh * fw * depth, 3, 4321, 1000, 555
    cases = [_spread_case(40 + b, fh, fw, depth, stride) for b in range(B)]
    assert B > 1 and counter0 != 0 and c != 0
    assert not np.array_equal(cases[0][0], cases[1][0]) and not np.array_equal(cases[1][0], cases[2][0])
    refs = []
    for b, cs in enumerate(cases):
        u = OX.uniform_stream(seed, counter0 + c + b * N, N)
        mo_ref, do_ref = OX.dynamic_anchor_routing(*cs, fh, fw, depth, stride, 0, 0, True, THRES, IGNORE_THRES, u=u)
        assert (mo_ref == 1).sum() > 0 and (mo_ref == -1).sum() > 0
        # the stream position matters: the same image replayed without the device counter, or from image 0's position, gives another result
        for start in (counter0 + b * N, counter0 + c):
            if start != counter0 + c + b * N:
                other = OX.dynamic_anchor_routing(*cs, fh, fw, depth, stride, 0, 0, True, THRES, IGNORE_THRES, u=OX.uniform_stream(seed, start, N))
                assert not np.array_equal(other[1], do_ref), (b, start)
        refs.append((mo_ref, do_ref))
    batch = [np.stack([cs[j] for cs in cases]) for j in range(4)]
    cdev = torch.tensor([c], dtype=torch.int64, device=dev)
    mo, do = _route_train(dev, batch, fh, fw, depth, stride, seed, counter0, cdev)
    assert mo.shape == (B, N) and do.shape == (B, N, 4)
    for b, (mo_ref, do_ref) in enumerate(refs):
        _assert_train(mo[b], do[b], mo_ref, do_ref, b)


@functools.lru_cache(maxsize=None)
def _hot_case(seed):
    """24 x 24 x 2 map, stride 8.  70 % of the sources sit on cell (10, 12) with their gt on the same cell (a pass-1 positive bucket of several
    hundred per depth slot), 20 % on cell (5, 5) with the gt centre three to four pixels to the right, i.e. in cell (5, 6) (a large bucket
    that pass 1 left at matched = 0), the rest spread.  Some gts are far enough off for the ignore band and for the no-candidate band."""
    fh = fw = 24
    depth, stride = 2, 8
    rng = np.random.RandomState(seed)
    N = fh * fw * depth
    grp = rng.choice(3, N, p=[0.7, 0.2, 0.1])
    cy = np.where(grp == 0, 10 * stride, 5 * stride) + rng.uniform(-3, 3, N)
    cx = np.where(grp == 0, 12 * stride + rng.uniform(-3, 3, N), 5 * stride + rng.uniform(2.2, 3.2, N))
    spread = grp == 2
    cy[spread], cx[spread] = rng.uniform(8, (fh - 1) * stride, spread.sum()), rng.uniform(8, (fw - 1) * stride, spread.sum())
    h, w = rng.uniform(24, 60, N), rng.uniform(24, 60, N)
    anchors = np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], -1).astype(F32)
    shift = np.zeros((N, 4))
    shift[grp == 1] += [0., 3.5, 0., 3.5]                                     # gt centre of the (5, 5) sources lands in cell (5, 6)
    far = rng.rand(N)
    shift[(far < 0.15) & (grp != 1)] += [9., -8., 9., -8.]                    # IoU around 0.4 - 0.5: candidates that also raise the ignore flag
    shift[(far > 0.9) & (grp != 1)] += [30., 30., 30., 30.]                   # IoU below ignore_thres: no candidates
    gt = (anchors + shift + rng.uniform(-0.4, 0.4, (N, 4))).astype(F32)
    labels = (rng.rand(N) < 0.85).astype(F32)
    mask_in = (rng.rand(N) < 0.9).astype(np.int32)
    return (anchors, gt, labels, mask_in), (fh, fw, depth, stride)


@pytest.mark.parametrize("seed", [0, 1])
def test_routing_train_with_buckets_of_several_hundred_sources(seed, dev):
    case, (fh, fw, depth, stride) = _hot_case(seed)
    N = fh * fw * depth
    count, matched = _buckets(*case, fh, fw, depth, stride)
    hot = int(np.argmax(count))
    assert count[hot] > 256 and matched[hot] == 1                               # a long bucket whose first accept probability is 1/2
    cold = np.flatnonzero((matched == 0) & (count >= 50))
    assert cold.size > 0                                                        # and a long one that starts at probability 1
    sd, c0 = 99 + seed, 31
    u = OX.uniform_stream(sd, c0, N)
    mo_ref, do_ref = OX.dynamic_anchor_routing(*case, fh, fw, depth, stride, 0, 0, True, THRES, IGNORE_THRES, u=u)
    assert (mo_ref == 1).sum() > 0 and (mo_ref == -1).sum() > 0
    assert mo_ref[hot] == 1 and np.abs(do_ref[hot]).sum() > 0 and all(np.abs(do_ref[c]).sum() > 0 for c in cold)    # the reservoirs accepted
    mo, do = _route_train(dev, case, fh, fw, depth, stride, sd, c0)
    _assert_train(mo, do, mo_ref, do_ref)


def test_routing_at_25600_cells_eval_and_train(dev):
    """The stride-4 level of a 640 input: route_scan_kernel sums 25 counts per thread, and non-empty buckets lie in more cells than the scan
    block has threads."""
    from dan_amd.utility import custom_op
    fh = fw = 160
    depth, stride = 1, 4
    N = fh * fw * depth
    case = _spread_case(7, fh, fw, depth, stride)
    assert N == 25600 and (N + 1023) // 1024 == 25
    count, _ = _buckets(*case, fh, fw, depth, stride)
    assert (count > 0).sum() > 1024 and count.max() > 1
    sd, c0 = 2024, 5
    u = OX.uniform_stream(sd, c0, N)
    mo_ref, do_ref = OX.dynamic_anchor_routing(*case, fh, fw, depth, stride, 0, 0, True, THRES, IGNORE_THRES, u=u)
    assert (mo_ref == 1).sum() > 0 and (mo_ref == -1).sum() > 0
    mo, do = _route_train(dev, case, fh, fw, depth, stride, sd, c0)
    _assert_train(mo, do, mo_ref, do_ref, "train")
    # eval mode on the same boxes: stage-2 scores with ties, small regression offsets
    rng = np.random.RandomState(8)
    scores = (np.round(rng.rand(N) * 8) / 8).astype(F32)
    offsets = (rng.randn(N, 4) * 0.2).astype(F32)
    emo_ref, edo_ref = OX.dynamic_anchor_routing(case[0], offsets, scores, case[3], fh, fw, depth, stride, 0, 0, False, 0.0, 0.0)
    assert (emo_ref == 1).sum() > 1024
    t = lambda a: torch.from_numpy(a).to(dev)
    emo, edo = custom_op.dynamic_anchor_routing(t(case[0]), t(offsets), t(scores), t(case[3]), fh, fw, depth, stride, 0, 0, False, 0.03, 0.0)
    assert np.array_equal(emo.cpu().numpy(), emo_ref)
    assert np.allclose(edo.cpu().numpy(), edo_ref, rtol=3e-7, atol=1e-5)      # exp() from the device libm


# ---------------------------------------------------------------------------------------------------------------------------------- NMS
def _nms_abi(dev, boxes, max_out, thr):
    """danhip_nms on boxes [B,K,4] already in score order -> (keep_idx [B,max_out], num_keep [B])."""
    from dan_amd._lib import call, ptr, stream
    B, K, _ = boxes.shape
    b = torch.from_numpy(np.ascontiguousarray(boxes, F32)).to(dev)
    keep = torch.full((B, max_out), -7, dtype=torch.int32, device=dev)
    num = torch.full((B,), -7, dtype=torch.int32, device=dev)
    call("danhip_nms", ptr(b), B, K, int(max_out), float(thr), ptr(keep), ptr(num), stream())
    torch.cuda.synchronize()
    return keep.cpu().numpy(), num.cpu().numpy()


def _assert_nms(keep, num, refs, max_out):
    for b, ref in enumerate(refs):
        assert num[b] == len(ref), (b, num[b], len(ref))
        assert np.array_equal(keep[b, :len(ref)], ref), b
        assert np.array_equal(keep[b, len(ref):], np.full(max_out - len(ref), -1)), b


def _swap_some(boxes, rng, share):
    """Swaps ymin / ymax and / or xmin / xmax in a share of the rows (both sides normalise the corners with min / max)."""
    sy, sx = rng.rand(boxes.shape[0]) < share, rng.rand(boxes.shape[0]) < share
    boxes[sy] = boxes[sy][:, [2, 1, 0, 3]]
    boxes[sx] = boxes[sx][:, [0, 3, 2, 1]]
    return int((sy | sx).sum())


@functools.lru_cache(maxsize=None)
def _mixed_batch(K):
    rng = np.random.RandomState(K)
    same = np.tile(np.asarray([10., 10., 50., 60.], F32), (K, 1))
    i = np.arange(K)
    apart = np.stack([(i // 33) * 10., (i % 33) * 10., (i // 33) * 10. + 8., (i % 33) * 10. + 8.], -1).astype(F32)
    cy, cx = rng.rand(K) * 150, rng.rand(K) * 150
    h, w = rng.rand(K) * 40 + 20, rng.rand(K) * 40 + 20                          # crowded: fewer than max_out survive
    rand =np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], -1).astype(F32)
    n_swapped = _swap_some(rand, rng, 0.2)
    rand[::17] = 0.0                                                            # zero-area rows, as sort_bboxes pads
    return np.stack([same, apart, rand]), n_swapped


@pytest.mark.parametrize("K", [1024, 1025, 1026])
def test_nms_batched_through_the_abi(K, dev):
    """nms_kernel's per-image `boxes += b*K*4; keep_idx += b*max_out; num_keep += b` with three different images, and K around the block's
    1024 threads: at 1025 the flag-clearing loop takes a second trip, at 1026 the suppression loop of candidate 0 does."""
    max_out, thr = 200, 0.3
    boxes, n_swapped = _mixed_batch(K)
    scores = np.arange(K, 0, -1).astype(F32)                                    # strictly descending: the oracle's order is the given one
    refs = [OA.nms_tf(boxes[b], scores, max_out, thr) for b in range(3)]
    assert boxes.shape[0] == 3 and n_swapped > K // 10
    assert len(refs[0]) == 1                                                    # identical boxes: one survivor
    assert len(refs[1]) == max_out and len(OA.nms_tf(boxes[1], scores, max_out + 1, thr)) == max_out + 1     # max_out binds: box 200 was next
    assert 1 < len(refs[2]) < max_out and refs[2].max() > max_out               # the random image stops on its own, deep in the list
    keep, num = _nms_abi(dev, boxes, max_out, thr)
    assert num[1] == max_out
    _assert_nms(keep, num, refs, max_out)


@functools.lru_cache(maxsize=None)
def _clustered_65536():
    """24 clusters of near-identical boxes (IoU > 0.9 with the cluster's first box).  Most of the list is ordered by cluster, so the oracle's
    most-recent-first check ends after one comparison; the last 8192 rows pick clusters at random; three boxes far away from every cluster
    sit deep in the list, one of them in the last row."""
    K, C = 65536, 24
    rng = np.random.RandomState(65536)
    cid = np.minimum(np.arange(K) // ((K - 8192) // C), C - 1)
    cid[K - 8192:] = rng.randint(0, C, 8192)
    y0 = (cid // 6) * 100. + rng.randint(0, 2, K)
    x0 = (cid % 6) * 100. + rng.randint(0, 2, K)
    boxes = np.stack([y0, x0, y0 + 40., x0 + 40.], -1).astype(F32)
    lone = [30000, 60000, K - 1]
    for k, i in enumerate(lone):
        boxes[i] = [5000. + 100. * k, 5000., 5040. + 100. * k, 5040.]
    _swap_some(boxes, rng, 0.1)
    return boxes, lone


def test_nms_at_the_declared_maximum_of_65536_candidates(dev):
    """K = 65 536: exactly 64 KB of dynamic LDS for the suppressed flags, with max_out = 200 not binding, so the walk reaches the last row."""
    K, max_out, thr = 65536, 200, 0.5
    boxes, lone = _clustered_65536()
    scores = np.arange(K, 0, -1).astype(F32)
    same = np.tile(np.asarray([3., 4., 30., 40.], F32), (K, 1))
    refs = [OA.nms_tf(boxes, scores, max_out, thr), OA.nms_tf(same, scores, max_out, thr)]
    assert 24 <= len(refs[0]) < max_out and all(i in refs[0] for i in lone) and refs[0][-1] == K - 1 and len(refs[1]) == 1
    keep, num = _nms_abi(dev, np.stack([boxes, same]), max_out, thr)
    _assert_nms(keep, num, refs, max_out)

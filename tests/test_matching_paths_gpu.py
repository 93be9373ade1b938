"""The matching kernels of csrc/anchors_exact.hip on the paths the realistic-face cases of test_anchors_gpu.py never reach, bit-exact against
the CPU oracle (oracle.extra_lib.small_mining_match, oracle.anchors.iou_matrix / do_dual_max_match / encode_anchors):

  batch_phase3_kernel   candidate lists above P3_LDS_HEAP = 2048 entries (the heap lives in the per-image HBM buffer `gheap = p.heap + b*A`
                        instead of LDS), the 2048 / 2049 switch, min_match != 6 (never reached / binding mid-list), p3_chunks(A) > 8
  smm_phase3_kernel     the same lists through the per-image entry point
  colmax_kernel, dual_max_match_body, smm_phase12_body     G at and above the 256-thread stride

Every case first proves from oracle-side data that it reaches its path (list lengths, pops, G) and only then compares.  The long lists come
from a dense grid of equal-size boxes at 1-px offsets around a gt of the same size: IoU depends on (|dy|, |dx|) only, so equal IoUs are
plentiful and the pop order is exactly the tie order of the reference's std::priority_queue."""
import functools

import numpy as np
import pytest
import torch

from oracle import anchors as OA
from oracle import extra_lib as OE

pytestmark = pytest.mark.gpu

F32 = np.float32
PS = [0.1, 0.1, 0.2, 0.2]
LOG_ATOL = 4 * np.finfo(np.float32).eps * 5 * 4      # the log() targets: 2 ulp of logf scaled by 1 / 0.2 (test_anchors_gpu.py)
P3_LDS_HEAP = 2048                                   # anchors_exact.hip
SIZE, REACH = 65, 48                                 # 65-px boxes at offsets -48 .. 48: 9409 anchors, 3065 of them with IoU > 0.3
# thresholds through the ABI: with 0.7 / 0.7 only 277 grid anchors are positives of the centred gt and 2788 stay phase-3 candidates
NEG_LOW, IGN, POS, STOP = 0.0, 0.7, 0.7, 0.3
POP_ALL, POP_SOME = 100000, 1277                     # min_match above every list + count / binding about 1000 pops into a list


def _grid(origin_y, origin_x):
    d = np.arange(-REACH, REACH + 1, dtype=F32)
    dy, dx = np.meshgrid(d, d, indexing="ij")
    y0, x0 = F32(origin_y) + dy.reshape(-1), F32(origin_x) + dx.reshape(-1)
    return np.stack([y0, x0, y0 + F32(SIZE - 1), x0 + F32(SIZE - 1)], -1).astype(F32)


def _box(y, x):
    return [y, x, y + SIZE - 1, x + SIZE - 1]


def _phase3_lists(ov, min_match, args=(NEG_LOW, IGN, POS), stop=STOP):
    """Per gt, from oracle results only: (length of the candidate list phase 3 builds for it, -1 when the gt is skipped; number of pops).
    min_match = 0 makes phase 3 skip every gt, which exposes the state after phases 1-2; an anchor that is negative there and matched in the
    full result was popped by that gt, so the list of gt g is: negative after phase 2, IoU > stop, not popped by a gt before g."""
    m12, _ = OE.small_mining_match(ov, *args, 0, stop)
    fin, _ = OE.small_mining_match(ov, *args, min_match, stop)
    lens, pops = [], []
    for g in range(ov.shape[1]):
        if int((m12 == g).sum()) >= min_match:
            lens.append(-1); pops.append(0)
            continue
        free = (m12 < 0) & ~((fin >= 0) & (fin < g))
        lens.append(int((free & (ov[:, g] > F32(stop))).sum()))
        pops.append(int(((m12 < 0) & (fin == g)).sum()))
    return lens, pops


def _encode_batched(dev, anchors, gts, mining, neg_low, ign, pos, min_match, stop):
    """danhip_encode_anchors_batched through the C ABI (AnchorEncoder._encode_batch hard-codes min_match = 6 and stop = 0.3): the four
    anchor arrays, an all-true inside mask, ragged gt lists."""
    from dan_amd import _lib
    from dan_amd._lib import call, ptr, stream
    a4 = [torch.from_numpy(np.ascontiguousarray(anchors[:, i])).to(dev) for i in range(4)]
    A, B = anchors.shape[0], len(gts)
    offs = np.concatenate([[0], np.cumsum([g.shape[0] for g in gts])]).astype(np.int32)
    gt = torch.from_numpy(np.concatenate(gts).astype(F32)).to(dev)
    goff = torch.from_numpy(offs).to(dev)
    inside = torch.ones((A,), dtype=torch.uint8, device=dev)
    T = torch.empty((B, A, 4), dtype=torch.float32, device=dev)
    L = torch.empty((B, A), dtype=torch.int32, device=dev)
    S = torch.empty((B, A), dtype=torch.float32, device=dev)
    M = torch.empty((B, A, 4), dtype=torch.float32, device=dev)
    n = _lib.lib().danhip_encode_anchors_batched_workspace_bytes(B, A, int(offs[-1]))
    ws = torch.empty(((n + 7) // 8,), dtype=torch.int64, device=dev)
    call("danhip_encode_anchors_batched", ptr(a4[0]), ptr(a4[1]), ptr(a4[2]), ptr(a4[3]), None, None, None, None, ptr(inside), ptr(gt), ptr(goff), B, A,
         int(offs[-1]), int(max(g.shape[0] for g in gts)), int(mining), float(neg_low), float(ign), float(pos), int(min_match), float(stop), *PS, 1.0,
         ptr(T), ptr(L), ptr(S), ptr(M), ptr(ws), n, stream())
    torch.cuda.synchronize()
    return T.cpu().numpy(), L.cpu().numpy(), S.cpu().numpy(), M.cpu().numpy()


def _assert_encoded(got, ref, what):
    (t, l, s, m), (t_ref, l_ref, s_ref, m_ref) = got, ref
    assert np.array_equal(l.astype(np.int64), l_ref), what
    assert np.array_equal(s, s_ref), what
    assert np.array_equal(m, m_ref), what
    assert np.array_equal(t[:, :2], t_ref[:, :2]), what                       # centre offsets: +, -, / only
    assert np.allclose(t[:, 2:], t_ref[:, 2:], rtol=0, atol=LOG_ATOL), what


def _check_mining_batch(dev, anchors, gts, min_match):
    """Batched call against oracle.anchors.encode_anchors with the same five parameters, and the per-image danhip_small_mining_match on
    the same IoU matrix against oracle.extra_lib.small_mining_match."""
    from dan_amd.utility import anchor_manipulator as AM
    a4 = tuple(anchors[:, i] for i in range(4))
    inside = np.ones(anchors.shape[0], bool)
    mf = lambda ov: OE.small_mining_match(ov, NEG_LOW, IGN, POS, min_match, STOP)
    T, L, S, M = _encode_batched(dev, anchors, gts, True, NEG_LOW, IGN, POS, min_match, STOP)
    n_pos = 0
    for b, gt in enumerate(gts):
        ref = OA.encode_anchors(gt, a4, inside, IGN, POS, PS, mf)
        _assert_encoded((T[b], L[b], S[b], M[b]), ref, ("batched", b))
        ov = OA.iou_matrix(anchors, gt)
        i_ref, s_ref = mf(ov)
        i_got, s_got = AM.small_mining_match(torch.from_numpy(ov).to(dev), NEG_LOW, IGN, POS, min_match, STOP)
        assert np.array_equal(i_got.cpu().numpy(), i_ref), ("per-image", b)
        assert np.array_equal(s_got.cpu().numpy(), s_ref), ("per-image", b)
        n_pos += int((ref[1] == 1).sum())
    assert n_pos > 0


@functools.lru_cache(maxsize=None)
def _long_list_batch():
    """B = 3 on one grid.  Image 0: one gt near the grid's corner (a short list: the LDS heap, in the same launch).  Image 1: three gts a few
    pixels apart, so an earlier gt's pops remove candidates from the later ones.  Image 2: another long list."""
    anchors = _grid(100, 100)
    gts = [np.asarray([_box(140, 138)], F32),
           np.asarray([_box(100, 100), _box(103, 98), _box(92, 109)], F32),
           np.asarray([_box(95, 104)], F32)]
    return anchors, gts


@pytest.mark.parametrize("min_match", [POP_ALL, POP_SOME])
def test_phase3_lists_above_the_lds_heap_in_a_batch(min_match, dev):
    """batch_phase3_kernel `heap = ncand <= P3_LDS_HEAP ? s_heap : gheap` with gheap = p.heap + b*A at b = 1 and b = 2, next to an LDS-heap
    image at b = 0; min_match = 100000 pops every candidate, min_match = 1277 stops about 1000 pops into each list.  (The heap is scratch:
    two images that wrongly shared one buffer would only differ through a race, which a comparison of results cannot pin.)"""
    anchors, gts = _long_list_batch()
    lens, pops = zip(*[_phase3_lists(OA.iou_matrix(anchors, gt), min_match) for gt in gts])
    assert 0 < lens[0][0] <= P3_LDS_HEAP                                        # b = 0: LDS heap
    assert lens[1][0] > P3_LDS_HEAP and lens[2][0] > P3_LDS_HEAP                # b = 1, 2: HBM heap at a non-zero image offset
    ov1 = OA.iou_matrix(anchors, gts[1])
    for g in (1, 2):                                                            # the earlier gts' pops shortened this list
        assert 0 < lens[1][g] < int(((OE.small_mining_match(ov1, NEG_LOW, IGN, POS, 0, STOP)[0] < 0) & (ov1[:, g] > F32(STOP))).sum())
    if min_match == POP_ALL:
        assert all(p == l for pp, ll in zip(pops, lens) for p, l in zip(pp, ll))     # every list is emptied
    else:
        assert all(0 < p < l for pp, ll in zip(pops, lens) for p, l in zip(pp, ll) if l > P3_LDS_HEAP)   # min_match binds inside the long lists
    _check_mining_batch(dev, anchors, gts, min_match)


@functools.lru_cache(maxsize=None)
def _trimmed_grid(n):
    """The grid with candidates of the centred gt removed (a fixed random choice) until its phase-3 list has exactly n entries."""
    anchors = _grid(100, 100)
    gt = np.asarray([_box(100, 100)], F32)
    ov = OA.iou_matrix(anchors, gt)
    m12, _ = OE.small_mining_match(ov, NEG_LOW, IGN, POS, 0, STOP)
    cand = np.flatnonzero((m12 < 0) & (ov[:, 0] > F32(STOP)))
    drop = np.random.RandomState(n).choice(cand, cand.size - n, replace=False)
    return np.delete(anchors, drop, axis=0), gt


@pytest.mark.parametrize("min_match", [POP_ALL, POP_SOME])
@pytest.mark.parametrize("n", [P3_LDS_HEAP, P3_LDS_HEAP + 1])
def test_phase3_list_of_exactly_2048_and_2049(n, min_match, dev):
    """The two sides of `ncand <= P3_LDS_HEAP`: the last list heaped in LDS and the first one heaped in HBM, at b = 1."""
    anchors, gt = _trimmed_grid(n)
    gts = [np.asarray([_box(60, 141)], F32), gt]
    lens, pops = _phase3_lists(OA.iou_matrix(anchors, gt), min_match)
    assert lens == [n]
    assert pops == [n] if min_match == POP_ALL else 0 < pops[0] < n
    _check_mining_batch(dev, anchors, gts, min_match)


@functools.lru_cache(maxsize=None)
def _tiled_grid():
    return np.concatenate([_grid(100, 100), _grid(100, 400)]), [np.asarray([_box(98, 403)], F32),
                                                                  np.asarray([_box(100, 100), _box(104, 397), _box(99, 102)], F32)]


@pytest.mark.parametrize("min_match", [POP_ALL, POP_SOME])
def test_phase3_with_more_than_eight_chunks_per_wave(min_match, dev):
    """A = 18818: p3_chunks(A) = 24, every wave walks three rounds of eight 64-anchor chunks, and the long lists lie in the second tile, i.e.
    in the upper waves' ranges."""
    anchors, gts = _tiled_grid()
    A = anchors.shape[0]
    assert ((((A + 15) // 16) + 511) // 512) * 8 > 8                            # p3_chunks(A), anchors_exact.hip
    lens, pops = zip(*[_phase3_lists(OA.iou_matrix(anchors, gt), min_match) for gt in gts])
    assert lens[0][0] > P3_LDS_HEAP and lens[1][0] > P3_LDS_HEAP and lens[1][1] > P3_LDS_HEAP
    assert min(np.flatnonzero(OA.iou_matrix(anchors, gts[0])[:, 0] > F32(STOP))) >= A // 2
    _check_mining_batch(dev, anchors, gts, min_match)


# ---------------------------------------------------------------------------------------------------------------- G above the block stride
LEVELS = np.asarray([0.0, 0.05, 0.31, 0.32, 0.35, 0.38, 0.41, 0.5, 0.7], F32)
BLOCK = 256                                          # colmax_kernel's block; the per-anchor loops of the two matchers run g = 0 .. G-1


@functools.lru_cache(maxsize=None)
def _level_matrix(G):
    """Tie-heavy level matrix as in test_small_mining_match_kats_and_ties, thinned to about 1.5 entries per row so that many gts stay below
    min_match = 6 and carry phase-3 lists; the last column owns a unique maximum on the last row."""
    rng = np.random.RandomState(1000 + G)
    A = 3000 + G % 7
    ov = LEVELS[rng.randint(0, len(LEVELS), (A, G))]
    ov[rng.rand(A, G) >= 1.5 / G] = 0.0
    ov[A - 1, :] = 0.0
    ov[A - 1, G - 1] = 0.9
    return ov


@pytest.mark.parametrize("G", [255, 256, 257, 300])
def test_matchers_with_G_at_and_above_the_block_stride(G, dev):
    """colmax_kernel `for (g = threadIdx.x; g < G; g += blockDim.x)` takes a second trip for G > 256; the matchers' `for g < G` loops and the
    phase-3 walk over gts run past 256."""
    from dan_amd.utility import anchor_manipulator as AM
    ov = _level_matrix(G)
    A = ov.shape[0]
    lens, pops = _phase3_lists(ov, 6, (0., 0.4, 0.4), 0.3)
    busy = [g for g in range(G) if pops[g] > 0]
    assert len(busy) >= 20 and (G <= BLOCK or max(busy) >= BLOCK)                # phase 3 pops for many gts, some of them beyond the stride
    i_ref, s_ref = OE.small_mining_match(ov, 0., 0.4, 0.4, 6, 0.3)
    d_ref, ds_ref = OA.do_dual_max_match(ov, 0.35, 0.35)
    assert i_ref[A - 1] == G - 1 and d_ref[A - 1] == G - 1                       # the last column is matched
    if G > BLOCK:
        for m in (i_ref, d_ref):                                                 # at least half the columns beyond the stride are matched
            assert len(np.unique(m[m >= BLOCK])) >= (G - BLOCK + 1) // 2
    t = torch.from_numpy(ov).to(dev)
    i_got, s_got = AM.small_mining_match(t, 0., 0.4, 0.4, 6, 0.3)
    assert np.array_equal(i_got.cpu().numpy(), i_ref)
    assert np.array_equal(s_got.cpu().numpy(), s_ref)
    d_got, ds_got = AM.do_dual_max_match(t, 0.35, 0.35)
    assert np.array_equal(d_got.cpu().numpy().astype(np.int64), d_ref)
    assert np.array_equal(ds_got.cpu().numpy(), ds_ref)


def _faces(n, h, w, seed):
    rng = np.random.RandomState(seed)
    side = np.exp(rng.uniform(np.log(8), np.log(min(h, w) * 0.6), n))
    cy, cx = rng.uniform(side / 2, h - side / 2, n), rng.uniform(side / 2, w - side / 2, n)
    b = np.stack([cy - side / 2, cx - side / 2, cy + side / 2, cx + side / 2], -1)
    return np.round(np.clip(b, 0, [h - 1, w - 1, h - 1, w - 1])).astype(F32)


@functools.lru_cache(maxsize=None)
def _ragged_case():
    from dan_amd.train_sfd import ALL_ANCHOR_SCALES, ALL_LAYER_STRIDES, layer_shapes
    h = w = 320
    hs, ws, ds = zip(*[OA.get_anchors_width_height(ALL_ANCHOR_SCALES[i], (), (1.0,)) for i in range(6)])
    ref = OA.get_all_anchors((h, w), list(hs), list(ws), list(ds), [0.5] * 6, layer_shapes(h, w), ALL_LAYER_STRIDES, [float(h)] * 6, [False] * 6)
    return ref, [_faces(300, h, w, 31), _faces(1, h, w, 32), _faces(257, h, w, 33)]


@pytest.mark.parametrize("mining", [True, False])
def test_batched_encode_with_ragged_lists_of_300_1_and_257_boxes(mining, dev):
    """danhip_encode_anchors_batched with max_gt = 300: batch_colmax_kernel's gt axis (gridDim.y = max_gt, `if (g >= G) return` for the
    shorter lists), the per-anchor loops of batch_phase12_kernel over 300 / 257 columns of the [G,A] copy, goff offsets 0, 300, 301."""
    from dan_amd.train_sfd import AnchorConfig
    ref, gts = _ragged_case()
    assert [g.shape[0] for g in gts] == [300, 1, 257]
    thr = 0.4 if mining else 0.35
    cfg = AnchorConfig(320, 320, dev, match_threshold=thr, neg_threshold=thr)
    for got, want in zip(cfg.anchors[:4], ref[:4]):
        assert np.array_equal(got.cpu().numpy(), want)
    mf = (lambda ov: OE.small_mining_match(ov, 0., 0.4, 0.4, 6, 0.3)) if mining else (lambda ov: OA.do_dual_max_match(ov, 0.35, 0.35))
    T, L, S, M = cfg.enc.encode_anchors_batch([torch.from_numpy(g).to(dev) for g in gts], *cfg.anchors, match_mining=mining)
    all_a = np.stack(ref[:4], -1)
    for b, gt in enumerate(gts):
        want = OA.encode_anchors(gt, ref[:4], ref[4], thr, thr, PS, mf)
        if gt.shape[0] > BLOCK:                                                 # anchors are matched to gts beyond column 256
            assert np.asarray(mf(OA.iou_matrix(all_a, gt) * ref[4].astype(F32)[:, None])[0]).max() >= BLOCK
        assert (want[1] == 1).sum() > 0
        _assert_encoded((T[b].cpu().numpy(), L[b].cpu().numpy(), S[b].cpu().numpy(), M[b].cpu().numpy()), want, b)

"""Test-time pipeline of the reference's eval_dan.py / eval_sfd.py on the GPU: single-scale detection,
flip test, multi-scale tests and box voting, with the same function names, argument order and return layout
(eval_dan.py:95-297).  Images are uint8 HWC device tensors; detections are device tensors whose rows are
(xmin, ymin, xmax, ymax, score).  The image resize (cv2.resize in the reference) and the voting loop (numpy in the
reference) are libdanhip kernels; everything stays on the device until write_to_txt."""
import ctypes
import itertools

import numpy as np
import torch

from . import ops
from ._lib import ResizeItem, call, lib, ptr, stream

NMS_THRESHOLD = 0.3          # eval_dan.py:69-70
MEMORY_LIMIT = 577.0         # :71-72
MAX_PER_IMAGE = 750          # :73-74
SELECT_THRESHOLD = 0.01      # :75-76
FILTER_NONE, FILTER_BIG, FILTER_SMALL = 0, 1, 2          # a pass's size filter (danhip_detect_select's codes): none / max(w, h) > 30 / min(w, h) < 100


class Detector(object):
    """The `net` argument of the reference's helpers ([sess, image_input, bboxes_pred, cls_pred], eval_dan.py:452):
    image uint8 [H,W,3] -> (bboxes [A,4] as (ymin,xmin,ymax,xmax), scores [A]).  Anchors are cached per image size
    (the reference rebuilds them inside the graph from tf.shape, eval_dan.py:320-342)."""

    def __init__(self, model, anchor_config_fn, precision="act"):
        """precision: "act" = the library build's 16-bit activations (fast path, 3 k img/s); "fp32" = the fp32 inference kernels end to end,
        the path whose box outputs agree with an fp32 reference to 1e-4 (tests/test_eval_f32_gpu.py); "split" = the same graph with every
        convolution as a split-operand product on the fp16 MFMA (csrc/split_infer.hip): the same bound at about three times the fp32 path's rate."""
        if precision not in ("act", "fp32", "split"):
            raise ValueError("precision must be 'act', 'fp32' or 'split'")
        self.model = model
        self.model.precision = precision
        self.anchor_config_fn = anchor_config_fn
        self._anchors = {}

    def anchors(self, h, w, device):
        key = (int(h), int(w))
        if key not in self._anchors:
            self._anchors[key] = self.anchor_config_fn(key[0], key[1], device)
        return self._anchors[key]

    def __call__(self, image):
        assert image.dtype == torch.uint8 and image.dim() == 3 and image.shape[2] == 3
        a = self.anchors(image.shape[0], image.shape[1], image.device)
        boxes, scores = self.model.predict(image.unsqueeze(0).contiguous(), a)
        return boxes[0], scores[0]

    def batch(self, images):
        """B images of one size in ONE forward pass: uint8 [B,H,W,3] -> (bboxes [B,A,4], scores [B,A])."""
        assert images.dtype == torch.uint8 and images.dim() == 4 and images.shape[3] == 3
        a = self.anchors(images.shape[1], images.shape[2], images.device)
        return self.model.predict(images.contiguous(), a)


def resize_image(image, fx, fy):
    """cv2.resize(image, None, None, fx=fx, fy=fy, interpolation=cv2.INTER_LINEAR) (eval_dan.py:97)."""
    image = image.contiguous()
    H, W, C = image.shape
    Wo, Ho = int(np.rint(W * fx)), int(np.rint(H * fy))
    out = torch.empty((Ho, Wo, C), dtype=torch.uint8, device=image.device)
    call("danhip_resize_u8_linear", ptr(image), H, W, ptr(out), Ho, Wo, C, float(fx), float(fy), stream())
    return out


def _order_desc(scores):
    """argsort()[::-1]; ties resolved as a stable ascending sort read backwards (numpy's default sort leaves it open): libdanhip's
    arg-sort with ties_high_index_first.  The detections are fp32 (or fp32 values held in float64: bbox_vote's input); a caller that
    passes scores an fp32 cannot hold gets them rounded to fp32 first."""
    if scores.dtype != torch.float32:
        # every score of this pipeline is an fp32 softmax output (detect_face), at most carried in a float64 container (flip_test,
        # bbox_vote's input): the cast back is exact, and no host round trip checks it
        scores = scores.to(torch.float32)
    return ops.argsort_desc(scores.contiguous(), ties_high_index_first=True)


def detect_face(net, image, shrink, max_per_image=MAX_PER_IMAGE):
    """eval_dan.py:95-118 -> det fp32 [K,5]."""
    if shrink != 1:
        image = resize_image(image, shrink, shrink)
    bboxes, scores = net(image)
    s = torch.tensor(float(shrink), dtype=torch.float32, device=bboxes.device)        # a tensor: true division, not x * (1/s)
    det = torch.stack((bboxes[:, 1] / s, bboxes[:, 0] / s, bboxes[:, 3] / s, bboxes[:, 2] / s, scores.to(torch.float32)), dim=1)
    top = min(det.shape[0] - 1, int(max_per_image * 1.5))
    return det[_order_desc(det[:, 4])[:top]]


def _mirror_back(det, width):
    """flip_test's map back (eval_dan.py:191-198) on det fp32 [..., 5]: fp32 arithmetic (w - x) - 1 in a float64 container."""
    w = torch.tensor(float(width), dtype=torch.float32, device=det.device)
    det_t = torch.empty(det.shape, dtype=torch.float64, device=det.device)
    det_t[..., 0] = (w - det[..., 2]) - 1
    det_t[..., 1] = det[..., 1]
    det_t[..., 2] = (w - det[..., 0]) - 1
    det_t[..., 3] = det[..., 3]
    det_t[..., 4] = det[..., 4]
    return det_t


def flip_test(net, image, shrink, max_per_image=MAX_PER_IMAGE):
    """eval_dan.py:188-199: detections of the mirrored image mapped back."""
    return _mirror_back(detect_face(net, image.flip(1).contiguous(), shrink, max_per_image), image.shape[1])


def _big_mask(det):
    return torch.maximum(det[..., 2] - det[..., 0] + 1, det[..., 3] - det[..., 1] + 1) > 30


def _small_mask(det):
    return torch.minimum(det[..., 2] - det[..., 0] + 1, det[..., 3] - det[..., 1] + 1) < 100


def _filter_mask(det, filt):
    """The rows of det [..., 5] a FILTER_* code keeps (eval_dan.py:126,147-148,153,160-170), in det's own precision -> bool [...]."""
    if filt == FILTER_NONE:
        return torch.ones(det.shape[:-1], dtype=torch.bool, device=det.device)
    return _big_mask(det) if filt == FILTER_BIG else _small_mask(det)


# ---- the scale plan: which passes an image of a given size gets.  Stated once; the three forms below (per image, B images of one size,
# images of any sizes) are three ways of walking it.
def _multi_scale_passes(max_shrink):
    """multi_scale_test's passes (eval_dan.py:121-148): the st pass, then the bt passes, whose common filter is decided by the bt the
    doubling loop ends on."""
    st = 0.5 if max_shrink >= 0.75 else 0.5 * max_shrink
    bt = min(2, max_shrink) if max_shrink > 1 else (st + max_shrink) / 2
    bs = [bt]
    if max_shrink > 2:
        bt *= 2
        while bt < max_shrink:
            bs.append(bt)
            bt *= 2
        bs.append(max_shrink)
    return [(st, 0, FILTER_BIG)] + [(b, 0, FILTER_SMALL if bt > 1 else FILTER_BIG) for b in bs]


def _pyramid_passes(max_shrink):
    """multi_scale_test_pyramid's passes (eval_dan.py:151-175)."""
    return [(0.25, 0, FILTER_BIG)] + [(st, 0, FILTER_SMALL if st > 1 else FILTER_BIG) for st in (0.75, 1.25, 1.5, 1.75) if st <= max_shrink]


def scale_passes(height, width, pyramid=True, memory_limit=MEMORY_LIMIT):
    """The passes of eval_dan.py:452-459 for an image of this size, in its order: [(scale, mirrored, filter)] (host arithmetic on the
    size).  The mirrored pass carries no filter."""
    shrink, max_shrink = get_shrink(height, width, memory_limit)
    passes = [(shrink, 0, FILTER_NONE), (shrink, 1, FILTER_NONE)] + _multi_scale_passes(max_shrink)      # detect_face, flip_test
    return passes + _pyramid_passes(max_shrink) if pyramid else passes


def _serial_walk(net, image, passes, max_per_image=MAX_PER_IMAGE):
    """The passes on one image -> their kept rows in the passes' order, one compacted tensor per run of passes that share a filter (the
    boolean index reads its count on the host: once per run).  Filtering a run's concatenation gives the same rows in the same order as
    filtering pass by pass and concatenating, whichever of the two the reference does at that place."""
    out = []
    for (mirrored, filt), run in itertools.groupby(passes, key=lambda p: p[1:]):
        dets = [(flip_test if mirrored else detect_face)(net, image, scale, max_per_image) for scale, _, _ in run]
        det = dets[0] if len(dets) == 1 else torch.cat(dets, dim=0)
        out.append(det[_filter_mask(det, filt)] if filt else det)
    return out


def multi_scale_test(net, image, max_im_shrink):
    """eval_dan.py:121-148 -> (det_s, det_b)."""
    passes = _multi_scale_passes(max_im_shrink)
    return _serial_walk(net, image, passes[:1])[0], _serial_walk(net, image, passes[1:])[0]


def multi_scale_test_pyramid(net, image, max_shrink):
    """eval_dan.py:151-175."""
    return torch.cat(_serial_walk(net, image, _pyramid_passes(max_shrink)), dim=0)


def _vote(packed, counts, nms_threshold, max_per_image):
    """The library call: packed float64 [B, n, 5] contiguous, each image's first counts[b] rows in voting order, counts int32 [B]
    -> (out fp32 [B, max_per_image, 5], num int32 [B]) on the device."""
    B, n = packed.shape[:2]
    out = torch.empty((B, max_per_image, 5), dtype=torch.float32, device=packed.device)
    num = torch.empty((B,), dtype=torch.int32, device=packed.device)
    ws = torch.empty((lib().danhip_bbox_vote_workspace_bytes(B, n),), dtype=torch.uint8, device=packed.device)
    call("danhip_bbox_vote", ptr(packed), ptr(counts), B, n, float(nms_threshold), int(max_per_image), ptr(out), ptr(num), ptr(ws), ws.numel(), stream())
    return out, num


def _vote_masked(det, valid, nms_threshold, max_per_image):
    """Box voting over fixed-size blocks: det float64 [B, n, 5], valid bool [B, n] -> (out, num) as _vote; nothing is read on the host.
    The voting input is the valid rows in descending score order (ties: higher index first, as np.argsort()[::-1]); invalid rows carry
    -inf and fall behind every real score (scores are softmax outputs >= 0), and the relative index order of the valid rows is the order
    of the serial concatenation, so ties resolve alike."""
    key = torch.where(valid, det[..., 4].to(torch.float32), torch.full((), float("-inf"), dtype=torch.float32, device=det.device))
    order = torch.stack([ops.argsort_desc(key[b].contiguous(), ties_high_index_first=True) for b in range(det.shape[0])])
    packed = torch.gather(det, 1, order.unsqueeze(2).expand(-1, -1, 5)).contiguous()
    return _vote(packed, valid.sum(dim=1).to(torch.int32), nms_threshold, max_per_image)


def bbox_vote_batch(dets, nms_threshold=NMS_THRESHOLD, max_per_image=MAX_PER_IMAGE):
    """bbox_vote for a list of per-image detection sets in one launch (one workgroup per image).
    Precondition (as bbox_vote): scores are fp32 values, possibly held in float64 - they are ordered after rounding to fp32."""
    B = len(dets)
    dev = dets[0].device
    nmax = max(1, max(d.shape[0] for d in dets))
    packed = torch.zeros((B, nmax, 5), dtype=torch.float64, device=dev)
    for i, d in enumerate(dets):
        d = d.to(torch.float64)
        packed[i, :d.shape[0]] = d[_order_desc(d[:, 4])]
    counts = torch.tensor([d.shape[0] for d in dets], dtype=torch.int32, device=dev)
    out, num = _vote(packed, counts, nms_threshold, max_per_image)
    n = num.tolist()
    return [out[i, :n[i]] for i in range(B)]


def bbox_vote(det, nms_threshold=NMS_THRESHOLD, max_per_image=MAX_PER_IMAGE):
    """eval_dan.py:201-241 -> fp32 [K,5], K <= max_per_image.
    Precondition: the scores (column 4) are fp32 values, possibly carried in a float64 tensor - what this pipeline produces (softmax outputs
    of detect_face).  They are ordered as fp32 (_order_desc): float64 scores that differ only below fp32 precision become ties and are
    taken higher index first, not in their float64 order."""
    return bbox_vote_batch([det], nms_threshold, max_per_image)[0]


def get_shrink(height, width, memory_limit=MEMORY_LIMIT):
    """eval_dan.py:263-297 -> (shrink, max_shrink); host arithmetic, including the reference's truncation of the
    decimal representation to two places."""
    v1 = (0x7fffffff / memory_limit / (height * width)) ** 0.5
    v2 = ((678 * 1024 * 2.0 * 2.0) / (height * width)) ** 0.5
    x = min(v1, v2)
    text = str(x)
    if '.' not in text:
        raise ValueError("get_shrink: %r has no decimal point (the reference returns None here)" % x)
    head, tail = text.split('.')
    if len(tail) >= 3:
        x = float(head + '.' + tail[:2])
    m = x - 0.3
    if 1.5 <= m < 2:
        m = m - 0.1
    elif 2 <= m < 3:
        m = m - 0.2
    elif 3 <= m < 4:
        m = m - 0.3
    elif 4 <= m < 5:
        m = m - 0.4
    elif m >= 5:
        m = m - 0.5
    return (m if m < 1 else 1), m


def write_to_txt(f, det, event, im_name, select_threshold=SELECT_THRESHOLD, min_height=10):
    """eval_dan.py:243-261 (same text format); det may be a device tensor.  `event` is the WIDER-FACE event entry
    (event[0][0] is its name) or a plain string.  min_height: the row filter ceil(height) >= 10 of eval_dan.py / eval_sfd.py;
    eval_pb.py:252 has 9 (dan_amd/eval_pb.py passes it)."""
    det = det.detach().cpu().numpy() if torch.is_tensor(det) else np.asarray(det)
    name = event if isinstance(event, str) else event[0][0]
    xmin, ymin, xmax, ymax, sc = (det[:, i] for i in range(5))
    bh, bw = ymax - ymin + 1, xmax - xmin + 1
    valid = np.logical_and(np.logical_and(np.ceil(bh) >= min_height, bw > 1), sc > select_threshold)
    f.write('{:s}\n'.format(name + '/' + im_name + '.jpg'))
    f.write('{}\n'.format(np.count_nonzero(valid)))
    for i in range(valid.shape[0]):
        if valid[i]:
            f.write('{:.1f} {:.1f} {:.1f} {:.1f} {:.3f}\n'.format(np.floor(xmin[i]), np.floor(ymin[i]), np.ceil(bw[i]), np.ceil(bh[i]), sc[i]))


# ---- B images of ONE size, without a host round trip: the plan depends on the image SIZE only, so every pass runs as one batched forward;
# the size filters become validity masks over fixed-size [B, top] blocks instead of boolean compactions (whose output shape the host would
# have to read), and the voting kernel takes the per-image counts from the device.
def resize_images(images, fx, fy):
    B, H, W, C = images.shape
    Wo, Ho = int(np.rint(W * fx)), int(np.rint(H * fy))
    out = torch.empty((B, Ho, Wo, C), dtype=torch.uint8, device=images.device)
    images = images.contiguous()
    for b in range(B):
        call("danhip_resize_u8_linear", ptr(images[b]), H, W, ptr(out[b]), Ho, Wo, C, float(fx), float(fy), stream())
    return out


def detect_face_batch(net, images, shrink, max_per_image=MAX_PER_IMAGE):
    """detect_face for [B,H,W,3] -> det fp32 [B, top, 5], rows ordered as eval_dan.py:115-116 orders them."""
    if shrink != 1:
        images = resize_images(images, shrink, shrink)
    bboxes, scores = net.batch(images)
    s = torch.tensor(float(shrink), dtype=torch.float32, device=bboxes.device)
    det = torch.stack((bboxes[..., 1] / s, bboxes[..., 0] / s, bboxes[..., 3] / s, bboxes[..., 2] / s, scores.to(torch.float32)), dim=2)
    top = min(det.shape[1] - 1, int(max_per_image * 1.5))
    order = torch.stack([_order_desc(det[b, :, 4])[:top] for b in range(det.shape[0])])
    return torch.gather(det, 1, order.unsqueeze(2).expand(-1, -1, 5))


def detect_images(net, images, pyramid=True, nms_threshold=NMS_THRESHOLD, max_per_image=MAX_PER_IMAGE, memory_limit=MEMORY_LIMIT):
    """detect_image for a batch: uint8 [B,H,W,3] -> (dets fp32 [B, max_per_image, 5], num int32 [B]) on the device; rows beyond num[b]
    are unspecified.  Per image the result equals detect_image(net, images[b], ...) whenever the forward passes agree (a batched
    forward may take another split-K plan than a single image: same math, another fp32 summation order)."""
    H, W = int(images.shape[1]), int(images.shape[2])
    dets, valid = [], []
    for scale, mirrored, filt in scale_passes(H, W, pyramid, memory_limit):
        det = detect_face_batch(net, images.flip(2).contiguous() if mirrored else images, scale, max_per_image)
        valid.append(_filter_mask(det, filt))
        dets.append(_mirror_back(det, W) if mirrored else det.to(torch.float64))
    return _vote_masked(torch.cat(dets, dim=1), torch.cat(valid, dim=1), nms_threshold, max_per_image)


def detect_image(net, image, pyramid=True, nms_threshold=NMS_THRESHOLD, max_per_image=MAX_PER_IMAGE, memory_limit=MEMORY_LIMIT):
    """The per-image body of eval_dan.py:452-459 (eval_sfd.py:323-328 without the pyramid pass)."""
    dets = _serial_walk(net, image, scale_passes(int(image.shape[0]), int(image.shape[1]), pyramid, memory_limit), max_per_image)
    return bbox_vote(torch.cat([d.to(torch.float64) for d in dets], dim=0), nms_threshold, max_per_image)


# ---- images of DIFFERENT sizes, without a host round trip.  The forward passes stay per (image, scale); everything around them is
# size-agnostic: ONE launch makes every resized / mirrored copy of every image (danhip_resize_u8_linear_batch), one library call per pass does
# detect_face's cut and order, the size filter and flip_test's mirror map into the image's rows of the packed voting buffer
# (danhip_detect_select: a radix select instead of the arg-sort of all A anchors, no boolean compaction), and the voting tail is detect_images'.
def resize_image_batch(images, requests):
    """Every resized / mirrored copy in ONE launch: images = list of contiguous uint8 [H,W,3] device tensors (separate tensors or views into
    one buffer, at any byte offset), requests = [(image index, fx, fy, mirror)] -> list of uint8 [Ho,Wo,3] tensors (views into one buffer),
    request for request equal to resize_image(image.flip(1).contiguous() if mirror else image, fx, fy).  One pinned table, one upload."""
    n = len(requests)
    assert n > 0
    device = images[0].device
    for im in images:
        assert im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3 and im.is_contiguous() and im.device == device
    base = min(im.data_ptr() for im in images)                # "one source buffer": the span of the sources' addresses
    src_bytes = max(im.data_ptr() + im.numel() for im in images) - base
    nitem = ctypes.sizeof(ResizeItem)
    staging = torch.empty(n * nitem, dtype=torch.uint8, pin_memory=True)
    first, at, nt, shapes = 0, 0, ctypes.c_int32(0), []
    for k, (i, fx, fy, mirror) in enumerate(requests):
        H, W = int(images[i].shape[0]), int(images[i].shape[1])
        Wo, Ho = int(np.rint(W * fx)), int(np.rint(H * fy))
        call("danhip_resize_item_init", ctypes.c_void_p(staging.data_ptr() + k * nitem), images[i].data_ptr() - base, H, W, 3 * W, at, Ho, Wo,
             float(fx), float(fy), int(mirror), first, ctypes.byref(nt))
        first += nt.value
        shapes.append((at, Ho, Wo))
        at += (3 * Ho * Wo + 255) // 256 * 256
    table = staging.to(device, non_blocking=True)
    out = torch.empty(at, dtype=torch.uint8, device=device)
    call("danhip_resize_u8_linear_batch", ctypes.c_void_p(staging.data_ptr()), ptr(table), n, ctypes.c_void_p(base), src_bytes, ptr(out), at, stream())
    return [out[o:o + 3 * ho * wo].view(ho, wo, 3) for o, ho, wo in shapes]


def detect_select(bboxes, scores, shrink, top, rows, valid, filter=FILTER_NONE, mirror_width=None):
    """The tail of one pass on the device (danhip_detect_select): rows float64 [top,5] and valid uint8 [top] are written in place.
    -> the number of kernel launches the call issued (a constant: _lib.DETECT_SELECT_LAUNCHES)."""
    A = int(scores.shape[0])
    bboxes, scores = bboxes.to(torch.float32).contiguous(), scores.to(torch.float32).contiguous()
    assert tuple(bboxes.shape) == (A, 4) and tuple(rows.shape) == (top, 5) and rows.dtype == torch.float64 and rows.is_contiguous()
    assert tuple(valid.shape) == (top,) and valid.dtype == torch.uint8 and valid.is_contiguous()
    nbytes = int(lib().danhip_detect_select_workspace_bytes(A))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=scores.device)
    launches = ctypes.c_int32(0)
    call("danhip_detect_select", ptr(bboxes), ptr(scores), A, int(top), float(shrink), int(filter), -1.0 if mirror_width is None else float(mirror_width),
         ptr(rows), ptr(valid), ptr(ws), nbytes, ctypes.byref(launches), stream())
    return launches.value


def detect_image_list(net, images, pyramid=True, nms_threshold=NMS_THRESHOLD, max_per_image=MAX_PER_IMAGE, memory_limit=MEMORY_LIMIT):
    """detect_image for a list of uint8 [H_i,W_i,3] device tensors of ANY sizes (they may be views into one buffer, the JPEG decoder's)
    -> (dets fp32 [B, max_per_image, 5], num int32 [B]) on the device, the layout WiderEvaluator.add takes; rows beyond num[b] are
    unspecified.  Per image the result equals detect_image(net, images[b], ...): the forwards are the same batch-1 calls.  No device
    value is read on the host between the first launch and the return."""
    B = len(images)
    assert B > 0
    device = images[0].device
    images = [im.contiguous() for im in images]
    cap = int(max_per_image * 1.5)
    plans = [scale_passes(int(im.shape[0]), int(im.shape[1]), pyramid, memory_limit) for im in images]
    requests, where = [], {}                                                   # one copy per distinct (image, scale, mirrored)
    for i, plan in enumerate(plans):
        for scale, mirror, _ in plan:
            if (scale != 1 or mirror) and (i, scale, mirror) not in where:
                where[(i, scale, mirror)] = len(requests)
                requests.append((i, scale, scale, mirror))
    copies = resize_image_batch(images, requests)
    n = max(len(plan) for plan in plans) * cap
    det = torch.empty((B, n, 5), dtype=torch.float64, device=device)
    valid = torch.zeros((B, n), dtype=torch.uint8, device=device)
    for i, plan in enumerate(plans):
        at = 0
        for scale, mirror, filt in plan:
            image = copies[where[(i, scale, mirror)]] if (scale != 1 or mirror) else images[i]
            bboxes, scores = net(image)
            top = min(int(scores.shape[0]) - 1, cap)
            if top > 0:
                detect_select(bboxes, scores, scale, top, det[i, at:at + top], valid[i, at:at + top], filt,
                              float(images[i].shape[1]) if mirror else None)
            at += max(top, 0)
    return _vote_masked(det, valid.bool(), nms_threshold, max_per_image)


def detect_encoded(net, datas, decoder, pyramid=True, nms_threshold=NMS_THRESHOLD, max_per_image=MAX_PER_IMAGE, memory_limit=MEMORY_LIMIT):
    """JPEG byte strings -> detections: dataset.jpeg.JpegDecoder.decode_batch (device decode; a stream the decoder refuses, a progressive one
    by default, takes its Pillow fallback) -> detect_image_list on the decoder's views."""
    return detect_image_list(net, decoder.decode_batch(list(datas)), pyramid, nms_threshold, max_per_image, memory_limit)


def main(argv=None, **kw):
    """`python -m dan_amd.eval_dan --data_dir WIDER_ROOT --checkpoint_path M`: the reference's `python eval_dan.py` (dan_amd/eval_cli.py)."""
    from .eval_cli import main as run
    return run(argv, model="dan", **kw)


if __name__ == "__main__":
    main()

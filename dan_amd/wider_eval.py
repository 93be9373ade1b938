"""WIDER FACE average precision on the device: from the detections eval_dan.write_to_txt would print to the easy / medium / hard AP.

    gt = WiderGroundTruth.from_mat("wider_face_val.mat", "wider_easy_val.mat", "wider_medium_val.mat", "wider_hard_val.mat")
    ev = WiderEvaluator(gt)                          # quantize=True: exactly what the official tools read from the text files
    dets, num = eval_dan.detect_images(net, images)  # device tensors, no host round trip
    ev.add(image_indices, dets, num)
    ap = ev.result()                                 # {"easy": .., "medium": .., "hard": .., "curves": .., ...}

    python -m dan_amd.wider_eval --pred DIR --split-mat F --easy F --medium F --hard F

The protocol (the kernels of csrc/wider_eval_exact.hip and the numpy restatement of tests/wider_protocol.py follow this text; all arithmetic
is IEEE double in the order written, without FMA contraction):

 1. Scores become (score - lo) / (hi - lo), lo / hi = minimum / maximum over every detection of every image, images without ground truth
    included - the scores are normalised over the WHOLE SET, so an image's AP contribution depends on the others.  hi == lo: all 0.
 2. Within an image the detections are taken by descending score, equal scores by ascending original index.
 3. Per image and subset: count_face += number of kept boxes.  An image with no detection or no box adds nothing else - its detections
    are NOT false positives (the protocol's behaviour; kept).  Otherwise, with corners x2 = x + w, y2 = y + h, the overlap of detection b
    and box q is iw * ih / (area(b) + area(q) - iw * ih) when iw = min(b.x2, q.x2) - max(b.x1, q.x1) + 1 > 0 and ih (likewise) > 0, else 0,
    area = (x2 - x1 + 1) * (y2 - y1 + 1).  Walking the detections h in order: j = the FIRST box of maximum overlap; overlap >= 0.5: box j
    not kept -> recall[j] = -1 and proposal[h] = -1 (ignored), else recall[j] turns 1 if it was 0.  A second detection of a matched kept
    box keeps proposal[h] = 1: it IS a false positive, as is a detection without a match.  pred_recall[h] = #{j: recall[j] == 1}.
 4. For t = 0..T-1, thr = 1 - (t + 1) / T, r = the last detection with score >= thr (none: nothing is added):
    curve[s][t] += (#{h <= r: proposal[h] == 1}, pred_recall[r]); summed over all images, in integers.
 5. precision = curve[..][1] / curve[..][0], 0 where curve[..][0] == 0 (then curve[..][1] == 0 too and the value cannot reach the AP);
    recall = curve[..][1] / count_face; mrec = [0, recall, 1], mpre = [0, precision, 0], mpre[k-1] = max(mpre[k-1], mpre[k]) from the
    back, AP = sum over k with mrec[k+1] != mrec[k] of (mrec[k+1] - mrec[k]) * mpre[k+1].  count_face == 0: AP = 0 (and recall = 0).
"""
import argparse
import os

import numpy as np
import torch

from ._lib import call, lib, ptr, stream

MAX_DETS = 2048              # include/danhip.h DANHIP_WIDER_MAX_DETS: detections of one image the match kernel holds
MAX_SUBSETS = 8
MAX_THRESHOLDS = 2046
_F32, _F64 = 0, 4            # in_dtype of danhip_wider_quantize
_STATUS = ((1, "an image index outside the ground truth's images"), (2, "an image was added twice"),
           (4, "an image has more detections than the evaluator's bound"), (8, "malformed offsets"))


class WiderGroundTruth(object):
    """The ground truth as the CSR arrays the kernels read: offsets int32 [I+1], boxes float64 [G,4] rows (x, y, w, h), keep uint8 [G]
    with bit s = kept in subset s.  boxes_per_image: I arrays [n_i,4]; keep_per_image: I arrays [n_i,S] of 0 / 1; names: I strings "event/file" (what write_to_txt prints, without ".jpg")."""

    def __init__(self, boxes_per_image, keep_per_image, names=None, subsets=("easy", "medium", "hard")):
        self.subsets = tuple(subsets)
        S = len(self.subsets)
        if not 1 <= S <= MAX_SUBSETS:
            raise ValueError("between 1 and %d subsets" % MAX_SUBSETS)
        if len(boxes_per_image) != len(keep_per_image) or len(boxes_per_image) == 0:
            raise ValueError("boxes_per_image and keep_per_image list the same, non-zero number of images")
        offsets, boxes, keep = [0], [], []
        for b, k in zip(boxes_per_image, keep_per_image):
            b = np.asarray(b, dtype=np.float64).reshape(-1, 4)
            k = np.asarray(k).reshape(b.shape[0], S)
            if not np.isin(k, (0, 1)).all():
                raise ValueError("keep flags are 0 or 1")
            bits = np.zeros((b.shape[0],), np.uint8)
            for s in range(S):
                bits |= (k[:, s].astype(np.uint8) << s).astype(np.uint8)
            boxes.append(b)
            keep.append(bits)
            offsets.append(offsets[-1] + b.shape[0])
        self.offsets = np.asarray(offsets, dtype=np.int32)
        self.boxes = np.concatenate(boxes, axis=0) if boxes else np.zeros((0, 4))
        self.keep = np.concatenate(keep, axis=0) if keep else np.zeros((0,), np.uint8)
        self.names = list(names) if names is not None else None
        if self.names is not None and len(self.names) != self.num_images:
            raise ValueError("one name per image")
        self._device = {}

    @property
    def num_images(self):
        return len(self.offsets) - 1

    def index_of(self, name):
        if self.names is None:
            raise ValueError("this ground truth has no image names")
        if not hasattr(self, "_index"):
            self._index = {n: i for i, n in enumerate(self.names)}
        return self._index[name]

    def image(self, i):
        """(boxes [n,4], keep [n,S]) of image i, as numpy arrays."""
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        bits = self.keep[a:b]
        return self.boxes[a:b], np.stack([(bits >> s) & 1 for s in range(len(self.subsets))], axis=1).astype(np.uint8)

    def to(self, device):
        """(offsets, boxes, keep) on the device; at least one element each so that the pointers are never NULL."""
        key = str(device)
        if key not in self._device:
            boxes = self.boxes if self.boxes.shape[0] else np.zeros((1, 4))
            keep = self.keep if self.keep.shape[0] else np.zeros((1,), np.uint8)
            self._device[key] = (torch.from_numpy(self.offsets).to(device), torch.from_numpy(np.ascontiguousarray(boxes)).to(device),
                                 torch.from_numpy(np.ascontiguousarray(keep)).to(device))
        return self._device[key]

    @classmethod
    def from_mat(cls, split_mat, easy_mat, medium_mat, hard_mat):
        """The dataset's annotation files: split_mat holds face_bbx_list / event_list / file_list (events x images cells), each subset
        file a gt_list of the 1-based indices of the boxes it keeps."""
        import scipy.io                                              # only here: the module imports without scipy
        split = scipy.io.loadmat(split_mat)
        subs = [scipy.io.loadmat(p)["gt_list"] for p in (easy_mat, medium_mat, hard_mat)]

        def cells(a):                                                # a MATLAB N x 1 cell -> the list of its entries
            return list(np.asarray(a, dtype=object).reshape(-1))

        def text(a):
            return str(np.asarray(a).reshape(-1)[0])

        boxes, keep, names = [], [], []
        events = cells(split["event_list"])
        for e, event in enumerate(events):
            files = cells(cells(split["file_list"])[e])
            bbx = cells(cells(split["face_bbx_list"])[e])
            kept = [cells(cells(g)[e]) for g in subs]
            for i, f in enumerate(files):
                b = np.asarray(bbx[i], dtype=np.float64).reshape(-1, 4)
                k = np.zeros((b.shape[0], 3), np.uint8)
                for s in range(3):
                    idx = np.asarray(kept[s][i]).reshape(-1).astype(np.int64)
                    k[idx - 1, s] = 1
                boxes.append(b)
                keep.append(k)
                names.append(text(event) + "/" + text(f))
        return cls(boxes, keep, names=names)


class WiderEvaluator(object):
    """Collects detections on the device and computes the AP there.  quantize=True (default): add() / add_rows() take fp32 rows
    (xmin, ymin, xmax, ymax, score) - what eval_dan.detect_images returns - and first apply what write_to_txt does to them, so the result
    is the one the official tools compute from the text files.  quantize=False: rows are (x, y, w, h, score) and pass unchanged.
    The store is a [I, max_per_image, 5] float64 tensor (97 MB for the 3226 validation images at 750 rows)."""

    def __init__(self, gt, quantize=True, iou_threshold=0.5, thresholds=1000, max_per_image=750, device="cuda"):
        if not 1 <= int(thresholds) <= MAX_THRESHOLDS:
            raise ValueError("thresholds between 1 and %d" % MAX_THRESHOLDS)
        if not 1 <= int(max_per_image) <= MAX_DETS:
            raise ValueError("max_per_image between 1 and %d (the match kernel's bound)" % MAX_DETS)
        self.gt, self.quantize, self.iou_threshold, self.T, self.cap = gt, bool(quantize), float(iou_threshold), int(thresholds), int(max_per_image)
        self.device = torch.device(device)
        I = gt.num_images
        self.rows = torch.zeros((I, self.cap, 5), dtype=torch.float64, device=self.device)
        self.counts = torch.full((I,), -1, dtype=torch.int32, device=self.device)
        self.status = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self._seen = set()

    def add(self, image_index, dets, num):
        """dets [B, Nmax, 5], num [B] as eval_dan.detect_images returns them, image_index the B images' indices in the ground truth (list or
        int tensor).  No host synchronisation; a list (or host tensor) of indices is checked for repeats here, a device tensor in result()."""
        if dets.dim() != 3 or dets.shape[2] != 5 or dets.shape[1] < 1:
            raise ValueError("dets is [B, Nmax, 5]")
        B, nmax = dets.shape[0], dets.shape[1]
        if nmax > self.cap:
            raise ValueError("dets holds %d rows per image, the evaluator was built for %d (max_per_image)" % (nmax, self.cap))
        if not (torch.is_tensor(image_index) and image_index.is_cuda):
            idx = [int(i) for i in (image_index.tolist() if torch.is_tensor(image_index) else image_index)]
            for i in idx:
                if not 0 <= i < self.gt.num_images:
                    raise IndexError("image index %d outside the ground truth's %d images" % (i, self.gt.num_images))
                if i in self._seen:
                    raise ValueError("image %d was added before" % i)
            if len(set(idx)) != len(idx):
                raise ValueError("an image index is listed twice")
            self._seen.update(idx)
            image_index = torch.tensor(idx, dtype=torch.int32).to(self.device, non_blocking=True)
        image_index = image_index.to(torch.int32).contiguous()
        if image_index.numel() != B or num.numel() != B:
            raise ValueError("one image index and one count per image")
        if self.quantize or dets.dtype != torch.float64:
            dets = dets.to(device=self.device, dtype=torch.float32)
        dets = dets.to(self.device).contiguous()
        num = num.to(device=self.device, dtype=torch.int32).contiguous()
        call("danhip_wider_quantize", ptr(dets), _F64 if dets.dtype == torch.float64 else _F32, ptr(num), ptr(image_index), B, nmax, int(self.quantize),
             ptr(self.rows), ptr(self.counts), self.gt.num_images, self.cap, ptr(self.status), stream())

    def add_rows(self, image_index, rows):
        """One image's [n, 5] rows (n may be 0)."""
        rows = torch.as_tensor(rows)
        n = rows.shape[0]
        if n == 0:
            rows = torch.zeros((1, 5), dtype=torch.float32)
        self.add([int(image_index)], rows.reshape(1, -1, 5), torch.tensor([n], dtype=torch.int32))

    def result(self):
        """{subset: AP, "curves": int64 [S,T,2], "count_face": int64 [S], "precision" / "recall": float64 [S,T], "score_range": (lo, hi)}.
        The only place that reads back to the host; the number of launches does not depend on the number of images.  Images never added
        count as images without detections."""
        gt, dev, T = self.gt, self.device, self.T
        I, S = gt.num_images, len(gt.subsets)
        counts = self.counts.clamp(min=0)
        offsets = torch.zeros((I + 1,), dtype=torch.int32, device=dev)
        offsets[1:] = torch.cumsum(counts, 0)
        head = torch.cat((self.status, offsets[-1:])).tolist()        # the one read-back before the evaluation: status word and D
        self._raise_on(head[0])
        D = int(head[1])
        mask = torch.arange(self.cap, device=dev, dtype=torch.int32).unsqueeze(0) < counts.unsqueeze(1)
        det_rows = self.rows[mask].contiguous() if D else torch.zeros((1, 5), dtype=torch.float64, device=dev)
        assert det_rows.shape[0] == max(D, 1)
        g_off, g_boxes, g_keep = gt.to(dev)
        G = int(gt.boxes.shape[0])
        L = lib()
        rng = torch.empty((2,), dtype=torch.float64, device=dev)
        ws_r = torch.empty((L.danhip_wider_score_range_workspace_bytes(),), dtype=torch.uint8, device=dev)
        call("danhip_wider_score_range", ptr(det_rows), D, ptr(rng), ptr(ws_r), ws_r.numel(), stream())
        ws = torch.empty((L.danhip_wider_eval_workspace_bytes(I, S, T),), dtype=torch.uint8, device=dev)
        call("danhip_wider_eval", ptr(offsets), ptr(det_rows), D, ptr(g_off), ptr(g_boxes), ptr(g_keep), G, ptr(rng), I, S, T, self.cap,
             self.iou_threshold, ptr(ws), ws.numel(), ptr(self.status), stream())
        curves = torch.empty((S, T, 2), dtype=torch.int64, device=dev)
        faces = torch.empty((S,), dtype=torch.int64, device=dev)
        prec = torch.empty((S, T), dtype=torch.float64, device=dev)
        rec = torch.empty((S, T), dtype=torch.float64, device=dev)
        ap = torch.empty((S,), dtype=torch.float64, device=dev)
        call("danhip_wider_ap", ptr(ws), ws.numel(), ptr(g_keep), G, I, S, T, ptr(curves), ptr(faces), ptr(prec), ptr(rec), ptr(ap), stream())
        tail = torch.cat((ap, rng, self.status.to(torch.float64))).tolist()
        self._raise_on(int(tail[-1]))
        out = {name: tail[s] for s, name in enumerate(gt.subsets)}
        out.update(curves=curves.cpu().numpy(), count_face=faces.cpu().numpy(), precision=prec.cpu().numpy(), recall=rec.cpu().numpy(),
                   score_range=(tail[S], tail[S + 1]))
        return out

    @staticmethod
    def _raise_on(status):
        what = [text for bit, text in _STATUS if status & bit]
        if what:
            raise ValueError("WiderEvaluator: " + "; ".join(what))


def parse_pred_text(text):
    """The records write_to_txt writes: "event/name.jpg", the number of rows, the rows "x y w h score" -> {"event/name": float64 [n,5]}."""
    out = {}
    lines = [l.strip() for l in text.splitlines() if l.strip()]
    p = 0
    while p < len(lines):
        name = lines[p]
        name = name[:-4] if name.lower().endswith(".jpg") else name
        n = int(lines[p + 1])
        rows = np.array([[float(v) for v in lines[p + 2 + k].split()] for k in range(n)], dtype=np.float64).reshape(n, 5)
        if name in out:
            raise ValueError("image %s appears twice" % name)
        out[name] = rows
        p += 2 + n
    return out


def read_pred_dir(path):
    """Every *.txt under path (the official layout is path/event/name.txt, one record per file) -> {"event/name": float64 [n,5]}."""
    out = {}
    for root, _, files in sorted(os.walk(path)):
        for f in sorted(files):
            if f.endswith(".txt"):
                with open(os.path.join(root, f)) as fh:
                    for k, v in parse_pred_text(fh.read()).items():
                        if k in out:
                            raise ValueError("image %s appears twice under %s" % (k, path))
                        out[k] = v
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="WIDER FACE easy / medium / hard AP of a directory of prediction files (host parsing, device evaluation)")
    ap.add_argument("--pred", required=True)
    ap.add_argument("--split-mat", required=True)
    ap.add_argument("--easy", required=True)
    ap.add_argument("--medium", required=True)
    ap.add_argument("--hard", required=True)
    a = ap.parse_args(argv)
    gt = WiderGroundTruth.from_mat(a.split_mat, a.easy, a.medium, a.hard)
    pred = read_pred_dir(a.pred)
    cap = max([1] + [v.shape[0] for v in pred.values()])
    ev = WiderEvaluator(gt, quantize=False, max_per_image=cap)
    for name, rows in pred.items():
        ev.add_rows(gt.index_of(name), torch.from_numpy(rows))
    res = ev.result()
    for s in gt.subsets:
        print("%s AP: %.6f" % (s, res[s]))
    return res


if __name__ == "__main__":
    main()

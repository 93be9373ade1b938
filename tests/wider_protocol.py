"""The WIDER FACE evaluation protocol, restated in plain numpy loop by loop from its definition (dan_amd/wider_eval.py's docstring, steps
1-5).  This is the yardstick of the device evaluator's tests: nothing here is vectorised cleverly, every quantity is a Python float
(IEEE double) computed in the order the definition writes it.  Also: a parser for the text eval_dan.write_to_txt writes."""
import io

import numpy as np


def overlap(b, q):
    """b, q = (x1, y1, x2, y2) corners; the +1 convention."""
    iw = min(b[2], q[2]) - max(b[0], q[0]) + 1
    ih = min(b[3], q[3]) - max(b[1], q[1]) + 1
    if iw > 0 and ih > 0:
        area_b = (b[2] - b[0] + 1) * (b[3] - b[1] + 1)
        area_q = (q[2] - q[0] + 1) * (q[3] - q[1] + 1)
        return iw * ih / (area_b + area_q - iw * ih)
    return 0.0


def best_boxes(dets, boxes):
    """For every detection (x, y, w, h, ..) the maximum overlap over the boxes (x, y, w, h) and the FIRST index that reaches it."""
    gt = [(float(q[0]), float(q[1]), float(q[0]) + float(q[2]), float(q[1]) + float(q[3])) for q in boxes]
    out = []
    for d in dets:
        b = (float(d[0]), float(d[1]), float(d[0]) + float(d[2]), float(d[1]) + float(d[3]))
        best, j = None, -1
        for k in range(len(gt)):
            o = overlap(b, gt[k])
            if best is None or o > best:                             # strict: the first index of the maximum
                best, j = o, k
        out.append((best, j))
    return out


def image_eval(matches, keep, iou_threshold):
    """The walk of step 3 for one image and subset: matches = best_boxes(...) in evaluation order, keep [m] -> (pred_recall [n], proposal [n])."""
    n, m = len(matches), len(keep)
    recall = [0] * m
    proposal = [1] * n
    pred_recall = [0] * n
    for h in range(n):
        best, j = matches[h]
        if best >= iou_threshold:
            if keep[j] == 0:
                recall[j] = -1
                proposal[h] = -1
            elif recall[j] == 0:
                recall[j] = 1
        pred_recall[h] = sum(1 for r in recall if r == 1)
    return pred_recall, proposal


def evaluate(dets_per_image, boxes_per_image, keep_per_image, num_subsets, iou_threshold=0.5, thresholds=1000):
    """dets_per_image: I arrays [n_i,5] rows (x, y, w, h, score); boxes_per_image: I arrays [m_i,4]; keep_per_image: I arrays [m_i,S].
    -> dict(ap [S], curves int64 [S,T,2], count_face [S], precision [S,T], recall [S,T], lo, hi, per_image = {(i, s): (pred_recall, proposal)})."""
    I, S, T = len(dets_per_image), num_subsets, thresholds
    dets_per_image = [np.asarray(d, dtype=np.float64).reshape(-1, 5) for d in dets_per_image]
    boxes_per_image = [np.asarray(b, dtype=np.float64).reshape(-1, 4) for b in boxes_per_image]
    keep_per_image = [np.asarray(k).reshape(len(b), S) for k, b in zip(keep_per_image, boxes_per_image)]
    # step 1
    lo, hi = None, None
    for d in dets_per_image:
        for row in d:
            s = float(row[4])
            lo = s if lo is None or s < lo else lo
            hi = s if hi is None or s > hi else hi
    if lo is None:
        lo = hi = 0.0
    normed = []
    for d in dets_per_image:
        rows = []
        for row in d:
            s = 0.0 if hi == lo else (float(row[4]) - lo) / (hi - lo)
            rows.append((float(row[0]), float(row[1]), float(row[2]), float(row[3]), s))
        # step 2: descending score, equal scores by ascending original index
        order = sorted(range(len(rows)), key=lambda k: (-rows[k][4], k))
        normed.append([rows[k] for k in order])
    curves = np.zeros((S, T, 2), dtype=np.int64)
    count_face = np.zeros((S,), dtype=np.int64)
    per_image = {}
    for i in range(I):
        dets, boxes = normed[i], boxes_per_image[i]
        for s in range(S):
            count_face[s] += sum(int(v) for v in keep_per_image[i][:, s])          # step 3
        if len(dets) == 0 or len(boxes) == 0:
            continue
        matches = best_boxes(dets, boxes)                            # the same for every subset
        scores = np.array([d[4] for d in dets], dtype=np.float64)
        for s in range(S):
            keep = [int(v) for v in keep_per_image[i][:, s]]
            pred_recall, proposal = image_eval(matches, keep, iou_threshold)
            per_image[(i, s)] = (pred_recall, proposal)
            proposal_arr = np.array(proposal)
            for t in range(T):                                       # step 4
                thr = 1 - (t + 1) / T
                r_index = np.where(scores >= thr)[0]
                if len(r_index) == 0:
                    continue
                r = int(r_index[-1])
                curves[s, t, 0] += len(np.where(proposal_arr[:r + 1] == 1)[0])
                curves[s, t, 1] += pred_recall[r]
    precision = np.zeros((S, T))
    recall = np.zeros((S, T))
    ap = np.zeros((S,))
    for s in range(S):                                               # step 5
        for t in range(T):
            c0, c1 = int(curves[s, t, 0]), int(curves[s, t, 1])
            precision[s, t] = 0.0 if c0 == 0 else c1 / c0
            recall[s, t] = 0.0 if count_face[s] == 0 else c1 / int(count_face[s])
        if count_face[s] == 0:
            continue
        mrec = [0.0] + [float(v) for v in recall[s]] + [1.0]
        mpre = [0.0] + [float(v) for v in precision[s]] + [0.0]
        for k in range(len(mpre) - 1, 0, -1):
            mpre[k - 1] = max(mpre[k - 1], mpre[k])
        total = 0.0
        for k in range(len(mrec) - 1):
            if mrec[k + 1] != mrec[k]:
                total += (mrec[k + 1] - mrec[k]) * mpre[k + 1]
        ap[s] = total
    return dict(ap=ap, curves=curves, count_face=count_face, precision=precision, recall=recall, lo=lo, hi=hi, per_image=per_image)


def parse_pred_text(text):
    """write_to_txt's records ("event/name.jpg", number of rows, rows "x y w h score") -> {"event/name": float64 [n,5]}."""
    out = {}
    lines = [l for l in text.split("\n") if l.strip() != ""]
    p = 0
    while p < len(lines):
        name = lines[p].strip()
        assert name.endswith(".jpg"), name
        n = int(lines[p + 1])
        rows = np.zeros((n, 5), dtype=np.float64)
        for k in range(n):
            parts = lines[p + 2 + k].split()
            assert len(parts) == 5, lines[p + 2 + k]
            rows[k] = [float(v) for v in parts]
        out[name[:-4]] = rows
        p += 2 + n
    return out


def text_route(write_to_txt, det_fp32, event="ev", name="im"):
    """One image's fp32 rows (xmin, ymin, xmax, ymax, score) through write_to_txt and back: float64 [n,5] rows (x, y, w, h, score)."""
    f = io.StringIO()
    write_to_txt(f, np.asarray(det_fp32, dtype=np.float32).reshape(-1, 5), event, name)
    return parse_pred_text(f.getvalue())[event + "/" + name]

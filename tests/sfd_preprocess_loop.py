"""Loop-by-loop numpy restatement of the host half of the reference's preprocessing/sfd_preprocessing.py (a helper, not a test:
tests/test_sfd_preprocess_cpu.py compares dan_amd/preprocessing/sfd_preprocessing.py with it).  Written from the reference's lines, one
statement per statement, one box at a time, float32 like the tf ops; every random op takes its value from `d` in the order the code
reaches it.  ScriptedDraws replays the draws of tests/golden/sfd_preprocess_kats.json."""
import numpy as np

F = np.float32
ORDERINGS = {0: ("brightness", "saturation", "hue", "contrast"), 1: ("saturation", "brightness", "contrast", "hue"),
             2: ("contrast", "hue", "brightness", "saturation"), 3: ("hue", "saturation", "contrast", "brightness")}     # :117-145


class ScriptedDraws(object):
    """Replays a recorded list of [kind, value]; a draw of another kind, or an integer outside the asked range, is an error."""

    def __init__(self, script):
        self.script, self.at = list(script), 0

    def _next(self, kind):
        assert self.at < len(self.script), "draw %d (%s) past the end of the script" % (self.at, kind)
        k, v = self.script[self.at]
        assert k == kind, "draw %d is %s, the code asked for %s" % (self.at, k, kind)
        self.at += 1
        return v

    def uniform(self, lo, hi):
        v = F(self._next("uniform"))
        assert F(lo) <= v <= F(hi)
        return v

    def randint(self, lo, hi):
        v = int(self._next("randint"))
        assert lo <= v < max(hi, lo + 1), (lo, v, hi)
        return v

    def choice(self, n):
        v = int(self._next("choice"))
        assert 0 <= v < n
        return v

    def done(self):
        return self.at == len(self.script)


def patch_wrapper_loop(height, width, bboxes, d):
    """sfd_preprocessing.py:353-436 -> ((y, x, h, w), [box, ...])."""
    fh, fw = F(height), F(width)
    shorter = min(fh, fw)                                                       # :408
    patch_list = [d.uniform(0.3, 1.), d.uniform(0.3, 1.), d.uniform(0.3, 1.), d.uniform(0.3, 1.), F(1.)]     # :411-416
    side = int(F(patch_list[d.choice(5)]) * shorter)                             # :417-418
    n = len(bboxes)
    cx = [F(F(bboxes[i][1] + bboxes[i][3]) / F(2)) for i in range(n)]            # :381
    cy = [F(F(bboxes[i][0] + bboxes[i][2]) / F(2)) for i in range(n)]
    index, roi, mask = 0, [F(0), F(0), fh - F(1), fw - F(1)], [False] * n        # :376-380
    while (sum(mask) < 1 and index < 25) or index < 1:                           # :383-386
        x = d.randint(0, width - side + 1)                                       # :389
        y = d.randint(0, height - side + 1)                                      # :390
        roi = [F(y), F(x), F(y + side) - F(1), F(x + side) - F(1)]               # :392
        mask = [bool(cy[i] > roi[0] and cx[i] > roi[1] and cy[i] < roi[2] and cx[i] < roi[3]) for i in range(n)]     # :394-396
        index += 1
    if sum(mask) > 0:                                                            # :404-405
        kept = [bboxes[i] for i in range(n) if mask[i]]
    else:                                                                        # :358-373 sample_around_bbox
        t = d.randint(0, n)                                                      # :364
        rcx, rcy = F(F(bboxes[t][1] + bboxes[t][3]) / F(2)), F(F(bboxes[t][0] + bboxes[t][2]) / F(2))
        half = F(F(side) / F(2))
        roi = [max(F(rcy - half), F(0)), max(F(rcx - half), F(0)), min(F(rcy + half), fh - F(1)), min(F(rcx + half), fw - F(1))]
        kept = [bboxes[i] for i in range(n) if cy[i] >= roi[0] and cx[i] >= roi[1] and cy[i] <= roi[2] and cx[i] <= roi[3]]
    win = (int(roi[0]), int(roi[1]), int(F(F(roi[2] - roi[0]) + F(1))), int(F(F(roi[3] - roi[1]) + F(1))))      # tf.to_int32 truncates
    out = []
    for b in kept:                                                               # :423-434
        ymin, xmin, ymax, xmax = F(b[0] - F(win[0])), F(b[1] - F(win[1])), F(b[2] - F(win[0])), F(b[3] - F(win[1]))
        cymin, cxmin = max(F(0), ymin), max(F(0), xmin)
        cymax, cxmax = min(F(win[2]) - F(1), ymax), min(F(win[3]) - F(1), xmax)
        out.append([min(cymin, cymax), min(cxmin, cxmax), cymax, cxmax])
    return win, out


def draw_for_train_loop(height, width, bboxes, out_shape, d):
    """The random and box half of preprocess_for_train (:495-552) -> (ops, window, flip, [box, ...] after the small-box filter)."""
    ordering = d.randint(0, 4)                                                   # :515-517
    ops = []
    for name in ORDERINGS[ordering]:                                             # :117-145, fast_mode=False
        if name == "brightness":
            ops.append((name, d.uniform(-32. / 255., 32. / 255.)))
        elif name == "hue":
            ops.append((name, d.uniform(-0.2, 0.2)))
        else:
            ops.append((name, d.uniform(0.5, 1.5)))
    win, boxes = patch_wrapper_loop(height, width, bboxes, d)                    # :519
    flip = bool(d.uniform(0., 1.) < 0.5)                                         # :485-486
    if flip:                                                                     # :490-492, about the WINDOW's width (before the resize)
        w = F(win[3])
        boxes = [[b[0], F(F(w - F(1.)) - b[3]), b[2], F(F(w - F(1.)) - b[1])] for b in boxes]
    th, tw, fh, fw = F(out_shape[0]), F(out_shape[1]), F(win[2]), F(win[3])      # :524-530
    out = []
    for b in boxes:
        ymin, ymax = F(F(b[0] * th) / fh), F(F(b[2] * th) / fh)
        xmin, xmax = F(F(b[1] * tw) / fw), F(F(b[3] * tw) / fw)
        if F(ymax - ymin) > F(6.) and F(xmax - xmin) > F(3.):                    # :544-551
            out.append([ymin, xmin, ymax, xmax])
    return ops, win, flip, out

"""Stand-ins for the test-time pipeline's tests (a helper, not a test): a deterministic network whose boxes / scores derive from the image
content with integer arithmetic only, so that the project and oracle/evalpipe.py see identical raw detections, and a recorder of the
library calls a pipeline form makes."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_trace  # noqa: E402

ANCHORS = 1500                   # what the stand-in answers per image, at every size


def fake_net_np(image):
    """Deterministic stand-in for sess.run: uint8 [H,W,3] array -> (boxes fp32 [ANCHORS,4] as (ymin,xmin,ymax,xmax), scores fp32 [ANCHORS])."""
    h, w = image.shape[:2]
    key = (int(image.astype(np.int64).sum()) + 7919 * h + 104729 * w) % (2 ** 31 - 1)
    rng = np.random.RandomState(key)
    n = ANCHORS
    cy, cx = rng.rand(n) * h, rng.rand(n) * w
    s = np.exp(rng.rand(n) * np.log(40)) * 6
    face = rng.randint(0, 12, n)                                              # 12 "faces" get many hits -> clusters across scales
    fy, fx, fs = (np.arange(12) * 37 % 11 + 1) / 12.0 * h, (np.arange(12) * 53 % 11 + 1) / 12.0 * w, (np.arange(12) % 4 + 1) * 0.06 * min(h, w)
    hit = rng.rand(n) < 0.5
    cy = np.where(hit, fy[face] + rng.randn(n) * fs[face] * 0.05, cy)
    cx = np.where(hit, fx[face] + rng.randn(n) * fs[face] * 0.05, cx)
    s = np.where(hit, fs[face] * (1 + rng.randn(n) * 0.05), s)
    boxes = np.stack([cy - s / 2, cx - s / 2, cy + s / 2, cx + s / 2], 1).astype(np.float32)
    scores = np.where(hit, 0.5 + rng.rand(n) * 0.5, rng.rand(n) * 0.3).astype(np.float32)
    return boxes, scores


def fake_net_torch(image):
    b, s = fake_net_np(image.cpu().numpy())
    return torch.from_numpy(b).to(image.device), torch.from_numpy(s).to(image.device)


class FakeNet(object):
    """The stand-in as a `net` with the Detector's two entry points: per image, or B images of one size in one call.  It makes no library
    call of its own; `shown` counts the images __call__ was given, `batches` the calls of batch."""

    def __init__(self):
        self.shown = self.batches = 0

    def __call__(self, image):
        self.shown += 1
        return fake_net_torch(image)

    def batch(self, images):
        self.batches += 1
        outs = [fake_net_torch(images[b]) for b in range(images.shape[0])]
        return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])


def traced(P, fn):
    """fn() with every library call of eval_dan / ops recorded by tests/launch_trace.py's Recorder AND carried out -> (result, call names)."""
    from dan_amd import ops
    rec = launch_trace.Recorder()
    real_p, real_o = P.call, ops.call

    def both(real):
        def call(name, *args):
            rec.call(name, *args)
            return real(name, *args)
        return call
    P.call, ops.call = both(real_p), both(real_o)
    try:
        result = fn()
    finally:
        P.call, ops.call = real_p, real_o
    return result, [e[1] for e in rec.events if e[0] == "call"]

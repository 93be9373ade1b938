"""One bottleneck unit of the ResNet backbone (net/resnet_danet.py bottleneck_block) against the oracle unit in float64: the case generator,
the oracle runs (float64, 16-bit storage emulation, and the unit with its shortcut's gradient scaled - the fault a gradient test must see),
the per-tensor relative L2 error and the bounds.  Shared by tests/test_resnet_unit_cpu.py (no GPU: the bounds restate their measurement, and a
missing or doubled shortcut gradient exceeds them) and tests/test_resnet_gpu.py (the device unit against the same reference).

Bound.  r0(kind, training) is the worst per-tensor relative L2 distance, over seeds 0..4, between the oracle unit in float64 and the same unit
with 16-bit storage emulated (Params(emulate_bf16=True): packed weights, stored activations and their gradients rounded to bf16, fp32
arithmetic) - the error of the number format itself.  The device may differ from float64 by that much and by its own fp32 summation order:
BOUND = 2 r0.  r0 is 0.08 .. 0.11: the forward output differs by 0.005 only, but a pre-activation within rounding of zero lands on the other
side in one of the two runs, and a flipped mask element carries its whole gradient, so the L2 error goes with the square root of the flipped
fraction.  The worst tensor is a gradient of the `reduce` or 3x3 layer's beta or kernel, behind two or three such masks.  (The figures and the device's errors:
tests/test_resnet_gpu.py.)"""
import torch
import torch.nn.functional as F

from oracle import nets as ON
from oracle import tf_ops as T

F64 = torch.float64
SCOPE = "unit"
N, H, W = 2, 15, 17                 # odd map: the strided unit samples its last row and column; 510 positions for the batch statistics
# kind -> (input channels, filters, need_reduce, is_root): block_1/conv_1 (projection, stride 1), block_2/conv_1 (projection and reduce at
# stride 2), block_1/conv_2 (identity shortcut)
UNITS = {"root": (64, 128, True, True), "strided": (256, 256, True, False), "identity": (256, 128, False, False)}
SEEDS = (0, 1, 2, 3, 4)
# r0 per (kind, training), measured on the CPU over SEEDS (tests/test_resnet_unit_cpu.py re-measures it); BOUND = 2 r0
R0 = {("root", False): 0.08349, ("root", True): 0.11252, ("strided", False): 0.08518, ("strided", True): 0.09138, ("identity", False): 0.08336,
      ("identity", True): 0.10156}


def bound(kind, training):
    return 2.0 * R0[(kind, training)]


def make_case(kind, seed):
    """-> (variables {name: float64}, x [N,H,W,Cin] and the upstream gradient dy, both float64 holding bf16 values).  Glorot kernels as the
    oracle creates them, non-trivial BN parameters and moving statistics (as tests/test_resnet_gpu._setup makes them)."""
    cin, filters, need_reduce, is_root = UNITS[kind]
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn((N, H, W, cin), generator=g).to(torch.bfloat16).to(F64)
    P = ON.Params(create=True, seed=77 + seed, dtype=F64)
    with torch.no_grad():
        out = ON.bottleneck_block(P, x, filters, SCOPE, False, need_reduce, is_root)
    for n in sorted(P.t):
        shape = P.t[n].shape
        if n.endswith("/bn/gamma") or n.endswith("/bn/moving_variance"):
            P.t[n] = (0.5 + torch.rand(shape, generator=g)).to(F64)
        elif n.endswith("/bn/beta") or n.endswith("/bn/moving_mean"):
            P.t[n] = (0.2 * torch.randn(shape, generator=g)).to(F64)
    dy = torch.randn(tuple(out.shape), generator=g).to(torch.bfloat16).to(F64)
    return dict(P.t), x, dy


def trainable(tensors):
    return sorted(n for n in tensors if "/moving_" not in n)


def shortcut_kernel(kind):
    return SCOPE + "/shortcut/conv2d/kernel" if UNITS[kind][2] else None


class _ScaleGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale):
        ctx.scale = scale
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return g * ctx.scale, None


def unit_with_scaled_shortcut(P, x, filters, training, need_reduce, is_root, scale):
    """oracle.nets.bottleneck_block restated with the gradient that flows back through the shortcut multiplied by `scale` (0: the shortcut
    contributes nothing to the backward pass, 2: it is handed over twice); scale = 1 is the oracle unit (asserted by the CPU test)."""
    s = 1 if (not need_reduce) or is_root else 2
    shortcut = ON.conv_bn(P, x, filters * 2, (1, 1), s, SCOPE + "/shortcut", training, "valid") if need_reduce else x
    shortcut = _ScaleGrad.apply(shortcut, scale)
    y = ON.conv_bn(P, x, filters // 2, (1, 1), s, SCOPE + "/reduce", training, "valid", relu=True)
    y = ON.conv_bn(P, F.pad(y, (0, 0, 1, 1, 1, 1)), filters // 2, (3, 3), 1, SCOPE + "/block_3x3", training, "valid", relu=True)
    y = ON.conv_bn(P, y, filters * 2, (1, 1), 1, SCOPE + "/increase", training)
    out = torch.relu(y + shortcut)
    return T.round_bf16(out, True, True) if P.emulate_bf16 else out


def oracle_unit(kind, training, tensors, x, dy, emulate=False, shortcut_scale=None):
    """-> {"out", "dx", every trainable variable's gradient}, float64.  emulate: fp32 arithmetic with 16-bit storage emulated."""
    cin, filters, need_reduce, is_root = UNITS[kind]
    dt = torch.float32 if emulate else F64
    leaves = {n: t.to(dt).clone().requires_grad_("/moving_" not in n) for n, t in tensors.items()}
    P = ON.Params(leaves, dtype=dt, emulate_bf16=emulate)
    xr = x.to(dt).clone().requires_grad_(True)
    if shortcut_scale is None:
        out = ON.bottleneck_block(P, xr, filters, SCOPE, training, need_reduce, is_root)
    else:
        out = unit_with_scaled_shortcut(P, xr, filters, training, need_reduce, is_root, shortcut_scale)
    out.backward(dy.to(dt))
    res = {"out": out.detach().to(F64), "dx": xr.grad.to(F64)}
    res.update({n: leaves[n].grad.to(F64) for n in trainable(tensors)})
    return res


def rel_l2(got, want):
    return ((got.to(F64) - want).norm() / want.norm()).item()


def errors(got, want):
    """per-tensor relative L2 error of every tensor of the reference"""
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    return {k: rel_l2(got[k], want[k]) for k in sorted(want)}

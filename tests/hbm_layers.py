"""Helper of tests/test_hbm_layers_gpu.py, tests/test_hbm_layers_cpu.py and the fp16 child (tests/fp16/cases.py); not collected by pytest.

The memory-bound layer kernels (dan_amd/csrc/elementwise.hip, dan_amd/csrc/layers2.hip) against float64 references on the CPU, at sizes
where their grid-stride loops take a second trip.  One `case_*` function per kernel family, taking (shape..., flags, act_dtype, dev): the
bf16 suite and the fp16 child run the same code.  References are plain torch on float64 tensors (oracle/tf_ops.py where it restates the
op; gradients from autograd), max pools in float32 (no arithmetic).

Tolerances (u = unit round-off of the storage type: 2^-8 bf16, 2^-11 fp16):
  * selection / copy kernels: torch.equal;
  * 16-bit element-wise outputs, per element:  |got - ref| <= 2 u |ref| + 2^-20 mag (+ 2^-25 absolute in the fp16 build), mag = the float64
    sum of the absolute values of the terms of that element (+ u |intermediate| where the two-launch form rounds one to 16 bits);
  * fp32 reductions: EXACT cases (every addend and every partial sum in any order is an fp32 integer multiple of one power of two below
    2^24 of them: bit-for-bit) and RANDOM cases (|got - S| <= 4 f A, f = the worst |S32 - S| / A of three plain float32 summation orders
    on the CPU, A = sum |addend|; 4 f <= 2^-18 is a precondition of the method).
    Exact cases: db and batch-norm sum(x), sum(x^2), dbeta from multiples of 1/4 resp. small integers; L2-norm dgamma from pixels with 4^k
    ones (inv = 2^-k, and rsqrtf returns it exactly).  Batch-norm backward's dgamma addend dy (x - mean) rstd has no exact form.
"""
import ctypes

import numpy as np
import torch

from oracle import tf_ops as T

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SIG_BITS = {torch.bfloat16: 8, torch.float16: 11}

# ---------------------------------------------------------------------------------------------------------------- launch constants
# Each mirrors the line of the launcher it names; the loop-trip conditions of the shape lists are computed from them (test_hbm_layers_cpu.py).
BLOCK = 256                       # elementwise.hip / layers2.hip: dim3(256) of every grid_for launch
GRID_FOR_CAP = 8192               # elementwise.hip `dh_grid_for(total, 256, 8192)` at every such launch; layers2.hip the same
POOL3_CAP = 4096                  # layers2.hip danhip_maxpool3x3s2_same_fwd/_bwd: `if (blocks > 4096) blocks = 4096;`
L2_FWD_BLOCKS, L2_FWD_WAVES = 4096, 4        # elementwise.hip danhip_l2norm_fwd: `if (blocks > 4096) blocks = 4096;`, b(256)
L2_BWD_BLOCKS, L2_BWD_WAVES = 512, 16        # elementwise.hip danhip_l2norm_bwd: `if (blocks > 512) blocks = 512;`, b(1024)
JUNCTION_BLOCKS, JUNCTION_WAVES = 512, 8     # elementwise.hip danhip_l2norm_bwd_pool_scatter: `if (blocks > 512)`, b(512)
RELU_BIAS_BLOCKS = 2048           # elementwise.hip danhip_relu_bwd_bias_grad: `if (blocks > 2048) blocks = 2048;`, block = 256
RELU_BITS_BLOCKS = 16384          # elementwise.hip danhip_relu_bits: `if (blocks > 16384) blocks = 16384;`
SLICE_BLOCKS = 8192               # elementwise.hip danhip_slice_deliver: `if (blocks > 8192) blocks = 8192;`
BN_REDUCE_BLOCKS = 1024           # layers2.hip danhip_batchnorm_fwd_train/_bwd: `if (grid > 1024) grid = 1024;`
PER_TRIP = GRID_FOR_CAP * BLOCK   # 2 097 152 work items per trip of a grid_for kernel


def l2_ppw(C):
    """pixels per wave: `const int lpp = C >= 512 ? 64 : C / 8, ppw = 64 / lpp;` (danhip_l2norm_fwd / _bwd)"""
    return 64 // (64 if C >= 512 else C // 8)


def rows_per_block(C):
    """`tpr = block / cg` of relu_bwd_bias_kernel and bn_reduce_kernel (block = 256, resp. 256 / cg * cg threads)"""
    return max(256 // (C // 8), 1)


def ceil_div(a, b):
    return -(-a // b)


# (work items, work items per trip) of every looping kernel a case launches: the CPU test asserts items > per_trip for the large shapes
def trips_maxpool2(N, H, W, C, **_):
    return [("maxpool2x2", N * ceil_div(H, 2) * ceil_div(W, 2) * (C // 8), PER_TRIP)]


def trips_maxpool3(N, H, W, C, **_):
    return [("maxpool3x3s2_fwd", N * ceil_div(H, 2) * ceil_div(W, 2) * (C // 8), POOL3_CAP * BLOCK), ("maxpool3x3s2_bwd", N * H * W * (C // 8), POOL3_CAP * BLOCK)]


def trips_l2norm(M, C, **_):
    return [("l2norm_fwd", M, L2_FWD_BLOCKS * L2_FWD_WAVES * l2_ppw(C)), ("l2norm_bwd", M, L2_BWD_BLOCKS * L2_BWD_WAVES * l2_ppw(C))]


def trips_junction(N, H, W, C, **_):
    nwin, per_block = N * ceil_div(H, 2) * ceil_div(W, 2), JUNCTION_WAVES * (64 // (C // 8))
    blocks = ceil_div(nwin, per_block)
    if blocks > JUNCTION_BLOCKS:
        blocks = ceil_div(blocks, ceil_div(blocks, JUNCTION_BLOCKS))
    return [("l2norm_bwd_pool_scatter", nwin, blocks * per_block)]


def trips_relu_bias(M, C, **_):
    return [("relu_bwd_bias_grad", M, RELU_BIAS_BLOCKS * rows_per_block(C))]


def trips_relu_bits(M, C, **_):
    return [("relu_bits", M * ceil_div(C, 32), RELU_BITS_BLOCKS * BLOCK)]


def trips_cast_pad(rows, c_src, **_):
    return [("cast_pad", rows * ceil_div(c_src, 8) * 8, PER_TRIP)]


def trips_slice(ldy, c0, C, masked, acc, M, **_):
    vec = C % 8 == 0 and c0 % 8 == 0 and ldy % 8 == 0           # danhip_slice_deliver: `const bool vec = ...` (the mask pitch is C here)
    return [("slice_deliver_vec" if vec else "slice_deliver_elem", M * (C // 8) if vec else M * ceil_div(C, 8) * 8, SLICE_BLOCKS * BLOCK)]


def trips_resize(N, Hi, Wi, Ho, Wo, C, **_):
    return [("resize_fwd", N * Ho * Wo * (C // 8), PER_TRIP), ("resize_bwd", N * Hi * Wi * (C // 8), PER_TRIP)]


def trips_avgpool(N, H, W, C, **_):
    return [("avgpool", N * H * W * (C // 8), PER_TRIP)]


def trips_batchnorm(M, C, **_):
    return [("bn_reduce", M, BN_REDUCE_BLOCKS * rows_per_block(C)), ("bn_apply", M * (C // 8), PER_TRIP)]


def trips_add16(n, **_):
    return [("add16 / residual_bwd", n // 8, PER_TRIP)]


def trips_preprocess(N, H, W, **_):
    return [("preprocess_u8", N * H * W, PER_TRIP)]


# ---------------------------------------------------------------------------------------------------------------- tolerance helpers
REPORT = []                       # (what, figure) lines of the last cases: floors f and observed ratios, printed by the callers


def note(what, **figs):
    line = "HBM %s: %s" % (what, ", ".join("%s=%.3g" % kv for kv in figs.items()))
    REPORT.append(line)
    print(line, flush=True)


def round_once(v, dt):
    """float64 -> the storage type's grid, ONE round-to-nearest-even (result kept in float64).  (tensor.to(dtype) from float64 may go
    through float32: two roundings.)  fp16 subnormals: spacing 2^-24 below 2^-14."""
    p = SIG_BITS[dt]
    _, e = torch.frexp(v)                                        # v = m 2^e, 0.5 <= |m| < 1
    if dt == torch.float16:
        e = e.clamp_min(-13)
    step = torch.ldexp(torch.ones_like(v), e - p)
    return torch.round(v / step) * step


def bound16(ref, mag, dt, extra=None):
    b = 2.0 * U[dt] * ref.abs() + 2.0 ** -20 * mag
    if dt == torch.float16:
        b = b + 2.0 ** -25
    if extra is not None:
        b = b + extra
    return b


FMAX = {torch.bfloat16: float(torch.finfo(torch.bfloat16).max), torch.float16: 65504.0}


def check16(got, ref, mag, dt, what, extra=None):
    """Per element, no element excluded; NaN fails.  Returns the worst |err| / bound over the finite-range elements.
    Range of the storage type: a reference beyond the largest finite value by more than the bound rounds to infinity, and the output must
    be that infinity (fp16: the gradient gamma * 1e5 * dy of an all-zero pixel of the L2 norm); within the bound of the largest finite
    value either is a correct rounding."""
    got = got.detach().cpu().double().reshape(ref.shape)
    b = bound16(ref, mag, dt, extra)
    over = ref.abs() - b > FMAX[dt] * (1 + U[dt])                # rounds to infinity whatever the fp32 error within the bound
    edge = ~over & (ref.abs() + b >= FMAX[dt] * (1 + U[dt]))     # may round either way
    inf = torch.copysign(torch.full_like(ref, float("inf")), ref)
    err = torch.where(over | (edge & (got == inf)), torch.zeros_like(ref), (got - ref).abs())
    bad = ~(err <= b) | (over & (got != inf))
    ratio = (err / b.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    assert not bad.any().item(), "%s: %d of %d elements outside the bound, worst error / bound = %.3g (first at flat index %d: got %r, want %r)" % (
        what, int(bad.sum()), bad.numel(), ratio, int(bad.flatten().nonzero()[0]), got.flatten()[bad.flatten()][0].item(), ref.flatten()[bad.flatten()][0].item())
    return ratio


def equal16(got, ref64, dt, what):
    """Selection / copy kernels: the 16-bit output equals the float64 reference value for value (a NaN left behind fails)."""
    got = got.detach().cpu().double().reshape(ref64.shape)
    ne = ~(got == ref64)
    assert not ne.any().item(), "%s: %d of %d elements differ" % (what, int(ne.sum()), ne.numel())


def float32_floor(add64):
    """add64 [M, K] float64 addends -> (S, A, f): float64 sums, sums of magnitudes and the worst relative-to-A error of three plain
    float32 summation orders on the CPU (torch.sum, strictly sequential, reversed sequential)."""
    S, A = add64.sum(0), add64.abs().sum(0)
    a32 = add64.float()
    seq = np.add.accumulate(a32.numpy(), axis=0, dtype=np.float32)[-1]
    rev = np.add.accumulate(a32.flip(0).contiguous().numpy(), axis=0, dtype=np.float32)[-1]
    f = 0.0
    for s32 in (a32.sum(0).double(), torch.from_numpy(seq.astype(np.float64)), torch.from_numpy(rev.astype(np.float64))):
        f = max(f, ((s32 - S).abs() / A.clamp_min(1e-300)).max().item())
    return S, A, f


def check_sum_random(got32, add64, what):
    """fp32 reduction, random case: |got - S| <= 4 f A.  A prefilled destination is passed as one more row of addends."""
    S, A, f = float32_floor(add64)
    assert 4.0 * f <= 2.0 ** -18, "%s: 4 f = %.3g exceeds 2^-18: the shape is too large for the float32-floor method" % (what, 4.0 * f)
    ratio = ((got32.detach().cpu().double() - S).abs() / A.clamp_min(1e-300)).max().item()
    note(what, f=f, device_ratio=ratio, rows=add64.shape[0])
    assert ratio <= 4.0 * f, "%s: device |got - S| / A = %.3g exceeds 4 f = %.3g" % (what, ratio, 4.0 * f)
    return f, ratio


def exact_precondition(add64):
    """Every addend an integer multiple of one power of two q, and sum |addend| / q < 2^24: every partial sum in any order is an fp32 value."""
    k = add64 * 2.0 ** 30
    if not bool((k == torch.round(k)).all()) or k.abs().max().item() >= 2.0 ** 62:
        return False
    k = k.to(torch.int64).abs()
    nz = k[k != 0]
    if nz.numel() == 0:
        return True
    q = int((nz & -nz).min())                                    # the largest power of two that divides every addend
    return (k // q).sum(0).max().item() < 2 ** 24


def check_sum_exact(got32, add64, what):
    assert exact_precondition(add64), what + ": the inputs of the exact case are not exact"
    got = got32.detach().cpu()
    want = add64.sum(0).to(got.dtype)
    assert torch.equal(got, want), "%s: %d of %d sums differ from the integer reference (worst %.3g)" % (
        what, int((got != want).sum()), want.numel(), (got.double() - want.double()).abs().max().item())


# ---------------------------------------------------------------------------------------------------------------- input builders
def gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def randn(shape, g, dt, scale=1.0, shift=0.0):
    return (torch.randn(shape, generator=g, device=g.device) * scale + shift).to(dt)


def quarters(shape, g, dt, lo=-4, hi=4):
    """multiples of 1/4 in [lo/4, hi/4]: sums of a few of them are exact in 8 significant bits"""
    return (torch.randint(lo, hi + 1, shape, generator=g, device=g.device).float() / 4.0).to(dt)


def relu_quantised(shape, g, dt):
    """ReLU zeros and many exact ties"""
    return torch.relu(torch.round(torch.randn(shape, generator=g, device=g.device) * 4) / 4).to(dt)


def d64(t):
    return t.detach().cpu().double()


def nan_like(t):
    return torch.full_like(t, float("nan"))


def _api():
    from dan_amd import _lib
    return _lib.call, _lib.ptr, _lib.stream()


def _act(dt):
    from dan_amd import _lib
    assert _lib.ACT_DTYPE == dt, "this process runs the %s build" % _lib.ACT_NAME


# ---------------------------------------------------------------------------------------------------------------- references
def maxpool2_argmax(x):
    """[N,H,W,C] -> (first-maximum index in window order (0,0),(0,1),(1,0),(1,1) [N,Ho,Wo,C], padded height, padded width)"""
    N, H, W, C = x.shape
    xp = torch.full((N, H + H % 2, W + W % 2, C), float("-inf"), dtype=x.dtype)
    xp[:, :H, :W] = x
    win = torch.stack([xp[:, 0::2, 0::2], xp[:, 0::2, 1::2], xp[:, 1::2, 0::2], xp[:, 1::2, 1::2]], 0)
    return win.argmax(0)                                         # torch.argmax returns the first maximum


def maxpool2_scatter(am, dy, H, W):
    """gradient of the 2 x 2 pool: dy goes to the first maximum of its window"""
    N, Ho, Wo, C = dy.shape
    wp = torch.zeros((N, 2 * Ho, 2 * Wo, C), dtype=dy.dtype)
    for t, (dh, dw) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        wp[:, dh::2, dw::2] = torch.where(am == t, dy, torch.zeros((), dtype=dy.dtype))
    return wp[:, :H, :W]


def maxpool2_codes(am):
    """2-bit codes as maxpool_fwd_kernel packs them: [pooled pixel][C/4] bytes, channel c in bits 2 (c % 4) of byte c / 4"""
    C = am.shape[-1]
    a = am.reshape(-1, C // 4, 4).to(torch.int32)
    return (a[..., 0] | (a[..., 1] << 2) | (a[..., 2] << 4) | (a[..., 3] << 6)).to(torch.uint8)


def maxpool3_grad(x64, dy64):
    """3 x 3 / 2 'same' max pool: autograd's rule is the first maximum in window scan order (pinned in test_hbm_layers_cpu.py)"""
    xr = x64.clone().requires_grad_(True)
    T.max_pool_3x3_s2_same(xr).backward(dy64)
    return xr.grad


def l2_terms(x, gamma, dy):
    """float64 [M, C]: the two terms of dx = gamma inv dy - x k, inv, and the dgamma addends dy x inv"""
    ss = (x * x).sum(-1, keepdim=True)
    inv = torch.rsqrt(torch.clamp(ss, min=1e-10))
    dot = (dy * gamma * x).sum(-1, keepdim=True)
    k = torch.where(ss > 1e-10, dot * inv ** 3, torch.zeros((), dtype=x.dtype))
    return gamma * inv * dy, x * k, inv, dy * x * inv


def l2_grads(x, gamma, dy):
    """float64 autograd through oracle/tf_ops.l2_normalize"""
    M, C = x.shape
    xr, gr = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True)
    T.l2_normalize(xr.view(1, 1, M, C), gr).backward(dy.view(1, 1, M, C))
    return xr.grad, gr.grad


def l2_input(M, C, g, dt, exact=False):
    """ReLU outputs with all-zero pixels (the 1e-10 clamp) at both ends and one pixel whose only non-zero is 2^-20; exact: 4^k ones per
    pixel, so that inv = 2^-k and the dgamma addends dy x inv are dyadic."""
    dev = g.device
    if exact:
        kmax = 0
        while 4 ** (kmax + 1) <= C:
            kmax += 1
        n = 4 ** torch.randint(0, kmax + 1, (M, 1), generator=g, device=dev)
        off = torch.randint(0, C, (M, 1), generator=g, device=dev)
        x = (((torch.arange(C, device=dev)[None] - off) % C) < n).to(dt)
    else:
        x = torch.relu(torch.randn((M, C), generator=g, device=dev)).to(dt)
    x[0] = 0
    x[M - 1] = 0
    if not exact and M > 2:
        x[1] = 0
        x[1, 3] = 2.0 ** -20
    return x


def gamma_input(C, g):
    gamma = (10.0 + torch.randn((C,), generator=g, device=g.device)).float()
    gamma[5] = 2.0 ** -6                                         # a channel with a small scale
    return gamma


# ---------------------------------------------------------------------------------------------------------------- cases
def case_maxpool2(N, H, W, C, acc, dyadic, dt, dev):
    """danhip_maxpool2x2_fwd, _fwd_arg, _bwd, _bwd_arg: outputs, codes and both backward forms against the first-maximum reference.
    dyadic: dy and the destination's old content are multiples of 1/4, so accumulate = 1 is exact as well."""
    _act(dt)
    call, ptr, s = _api()
    g = gen(dev, N * 1000 + H)
    x = relu_quantised((N, H, W, C), g, dt)
    x[0, :2, :2] = 0                                             # an all-equal window: the first index wins
    Ho, Wo = ceil_div(H, 2), ceil_div(W, 2)
    y0 = nan_like(x[:, :Ho, :Wo].contiguous())
    y1 = nan_like(y0)
    arg = torch.full((N * Ho * Wo, C // 4), 255, dtype=torch.uint8, device=dev)
    call("danhip_maxpool2x2_fwd", ptr(x), ptr(y0), N, H, W, C, s)
    call("danhip_maxpool2x2_fwd_arg", ptr(x), ptr(y1), ptr(arg), N, H, W, C, s)
    xc = x.cpu().float()
    want = T.max_pool_2x2_same(xc)
    assert torch.equal(y0.cpu().float(), want) and torch.equal(y1.cpu().float(), want), "maxpool2x2_fwd"
    am = maxpool2_argmax(xc)
    del xc, want
    assert torch.equal(arg.cpu(), maxpool2_codes(am)), "maxpool2x2_fwd_arg: arg-max codes"
    mk = quarters if dyadic else (lambda shape, g_, dt_: randn(shape, g_, dt_))
    dy = mk((N, Ho, Wo, C), g, dt)
    old = mk((N, H, W, C), g, dt) if acc else nan_like(x)        # accumulate = 0: a fresh slot holds garbage and is not read
    sel = maxpool2_scatter(am, dy.cpu().float(), H, W).double()
    del am
    ref = sel + d64(old) if acc else sel
    mag = sel.abs() + d64(old).abs() if acc and not dyadic else None
    for name, first in (("danhip_maxpool2x2_bwd", x), ("danhip_maxpool2x2_bwd_arg", arg)):
        dx = old.clone()
        call(name, ptr(first), ptr(dy), ptr(dx), N, H, W, C, acc, s)
        if acc and not dyadic:
            check16(dx, ref, mag, dt, name + " accumulate")
        else:
            equal16(dx, ref, dt, name)
        del dx


def case_maxpool3(N, H, W, C, dt, dev):
    """danhip_maxpool3x3s2_same_fwd/_bwd; dy in multiples of 1/4: the up to four gradients an input collects sum exactly."""
    _act(dt)
    call, ptr, s = _api()
    g = gen(dev, N * 1000 + W)
    x = relu_quantised((N, H, W, C), g, dt) - 1                  # ties, and negative values next to the -inf padding
    Ho, Wo = ceil_div(H, 2), ceil_div(W, 2)
    y = nan_like(x[:, :Ho, :Wo].contiguous())
    call("danhip_maxpool3x3s2_same_fwd", ptr(x), ptr(y), N, H, W, C, s)
    xc = d64(x)
    assert torch.equal(y.cpu().double(), T.max_pool_3x3_s2_same(xc)), "maxpool3x3s2_same_fwd"
    dy = quarters((N, Ho, Wo, C), g, dt)
    dx = nan_like(x)
    call("danhip_maxpool3x3s2_same_bwd", ptr(x), ptr(dy), ptr(dx), N, H, W, C, s)
    equal16(dx, maxpool3_grad(xc, d64(dy)), dt, "maxpool3x3s2_same_bwd")


def case_l2norm(M, C, acc, relu_mask, exact, dt, dev):
    """danhip_l2norm_fwd and danhip_l2norm_bwd (dx per element; dgamma accumulated into a prefilled buffer: random or exact)."""
    _act(dt)
    call, ptr, s = _api()
    g = gen(dev, M + C)
    x = l2_input(M, C, g, dt, exact)
    gamma = gamma_input(C, g)
    y = nan_like(x)
    call("danhip_l2norm_fwd", ptr(x), ptr(gamma), ptr(y), M, C, s)
    x64, g64 = d64(x), d64(gamma)
    ref = T.l2_normalize(x64.view(1, 1, M, C), g64).view(M, C)
    r = check16(y, ref, ref.abs(), dt, "l2norm_fwd M=%d C=%d" % (M, C))
    dy = quarters((M, C), g, dt) if exact else randn((M, C), g, dt)
    old = randn((M, C), g, dt) if acc else nan_like(x)
    dg0 = torch.randint(-8, 9, (C,), generator=g, device=dev).float() if exact else torch.randn((C,), generator=g, device=dev)
    dx, dg = old.clone(), dg0.clone()
    call("danhip_l2norm_bwd", ptr(x), ptr(gamma), ptr(dy), ptr(dx), ptr(dg), M, C, acc, relu_mask, s)
    dy64 = d64(dy)
    t1, t2, _, addend = l2_terms(x64, g64, dy64)
    ref, _ = l2_grads(x64, g64, dy64)
    mag = t1.abs() + t2.abs()
    if relu_mask:                                                # the mask comes from the input tensor
        ref, mag = ref * (x64 > 0), mag * (x64 > 0)
    if acc:
        ref, mag = ref + d64(old), mag + d64(old).abs()
    r2 = check16(dx, ref, mag, dt, "l2norm_bwd dx M=%d C=%d acc=%d relu_mask=%d" % (M, C, acc, relu_mask))
    note("l2norm M=%d C=%d" % (M, C), fwd_ratio=r, dx_ratio=r2)
    rows = torch.cat([d64(dg0)[None], addend], 0)
    if exact:
        check_sum_exact(dg, rows, "l2norm_bwd dgamma exact M=%d C=%d" % (M, C))
    else:
        check_sum_random(dg, rows, "l2norm_bwd dgamma M=%d C=%d" % (M, C))


def case_junction(N, H, W, C, acc, relu_mask, pool_first, dt, dev):
    """danhip_l2norm_bwd_pool_scatter against the float64 sum of the two gradients; the 16-bit rounding of the first delivery is modelled
    as one more u |first delivery| of slack."""
    _act(dt)
    call, ptr, s = _api()
    g = gen(dev, N * 100 + H)
    M = N * H * W
    x = torch.relu(torch.randn((N, H, W, C), generator=g, device=dev)).to(dt)
    x[0, 0, 0] = 0
    x[-1, H - 1, W - 1] = 0
    x[0, 2:4, 2:4] = 0
    gamma = gamma_input(C, g)
    dy = randn((N, H, W, C), g, dt)
    Ho, Wo = ceil_div(H, 2), ceil_div(W, 2)
    pdy = randn((N, Ho, Wo, C), g, dt)
    old = randn((N, H, W, C), g, dt) if acc else nan_like(x)
    dg0 = torch.randn((C,), generator=g, device=dev)
    am = maxpool2_argmax(x.cpu().float())
    arg = maxpool2_codes(am).to(dev)                             # the reference codes (case_maxpool2 checks the kernel writes the same)
    dx, dg = old.clone(), dg0.clone()
    call("danhip_l2norm_bwd_pool_scatter", ptr(x), ptr(gamma), ptr(dy), ptr(arg), ptr(pdy), ptr(dx), ptr(dg), N, H, W, C, acc, relu_mask, pool_first, s)
    x64, g64, dy64 = d64(x).view(M, C), d64(gamma), d64(dy).view(M, C)
    t1, t2, _, addend = l2_terms(x64, g64, dy64)
    b, _ = l2_grads(x64, g64, dy64)
    mag = t1.abs() + t2.abs()
    if relu_mask:
        b, mag = b * (x64 > 0), mag * (x64 > 0)
    a = maxpool2_scatter(am, d64(pdy), H, W).reshape(M, C)
    first = a if pool_first else b
    if acc:
        first = first + d64(old).view(M, C)
        mag = mag + d64(old).view(M, C).abs()
    ref = first + (b if pool_first else a)
    r = check16(dx, ref, mag + a.abs(), dt, "l2norm_bwd_pool_scatter dx %s acc=%d relu_mask=%d pool_first=%d" % ((N, H, W, C), acc, relu_mask, pool_first),
                extra=U[dt] * first.abs())
    note("junction %s" % ((N, H, W, C),), dx_ratio=r)
    check_sum_random(dg, torch.cat([d64(dg0)[None], addend], 0), "l2norm_bwd_pool_scatter dgamma %s" % ((N, H, W, C),))


def case_relu_bias(M, C, with_y, with_db, exact, dt, dev):
    """danhip_relu_bwd_bias_grad: dy masked in place (selection) and db accumulated into a prefilled buffer."""
    _act(dt)
    call, ptr, s = _api()
    g = gen(dev, M + C)
    if exact:
        dy = quarters((M, C), g, dt)
        y = torch.randint(0, 3, (M, C), generator=g, device=dev).to(dt)
        db0 = torch.randint(-8, 9, (C,), generator=g, device=dev).float()
    else:
        dy = randn((M, C), g, dt)
        y = torch.relu(torch.randn((M, C), generator=g, device=dev)).to(dt)
        db0 = torch.randn((C,), generator=g, device=dev)
    want = torch.where(d64(y) > 0, d64(dy), torch.zeros((), dtype=torch.float64)) if with_y else d64(dy)
    db = db0.clone()
    call("danhip_relu_bwd_bias_grad", ptr(dy), ptr(y) if with_y else None, ptr(db) if with_db else None, M, C, s)
    equal16(dy, want, dt, "relu_bwd_bias_grad dy M=%d C=%d" % (M, C))
    if with_db:
        rows = torch.cat([d64(db0)[None], want], 0)
        what = "relu_bwd_bias_grad db M=%d C=%d" % (M, C)
        if exact:
            check_sum_exact(db, rows, what + " exact")
        else:
            check_sum_random(db, rows, what)


def case_relu_bits(M, C, dt, dev):
    """danhip_relu_bits: bits[m][j] bit i = x[m][8 j + i] > 0"""
    _act(dt)
    call, ptr, s = _api()
    g = gen(dev, C)
    x = randn((M, C), g, dt)
    x[0] = 0
    x[M - 1, ::2] = -0.0
    bits = torch.full((M, C // 8), 0xA5, dtype=torch.uint8, device=dev)
    call("danhip_relu_bits", ptr(x), ptr(bits), M, C, s)
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8)
    want = ((x.cpu() > 0).view(M, C // 8, 8).to(torch.uint8) * w).sum(-1, dtype=torch.int32).to(torch.uint8)
    assert torch.equal(bits.cpu(), want), "relu_bits M=%d C=%d" % (M, C)


def case_cast_pad(rows, c_src, with_relu, dt, dev):
    """danhip_cast_pad_f32_to_bf16: fp32 [rows, c_src] -> 16 bit [rows, c_dst], zero padded, optionally masked by a ReLU output."""
    _act(dt)
    call, ptr, s = _api()
    c_dst = ceil_div(c_src, 8) * 8
    g = gen(dev, rows + c_src)
    src = torch.randn((rows, c_src), generator=g, device=dev) * 3
    src[0, 0] = 1.0 + 2.0 ** -(SIG_BITS[dt])                     # a tie of the storage rounding: to even
    ry = torch.relu(torch.randn((rows, c_src), generator=g, device=dev)).to(dt)
    dst = torch.full((rows, c_dst), float("nan"), dtype=dt, device=dev)
    call("danhip_cast_pad_f32_to_bf16", ptr(src), ptr(ry) if with_relu else None, ptr(dst), rows, c_src, c_dst, s)
    v = d64(src)
    if with_relu:
        v = v * (d64(ry) > 0)
    want = round_once(v, dt)
    assert torch.equal(want, v.float().to(dt).double()), "cast_pad: the once-rounded reference is not tensor.to(dtype)"
    equal16(dst, torch.cat([want, torch.zeros((rows, c_dst - c_src), dtype=torch.float64)], 1), dt, "cast_pad rows=%d c_src=%d" % (rows, c_src))


def case_slice_deliver(ldy, c0, C, masked, acc, M, dt, dev):
    """danhip_slice_deliver (vector and ragged kernels): the parametrisation of test_concat_gpu.py::test_slice_deliver_kernel."""
    _act(dt)
    call, ptr, s = _api()
    Cpad = ceil_div(C, 8) * 8
    g = gen(dev, ldy + c0 + C)
    dy = randn((M, ldy), g, dt)
    mask = randn((M, C), g, dt)
    old = randn((M, Cpad), g, dt) if acc else torch.full((M, Cpad), float("nan"), dtype=dt, device=dev)
    out = old.clone()
    call("danhip_slice_deliver", ptr(dy), ldy, c0, C, ptr(mask) if masked else None, C, ptr(out), Cpad, acc, M, s)
    v = d64(dy[:, c0:c0 + C])
    if masked:
        v = v * (d64(mask) > 0)
    v = torch.cat([v, torch.zeros((M, Cpad - C), dtype=torch.float64)], 1)
    what = "slice_deliver %s" % ((ldy, c0, C, masked, acc, M),)
    if acc:
        note(what, ratio=check16(out, v + d64(old), v.abs() + d64(old).abs(), dt, what))
    else:
        equal16(out, v, dt, what)


def _resize_ref(up64, out_hw, dy64=None):
    """float64 resize (+ its gradient when dy64 is given)"""
    if dy64 is None:
        return T.resize_bilinear_legacy(up64, *out_hw)
    ur = up64.clone().requires_grad_(True)
    T.resize_bilinear_legacy(ur, *out_hw).backward(dy64)
    return ur.grad


def case_resize(N, Hi, Wi, Ho, Wo, C, lateral, acc, dt, dev):
    """danhip_resize_bilinear_add_fwd/_bwd; the float64 reference runs one image at a time (working set)."""
    _act(dt)
    call, ptr, s = _api()
    g = gen(dev, N + Hi + Wo)
    up = randn((N, Hi, Wi, C), g, dt)
    lat = randn((N, Ho, Wo, C), g, dt) if lateral else None
    out = torch.full((N, Ho, Wo, C), float("nan"), dtype=dt, device=dev)
    call("danhip_resize_bilinear_add_fwd", ptr(up), ptr(lat), ptr(out), N, Hi, Wi, Ho, Wo, C, s)
    dout = randn((N, Ho, Wo, C), g, dt)
    old = randn((N, Hi, Wi, C), g, dt) if acc else nan_like(up)
    dup = old.clone()
    call("danhip_resize_bilinear_add_bwd", ptr(dout), ptr(dup), N, Hi, Wi, Ho, Wo, C, acc, s)
    rf = rb = 0.0
    for n in range(N):
        u = d64(up[n:n + 1])
        ref, mag = _resize_ref(u, (Ho, Wo)), _resize_ref(u.abs(), (Ho, Wo))       # interpolation: mag = the weighted sum of |corner|
        if lateral:
            ref, mag = ref + d64(lat[n:n + 1]), mag + d64(lat[n:n + 1]).abs()
        rf = max(rf, check16(out[n:n + 1], ref, mag, dt, "resize_bilinear_add_fwd %s image %d" % ((N, Hi, Wi, Ho, Wo, C), n)))
        d = d64(dout[n:n + 1])
        ref, mag = _resize_ref(u, (Ho, Wo), d), _resize_ref(u, (Ho, Wo), d.abs())
        if acc:
            ref, mag = ref + d64(old[n:n + 1]), mag + d64(old[n:n + 1]).abs()
        rb = max(rb, check16(dup[n:n + 1], ref, mag, dt, "resize_bilinear_add_bwd %s image %d" % ((N, Hi, Wi, Ho, Wo, C), n)))
    note("resize %s" % ((N, Hi, Wi, Ho, Wo, C),), fwd_ratio=rf, bwd_ratio=rb)


def _avg_grad(shape, dy64):
    xr = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    T.avg_pool_2x2_s1_same(xr).backward(dy64)
    return xr.grad


def case_avgpool(N, H, W, C, relu, masked, acc, dt, dev, x_pitch=256, y_pitch=192):
    """danhip_avgpool2x2s1_same_fwd/_bwd and the _strided forms on channel-slice views (the context block's pitches)."""
    _act(dt)
    call, ptr, s = _api()
    g = gen(dev, N + H + C)
    shape = (N, H, W, C)
    x = randn(shape, g, dt)
    y = nan_like(x)
    call("danhip_avgpool2x2s1_same_fwd", ptr(x), ptr(y), N, H, W, C, s)
    x64 = d64(x)
    ref, mag = T.avg_pool_2x2_s1_same(x64), T.avg_pool_2x2_s1_same(x64.abs())
    r = [check16(y, ref, mag, dt, "avgpool2x2s1_same_fwd %s" % (shape,))]
    # strided: x is channels [x_pitch - C, x_pitch) of a pitch-x_pitch buffer, y channels [8, 8 + C) of a pitch-y_pitch one
    if x_pitch >= C and y_pitch >= C + 8:
        xb = randn((N, H, W, x_pitch), g, dt)
        xb[..., x_pitch - C:] = x
        yb = torch.full((N, H, W, y_pitch), 3.0, dtype=dt, device=dev)
        es = 2
        xp = ctypes.c_void_p(xb.data_ptr() + (x_pitch - C) * es)
        yp = ctypes.c_void_p(yb.data_ptr() + 8 * es)
        call("danhip_avgpool2x2s1_same_fwd_strided", xp, x_pitch, yp, y_pitch, N, H, W, C, int(relu), s)
        r.append(check16(yb[..., 8:8 + C], torch.relu(ref) if relu else ref, mag, dt, "avgpool2x2s1_same_fwd_strided %s" % (shape,)))
        assert bool((yb[..., :8] == 3).all()) and bool((yb[..., 8 + C:] == 3).all()), "avgpool_fwd_strided wrote outside its channel slice"
        dyb = randn((N, H, W, y_pitch), g, dt)
        dxb = torch.full((N, H, W, x_pitch), 3.0, dtype=dt, device=dev)
        call("danhip_avgpool2x2s1_same_bwd_strided", ctypes.c_void_p(dyb.data_ptr() + 8 * es), y_pitch, ctypes.c_void_p(dxb.data_ptr() + (x_pitch - C) * es),
             x_pitch, N, H, W, C, s)
        d = d64(dyb[..., 8:8 + C])
        r.append(check16(dxb[..., x_pitch - C:], _avg_grad(shape, d), _avg_grad(shape, d.abs()), dt, "avgpool2x2s1_same_bwd_strided %s" % (shape,)))
        assert bool((dxb[..., :x_pitch - C] == 3).all()), "avgpool_bwd_strided wrote outside its channel slice"
        del xb, yb, dyb, dxb
    dy = randn(shape, g, dt)
    xm = torch.relu(randn(shape, g, dt)) if masked else None
    old = randn(shape, g, dt) if acc else nan_like(x)
    dx = old.clone()
    call("danhip_avgpool2x2s1_same_bwd", ptr(dy), ptr(xm), ptr(dx), N, H, W, C, acc, s)
    ref, mag = _avg_grad(shape, d64(dy)), _avg_grad(shape, d64(dy).abs())
    if masked:
        ref, mag = ref * (d64(xm) > 0), mag * (d64(xm) > 0)
    if acc:
        ref, mag = ref + d64(old), mag + d64(old).abs()
    r.append(check16(dx, ref, mag, dt, "avgpool2x2s1_same_bwd %s masked=%d acc=%d" % (shape, masked, acc)))
    note("avgpool %s" % (shape,), worst_ratio=max(r))


BN_EPS = 1e-5
BN_MOMENTUM = float(torch.tensor(0.997, dtype=torch.float32))    # the fp32 value the kernel receives


def bn_input(M, C, kind, g, dt):
    """random: zero-mean; shifted: |mean| / std = 16; exact: integers in [-3, 3] (sum x, sum x^2 < 2^24 up to 1.8 M rows).
    Channel 1 has zero variance in the random kinds."""
    dev = g.device
    if kind == "exact":
        return torch.randint(-3, 4, (M, C), generator=g, device=dev).to(dt)
    x = torch.randn((M, C), generator=g, device=dev) * (1.0 if kind == "shifted" else 2.0) + (16.0 if kind == "shifted" else 0.0)
    x[:, 1] = 1.5
    return x.to(dt)


def case_batchnorm(M, C, relu, kind, dt, dev):
    """danhip_batchnorm_fwd_train/_infer/_bwd.  The sums (left in the workspace; dbeta, dgamma) are judged as reductions; save_mean, save_rstd
    and the moving averages against float64 with the variance allowed 2^-20 (E[x^2] + mean^2); y and dx per element against float64
    formulas fed the device's own (checked) statistics, as the backward entry point itself is."""
    _act(dt)
    call, ptr, s = _api()
    g = gen(dev, M + C)
    x = bn_input(M, C, kind, g, dt)
    gamma = (torch.rand((C,), generator=g, device=dev) + 0.5).float()
    gamma[min(5, C - 1)] = 2.0 ** -6
    beta = (torch.randn((C,), generator=g, device=dev) * 0.1).float()
    y = nan_like(x)
    mean, rstd = torch.empty((C,), device=dev), torch.empty((C,), device=dev)
    mm0, mv0 = torch.randn((C,), generator=g, device=dev), torch.rand((C,), generator=g, device=dev) + 0.5
    mm, mv = mm0.clone(), mv0.clone()
    ws = torch.full((2 * C,), float("nan"), dtype=torch.float64, device=dev)      # sum x, sum x^2: double
    call("danhip_batchnorm_fwd_train", ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), ptr(mm), ptr(mv), M, C, BN_EPS, BN_MOMENTUM, int(relu), ptr(ws), s)
    x64, g64, b64 = d64(x), d64(gamma), d64(beta)
    what = "batchnorm M=%d C=%d %s" % (M, C, kind)
    _, mu, var = T.batch_norm_train(x64.view(1, 1, M, C), g64, b64, BN_EPS)
    ex2 = (x64 * x64).mean(0)
    if kind == "exact":
        check_sum_exact(ws[:C], x64, what + " sum(x)")
        check_sum_exact(ws[C:], x64 * x64, what + " sum(x^2)")
    elif kind == "random":
        check_sum_random(ws[:C], x64, what + " sum(x)")
        if M <= 128:                                             # positive addends: the sequential float32 floor grows as sqrt(M)
            check_sum_random(ws[C:], x64 * x64, what + " sum(x^2)")
    # statistics: var = E[x^2] - mean^2 in fp32 is allowed 2^-20 (E[x^2] + mean^2); mean the same relative to E|x|; fp32 results, no 16-bit term
    vtol = 2.0 ** -20 * (ex2 + mu * mu)
    mtol = 2.0 ** -20 * x64.abs().mean(0)
    mean64, rstd64 = d64(mean), d64(rstd)
    assert bool(((mean64 - mu).abs() <= mtol).all()), (what, "save_mean", ((mean64 - mu).abs() / mtol.clamp_min(1e-300)).max().item())
    lo = torch.rsqrt(var + vtol + BN_EPS) * (1 - 2.0 ** -21)
    hi = torch.rsqrt((var - vtol).clamp_min(0) + BN_EPS) * (1 + 2.0 ** -21)
    var_dev = 1.0 / (rstd64 * rstd64) - BN_EPS                   # the variance the device normalised with
    note(what, var_err_over_bound=((var_dev - var).abs() / vtol.clamp_min(1e-300)).max().item(), mean_err_over_bound=((mean64 - mu).abs() / mtol.clamp_min(1e-300)).max().item())
    assert bool(((rstd64 >= lo) & (rstd64 <= hi)).all()), (what, "save_rstd outside the interval of var +- 2^-20 (E[x^2] + mean^2)")
    mom = BN_MOMENTUM
    mm_ref = d64(mm0) * mom + mu * (1 - mom)
    assert bool(((d64(mm) - mm_ref).abs() <= mtol * (1 - mom) + 2.0 ** -22 * (d64(mm0).abs() * mom + mu.abs() * (1 - mom))).all()), (what, "moving_mean")
    bessel = M / (M - 1.0) if M > 1 else 1.0
    mv_ref = d64(mv0) * mom + var * bessel * (1 - mom)
    assert bool(((d64(mv) - mv_ref).abs() <= vtol * bessel * (1 - mom) + 2.0 ** -22 * mv_ref.abs()).all()), (what, "moving_variance")
    # apply, per element, from the device's statistics
    t = (x64 - mean64) * rstd64 * g64
    ref = t + b64
    r = [check16(y, torch.relu(ref) if relu else ref, t.abs() + b64.abs(), dt, what + " y")]
    yi = nan_like(x)
    call("danhip_batchnorm_fwd_infer", ptr(x), ptr(gamma), ptr(beta), ptr(mean), ptr(rstd), ptr(yi), M, C, int(relu), s)
    r.append(check16(yi, torch.relu(ref) if relu else ref, t.abs() + b64.abs(), dt, what + " infer y"))
    del t, ref, y, yi
    # backward
    dy = quarters((M, C), g, dt) if kind == "exact" else randn((M, C), g, dt)
    dx = nan_like(x)
    dgam, dbet = torch.full((C,), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)   # both are overwritten
    call("danhip_batchnorm_bwd", ptr(x), ptr(dy), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(dgam), ptr(dbet), M, C, s)
    dy64 = d64(dy)
    xh = (x64 - mean64) * rstd64
    if kind == "exact":
        check_sum_exact(dbet, dy64, what + " dbeta")
    else:
        check_sum_random(dbet, dy64, what + " dbeta")
    check_sum_random(dgam, dy64 * xh, what + " dgamma")
    sdy, sdyx = d64(dbet) / M, d64(dgam) / M
    ref = g64 * rstd64 * (dy64 - sdy - xh * sdyx)
    mag = (g64 * rstd64).abs() * (dy64.abs() + sdy.abs() + (xh * sdyx).abs())
    r.append(check16(dx, ref, mag, dt, what + " dx"))
    note(what, worst_elementwise_ratio=max(r))


def case_add16(n, dt, dev):
    _act(dt)
    call, ptr, s = _api()
    g = gen(dev, n)
    a, b = randn((n,), g, dt), randn((n,), g, dt, scale=0.01)
    out = nan_like(a)
    call("danhip_add16", ptr(a), ptr(b), ptr(out), n, s)
    note("add16 n=%d" % n, ratio=check16(out, d64(a) + d64(b), d64(a).abs() + d64(b).abs(), dt, "add16 n=%d" % n))


def case_residual_bwd(n, masked, with_dx, acc, dt, dev):
    """danhip_residual_bwd: dr = dy (r > 0) is a selection; dx (+)= dy (x_mask > 0 | no mask)"""
    _act(dt)
    call, ptr, s = _api()
    g = gen(dev, n + 1)
    dy = randn((n,), g, dt)
    r = torch.relu(randn((n,), g, dt))
    xm = torch.relu(randn((n,), g, dt)) if masked else None
    old = randn((n,), g, dt) if acc else nan_like(dy)
    dr, dx = nan_like(dy), old.clone()
    call("danhip_residual_bwd", ptr(dy), ptr(r), ptr(xm), ptr(dr), ptr(dx) if with_dx else None, acc, n, s)
    dy64 = d64(dy)
    equal16(dr, dy64 * (d64(r) > 0), dt, "residual_bwd dr n=%d" % n)
    if with_dx:
        v = dy64 * (d64(xm) > 0) if masked else dy64
        if acc:
            check16(dx, v + d64(old), v.abs() + d64(old).abs(), dt, "residual_bwd dx accumulate n=%d" % n)
        else:
            equal16(dx, v, dt, "residual_bwd dx n=%d" % n)


PREPROCESS_MEANS = [float(torch.tensor(m, dtype=torch.float32)) for m in (103.94, 116.78, 123.68)]    # B, G, R: preprocess_kernel's fp32 constants


def preprocess_reference(img_rgb_u8, dt):
    """(once-rounded float64 reference [.., 3] in B, G, R order, mask of the elements where rounding the exact difference to fp32 first and
    to the storage type second gives another value: there the kernel, which subtracts in fp32, is allowed one storage ulp)"""
    v = img_rgb_u8.double()[..., [2, 1, 0]] - torch.tensor(PREPROCESS_MEANS, dtype=torch.float64)
    once = round_once(v, dt)
    twice = v.float().to(dt).double()
    return v, once, once != twice


def case_preprocess(N, H, W, dt, dev):
    _act(dt)
    call, ptr, s = _api()
    g = gen(dev, H)
    img = torch.randint(0, 256, (N, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
    img.view(-1, 3)[:256] = torch.arange(256, device=dev, dtype=torch.uint8)[:, None]          # all 256 byte values in every colour plane
    img.view(-1, 3)[-256:] = torch.arange(256, device=dev, dtype=torch.uint8)[:, None]         # ... also in the last trip
    out = torch.full((N, H, W, 8), float("nan"), dtype=dt, device=dev)
    call("danhip_preprocess_u8", ptr(img), ptr(out), N * H * W, s)
    v, once, double_rounded = preprocess_reference(img.cpu(), dt)
    got = out.cpu().double()
    assert bool((got[..., 3:] == 0).all()), "preprocess_u8: padding channels"
    err = (got[..., :3] - once).abs()
    ulp = 2.0 * U[dt] * 2.0 ** torch.floor(torch.log2(once.abs().clamp_min(2.0 ** -14)))
    assert bool((err <= torch.where(double_rounded, ulp, torch.zeros(()).double())).all()), "preprocess_u8: %d elements differ" % int((err > 0).sum())


# ---------------------------------------------------------------------------------------------------------------- shape lists
# (id, case function, trips function, keyword arguments, large).  large: at least one kernel of the case takes a second trip; the CPU
# test asserts that, and that every looping kernel has a large case whose last trip is partial and every family a small odd one.
def _c(cid, fn, trips, large=False, **kw):
    return (cid, fn, trips, kw, large)


CASES = [
    # 2 x 2 max pool: flags at the small odd shapes, one looping shape with accumulate = 1 (exact: dyadic gradients)
    _c("maxpool2-odd-acc0", case_maxpool2, trips_maxpool2, N=3, H=7, W=9, C=8, acc=0, dyadic=False),
    _c("maxpool2-odd-acc1", case_maxpool2, trips_maxpool2, N=1, H=33, W=47, C=128, acc=1, dyadic=False),
    _c("maxpool2-loops", case_maxpool2, trips_maxpool2, True, N=3, H=321, W=643, C=128, acc=1, dyadic=True),
    _c("maxpool2-loops-even", case_maxpool2, trips_maxpool2, True, N=4, H=640, W=640, C=64, acc=0, dyadic=True),
    _c("maxpool3-even", case_maxpool3, trips_maxpool3, N=1, H=8, W=10, C=8),
    _c("maxpool3-odd", case_maxpool3, trips_maxpool3, N=2, H=7, W=9, C=16),
    _c("maxpool3-mixed", case_maxpool3, trips_maxpool3, N=1, H=7, W=10, C=8),
    _c("maxpool3-loops", case_maxpool3, trips_maxpool3, True, N=3, H=481, W=483, C=64),
]
# L2 norm: every instantiation <8,1> .. <64,2> at a looping M that is not a multiple of PPW, and at M = 61; the four accumulate x
# relu_mask combinations at the small shape, accumulate = 1 at the large ones
for _C, _M in ((64, 140003), (128, 70003), (256, 40001), (512, 20001), (1024, 20001)):
    CASES.append(_c("l2norm-C%d-loops" % _C, case_l2norm, trips_l2norm, True, M=_M, C=_C, acc=1, relu_mask=_C in (64, 256, 1024), exact=False))
    CASES.append(_c("l2norm-C%d-odd" % _C, case_l2norm, trips_l2norm, M=61, C=_C, acc=0, relu_mask=_C in (128, 512), exact=False))
for _acc, _rm in ((0, 0), (0, 1), (1, 0), (1, 1)):
    CASES.append(_c("l2norm-flags-acc%d-mask%d" % (_acc, _rm), case_l2norm, trips_l2norm, M=61, C=64, acc=_acc, relu_mask=_rm, exact=False))
CASES += [
    _c("l2norm-exact-C64", case_l2norm, trips_l2norm, True, M=140003, C=64, acc=0, relu_mask=1, exact=True),
    _c("l2norm-exact-C1024", case_l2norm, trips_l2norm, True, M=20001, C=1024, acc=1, relu_mask=0, exact=True),
    _c("junction-loops", case_junction, trips_junction, True, N=2, H=160, W=160, C=256, acc=1, relu_mask=1, pool_first=0),
    _c("junction-loops-pool-first", case_junction, trips_junction, True, N=3, H=81, W=83, C=512, acc=1, relu_mask=0, pool_first=1),
    _c("junction-odd", case_junction, trips_junction, N=1, H=37, W=53, C=64, acc=0, relu_mask=1, pool_first=0),
    _c("junction-odd-pool-first", case_junction, trips_junction, N=1, H=5, W=7, C=128, acc=0, relu_mask=0, pool_first=1),
    # ReLU backward + bias gradient
    _c("relu-bias-C64-loops", case_relu_bias, trips_relu_bias, True, M=70001, C=64, with_y=True, with_db=True, exact=False),
    _c("relu-bias-C72-loops", case_relu_bias, trips_relu_bias, True, M=60001, C=72, with_y=True, with_db=True, exact=False),
    _c("relu-bias-C200-loops", case_relu_bias, trips_relu_bias, True, M=21001, C=200, with_y=False, with_db=True, exact=False),
    _c("relu-bias-C2048-loops", case_relu_bias, trips_relu_bias, True, M=2051, C=2048, with_y=True, with_db=True, exact=False),
    _c("relu-bias-exact-C64", case_relu_bias, trips_relu_bias, True, M=300001, C=64, with_y=True, with_db=True, exact=True),
    _c("relu-bias-exact-C72", case_relu_bias, trips_relu_bias, True, M=60001, C=72, with_y=True, with_db=True, exact=True),
    _c("relu-bias-exact-C2048", case_relu_bias, trips_relu_bias, True, M=2051, C=2048, with_y=False, with_db=True, exact=True),
    _c("relu-bias-odd", case_relu_bias, trips_relu_bias, M=61, C=8, with_y=True, with_db=True, exact=False),
    _c("relu-bias-no-db", case_relu_bias, trips_relu_bias, M=61, C=72, with_y=True, with_db=False, exact=False),
    _c("relu-bias-no-y", case_relu_bias, trips_relu_bias, M=333, C=200, with_y=False, with_db=True, exact=False),
    # ReLU bit masks
    _c("relu-bits-C8-loops", case_relu_bits, trips_relu_bits, True, M=4200001, C=8),
    _c("relu-bits-C32-loops", case_relu_bits, trips_relu_bits, True, M=4194381, C=32),
    _c("relu-bits-C40", case_relu_bits, trips_relu_bits, M=333, C=40),
    _c("relu-bits-C72", case_relu_bits, trips_relu_bits, M=61, C=72),
    _c("relu-bits-C256", case_relu_bits, trips_relu_bits, M=1001, C=256),
]
for _cs, _rows in ((6, 270001), (30, 66001), (85, 24001)):
    CASES.append(_c("cast-pad-%d-loops" % _cs, case_cast_pad, trips_cast_pad, True, rows=_rows, c_src=_cs, with_relu=_cs != 30))
    CASES.append(_c("cast-pad-%d-odd" % _cs, case_cast_pad, trips_cast_pad, rows=61, c_src=_cs, with_relu=_cs == 30))
# slice delivery: test_concat_gpu.py's parametrisation, each at the smallest convenient M that loops, and at M = 333
for _p, _M in (((256, 64, 32, True, 0), 524301), ((256, 0, 64, False, 1), 262201), ((256, 85, 171, True, 0), 12001), ((256, 0, 85, True, 1), 24001),
               ((24, 8, 8, True, 1), 2097201), ((16, 3, 5, False, 0), 262201)):
    CASES.append(_c("slice-%d-%d-%d-loops" % _p[:3], case_slice_deliver, trips_slice, True, ldy=_p[0], c0=_p[1], C=_p[2], masked=_p[3], acc=_p[4], M=_M))
    CASES.append(_c("slice-%d-%d-%d-odd" % _p[:3], case_slice_deliver, trips_slice, ldy=_p[0], c0=_p[1], C=_p[2], masked=_p[3], acc=_p[4], M=333))
CASES += [
    # resize + add: the LFPN's pairs with N large enough for the forward loop (80 -> 160 at N = 11: the backward loops as well)
    _c("resize-20-40-loops", case_resize, trips_resize, True, N=41, Hi=20, Wi=20, Ho=40, Wo=40, C=256, lateral=True, acc=0),
    _c("resize-40-80-loops", case_resize, trips_resize, True, N=11, Hi=40, Wi=40, Ho=80, Wo=80, C=256, lateral=True, acc=1),
    _c("resize-80-160-loops", case_resize, trips_resize, True, N=11, Hi=80, Wi=80, Ho=160, Wo=160, C=256, lateral=True, acc=1),
    _c("resize-ragged", case_resize, trips_resize, N=1, Hi=6, Wi=5, Ho=11, Wo=9, C=8, lateral=True, acc=0),
    _c("resize-ragged-no-lateral", case_resize, trips_resize, N=2, Hi=5, Wi=7, Ho=13, Wo=10, C=16, lateral=False, acc=1),
    _c("resize-identity", case_resize, trips_resize, N=1, Hi=8, Wi=8, Ho=8, Wo=8, C=8, lateral=False, acc=0),
    # average pool
    _c("avgpool-loops", case_avgpool, trips_avgpool, True, N=5, H=240, W=241, C=64, relu=True, masked=True, acc=1),
    _c("avgpool-odd", case_avgpool, trips_avgpool, N=1, H=5, W=7, C=8, relu=False, masked=False, acc=0),
    _c("avgpool-odd-relu-mask", case_avgpool, trips_avgpool, N=2, H=2, W=9, C=64, relu=True, masked=True, acc=0),
    _c("avgpool-1x1", case_avgpool, trips_avgpool, N=1, H=1, W=1, C=8, relu=False, masked=True, acc=1),
    # batch norm
    _c("bn-C8-loops", case_batchnorm, trips_batchnorm, True, M=2100001, C=8, relu=False, kind="random"),
    _c("bn-C64-shifted-loops", case_batchnorm, trips_batchnorm, True, M=270001, C=64, relu=True, kind="shifted"),
    _c("bn-C64-exact-loops", case_batchnorm, trips_batchnorm, True, M=270001, C=64, relu=False, kind="exact"),
    _c("bn-C72-loops", case_batchnorm, trips_batchnorm, True, M=30001, C=72, relu=False, kind="random"),
    _c("bn-C256-loops", case_batchnorm, trips_batchnorm, True, M=66001, C=256, relu=True, kind="random"),
    _c("bn-C2048-loops", case_batchnorm, trips_batchnorm, True, M=8201, C=2048, relu=False, kind="exact"),
    _c("bn-C2048-random", case_batchnorm, trips_batchnorm, True, M=1031, C=2048, relu=False, kind="random"),
    _c("bn-odd-C8", case_batchnorm, trips_batchnorm, M=61, C=8, relu=True, kind="random"),
    _c("bn-odd-C72", case_batchnorm, trips_batchnorm, M=101, C=72, relu=False, kind="random"),
    # add16 / residual backward
    _c("add16-loops", case_add16, trips_add16, True, n=8 * 2100001),
    _c("add16-odd", case_add16, trips_add16, n=8 * 61),
    _c("residual-loops", case_residual_bwd, trips_add16, True, n=8 * 2100001, masked=True, with_dx=True, acc=1),
    _c("residual-no-mask", case_residual_bwd, trips_add16, n=8 * 61, masked=False, with_dx=True, acc=0),
    _c("residual-no-dx", case_residual_bwd, trips_add16, n=8 * 61, masked=False, with_dx=False, acc=0),
    _c("residual-mask-acc0", case_residual_bwd, trips_add16, n=8 * 333, masked=True, with_dx=True, acc=0),
    _c("preprocess-loops", case_preprocess, trips_preprocess, True, N=6, H=640, W=640),
    _c("preprocess-odd", case_preprocess, trips_preprocess, N=2, H=9, W=33),
]

# the fp16 child's reduced list: one looping shape per kernel family plus the odd shape
FP16_IDS = ["maxpool2-loops", "maxpool2-odd-acc0", "maxpool3-loops", "maxpool3-odd", "l2norm-C64-loops", "l2norm-C128-loops", "l2norm-C256-loops",
            "l2norm-C512-loops", "l2norm-C1024-loops", "l2norm-C64-odd", "l2norm-C128-odd", "l2norm-C256-odd", "l2norm-C512-odd", "l2norm-C1024-odd",
            "l2norm-exact-C64", "junction-loops", "junction-odd", "relu-bias-C72-loops", "relu-bias-exact-C72", "relu-bias-odd", "relu-bits-C8-loops",
            "relu-bits-C72", "cast-pad-85-loops", "cast-pad-6-odd", "slice-256-0-64-loops", "slice-16-3-5-loops", "slice-256-85-171-odd",
            "resize-80-160-loops", "resize-ragged", "avgpool-loops", "avgpool-odd", "bn-C64-shifted-loops", "bn-C64-exact-loops", "bn-odd-C72",
            "add16-loops", "add16-odd", "residual-loops", "residual-no-mask", "preprocess-loops", "preprocess-odd"]


def run_case(cid, dt, dev):
    for c in CASES:
        if c[0] == cid:
            c[1](dt=dt, dev=dev, **c[3])
            if dev.type == "cuda":
                torch.cuda.empty_cache()
            return
    raise KeyError(cid)

"""Exact integer cases for the convolution kernels (conv_*.hip): generators, float64 reference, launch-plan restatements, case tables and the
runners tests/test_conv_exact_gpu.py and the fp16 child (tests/fp16/cases.py) share.

Why equality is the right check.  Every convolution kernel multiplies 16-bit operands with fp32 accumulation, combines partial sums in fp32 and
rounds once in its epilogue.  With integer-valued operands every partial sum is an integer below 2^24, exact in any order, so the result does
not depend on summation order, split, slab or atomic form: the device result must EQUAL the float64 reference, and a term counted zero times
or twice shows as a whole-number difference.  A 16-bit output is exact as long as |value| <= 256 (every integer up to 256 is a bf16 value; IEEE
half reaches 2048): LIMIT16 is asserted on the reference of every case whose output is stored in 16 bits, before anything is compared.

The same argument covers the second set of entry points - the channel-slice view calls (danhip_conv2d_*_strided, kinds vfwd / vdgrad / vwgrad:
operands inside wider buffers whose other channels hold a NaN pattern), danhip_conv2d_fwd_concat2, padding='valid' - and, with quarters instead
of integers, the whole DAN context block against its unfused float64 composition (BLOCK_CASES, tests/test_conv_views_exact_gpu.py).

Nothing in the first three sections needs a GPU or the library; the runners at the end import dan_amd lazily."""
import ctypes
import functools

import torch
import torch.nn.functional as F

LIMIT16 = 256           # largest |value| a 16-bit output may hold in these cases
BUDGET = 1024           # expected number of non-zero products per output: density p = min(1, BUDGET / K)
F64 = torch.float64


# ================================================================================================================ reference (float64, CPU)
def same_pad(n, k, s):
    """TF 'same': out = ceil(n / s), total = max((out - 1) s + k - n, 0), the odd pixel goes after (bottom / right)."""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return total // 2, total - total // 2, out


def out_size(n, k, s, valid=False):
    """Output length of one axis: 'valid' floor((n - k) / s) + 1 (no padding), TF 'same' ceil(n / s)."""
    return (n - k) // s + 1 if valid else same_pad(n, k, s)[2]


def conv_ref(x, w, b=None, stride=1, valid=False):
    """x [N,H,W,Cin], w [kh,kw,Cin,Cout], b [Cout] or None, all float64 -> [N,Ho,Wo,Cout] float64 (cross-correlation; explicit 'same' padding,
    or none at all with valid: the windows that fit, rows / columns behind the last window are not read)."""
    assert x.dtype == F64 and w.dtype == F64
    kh, kw = w.shape[0], w.shape[1]
    xp = x.permute(0, 3, 1, 2)
    if not valid:
        pt, pb, _ = same_pad(x.shape[1], kh, stride)
        pl, pr, _ = same_pad(x.shape[2], kw, stride)
        xp = F.pad(xp, (pl, pr, pt, pb))
    return F.conv2d(xp, w.permute(3, 2, 0, 1), b, stride=stride).permute(0, 2, 3, 1).contiguous()


def dgrad_ref(dy, w, H, W, stride=1, valid=False):
    """Data gradient from autograd: d/dx of <conv_ref(x, w), dy>."""
    x = torch.zeros((dy.shape[0], H, W, w.shape[2]), dtype=F64, requires_grad=True)
    conv_ref(x, w, None, stride, valid).backward(dy)
    return x.grad


def wgrad_ref(x, dy, kh, kw, stride=1, valid=False):
    """Weight and bias gradient from autograd."""
    w = torch.zeros((kh, kw, x.shape[3], dy.shape[3]), dtype=F64, requires_grad=True)
    b = torch.zeros((dy.shape[3],), dtype=F64, requires_grad=True)
    conv_ref(x, w, b, stride, valid).backward(dy)
    return w.grad, b.grad


def pool_ref(y):
    """2x2 / stride-2 'same' max-pool of [N,H,W,C]: (pooled, code) with code = 2 dh + dw of the FIRST maximum in row-major window order
    (a later element replaces the running maximum only when strictly larger); elements outside the map do not exist."""
    N, H, W, C = y.shape
    Hp, Wp = (H + 1) // 2, (W + 1) // 2
    best = y[:, 0::2, 0::2].clone()
    code = torch.zeros((N, Hp, Wp, C), dtype=torch.int64)
    for k, (dh, dw) in ((1, (0, 1)), (2, (1, 0)), (3, (1, 1))):
        v = y[:, dh::2, dw::2]
        h, w_ = v.shape[1], v.shape[2]
        gt = v > best[:, :h, :w_]
        best[:, :h, :w_] = torch.where(gt, v, best[:, :h, :w_])
        code[:, :h, :w_] = torch.where(gt, torch.full_like(code[:, :h, :w_], k), code[:, :h, :w_])
    return best, code


def pack_codes(code):
    """[.., C] codes -> [pixels][C/4] bytes: channel c in bits 2 (c % 4) of byte c / 4 (conv_common.h: pool_arg_out)."""
    C = code.shape[-1]
    c = code.reshape(-1, C // 4, 4)
    return (c[..., 0] + 4 * c[..., 1] + 16 * c[..., 2] + 64 * c[..., 3]).to(torch.uint8)


def relu_bits(y):
    """[.., C] -> [pixels][C/8] bytes: bit r of byte k = (channel 8 k + r) > 0."""
    C = y.shape[-1]
    p = (y.reshape(-1, C // 8, 8) > 0).to(torch.int64)
    return (p * (2 ** torch.arange(8))).sum(-1).to(torch.uint8)


def pool_scatter(code, dy, H, W):
    """Backward of the pool through its codes: dy goes to the element its window's code names."""
    N, Hp, Wp, C = dy.shape
    out = torch.zeros((N, 2 * Hp, 2 * Wp, C), dtype=dy.dtype)
    for k, (dh, dw) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        out[:, dh::2, dw::2] = dy * (code == k)
    return out[:, :H, :W].contiguous()


def late_ties(y):
    """Number of pool windows whose maximum occurs more than once with the first occurrence not at code 0."""
    N, H, W, C = y.shape
    m, code = pool_ref(y)
    yp = torch.full((N, H + H % 2, W + W % 2, C), float("-inf"), dtype=y.dtype)
    yp[:, :H, :W] = y
    cnt = sum((yp[:, dh::2, dw::2] == m).to(torch.int64) for dh in (0, 1) for dw in (0, 1))
    return int(((cnt > 1) & (code > 0)).sum())


# ================================================================================================================ generators (integers only)
def gen(seed):
    return torch.Generator().manual_seed(seed)


def signs(shape, g):
    """dense +-1, never 0: no (tap, ci, co) is silent"""
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).to(F64)


def ternary(shape, p, g):
    """{-1, 0, 1}, non-zero with probability p"""
    keep = torch.rand(shape, generator=g) < p
    return signs(shape, g) * keep


def small(shape, g, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def density(K):
    return min(1.0, BUDGET / K)


def co8_of(cout):
    return (cout + 7) // 8 * 8


def cin_real_of(shape, cin_real=None):
    return cin_real if cin_real else (3 if shape[3] == 8 and shape[4] == 64 and shape[5] == 3 else shape[3])


@functools.lru_cache(maxsize=2)
def forward_inputs(shape, seed=1, cin_real=None, valid=False):
    """x (ternary, density 1024 / K), w (+-1), bias and residual in [-8, 8]; pre = conv + bias in float64.  A first-layer shape (Cin = 8 -> 64)
    has 3 real channels: channels 3..7 of the image stay zero and the weight is [3,3,3,64]."""
    N, H, W, Cin, Cout, kh, kw, s = shape
    g = gen(seed + sum(shape))
    cr = cin_real_of(shape, cin_real)
    x = torch.zeros((N, H, W, Cin), dtype=F64)
    x[..., :cr] = ternary((N, H, W, cr), density(kh * kw * cr), g)
    w = signs((kh, kw, cr, Cout), g)
    b = small((Cout,), g)
    pre = conv_ref(x[..., :cr].contiguous(), w, b, s, valid)
    res = small(tuple(pre.shape), g)
    return dict(x=x, w=w, b=b, res=res, pre=pre, cin_real=cr)


@functools.lru_cache(maxsize=2)
def dgrad_inputs(shape, seed=2, valid=False):
    """dy (ternary, density 1024 / (taps Cout), channels Cout .. Cout8 zero), w (+-1), mask in [-2, 2] (zeros and negatives), old dx in [-8, 8]."""
    N, H, W, Cin, Cout, kh, kw, s = shape
    g = gen(seed + sum(shape))
    Ho, Wo = out_size(H, kh, s, valid), out_size(W, kw, s, valid)
    dy = torch.zeros((N, Ho, Wo, co8_of(Cout)), dtype=F64)
    dy[..., :Cout] = ternary((N, Ho, Wo, Cout), density(kh * kw * Cout), g)
    w = signs((kh, kw, Cin, Cout), g)
    mask = small((N, H, W, Cin), g, -2, 2)
    old = small((N, H, W, Cin), g)
    dx = dgrad_ref(dy[..., :Cout].contiguous(), w, H, W, s, valid)
    return dict(dy=dy, w=w, mask=mask, old=old, dx=dx)


@functools.lru_cache(maxsize=2)
def wgrad_inputs(shape, seed=3, cin_real=None, valid=False):
    """x, dy dense ternary (p = 2/3), pre-filled dw / db in [-8, 8]; |dw| <= N H W + 8 < 2^24."""
    N, H, W, Cin, Cout, kh, kw, s = shape
    g = gen(seed + sum(shape) + (cin_real or 0))
    cr = cin_real_of(shape, cin_real)
    Ho, Wo = out_size(H, kh, s, valid), out_size(W, kw, s, valid)
    x = torch.zeros((N, H, W, Cin), dtype=F64)
    x[..., :cr] = ternary((N, H, W, cr), 2 / 3, g)
    dy = torch.zeros((N, Ho, Wo, co8_of(Cout)), dtype=F64)
    dy[..., :Cout] = ternary((N, Ho, Wo, Cout), 2 / 3, g)
    dw0, db0 = small((kh, kw, cr, Cout), g), small((Cout,), g)
    dw, db = wgrad_ref(x[..., :cr].contiguous(), dy[..., :Cout].contiguous(), kh, kw, s, valid)
    return dict(x=x, dy=dy, dw0=dw0, db0=db0, dw=dw + dw0, db=db + db0, cin_real=cr)


@functools.lru_cache(maxsize=2)
def fold_inputs(nhw, seed=4):
    """Second-layer data gradient (64 -> 64, 3x3) with the first layer's weight gradient folded in: dy, w2, the first layer's output y1 (only its
    sign pattern is used, as a bit mask), the 8-channel image x8 (3 real channels), pre-filled dw8 / db8.  Reference chain:
    dx = dgrad(dy) * (y1 > 0), dw8 = wgrad(x8, dx), db8 = sum dx."""
    N, H, W = nhw
    g = gen(seed + N + H + W)
    dy = ternary((N, H, W, 64), density(9 * 64), g)
    w2 = signs((3, 3, 64, 64), g)
    y1 = small((N, H, W, 64), g, -2, 2)
    x8 = torch.zeros((N, H, W, 8), dtype=F64)
    x8[..., :3] = ternary((N, H, W, 3), 2 / 3, g)
    dw0, db0 = small((3, 3, 3, 64), g), small((64,), g)
    dx = dgrad_ref(dy, w2, H, W, 1) * (y1 > 0)
    dw, db = wgrad_ref(x8[..., :3].contiguous(), dx, 3, 3, 1)
    return dict(dy=dy, w2=w2, y1=y1, x8=x8, dw0=dw0, db0=db0, dx=dx, dw=dw + dw0, db=db + db0)


# ---- the conditions a case must meet, asserted on the reference alone
def forward_outputs(inp, relu, residual):
    y = torch.relu(inp["pre"]) if relu else inp["pre"]
    return y + inp["res"] if residual else y


def check_forward_inputs(inp, relu=True, pool=False):
    pre = inp["pre"]
    assert pre.abs().max().item() + 8 <= LIMIT16, ("forward value beyond the 16-bit exact range", pre.abs().max().item())
    if relu:
        assert int((pre == 0).sum()) >= 1, "no output is exactly 0 before the activation"
    if pool:
        assert late_ties(torch.relu(pre)) >= 1, "no pool window has a repeated maximum whose first occurrence is not at code 0"


def dgrad_outputs(inp, masked, acc):
    dx = inp["dx"] * (inp["mask"] > 0) if masked else inp["dx"]
    return dx + inp["old"] if acc else dx


def check_dgrad_inputs(inp):
    assert inp["dx"].abs().max().item() + 8 <= LIMIT16, ("data gradient beyond the 16-bit exact range", inp["dx"].abs().max().item())
    m = inp["mask"]
    assert int((m == 0).sum()) >= 1 and int((m < 0).sum()) >= 1 and int((m > 0).sum()) >= 1


def check_dgrad_unreached(inp, shp):
    """A 1x1 / stride-2 data gradient has no term on a pixel with an odd row or column: the reference is 0 there and the buffer the call
    finds is not - so the acc = 0 comparison is a test of the zero store, the acc = 1 one of leaving the old value.  (A 1x1 map has no such
    pixel; the first half holds there emptily.)  -> the number of unreached pixels"""
    if not (shp[5] == 1 and shp[6] == 1 and shp[7] == 2):
        return None
    H, W = shp[1], shp[2]
    odd = ((torch.arange(H) % 2 == 1).reshape(H, 1) | (torch.arange(W) % 2 == 1).reshape(1, W)).reshape(1, H, W, 1)
    assert int(((inp["dx"] != 0) & odd).sum()) == 0, "a 1x1 / stride-2 data gradient with a term on an odd row or column"
    if H * W > 1:
        assert int(((inp["old"] != 0) & odd).sum()) >= 1, "the pre-filled dx is zero on every unreached pixel: a missing zero store would not show"
    return int(odd.sum()) * shp[0]


def check_wgrad_inputs(inp):
    x = inp["x"]
    assert x.shape[0] * x.shape[1] * x.shape[2] + 8 < 2 ** 24 and inp["dw"].abs().max().item() < 2 ** 24 and inp["db"].abs().max().item() < 2 ** 24


def check_wgrad_cuts(shp, edge, cus):
    """The cut a row-streaming weight-gradient case is there for, from the restated plan."""
    if edge not in ("cuts", "one_row"):
        return
    c, p = wg_rows_cuts(shp, cus), plan_wg_rows(shp, cus)
    if edge == "cuts":
        assert c["mid_strip"] >= 1 and c["crossing"] >= 1 and c["mid_image"] >= 1 and shp[1] % p["rows_per_split"] != 0 and c["last_strip_width"] == 8, (c, p)
    else:
        assert p["rows_per_split"] == 1 and p["splits"] == p["total_rows"] and c["mid_strip"] >= 1 and c["crossing"] == 0, (c, p)


def check_fold_inputs(inp):
    dx = inp["dx"]
    assert dx.abs().max().item() <= LIMIT16, "the folded form holds dX in 16 bits in LDS: exact only within the 16-bit exact range"
    assert dx.shape[0] * dx.shape[1] * dx.shape[2] * LIMIT16 + 8 < 2 ** 24
    assert int((inp["y1"] <= 0).sum()) >= 1 and int((dx != 0).sum()) >= 1


# ================================================================================================================ launch plans, restated
def cdiv(a, b):
    return (a + b - 1) // b


def wg_rows_eligible(shape):
    N, H, W, Cin, Cout, kh, kw, s = shape
    return kh == 3 and kw == 3 and s == 1 and Cin % 64 == 0 and W / (cdiv(W, 32) * 32) >= 0.6


def plan_wg_rows(shape, cus):
    """conv_wgrad_rows.hip plan_wg_rows: a K-step is one row of a 32-pixel-wide column strip of one image; row index k -> strip k // H
    (image strip // tiles_x, first column 32 (strip % tiles_x)), row k % H; split i owns rows [i rows_per_split, (i + 1) rows_per_split)."""
    N, H, W, Cin, Cout = shape[:5]
    cot = 128 if cdiv(Cout, 64) * 64 % 128 == 0 else 64
    p = dict(cot=cot, co8=co8_of(Cout), ci_tiles=Cin // 64)
    p["co_tiles"] = cdiv(p["co8"], cot)
    p["pairs"] = p["ci_tiles"] * p["co_tiles"]
    p["tiles_x"] = cdiv(W, 32)
    p["total_rows"] = N * p["tiles_x"] * H
    splits = min(max(cus // p["pairs"], 1), p["total_rows"])
    p["rows_per_split"] = cdiv(p["total_rows"], splits)
    p["splits"] = cdiv(p["total_rows"], p["rows_per_split"])
    p["slab"] = p["splits"] >= 2 and p["rows_per_split"] <= 192
    p["slab_bytes"] = cus * 9 * (cot // 32) * 512 * 16
    return p


def wg_rows_cuts(shape, cus):
    """What the split boundaries of a row-streaming launch do: (splits that start inside a strip, splits that walk from one strip into the
    next - two more warm-up steps, boundaries inside an image, rows of the last split, width of the last strip)."""
    N, H, W = shape[:3]
    p = plan_wg_rows(shape, cus)
    rps, total = p["rows_per_split"], p["total_rows"]
    begins = [i * rps for i in range(p["splits"])]
    ends = [min(total, b + rps) for b in begins]
    mid_strip = sum(1 for b in begins if b % H != 0)
    crossing = sum(1 for b, e in zip(begins, ends) if b // H != (e - 1) // H)
    mid_image = sum(1 for b in begins[1:] if b % (H * p["tiles_x"]) != 0)
    return dict(mid_strip=mid_strip, crossing=crossing, mid_image=mid_image, last_rows=ends[-1] - begins[-1], last_strip_width=W - (p["tiles_x"] - 1) * 32)


def wg_pw_eligible(shape):
    N, H, W, Cin, Cout, kh, kw, s = shape
    M = N * H * W
    return kh == 1 and kw == 1 and s == 1 and Cin % 64 == 0 and Cin >= 128 and co8_of(Cout) >= 64 and M >= 4096 and M * Cin < 2 ** 31 and M * co8_of(Cout) < 2 ** 31


def plan_wg_pw(shape, cus):
    """conv_wgrad_pw.hip plan_wg_pw: a K-step is 32 pixels; 256 x 256 (ci, co) tiles."""
    N, H, W, Cin, Cout = shape[:5]
    p = dict(co8=co8_of(Cout), ksteps=cdiv(N * H * W, 32), ci_tiles=cdiv(Cin, 256))
    p["co_tiles"] = cdiv(p["co8"], 256)
    p["pairs"] = p["ci_tiles"] * p["co_tiles"]
    splits = min(max(cus // p["pairs"], 1), p["ksteps"])
    p["steps_per_split"] = cdiv(p["ksteps"], splits)
    p["splits"] = cdiv(p["ksteps"], p["steps_per_split"])
    p["slab"] = p["splits"] >= 2 and p["steps_per_split"] <= 192
    p["slab_bytes"] = cus * 32 * 512 * 16
    return p


def wgrad_workspace_bytes(shape, cus):
    """danhip_conv2d_bwd_weight_workspace_bytes with the default options: the row-streaming plan's slab, else the pointwise plan's."""
    if wg_rows_eligible(shape):
        p = plan_wg_rows(shape, cus)
        if p["slab"]:
            return p["slab_bytes"]
    if wg_pw_eligible(shape):
        p = plan_wg_pw(shape, cus)
        if p["slab"]:
            return p["slab_bytes"]
    return 0


def plan_splitk(shape, which, cus, valid=False):
    """conv_igemm.hip plan_splitk for a forward (which = 0) / data-gradient (which = 1) call: (splits, K tiles per split, M, Co); splits = 1: none."""
    N, H, W, Cin, Cout, kh, kw, s = shape
    Ho, Wo = out_size(H, kh, s, valid), out_size(W, kw, s, valid)
    if which == 0:
        M, Co, C = N * Ho * Wo, Cout, Cin
    else:
        M, Co, C = N * H * W, Cin, co8_of(Cout)
        if s & (s - 1):
            return 1, 0, M, Co
    ktiles = cdiv(kh * kw * C, 64)
    bn = 128 if Co % 128 == 0 else 64 if Co % 64 == 0 else 16 if Co <= 16 else 32 if Co <= 32 else 64
    bm = 128 if bn == 128 else (64 if M <= 256 * 128 else 256) if bn == 16 else 256
    tiles = cdiv(M, bm) * cdiv(Co, bn)
    target = (8 if bn == 16 else 2) * cus
    if tiles * 2 > target or ktiles < 8:
        return 1, ktiles, M, Co
    splits = min(cdiv(target, tiles), ktiles // 4, 36)
    if splits < 2:
        return 1, ktiles, M, Co
    per = cdiv(ktiles, splits)
    return cdiv(ktiles, per), per, M, Co


def conv_workspace_bytes(shape, which, cus, valid=False):
    splits, _, M, Co = plan_splitk(shape, which, cus, valid)
    return splits * M * Co * 4 if splits >= 2 else 0


# ================================================================================================================ case tables
def S(N, H, W, Cin, Cout, k=3, s=1):
    kh, kw = (k, k) if isinstance(k, int) else k
    return (N, H, W, Cin, Cout, kh, kw, s)


HALO = "conv3x3_halo_kernel<"
PW = "conv_pointwise_kernel<"
FLAT = "conv_igemm_kernel<"
# Forward edge shapes: (id, shape, family of the single-pass call - a prefix, ' * ' standing for the rest, extra)
#   extra: "f32only" (Cout % 8 != 0: fp32 output only), "splitk" (the call with scratch must split K: asserted from the restated plan)
FWD_EDGES = [
    ("halo8x32_ragged_edges", S(2, 30, 62, 128, 64), HALO + "8, 32, 64, * >", ""),
    ("halo16x16", S(8, 48, 48, 64, 128), HALO + "16, 16, 128, * >", ""),
    ("halo_second_round", S(5, 56, 96, 128, 128), HALO + "8, 32, 128, * >", ""),                  # 630 work items on 256 persistent workgroups
    ("head8", S(2, 16, 32, 256, 8), HALO + "8, 32, 64, * 3, 3, false, 1, false>", ""),
    ("head6", S(1, 32, 32, 64, 6), HALO + "8, 32, 64, * 3, 3, false, 1, false>", "f32only"),
    ("ragged_cin136_cout200", S(1, 32, 32, 136, 200), HALO + "8, 32, 128, * >", ""),
    ("ragged_cin72", S(2, 16, 32, 72, 128), HALO + "8, 32, 128, * >", ""),
    ("c64_ragged_edges", S(1, 30, 62, 64, 64), "conv3x3_c64_kernel<false>", ""),
    ("first_layer_one_column", S(1, 5, 1, 8, 64), "conv3x3_c8_kernel<true>", ""),
    ("first_layer_ragged", S(2, 17, 45, 8, 64), "conv3x3_c8_kernel<true>", ""),
    ("pointwise_k2304", S(1, 64, 72, 2304, 256, 1), PW + "256, * false>", ""),
    ("pointwise_ragged_cout72", S(1, 65, 67, 64, 72, 1), FLAT + "256, 64, 1, true>", ""),
    ("taps_3x1", S(2, 40, 44, 128, 64, (3, 1)), PW + "64, * true>", ""),
    ("taps_1x3", S(2, 40, 44, 64, 128, (1, 3)), PW + "128, * true>", ""),
    ("taps_stride2", S(6, 40, 40, 256, 256, 3, 2), PW + "256, * true>", ""),
    ("taps_192_320", S(3, 37, 41, 192, 320), PW + "64, * true>", ""),
    ("flat_slow", S(1, 7, 9, 72, 24), FLAT + "256, 32, 1, false>", ""),
    ("splitk_512", S(1, 10, 10, 512, 512), FLAT + "128, 128, 2, true>", "splitk"),
    ("splitk_1024", S(1, 6, 6, 512, 1024), FLAT + "128, 128, 2, true>", "splitk"),
    ("splitk_stride2", S(2, 20, 20, 256, 512, 3, 2), FLAT + "128, 128, 2, true>", "splitk"),
]
# Data-gradient edge shapes: the forward list's 3x3 / 1x1 shapes with Cout % 8 == 0, ragged Cout, the strided kernel, and (extra = "pw256") the
# 256-wide pointwise tiles with epilogue inputs (option pw_dgrad_ld_bn = 256).  Family: of the single-pass call WITH a mask.
DGRAD_EDGES = [
    ("halo8x32_ragged_edges", S(2, 30, 62, 128, 64), HALO + "8, 32, 128, * true, 0, false>", ""),
    ("halo16x16", S(8, 48, 48, 64, 128), HALO + "16, 16, 64, * true, 0, false>", ""),
    ("halo_second_round", S(5, 56, 96, 128, 128), HALO + "8, 32, 128, * true, 0, false>", ""),
    ("head8", S(2, 16, 32, 256, 8), FLAT + "128, 128, 2, false>", ""),
    ("ragged_cin136_cout200", S(1, 32, 32, 136, 200), HALO + "8, 32, 64, * true, 0, false>", ""),
    ("ragged_cin72", S(2, 16, 32, 72, 128), HALO + "8, 32, 128, * true, 0, false>", ""),
    ("c64_ragged_edges", S(1, 30, 62, 64, 64), "conv3x3_c64_kernel<true>", ""),
    ("first_layer_one_column", S(1, 5, 1, 8, 64), FLAT + "64, 16, 1, true>", ""),
    ("first_layer_ragged", S(2, 17, 45, 8, 64), FLAT + "64, 16, 1, true>", ""),
    ("pointwise_k2304", S(1, 64, 72, 2304, 256, 1), PW + "128, 4, true, true, false>", ""),
    ("pointwise_ragged_cout72", S(1, 65, 67, 64, 72, 1), FLAT + "256, 64, 1, false>", ""),
    ("stride2", S(6, 40, 40, 256, 256, 3, 2), FLAT + "128, 128, 2, true>", ""),
    ("taps_192_320", S(3, 37, 41, 192, 320), PW + "64, 4, true, true, true>", ""),
    ("flat_slow", S(1, 7, 9, 72, 24), FLAT + "256, 64, 1, false>", ""),
    ("splitk_512", S(1, 10, 10, 512, 512), FLAT + "128, 128, 2, true>", "splitk"),
    ("splitk_1024", S(1, 6, 6, 512, 1024), FLAT + "128, 128, 2, true>", "splitk"),
    ("splitk_stride2", S(2, 20, 20, 256, 512, 3, 2), FLAT + "128, 128, 2, true>", "splitk"),
    ("ragged_cout85", S(2, 40, 48, 256, 85, 1), FLAT + "128, 128, 2, false>", ""),
    ("ragged_cout30", S(1, 12, 12, 64, 30), FLAT + "256, 64, 1, false>", ""),
    ("stride3_direct", S(1, 9, 9, 8, 8, 3, 3), "conv_bwd_data_strided_kernel", ""),
    ("pw256_3x3", S(3, 37, 40, 256, 128), PW + "256, 3, true, true, true>", "pw256"),
    ("pw256_3x1", S(2, 40, 40, 256, 64, (3, 1)), PW + "256, 3, true, true, true>", "pw256"),
]
# Weight-gradient edge shapes: (id, shape, family, cin_real or None, extra); extra "cuts": the row-streaming plan must cut inside a strip and
# inside an image, a split must walk into the next strip (rows_per_split does not divide H), and the last strip is 8 columns wide;
# "one_row": every split is one row and its two warm-up steps, and splits start inside a strip
WGRAD_EDGES = [
    ("rows_cuts_w40", S(3, 37, 40, 256, 128), "conv_wgrad_rows_kernel<128>", None, "cuts"),
    ("rows64_cuts_w40", S(3, 37, 40, 128, 64), "conv_wgrad_rows_kernel<64>", None, "cuts"),     # the 64-wide tile: 111 splits of 2 rows
    ("rows_one_row_per_split", S(1, 33, 47, 64, 64), "conv_wgrad_rows_kernel<64>", None, "one_row"),     # 66 rows on 256 CUs
    ("rows_ragged_cout72", S(2, 32, 64, 256, 72), "conv_wgrad_rows_kernel<128>", None, ""),
    ("rows_head8", S(2, 16, 32, 256, 8), "conv_wgrad_rows_kernel<64>", None, ""),
    ("pw_k2304", S(1, 64, 72, 2304, 256, 1), "conv_wgrad_pw_kernel", None, ""),
    ("pw_320_192", S(3, 40, 40, 320, 192, 1), "conv_wgrad_pw_kernel", None, ""),
    ("pw_128_512", S(2, 50, 50, 128, 512, 1), "conv_wgrad_pw_kernel", None, ""),
    ("tiles_stride2", S(2, 10, 10, 128, 256, 3, 2), "conv_wgrad_kernel<128, 128, 2>", None, ""),
    ("tiles_stride2_odd", S(1, 5, 5, 128, 256, 3, 2), "conv_wgrad_kernel<128, 128, 2>", None, ""),
    ("tiles_3x1", S(1, 12, 12, 64, 32, (3, 1)), "conv_wgrad_kernel<64, 64, 2>", None, ""),
    ("tiles_1x3", S(1, 12, 12, 64, 32, (1, 3)), "conv_wgrad_kernel<64, 64, 2>", None, ""),
    ("tiles_ragged_cout171", S(1, 33, 20, 64, 171, 1), "conv_wgrad_kernel<64, 128, 2>", None, ""),
    ("tiles_head6", S(1, 8, 8, 512, 6), "conv_wgrad_kernel<128, 64, 2>", None, ""),
]
# ... and the first layer: every shape with 3, 4 and 1 real input channels
WGRAD_EDGES += [("c8_%s_cin%d" % (n, c), S(*nhw, 8, 64), "conv_wgrad_c8_kernel", c, "") for n, nhw in (("one_column", (1, 5, 1)), ("ragged", (2, 37, 131)), ("wide", (3, 64, 100)))
                for c in (3, 4, 1)]
# Fused pool / masks: even sizes, odd sizes (the last window has one row / column)
POOL_EDGES = [
    ("c64_even", S(2, 16, 64, 64, 64), "conv3x3_c64_kernel<false>"),
    ("halo128_even", S(3, 32, 64, 64, 128), HALO + "8, 32, 128, * false, 0, true>"),
    ("c64_odd", S(1, 30, 62, 64, 64), "conv3x3_c64_kernel<false>"),
    ("halo16x16_odd", S(1, 31, 45, 128, 256), HALO + "16, 16, 128, * false, 0, true>"),
]
FOLD_SHAPES = [(1, 30, 62), (3, 40, 96)]


# 'valid' padding (the ResNet stem and one 3x3): (id, kind, shape, family, cin_real, extra)
VALID_CASES = [
    ("fwd_valid_stem", "fwd", S(2, 29, 35, 8, 64, 7, 2), FLAT + "256, 64, 1, false>", 3, ""),
    ("dgrad_valid_stem", "dgrad", S(2, 29, 35, 8, 64, 7, 2), FLAT + "64, 16, 1, true>", None, "splitk"),
    ("wgrad_valid_stem", "wgrad", S(2, 29, 35, 8, 64, 7, 2), "conv_wgrad_kernel<64, 64, 2>", 3, ""),
    ("fwd_valid_3x3", "fwd", S(1, 9, 11, 64, 64), FLAT + "256, 64, 1, true>", None, "splitk"),
    ("dgrad_valid_3x3", "dgrad", S(1, 9, 11, 64, 64), FLAT + "256, 64, 1, true>", None, "splitk"),
    ("wgrad_valid_3x3", "wgrad", S(1, 9, 11, 64, 64), "conv_wgrad_kernel<64, 64, 2>", None, ""),
]

# ---- the ResNet backbone's convolutions (net/resnet_danet.py) at its channel counts: the 1x1 / stride-2 projection shortcut and `reduce`
# (padding='valid', what the backbone passes; for a 1x1 window 'valid' and 'same' describe the same map, one shape runs under both), K or
# Cout of 2048, and the 3x3 / stride-2 extra layers on the 2x2 and 1x1 maps a 64-pixel input leaves them.
# A 1x1 / stride-2 data gradient reaches one pixel in four: acc = 0 must store 0 on the others (dx is pre-filled with `old`), acc = 1 must
# leave `old` there; the weight gradient must skip the same three quarters of x; an odd map samples its last row and column, an even one
# never reads them.
#   (id, shape, valid, forward family, forward extra, data-gradient family, data-gradient extra, weight-gradient family); the families are the
#   label functions' answers, extra "splitk" where plan_splitk splits K on 256 CUs.  Forward: the streaming GEMM takes 2048 output pixels and
#   up - pw_s2_taps is the projection on a map large enough for its one-tap TAPS form, every other shape runs the flat-M kernel.  Data
#   gradient: the streaming GEMM declines dstride != 1, so every stride-2 shape is the flat-M kernel's fractionally strided gather.
F128 = FLAT + "128, 128, 2, true>"
WG128 = "conv_wgrad_kernel<128, 128, 2>"
RESNET_CASES = [
    ("pw_s2_256_512", S(2, 15, 17, 256, 512, 1, 2), True, F128, "", F128, "splitk", WG128),              # projection shortcut, odd map
    ("pw_s2_256_512_same", S(2, 15, 17, 256, 512, 1, 2), False, F128, "", F128, "splitk", WG128),
    ("pw_s2_256_128", S(2, 15, 17, 256, 128, 1, 2), True, F128, "", F128, "", WG128),                    # strided reduce
    ("pw_s2_512_1024_even", S(2, 8, 10, 512, 1024, 1, 2), True, F128, "splitk", F128, "splitk", WG128),  # even map: last row / column never read
    ("pw_s2_1024_2048", S(1, 9, 7, 1024, 2048, 1, 2), True, F128, "splitk", F128, "splitk", WG128),      # the widest projection
    ("pw_s2_1x1map", S(2, 1, 1, 256, 512, 1, 2), True, F128, "", F128, "splitk", WG128),                 # one pixel in, one pixel out
    ("pw_k2048", S(1, 5, 7, 2048, 512, 1, 1), True, F128, "splitk", F128, "splitk", WG128),              # conv6_1
    ("pw_cout2048", S(1, 6, 6, 512, 2048, 1, 1), True, F128, "splitk", F128, "splitk", WG128),           # increase of the last stage
    ("x3s2_2x2", S(2, 2, 2, 512, 512, 3, 2), False, F128, "splitk", F128, "splitk", WG128),              # conv6_2: 2x2 -> 1x1
    ("x3s2_1x1map", S(2, 1, 1, 128, 256, 3, 2), False, F128, "splitk", F128, "splitk", WG128),           # conv7_2: only the centre tap exists
    ("pw_s2_taps", S(2, 63, 67, 256, 512, 1, 2), True, PW + "256, 3, false, true, true>", "", F128, "splitk", WG128),      # 32 x 34 outputs: 17 items
]

# ---- channel-slice views (danhip_conv2d_{fwd,bwd_data,bwd_weight}_strided): every operand is channels c0 : c0 + C of a wider NHWC buffer whose
# other channels hold NAN16, a bit pattern that is a NaN in bf16 and in IEEE half.  A read outside the slice poisons the result, a store
# outside it changes the pattern (compared as int16: a stray store of 0 shows too).  The buffers are the context block's (ops._ContextBlock):
# T 192 wide, hyper 256, the block input C or C + 128; slices at 0:64, 64:128, 128:192, 192:256.
NAN16 = 0x7FFF
C64F, C64D = "conv3x3_c64_kernel<false>", "conv3x3_c64_kernel<true>"
# forward: (id, shape, label of the table's call, (x width, x c0, y width, y c0), relu_channels strictly inside, extra)
#   the table's call: with the scratch the library asks for, ReLU on all channels - on `inside` channels where extra says "partial"
#   extra: "plus" (the weight the block packs a 3x1 and a 1x3 convolution into), "splitk" (the call with scratch splits K: restated plan)
VFWD_CASES = [
    ("pw_cat192", S(1, 40, 56, 256, 192, 1), PW + "64, 4, false, true, false>", (384, 64, 256, 64), 128, "partial"),      # 17.5 items of 128 pixels
    ("pw_b1", S(1, 40, 56, 256, 64, 1), PW + "64, 4, false, true, false>", (256, 0, 256, 0), 32, ""),
    ("c64", S(1, 30, 62, 64, 64), C64F, (192, 64, 256, 192), 32, ""),
    ("c64_plus", S(1, 30, 62, 64, 64), C64F, (192, 0, 256, 128), 32, "plus"),
    ("splitk_2x6x6", S(2, 6, 6, 64, 64), FLAT + "256, 64, 1, true>", (192, 0, 256, 128), 32, "splitk"),
    ("splitk_cat192", S(16, 3, 3, 1024, 192, 1), FLAT + "256, 64, 1, true>", (1024, 0, 256, 64), 128, "splitk partial"),
]
# data gradient: (id, shape, label of the masked accumulating call with scratch, (dy width, c0, dx width, c0, mask width, c0), extra)
VDGRAD_CASES = [
    ("c64", S(1, 30, 62, 64, 64), C64D, (256, 128, 192, 0, 192, 0), ""),
    ("c64_plus", S(1, 30, 62, 64, 64), C64D, (256, 192, 192, 64, 192, 64), "plus"),
    ("splitk_2x6x6", S(2, 6, 6, 64, 64), FLAT + "256, 64, 1, true>", (256, 128, 192, 0, 256, 64), "splitk"),
    ("flat_cat192", S(16, 3, 3, 1024, 192, 1), FLAT + "128, 128, 2, true>", (256, 64, 1152, 64, 1088, 64), ""),      # K = 192: three K tiles, no split
    ("splitk_res", S(16, 3, 3, 256, 1024, 1), FLAT + "128, 128, 2, true>", (1088, 64, 384, 64, 320, 64), "splitk"),   # the residual conv's: 4 splits
    ("pw_cat192", S(1, 40, 56, 256, 192, 1), PW + "128, 4, true, true, false>", (256, 64, 384, 64, 320, 64), ""),
]
# weight gradient: (id, shape, label, (x width, c0, dy width, c0), extra); "det": also twice in deterministic mode, "pitch": declined by the
# row-streaming kernel (its lane offsets hold pitches up to 65535)
VWGRAD_CASES = [
    ("rows", S(3, 37, 40, 64, 64), "conv_wgrad_rows_kernel<64>", (192, 0, 256, 128), "det"),
    ("pw", S(2, 50, 50, 256, 192, 1), "conv_wgrad_pw_kernel", (384, 64, 256, 64), "det"),
    ("generic", S(16, 3, 3, 1024, 192, 1), "conv_wgrad_kernel<128, 128, 2>", (1088, 64, 256, 64), ""),
    ("pitch65600", S(1, 4, 40, 64, 64), "conv_wgrad_kernel<64, 64, 2>", (65600, 64, 256, 128), "pitch"),
]
# danhip_conv2d_fwd_concat2: (id, (N, H, W), c1, c2, Cout, src_pitch, label); 2240 pixels = 17.5 items
CONCAT2_CASES = [
    ("64_192_128", (1, 40, 56), 64, 192, 128, 256, "conv_pointwise_concat2_kernel<128, 4>"),
    ("256_64_64", (1, 40, 56), 256, 64, 64, 320, "conv_pointwise_concat2_kernel<64, 4>"),
    ("256_256_256", (1, 40, 56), 256, 256, 256, 256, "conv_pointwise_concat2_kernel<256, 3>"),
]


def plus_mask():
    """[3,3,64,64] 0 / 1: the 3x1 taps in the middle column for outputs 0..31, the 1x3 taps in the middle row for outputs 32..63."""
    m = torch.zeros((3, 3, 64, 64), dtype=F64)
    m[:, 1, :, :32] = 1
    m[1, :, :, 32:] = 1
    return m


def view_kernel(shape, which, cus, scratch=False, partial=False, ld=True):
    """select_conv (conv_igemm.hip) restated for a stride-1 'same' view call: the label of a forward (which = 0; partial: ReLU on some columns
    only) or data-gradient (which = 1; ld: with a mask or accumulating) call, with / without the scratch the library asks for."""
    N, H, W, Cin, Cout, kh, kw, s = shape
    assert s == 1
    M = N * H * W
    C, Co = (Cin, Cout) if which == 0 else (co8_of(Cout), Cin)
    tf = lambda v: "true" if v else "false"
    if kh == 3 and kw == 3 and C == 64 and Co == 64 and not partial and H * W / (cdiv(H, 8) * 8 * cdiv(W, 32) * 32) >= 0.78:
        return C64F if which == 0 else C64D
    prefer = scratch and plan_splitk(shape, which, cus)[0] >= 2 and cdiv(M, 128) * cdiv(Co, 128) * 2 <= cus
    if not prefer and C % 64 == 0 and Co % 64 == 0 and M >= 2048 and kh * kw <= 32:
        ld = ld or which == 0
        bn = 256 if Co % 256 == 0 and not (which == 1 and ld) else 128 if Co % 128 == 0 else 64
        return PW + "%d, %d, %s, %s, %s>" % (bn, 3 if bn == 256 else 4, tf(which == 1), tf(ld), tf(kh * kw > 1))
    bn = 128 if Co % 128 == 0 else 64 if Co % 64 == 0 else 16 if Co <= 16 else 32 if Co <= 32 else 64
    tile = {128: "128, 128, 2", 64: "256, 64, 1", 32: "256, 32, 1", 16: "64, 16, 1" if M <= 256 * 128 else "256, 16, 1"}[bn]
    return FLAT + "%s, %s>" % (tile, tf(C % 64 == 0))


def view_forward_inputs(shape, plus=False):
    inp = dict(forward_inputs(shape))
    if plus:
        inp["w"] = inp["w"] * plus_mask()
        inp["pre"] = conv_ref(inp["x"], inp["w"], inp["b"], 1)
    return inp


def view_forward_outputs(inp, relu_co):
    y = inp["pre"].clone()
    y[..., :relu_co] = torch.relu(y[..., :relu_co])
    return y


def view_dgrad_inputs(shape, plus=False):
    inp = dict(dgrad_inputs(shape))
    if plus:
        N, H, W, Cin, Cout = shape[:5]
        inp["w"] = inp["w"] * plus_mask()
        inp["dx"] = dgrad_ref(inp["dy"][..., :Cout].contiguous(), inp["w"], H, W, 1)
    return inp


def concat2_shape(case):
    cid, nhw, c1, c2, cout, pitch, label = case
    return S(*nhw, c1 + c2, cout, 1)


def check_vfwd(case, cus):
    cid, kind, shp, family, extra = case
    Cout, inside, edge = shp[4], extra["inside"], extra["edge"]
    inp = view_forward_inputs(shp, "plus" in edge)
    check_forward_inputs(inp, relu=True)
    pre = inp["pre"]
    assert 0 < inside < Cout and inside % 8 == 0
    # partial ReLU: the linear columns hold a negative value (a ReLU there shows), the ReLU columns a negative pre-activation and an exact 0
    assert int((pre[..., inside:] < 0).sum()) >= 1 and int((pre[..., :inside] < 0).sum()) >= 1
    assert int((view_forward_outputs(inp, inside)[..., :inside] == 0).sum()) >= 1
    nws = conv_workspace_bytes(shp, 0, cus)
    if "splitk" in edge:
        assert plan_splitk(shp, 0, cus)[0] >= 2, "the case is there for a split K"
    assert view_kernel(shp, 0, cus, scratch=bool(nws), partial="partial" in edge) == family, "the table's family is not what the selection reads as"
    if "plus" in edge:
        assert int((inp["w"] == 0).sum()) == 6 * 64 * 64 and inp["w"][1, 1].abs().min().item() == 1
    xw, xc, yw, yc = extra["geom"]
    assert xc + shp[3] <= xw and yc + Cout <= yw and (xw | xc | yw | yc) % 8 == 0
    return dict(max=pre.abs().max().item(), zeros=int((pre == 0).sum()), splits=plan_splitk(shp, 0, cus)[0])


def check_vdgrad(case, cus):
    cid, kind, shp, family, extra = case
    inp = view_dgrad_inputs(shp, "plus" in extra["edge"])
    check_dgrad_inputs(inp)
    assert int((inp["dx"] != 0).sum()) >= 1
    nws = conv_workspace_bytes(shp, 1, cus)
    if "splitk" in extra["edge"]:
        assert plan_splitk(shp, 1, cus)[0] >= 2, "the case is there for a split K"
    assert view_kernel(shp, 1, cus, scratch=bool(nws), ld=True) == family, "the table's family is not what the selection reads as"
    yw, yc, xw, xc, mw, mc = extra["geom"]
    assert yc + co8_of(shp[4]) <= yw and xc + shp[3] <= xw and mc + shp[3] <= mw and (yw | yc | xw | xc | mw | mc) % 8 == 0
    return dict(max=inp["dx"].abs().max().item(), splits=plan_splitk(shp, 1, cus)[0])


def check_vwgrad(case, cus):
    cid, kind, shp, family, extra = case
    inp = wgrad_inputs(shp)
    check_wgrad_inputs(inp)
    xw, xc, yw, yc = extra["geom"]
    assert xc + shp[3] <= xw and yc + co8_of(shp[4]) <= yw and (xw | xc | yw | yc) % 8 == 0 and shp[0] * shp[1] * shp[2] * max(xw, yw) < 2 ** 31
    rows, pw = wg_rows_eligible(shp) and max(xw, yw) <= 0xFFFF, wg_pw_eligible(shp)
    assert family.startswith("conv_wgrad_rows_kernel<") == rows and (family == "conv_wgrad_pw_kernel") == (pw and not rows)
    if extra["edge"] == "pitch":
        assert wg_rows_eligible(shp) and xw > 0xFFFF, "the case is there for a pitch the row-streaming kernel declines"
    return dict(max=inp["dw"].abs().max().item())


def check_concat2(case, cus):
    cid, kind, shp, family, extra = case
    inp = forward_inputs(shp)
    check_forward_inputs(inp, relu=True)
    M, c1, c2, pitch = shp[0] * shp[1] * shp[2], extra["c1"], shp[3] - extra["c1"], extra["pitch"]
    assert M >= 2048 and M % 128 != 0 and c1 % 64 == 0 and c2 % 64 == 0 and pitch >= max(c1, c2) and pitch % 8 == 0
    # both sources matter to every output column: a K-step taken from the wrong source, or skipped, changes the sums
    assert int((inp["x"][..., :c1] != 0).sum()) >= 1 and int((inp["x"][..., c1:] != 0).sum()) >= 1
    return dict(max=inp["pre"].abs().max().item(), zeros=int((inp["pre"] == 0).sum()))


VIEW_CHECKS = dict(vfwd=check_vfwd, vdgrad=check_vdgrad, vwgrad=check_vwgrad, concat2=check_concat2)


# ---- the DAN context block (net/danet.py se_inception_block), unfused, in float64: ten convolutions, TF 'same' 2x2 / stride-1 average pool,
# concat, residual add - and its autograd.  ops.context_block computes the same function another way (three 1x1s as one, branch 2's 1x1 in
# front of its pool, each 3x1 / 1x3 pair as one 3x3, slices instead of a concat); with the operands below every value either route stores in
# 16 bits is a multiple of 1/4 that both 16-bit types hold exactly and every fp32 sum is exact, so the two agree to the last bit.
BLOCK_LAYERS = [("branch1_conv_1x1", 1, 1, None, 64), ("branch2_conv_1x1", 1, 1, None, 64), ("branch3_conv_1x1", 1, 1, None, 64), ("branch3_conv_3x1", 3, 1, 64, 32),
                ("branch3_conv_1x3", 1, 3, 64, 32), ("branch4_conv_1x1", 1, 1, None, 64), ("branch4_conv_3x3", 3, 3, 64, 64), ("branch4_conv_1x3", 3, 1, 64, 32),
                ("branch4_conv_3x1", 1, 3, 64, 32), ("residual_conv", 1, 1, 256, None)]          # (kh, kw, Cin, Cout); None = the block's channel count
# (id, (N, H, W, C), seed, non-zero products per output of the layers above, density of x and of the upstream gradient)
#   streaming: 2079 pixels = 16.2 items of the streaming GEMM (its floor is 2048), 33 x 63 of 40 x 64 tile pixels = 0.81: the register-resident
#   64 -> 64 kernel takes the 3x3s, the row-streaming kernel their weight gradients; splitk: 72 pixels, every convolution with >= 8 K tiles splits
BLOCK_CASES = [
    ("streaming_1x33x63", (1, 33, 63, 256), 1, (4, 4, 4, 4, 4, 4, 6, 4, 4, 4), 0.25, 0.05),
    ("splitk_2x6x6", (2, 6, 6, 256), 2, (4, 4, 4, 4, 4, 4, 6, 4, 4, 4), 0.25, 0.05),
]


def conv_taps(x, w, b):
    """conv_ref for stride 1 / 'same' as one float64 matrix product per tap over the shifted map (the block's reference: many times faster on
    a CPU than the float64 convolution, and differentiable the same way)."""
    kh, kw = w.shape[0], w.shape[1]
    N, H, W, _ = x.shape
    (pt, pb, _), (pl, pr, _) = same_pad(H, kh, 1), same_pad(W, kw, 1)
    xp = F.pad(x, (0, 0, pl, pr, pt, pb))
    y = b.reshape(1, 1, 1, -1)
    for i in range(kh):
        for j in range(kw):
            y = y + xp[:, i:i + H, j:j + W] @ w[i, j]
    return y


def avg_pool_ref(x):
    """tf.layers.average_pooling2d(x, (2, 2), 1, 'same'): window rows h, h + 1 and columns w, w + 1, divided by the number of them inside the map."""
    N, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 0, 1, 0, 1))
    s = xp[:, :H, :W] + xp[:, 1:, :W] + xp[:, :H, 1:] + xp[:, 1:, 1:]
    cnt = torch.full((H, W), 4.0, dtype=F64)
    cnt[H - 1, :], cnt[:, W - 1] = 2.0, 2.0
    cnt[H - 1, W - 1] = 1.0
    return s / cnt.reshape(1, H, W, 1)


@functools.lru_cache(maxsize=2)
def block_inputs(nhwc, seed, products, px, pdy):
    """Sparse integer input and upstream gradient, sparse ternary kernels (about `products` non-zero taps per output), biases in [-1, 1]."""
    N, H, W, C = nhwc
    g = gen(seed)
    P = {}
    for (name, kh, kw, cin, cout), k in zip(BLOCK_LAYERS, products):
        cin, cout = cin or C, cout or C
        P[name + "/kernel"] = ternary((kh, kw, cin, cout), min(1.0, k / (kh * kw * cin)), g)
        P[name + "/bias"] = small((cout,), g, -1, 1)
    x = ternary((N, H, W, C), px, g) * small((N, H, W, C), g, 1, 2)
    dy = ternary((N, H, W, C), pdy, g)
    return dict(x=x, dy=dy, P=P)


def block_ref(x, P, commuted=False):
    """-> (out, dict of every intermediate).  commuted: branch 2 as conv-then-pool (the order ops.context_block takes; the same function)."""
    t = {}

    def cr(inp, name, key):
        t[key + "_pre"] = conv_taps(inp, P[name + "/kernel"], P[name + "/bias"])
        t[key + "_pre"].retain_grad() if t[key + "_pre"].requires_grad else None
        t[key] = torch.relu(t[key + "_pre"])
        return t[key]

    b1 = cr(x, "branch1_conv_1x1", "b1")
    if commuted:
        t["p2"] = conv_taps(x, P["branch2_conv_1x1/kernel"], P["branch2_conv_1x1/bias"])
        t["p2"].retain_grad() if t["p2"].requires_grad else None
        t["b2_pre"] = avg_pool_ref(t["p2"])
        t["b2_pre"].retain_grad() if t["b2_pre"].requires_grad else None
        b2 = t["b2"] = torch.relu(t["b2_pre"])
    else:
        t["avg"] = avg_pool_ref(x)
        b2 = cr(t["avg"], "branch2_conv_1x1", "b2")
    b3 = cr(x, "branch3_conv_1x1", "b3")
    b3a, b3b = cr(b3, "branch3_conv_3x1", "b3a"), cr(b3, "branch3_conv_1x3", "b3b")
    b4 = cr(x, "branch4_conv_1x1", "b4")
    b43 = cr(b4, "branch4_conv_3x3", "b43")
    b4a, b4b = cr(b43, "branch4_conv_1x3", "b4a"), cr(b43, "branch4_conv_3x1", "b4b")
    t["hyper"] = torch.cat([b1, b2, b3a, b3b, b4a, b4b], dim=-1)
    r = cr(t["hyper"], "residual_conv", "res")
    t["out"] = r + x
    return t["out"], t


RELUS = ("b1", "b2", "b3", "b3a", "b3b", "b4", "b43", "b4a", "b4b", "res")


@functools.lru_cache(maxsize=4)
def block_reference(case, commuted=False):
    """The reference of one BLOCK_CASES entry: (inputs, dict of out, dx, the 20 variable gradients and every intermediate with its gradient)."""
    cid, nhwc, seed, products, px, pdy = case
    inp = block_inputs(nhwc, seed, products, px, pdy)
    x = inp["x"].clone().requires_grad_(True)
    P = {n: v.clone().requires_grad_(True) for n, v in inp["P"].items()}
    out, t = block_ref(x, P, commuted)
    out.backward(inp["dy"])
    return inp, dict(out=out.detach(), dx=x.grad, grads={n: v.grad for n, v in P.items()}, t=t)


def holds16(v):
    """every element survives a round trip through bf16 and through IEEE half"""
    v = v.detach()
    return bool(torch.equal(v.to(torch.bfloat16).to(F64), v)) and bool(torch.equal(v.to(torch.float16).to(F64), v))


def check_block_case(case):
    """The conditions of an exact block case, on the reference alone; returns figures for the log."""
    (inp, ref), (_, com) = block_reference(case, False), block_reference(case, True)
    x, dy, t, tc = inp["x"], inp["dy"], ref["t"], com["t"]
    # the two orders of branch 2 are the same function, exactly (every quarter and half is dyadic)
    assert torch.equal(ref["out"], com["out"]) and torch.equal(ref["dx"], com["dx"]) and all(torch.equal(ref["grads"][n], com["grads"][n]) for n in ref["grads"])
    # ---- every tensor either route stores in 16 bits: forward ...
    stored = {"x": x, "avg(x)": t["avg"], "p2 = conv(x) before the pool": tc["p2"], "T[b3 | b4]": torch.cat([t["b3"], t["b4"]], -1), "hyper": t["hyper"], "U": t["b43"],
              "r": t["res"], "out": t["out"], "dy": dy}
    # ... and backward: gr = dy (r > 0); d hyper, dU, dT with their ReLU masks applied = the gradients of the pre-activations; dT[128:192] = the
    # pool's backward; x's buffer after each of its three deliveries (skip path, the fused 1x1's data gradient, branch 1's)
    g = {k: t[k + "_pre"].grad for k in RELUS}
    stored.update({"gr": g["res"], "d hyper": torch.cat([g["b1"], g["b2"], g["b3a"], g["b3b"], g["b4a"], g["b4b"]], -1), "dU": g["b43"],
                   "dT": torch.cat([g["b3"], g["b4"], tc["p2"].grad], -1)})
    dx_b1 = dgrad_ref(g["b1"], inp["P"]["branch1_conv_1x1/kernel"], x.shape[1], x.shape[2])
    stored.update({"xbuf after the skip path": dy, "xbuf after the fused 1x1": ref["dx"] - dx_b1, "xbuf = dx": ref["dx"]})
    for name, v in stored.items():
        assert holds16(v), (name, "does not survive 16 bits", v.abs().max().item())
        assert torch.equal(v * 4, (v * 4).round()), name
    # ---- every fp32 sum below 2^24 in units of its terms (quarters): the sum of the magnitudes of a convolution's terms, forward and weight gradient
    worst = 0.0
    for (name, kh, kw, _, _), key, src in zip(BLOCK_LAYERS, ("b1", "b2", "b3", "b3a", "b3b", "b4", "b43", "b4a", "b4b", "res"),
                                              (x, t["avg"], x, t["b3"], t["b3"], x, t["b4"], t["b43"], t["b43"], t["hyper"])):
        w, b = inp["P"][name + "/kernel"], inp["P"][name + "/bias"]
        fwd = conv_ref(src.detach().abs(), w.abs(), b.abs()).max().item()
        dw, db = wgrad_ref(src.detach().abs(), g[key].abs(), kh, kw)
        dxs = dgrad_ref(g[key].abs(), w.abs(), x.shape[1], x.shape[2]).max().item()
        worst = max(worst, fwd, dw.max().item(), db.max().item(), dxs)
    assert worst * 4 < 2 ** 24, worst
    # ---- the case cannot go trivial
    for k in RELUS:
        assert int((t[k] != 0).sum()) >= 1, (k, "is all zero")
        assert int((t[k + "_pre"] <= 0).sum()) >= 1 and int((t[k + "_pre"] > 0).sum()) >= 1, (k, "ReLU without zeros or without positives")
    assert all(int((v != 0).sum()) >= 1 for v in ref["grads"].values()) and len(ref["grads"]) == 20 and int((ref["dx"] != dy).sum()) >= 1
    return dict(max16=max(v.abs().max().item() for v in stored.values()), worst_sum=worst, dx_nonzero=int((ref["dx"] != 0).sum()),
                grad_nonzero={n: int((v != 0).sum()) for n, v in ref["grads"].items()})


def dispatch_rows():
    """The 30 rows of tests/test_conv_dispatch_gpu.CASES as (id, shape8, call, family)."""
    import test_conv_dispatch_gpu as D
    return [(name, S(*shp[:5], shp[5], shp[6]), call, family) for name, shp, call, family in D.CASES]


def all_cases():
    """Every exact case as (id, kind, shape, family, extra): kind in fwd / pool / dgrad / wgrad / fold; extra is a dict."""
    out = []
    for name, shp, call, family in dispatch_rows():
        kind = {"fwd": "fwd", "fwd_pool": "pool", "fwd_pool_bits": "pool", "dgrad": "dgrad", "dgrad_mask": "dgrad", "dgrad_bits": "dgrad", "wgrad": "wgrad"}[call]
        out.append(("row_" + name, kind, shp, family, dict(row=call)))
    out += [("fwd_" + n, "fwd", s, f, dict(edge=e)) for n, s, f, e in FWD_EDGES]
    out += [("dgrad_" + n, "dgrad", s, f, dict(edge=e)) for n, s, f, e in DGRAD_EDGES]
    out += [("wgrad_" + n, "wgrad", s, f, dict(edge=e, cin_real=c)) for n, s, f, c, e in WGRAD_EDGES]
    out += [("pool_" + n, "pool", s, f, dict(edge="")) for n, s, f in POOL_EDGES]
    out += [("fold_%dx%dx%d" % nhw, "fold", S(*nhw, 64, 64), "conv3x3_c64_kernel<true, true>", dict(edge="")) for nhw in FOLD_SHAPES]
    out += [(n, k, s, f, dict(edge=e, cin_real=c, valid=True)) for n, k, s, f, c, e in VALID_CASES]
    for n, s, v, ff, fe, df, de, wf in RESNET_CASES:
        out += [("fwd_" + n, "fwd", s, ff, dict(edge=fe, valid=v)), ("dgrad_" + n, "dgrad", s, df, dict(edge=de, valid=v)),
                ("wgrad_" + n, "wgrad", s, wf, dict(edge="", valid=v))]
    out += [("vfwd_" + n, "vfwd", s, f, dict(edge=e, geom=g, inside=i)) for n, s, f, g, i, e in VFWD_CASES]
    out += [("vdgrad_" + n, "vdgrad", s, f, dict(edge=e, geom=g)) for n, s, f, g, e in VDGRAD_CASES]
    out += [("vwgrad_" + n, "vwgrad", s, f, dict(edge=e, geom=g)) for n, s, f, g, e in VWGRAD_CASES]
    out += [("concat2_" + c[0], "concat2", concat2_shape(c), c[6], dict(edge="", c1=c[2], pitch=c[5])) for c in CONCAT2_CASES]
    return out


def check_case_inputs(case, cus=256):
    """The conditions of one case on its reference and on the restated plans (no GPU); returns the figures for the log."""
    cid, kind, shp, family, extra = case
    edge, row, valid = extra.get("edge", ""), extra.get("row"), bool(extra.get("valid"))
    if kind in VIEW_CHECKS:
        return VIEW_CHECKS[kind](case, cus)
    if kind == "fwd":
        inp = forward_inputs(shp, cin_real=extra.get("cin_real"), valid=valid)
        check_forward_inputs(inp, relu=True)
        if edge == "splitk":
            assert plan_splitk(shp, 0, cus, valid)[0] >= 2, "the case is there for a split K"
        return dict(max=inp["pre"].abs().max().item(), zeros=int((inp["pre"] == 0).sum()))
    if kind == "pool":
        inp = forward_inputs(shp)
        check_forward_inputs(inp, relu=True, pool=True)
        return dict(max=inp["pre"].abs().max().item(), zeros=int((inp["pre"] == 0).sum()), late_ties=late_ties(torch.relu(inp["pre"])))
    if kind == "dgrad":
        inp = dgrad_inputs(shp, valid=valid)
        check_dgrad_inputs(inp)
        if edge == "splitk":
            assert plan_splitk(shp, 1, cus, valid)[0] >= 2, "the case is there for a split K"
        unreached = check_dgrad_unreached(inp, shp)
        return dict(max=inp["dx"].abs().max().item(), **({} if unreached is None else dict(unreached=unreached)))
    if kind == "wgrad":
        inp = wgrad_inputs(shp, cin_real=extra.get("cin_real"), valid=valid)
        check_wgrad_inputs(inp)
        check_wgrad_cuts(shp, edge, cus)
        return dict(max=inp["dw"].abs().max().item())
    inp = fold_inputs(shp[:3])
    check_fold_inputs(inp)
    return dict(max=inp["dx"].abs().max().item())


# ================================================================================================================ runners (GPU)
def assert_equal(got, want, what):
    """torch.equal on values (-0.0 == 0.0); on failure the count of differing elements and the first few (index, got, want)."""
    got = got.detach().cpu()
    got = got.to(F64) if got.is_floating_point() else got
    want = want.to(got.dtype).reshape(got.shape)
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    first = [(tuple(i.tolist()), got[tuple(i)].item(), want[tuple(i)].item()) for i in bad[:6]]
    raise AssertionError("%s: %d of %d elements differ, first (index, got, want): %s" % (what, bad.shape[0], got.numel(), first))


# Variants of a case's call that the family's select() does not take, and the kernel that runs them instead (a label prefix).  The words name
# the variant: scratch (the call brings the split-K scratch the shape asks for), f32 (fp32 output), residual, plain (a data gradient with no
# mask and no accumulation), acc.  The first entry whose words all describe the call holds; a call that no entry describes stays in the family.
#   scratch: a map this small prefers to split K (select_conv asks prefer_splitk before the halo and streaming families);
#   f32 / residual: the first-layer and the streaming kernel take neither, the thin head no residual, the 64 -> 64 kernel no fp32 output (the
#   halo kernel takes that one); plain / acc: the streaming kernel's other instance, without / with the loads of the epilogue inputs.
_SPLITS = (("scratch", FLAT),)
_NO_F32_RES = (("f32", FLAT), ("residual", FLAT))
MOVED = {
    "fwd_halo8x32_ragged_edges": _SPLITS,
    "fwd_head8": _SPLITS + (("residual", FLAT),),
    "fwd_head6": _SPLITS,
    "fwd_ragged_cin136_cout200": _SPLITS,
    "fwd_ragged_cin72": _SPLITS,
    "fwd_c64_ragged_edges": (("scratch f32", FLAT), ("f32", HALO)),
    "fwd_first_layer_one_column": _NO_F32_RES,
    "fwd_first_layer_ragged": _NO_F32_RES,
    "fwd_pointwise_k2304": _SPLITS + _NO_F32_RES,
    "fwd_taps_3x1": _NO_F32_RES,
    "fwd_taps_1x3": _NO_F32_RES,
    "fwd_taps_stride2": _SPLITS + _NO_F32_RES,
    "fwd_taps_192_320": _SPLITS + _NO_F32_RES,
    "dgrad_halo8x32_ragged_edges": _SPLITS,
    "dgrad_ragged_cin136_cout200": _SPLITS,
    "dgrad_ragged_cin72": _SPLITS,
    "dgrad_pointwise_k2304": (("plain", PW),),
    "dgrad_taps_192_320": _SPLITS + (("plain", PW),),
    "dgrad_pw256_3x3": _SPLITS,
    "row_pointwise_dgrad": (("acc", PW),),
    "fwd_pw_s2_taps": _NO_F32_RES,                                    # (no split: K = 256 is four K tiles; every other ResNet row is flat-M in every variant)
    "fold_1x30x62": (("unfolded", "conv3x3_c64_kernel<true>"),),      # the same kernel without the folded gradient
    "fold_3x40x96": (("unfolded", "conv3x3_c64_kernel<true>"),),
}


def moved_to(cid, variant):
    have = variant.split()
    for words, kernel in MOVED.get(cid, ()):
        if all(w in have for w in words.split()):
            return kernel
    return None


class _Api:
    def __init__(self, dev):
        from dan_amd import _lib, ops
        from test_conv_dispatch_gpu import in_family
        self.dev, self.L, self.ops, self.lib = dev, _lib.lib(), ops, _lib
        self.ptr, self.act, self.in_family = _lib.ptr, _lib.ACT_DTYPE, in_family
        self.cus = torch.cuda.get_device_properties(dev).multi_processor_count

    def stream(self):
        return self.lib.stream()

    def desc(self, shp, valid=False):
        return self.ops._desc(*shp, valid=valid)

    def a16(self, t):
        return t.to(self.act).to(self.dev)

    def f32(self, t):
        return t.to(torch.float32).to(self.dev)

    def scratch(self, n):
        return (torch.full((n,), 0x7f, dtype=torch.uint8, device=self.dev), n) if n else (None, 0)

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError("danhip call failed (%d): %s" % (rc, self.L.danhip_last_error().decode()))
        torch.cuda.synchronize()

    def launched(self, cid, call, family, want=None, variant=""):
        """After EVERY call: the launched instance is in the family the case is listed for - or, for a variant of the call that MOVED lists, an
        instance of the kernel named there; want: the label function's answer, where it describes this call."""
        got = self.L.danhip_conv_last_launch_label().decode()
        if want is not None:
            assert got == want, (cid, call, got, want)
        moved = moved_to(cid, variant)
        if moved is not None:
            assert got.startswith(moved), "%s %s: launched %s, this variant belongs to %s" % (cid, call, got, moved)
        else:
            assert self.in_family(got, family), "%s %s: launched %s, the case is there for %s" % (cid, call, got, family)
        return got

    def label(self, d, which):
        return self.L.danhip_conv_kernel_label(ctypes.byref(d), which).decode()


def run_fwd(api, cid, shp, family, extra):
    N, H, W, Cin, Cout, kh, kw, s = shp
    valid = bool(extra.get("valid"))
    inp = forward_inputs(shp, cin_real=extra.get("cin_real"), valid=valid)
    check_forward_inputs(inp, relu=True)
    d, L, ptr = api.desc(shp, valid), api.L, api.ptr
    dp = ctypes.byref(d)
    x, w, b, res = api.a16(inp["x"]), api.f32(inp["w"]), api.f32(inp["b"]), api.a16(inp["res"])
    wf, _ = api.ops.pack_conv_weight(d, w, need_bwd=False)
    nws = L.danhip_conv2d_workspace_bytes(dp, 0)
    assert nws == conv_workspace_bytes(shp, 0, api.cus, valid)
    ws, nws = api.scratch(nws)
    row, edge = extra.get("row"), extra.get("edge", "")

    def call(use_ws, f32out, relu, residual):
        y = torch.full((N, d.Ho, d.Wo, Cout), float("nan"), dtype=torch.float32 if f32out else api.act, device=api.dev)
        api.ok(L.danhip_conv2d_fwd_ws(dp, ptr(x), ptr(wf), ptr(b), ptr(y), api.lib.F32 if f32out else api.lib.BF16, int(relu), ptr(res) if residual else None,
                                      ptr(ws) if use_ws else None, nws if use_ws else 0, api.stream()))
        return y

    def bits_call():                                      # the same conv_relu through the entry point that also writes the ReLU bit mask of y
        y = torch.full((N, d.Ho, d.Wo, Cout), float("nan"), dtype=api.act, device=api.dev)
        yb = torch.full((N * d.Ho * d.Wo, Cout // 8), 0xA5, dtype=torch.uint8, device=api.dev)
        api.ok(L.danhip_conv2d_fwd_relu_bits_arg(dp, ptr(x), ptr(wf), ptr(b), ptr(y), ptr(yb), None, None, None, api.stream()))
        api.launched(cid, "bits", family)
        assert_equal(y, forward_outputs(inp, True, False), cid + " bits: y")
        assert_equal(yb, relu_bits(forward_outputs(inp, True, False)), cid + " bits: mask of y")

    if row:                                               # the dispatch table's call: with the scratch the library asks for, bias, ReLU, 16-bit
        y = call(True, False, True, False)
        api.launched(cid, "row", family, want=api.label(d, 0))
        assert_equal(y, forward_outputs(inp, True, False), cid)
        if Cout % 8 == 0 and L.danhip_conv2d_fwd_emits_bits(dp, 0):
            bits_call()
        return
    if edge == "splitk":
        assert nws and plan_splitk(shp, 0, api.cus, valid)[0] >= 2
    outs = [False, True] if edge != "f32only" else [True]
    for use_ws in ([False, True] if nws else [False]):
        for f32out in outs:
            for relu, residual in ((False, False), (True, False)) + (((True, True),) if not f32out else ()):
                y = call(use_ws, f32out, relu, residual)
                what = "ws=%d f32=%d relu=%d residual=%d" % (use_ws, f32out, relu, residual)
                # the label function describes the call with bias, without residual, in the output type the case is there for
                described = not residual and f32out == (edge == "f32only")
                want = api.label(d, 0 if use_ws else 16) if described else None
                variant = " ".join(w for w, on in (("scratch", use_ws), ("f32", f32out), ("residual", residual)) if on)
                api.launched(cid, what, family, want=want, variant=variant)
                assert_equal(y, forward_outputs(inp, relu, residual), cid + " " + what)
    if Cout % 8 == 0 and L.danhip_conv2d_fwd_emits_bits(dp, 0):
        bits_call()


def run_dgrad(api, cid, shp, family, extra):
    N, H, W, Cin, Cout, kh, kw, s = shp
    valid = bool(extra.get("valid"))
    inp = dgrad_inputs(shp, valid=valid)
    check_dgrad_inputs(inp)
    check_dgrad_unreached(inp, shp)
    d, L, ptr = api.desc(shp, valid), api.L, api.ptr
    dp = ctypes.byref(d)
    dy, mask, old = api.a16(inp["dy"]), api.a16(inp["mask"]), api.a16(inp["old"])
    _, wb = api.ops.pack_conv_weight(d, api.f32(inp["w"]), need_bwd=True)
    nws = L.danhip_conv2d_workspace_bytes(dp, 1)
    assert nws == conv_workspace_bytes(shp, 1, api.cus, valid)
    ws, nws = api.scratch(nws)
    takes_bits = bool(L.danhip_conv2d_bwd_data_takes_bits(dp))
    bits = relu_bits(inp["mask"]).to(api.dev) if takes_bits else None
    row, edge = extra.get("row"), extra.get("edge", "")

    def call(form, use_ws, acc):
        dx = old.clone()
        if form == "bits":
            api.ok(L.danhip_conv2d_bwd_data_bits(dp, ptr(dy), ptr(wb), ptr(bits), ptr(dx), acc, api.stream()))
        else:
            api.ok(L.danhip_conv2d_bwd_data_ws(dp, ptr(dy), ptr(wb), ptr(mask) if form == "mask" else None, ptr(dx), acc, ptr(ws) if use_ws else None,
                                               nws if use_ws else 0, api.stream()))
        return dx

    if row:
        form = {"dgrad": "none", "dgrad_mask": "mask", "dgrad_bits": "bits"}[row]
        assert form != "bits" or takes_bits
        for acc in (0, 1):
            dx = call(form, True, acc)
            # (accumulation alone is an epilogue input too: the plain label describes acc = 0)
            described = form != "none" or not acc
            want = api.label(d, 5 if form != "none" else 1) if described else None
            api.launched(cid, "row acc=%d" % acc, family, want=want, variant="acc" if acc else "")
            assert_equal(dx, dgrad_outputs(inp, form != "none", acc), "%s acc=%d" % (cid, acc))
        return
    if edge == "splitk":
        assert nws and plan_splitk(shp, 1, api.cus, valid)[0] >= 2
    if edge == "pw256":
        assert L.danhip_set_option(b"pw_dgrad_ld_bn", 256) == 0
    try:
        for form in ["none", "mask"] + (["bits"] if takes_bits else []):
            for use_ws in ([False, True] if nws and form != "bits" else [False]):
                for acc in (0, 1):
                    if edge == "pw256" and form == "none" and not acc:
                        continue                              # (no epilogue input: the option does not apply)
                    dx = call(form, use_ws, acc)
                    what = "form=%s ws=%d acc=%d" % (form, use_ws, acc)
                    want = None
                    if form == "bits":
                        want = api.label(d, 5 | 16)
                    elif edge != "pw256" and (form == "mask" or not acc):      # (the option is not part of the label function's call)
                        want = api.label(d, (5 if form == "mask" else 1) | (0 if use_ws else 16))
                    variant = " ".join(w for w, on in (("scratch", use_ws), ("plain", form == "none" and not acc), ("acc", acc)) if on)
                    api.launched(cid, what, family, want=want, variant=variant)
                    assert_equal(dx, dgrad_outputs(inp, form != "none", acc), cid + " " + what)
    finally:
        if edge == "pw256":
            L.danhip_set_option(b"pw_dgrad_ld_bn", 128)


def run_wgrad(api, cid, shp, family, extra):
    N, H, W, Cin, Cout, kh, kw, s = shp
    valid = bool(extra.get("valid"))
    inp = wgrad_inputs(shp, cin_real=extra.get("cin_real"), valid=valid)
    check_wgrad_inputs(inp)
    cr = inp["cin_real"]
    d, L, ptr = api.desc(shp, valid), api.L, api.ptr
    dp = ctypes.byref(d)
    x, dy = api.a16(inp["x"]), api.a16(inp["dy"])
    nws = L.danhip_conv2d_bwd_weight_workspace_bytes(dp)
    assert nws == wgrad_workspace_bytes(shp, api.cus)
    edge = extra.get("edge", "")
    check_wgrad_cuts(shp, edge, api.cus)
    ws, nws = api.scratch(nws)
    want = L.danhip_conv_wgrad_kernel_label(dp).decode()
    for form in ("atomic", "ws"):
        dw, db = api.f32(inp["dw0"]), api.f32(inp["db0"])
        if form == "atomic":
            api.ok(L.danhip_conv2d_bwd_weight(dp, ptr(x), ptr(dy), ptr(dw), ptr(db), cr, api.stream()))
        else:
            api.ok(L.danhip_conv2d_bwd_weight_ws(dp, ptr(x), ptr(dy), ptr(dw), ptr(db), cr, ptr(ws), nws, api.stream()))
        api.launched(cid, form, family, want=want)
        assert_equal(dw, inp["dw"], "%s %s dw" % (cid, form))
        assert_equal(db, inp["db"], "%s %s db" % (cid, form))


def run_pool(api, cid, shp, family, extra):
    N, H, W, Cin, Cout, kh, kw, s = shp
    inp = forward_inputs(shp)
    check_forward_inputs(inp, relu=True, pool=True)
    d, L, ptr = api.desc(shp), api.L, api.ptr
    dp = ctypes.byref(d)
    x, b = api.a16(inp["x"]), api.f32(inp["b"])
    wf, _ = api.ops.pack_conv_weight(d, api.f32(inp["w"]), need_bwd=False)
    y_ref = torch.relu(inp["pre"])
    p_ref, code = pool_ref(y_ref)
    Hp, Wp = (d.Ho + 1) // 2, (d.Wo + 1) // 2
    want = api.label(d, 4)

    def outs():
        u8 = lambda *dims: torch.full(dims, 0xA5, dtype=torch.uint8, device=api.dev)
        return (torch.full((N, d.Ho, d.Wo, Cout), float("nan"), dtype=api.act, device=api.dev), torch.full((N, Hp, Wp, Cout), float("nan"), dtype=api.act, device=api.dev),
                u8(N * Hp * Wp, max(Cout // 4, 1)), u8(N * d.Ho * d.Wo, max(Cout // 8, 1)), u8(N * Hp * Wp, max(Cout // 8, 1)))

    row = extra.get("row")
    if row != "fwd_pool_bits":
        assert L.danhip_conv2d_workspace_bytes(dp, 0) == 0 or not row      # (ops pools after danhip_conv2d_fwd_ws where the shape wants scratch)
        y, p, arg, _, _ = outs()
        api.ok(L.danhip_conv2d_fwd_pool_arg(dp, ptr(x), ptr(wf), ptr(b), ptr(y), ptr(p), ptr(arg), api.stream()))
        api.launched(cid, "pool", family, want=want)
        assert_equal(y, y_ref, cid + " y")
        assert_equal(p, p_ref, cid + " pooled")
        if Cout % 4 == 0:
            assert_equal(arg, pack_codes(code), cid + " arg-max codes")
        if L.danhip_conv2d_fwd_pool_only(dp):
            _, p2, arg2, _, _ = outs()
            api.ok(L.danhip_conv2d_fwd_pool_arg(dp, ptr(x), ptr(wf), ptr(b), None, ptr(p2), ptr(arg2), api.stream()))
            api.launched(cid, "pool-only", family)
            assert_equal(p2, p_ref, cid + " pool-only pooled")
            assert_equal(arg2, pack_codes(code), cid + " pool-only codes")
    else:
        arg = None
    if L.danhip_conv2d_fwd_emits_bits(dp, 1):
        y, p, arg, yb, pb = outs()
        api.ok(L.danhip_conv2d_fwd_relu_bits_arg(dp, ptr(x), ptr(wf), ptr(b), ptr(y), ptr(yb), ptr(p), ptr(pb), ptr(arg), api.stream()))
        api.launched(cid, "bits", family)
        assert_equal(y, y_ref, cid + " bits: y")
        assert_equal(p, p_ref, cid + " bits: pooled")
        assert_equal(arg, pack_codes(code), cid + " bits: arg-max codes")
        assert_equal(yb, relu_bits(y_ref), cid + " bits: mask of y")
        assert_equal(pb, relu_bits(p_ref), cid + " bits: mask of the pooled map")
        if L.danhip_conv2d_fwd_pool_only(dp):                 # training's conv1_2 / conv2_2: y == NULL, the lean epilogue stores everything but y
            _, p2, arg2, yb2, pb2 = outs()
            api.ok(L.danhip_conv2d_fwd_relu_bits_arg(dp, ptr(x), ptr(wf), ptr(b), None, ptr(yb2), ptr(p2), ptr(pb2), ptr(arg2), api.stream()))
            api.launched(cid, "bits pool-only", family)
            assert_equal(p2, p_ref, cid + " bits pool-only: pooled")
            assert_equal(arg2, pack_codes(code), cid + " bits pool-only: arg-max codes")
            assert_equal(yb2, relu_bits(y_ref), cid + " bits pool-only: mask of y")
            assert_equal(pb2, relu_bits(p_ref), cid + " bits pool-only: mask of the pooled map")
    else:
        assert row != "fwd_pool_bits"
    if arg is not None and Cout % 8 == 0:                     # one step further: the pool's backward through the codes the call wrote
        g = gen(7)
        dyp, old = small((N, Hp, Wp, Cout), g), small((N, d.Ho, d.Wo, Cout), g)
        for acc in (0, 1):
            dx = api.a16(old)
            dyd = api.a16(dyp)
            api.ok(L.danhip_maxpool2x2_bwd_arg(ptr(arg), ptr(dyd), ptr(dx), N, d.Ho, d.Wo, Cout, acc, api.stream()))
            assert_equal(dx, pool_scatter(code, dyp, d.Ho, d.Wo) + (old if acc else 0), "%s scatter acc=%d" % (cid, acc))


def run_fold(api, cid, shp, family, extra):
    N, H, W = shp[:3]
    inp = fold_inputs((N, H, W))
    check_fold_inputs(inp)                                    # exact only while |dX| <= 256 survives the 16-bit tile in LDS
    d, L, ptr = api.desc(shp), api.L, api.ptr
    dp = ctypes.byref(d)
    assert L.danhip_conv2d_bwd_data_first_supported(dp) == 1
    dy, x8 = api.a16(inp["dy"]), api.a16(inp["x8"])
    bits = relu_bits(inp["y1"]).to(api.dev)
    _, wb = api.ops.pack_conv_weight(d, api.f32(inp["w2"]), need_bwd=True)
    dw, db = api.f32(inp["dw0"]), api.f32(inp["db0"])
    api.ok(L.danhip_conv2d_bwd_data_bits_first(dp, ptr(dy), ptr(wb), ptr(bits), ptr(x8), 3, ptr(dw), ptr(db), api.stream()))
    api.launched(cid, "folded", family)
    assert_equal(dw, inp["dw"], cid + " dw8")
    assert_equal(db, inp["db"], cid + " db8")
    dx = torch.full((N, H, W, 64), float("nan"), dtype=api.act, device=api.dev)
    api.ok(L.danhip_conv2d_bwd_data_bits(dp, ptr(dy), ptr(wb), ptr(bits), ptr(dx), 0, api.stream()))
    api.launched(cid, "unfolded", family, variant="unfolded")
    assert_equal(dx, inp["dx"], cid + " dx of the unfolded call")


# ---- channel-slice views
def view_buffer(api, dims, width, c0, t=None):
    """[N,H,W,width] of NAN16 with t (float64 [N,H,W,C], or nothing) in channels c0 : c0 + C -> (buffer, the slice as a view)."""
    N, H, W, C = dims
    buf = torch.full((N, H, W, width), NAN16, dtype=torch.int16, device=api.dev).view(api.act)
    if t is not None:
        buf[..., c0:c0 + C] = api.a16(t)
    return buf, buf[..., c0:c0 + C]


def assert_background(buf, c0, C, what):
    raw = buf.view(torch.int16)
    changed = int((raw[..., :c0] != NAN16).sum()) + int((raw[..., c0 + C:] != NAN16).sum())
    assert changed == 0, "%s: %d elements outside the written slice changed" % (what, changed)


def run_vfwd(api, cid, shp, family, extra):
    N, H, W, Cin, Cout, kh, kw, s = shp
    edge, inside = extra["edge"], extra["inside"]
    inp = view_forward_inputs(shp, "plus" in edge)
    check_forward_inputs(inp, relu=True)
    d, L, ptr, vptr = api.desc(shp), api.L, api.ptr, api.ops._vptr
    dp = ctypes.byref(d)
    xw, xc, yw, yc = extra["geom"]
    xbuf, xv = view_buffer(api, (N, H, W, Cin), xw, xc, inp["x"])
    wf, _ = api.ops.pack_conv_weight(d, api.f32(inp["w"]), need_bwd=False)
    b = api.f32(inp["b"])
    nws = L.danhip_conv2d_workspace_bytes(dp, 0)
    assert nws == conv_workspace_bytes(shp, 0, api.cus)
    if "splitk" in edge:
        assert nws and plan_splitk(shp, 0, api.cus)[0] >= 2
    ws, nws = api.scratch(nws)
    pitch = api.lib.ConvPitch(xw, yw, 0)
    for use_ws in ([False, True] if nws else [False]):
        for relu, relu_ch in ((1, Cout), (1, inside), (1, 0), (0, Cout)):
            ybuf, yv = view_buffer(api, (N, H, W, Cout), yw, yc)
            api.ok(L.danhip_conv2d_fwd_strided(dp, vptr(xv), ptr(wf), ptr(b), vptr(yv), relu, relu_ch, ctypes.byref(pitch), ptr(ws) if use_ws else None,
                                               nws if use_ws else 0, api.stream()))
            relu_co = relu_ch if relu else 0
            what = "%s ws=%d relu=%d relu_channels=%d" % (cid, use_ws, relu, relu_ch)
            want = view_kernel(shp, 0, api.cus, scratch=use_ws, partial=0 < relu_co < Cout)
            if use_ws == bool(nws) and (0 < relu_co < Cout) == ("partial" in edge):
                assert want == family, (what, want, family)       # the call the table lists
            api.launched(cid, what, want, want=want)
            assert_equal(yv, view_forward_outputs(inp, relu_co), what)
            assert_background(ybuf, yc, Cout, what)


def run_vdgrad(api, cid, shp, family, extra):
    N, H, W, Cin, Cout, kh, kw, s = shp
    edge = extra["edge"]
    inp = view_dgrad_inputs(shp, "plus" in edge)
    check_dgrad_inputs(inp)
    d, L, ptr, vptr = api.desc(shp), api.L, api.ptr, api.ops._vptr
    dp = ctypes.byref(d)
    co8 = co8_of(Cout)
    yw, yc, xw, xc, mw, mc = extra["geom"]
    dybuf, dyv = view_buffer(api, (N, H, W, co8), yw, yc, inp["dy"])
    mbuf, mv = view_buffer(api, (N, H, W, Cin), mw, mc, inp["mask"])
    mdense = api.a16(inp["mask"])
    _, wb = api.ops.pack_conv_weight(d, api.f32(inp["w"]), need_bwd=True)
    nws = L.danhip_conv2d_workspace_bytes(dp, 1)
    assert nws == conv_workspace_bytes(shp, 1, api.cus)
    if "splitk" in edge:
        assert nws and plan_splitk(shp, 1, api.cus)[0] >= 2
    ws, nws = api.scratch(nws)
    for form in ("none", "view", "dense"):                   # no mask / the mask a slice of a third buffer (aux_pitch) / a dense mask (aux_pitch = 0)
        pitch = api.lib.ConvPitch(yw, xw, mw if form == "view" else 0)
        m = None if form == "none" else vptr(mv) if form == "view" else ptr(mdense)
        for use_ws in ([False, True] if nws else [False]):
            for acc in (0, 1):
                dxbuf, dxv = view_buffer(api, (N, H, W, Cin), xw, xc, inp["old"])
                api.ok(L.danhip_conv2d_bwd_data_strided(dp, vptr(dyv), ptr(wb), m, vptr(dxv), acc, ctypes.byref(pitch), ptr(ws) if use_ws else None,
                                                        nws if use_ws else 0, api.stream()))
                what = "%s mask=%s ws=%d acc=%d" % (cid, form, use_ws, acc)
                want = view_kernel(shp, 1, api.cus, scratch=use_ws, ld=form != "none" or bool(acc))
                if use_ws == bool(nws) and form != "none" and acc:
                    assert want == family, (what, want, family)   # the call the table lists
                api.launched(cid, what, want, want=want)
                assert_equal(dxv, dgrad_outputs(inp, form != "none", acc), what)
                assert_background(dxbuf, xc, Cin, what)


def run_vwgrad(api, cid, shp, family, extra):
    N, H, W, Cin, Cout, kh, kw, s = shp
    edge = extra["edge"]
    inp = wgrad_inputs(shp)
    check_wgrad_inputs(inp)
    d, L, ptr, vptr = api.desc(shp), api.L, api.ptr, api.ops._vptr
    dp = ctypes.byref(d)
    xw, xc, yw, yc = extra["geom"]
    xbuf, xv = view_buffer(api, (N, H, W, Cin), xw, xc, inp["x"])
    dybuf, dyv = view_buffer(api, (N, H, W, co8_of(Cout)), yw, yc, inp["dy"])
    pitch = api.lib.ConvPitch(xw, yw, 0)

    def call(ws, nws):
        dw, db = api.f32(inp["dw0"]), api.f32(inp["db0"])
        rc = L.danhip_conv2d_bwd_weight_strided(dp, vptr(xv), vptr(dyv), ptr(dw), ptr(db), Cin, ctypes.byref(pitch), ptr(ws) if nws else None, nws, api.stream())
        return rc, dw, db

    def exact(rc, dw, db, what):
        api.ok(rc)
        got = api.launched(cid, what, family)
        assert_equal(dw, inp["dw"], "%s %s dw" % (cid, what))
        assert_equal(db, inp["db"], "%s %s db" % (cid, what))
        return got

    assert L.danhip_get_option(b"deterministic") == 0
    nws = L.danhip_conv2d_bwd_weight_workspace_bytes(dp)      # (the query answers for dense pitches)
    assert nws == wgrad_workspace_bytes(shp, api.cus)
    ws, nws = api.scratch(nws)
    dense = L.danhip_conv_wgrad_kernel_label(dp).decode()
    for form in ("atomic", "ws"):
        got = exact(*call(ws, nws if form == "ws" else 0), form)
        if edge == "pitch":                                  # the row-streaming kernel declines: the generic tiles take the call
            assert dense.startswith("conv_wgrad_rows_kernel<") and got.startswith("conv_wgrad_kernel<"), (dense, got)
        else:
            assert got == dense, (got, dense)
    if edge not in ("det", "pitch"):
        return
    assert L.danhip_set_option(b"deterministic", 1) == 0
    try:
        nws = L.danhip_conv2d_bwd_weight_workspace_bytes(dp)
        assert nws > 0
        ws, nws = api.scratch(nws)
        if edge == "pitch":                                  # danhip.h: the query cannot answer for this call's family -> DANHIP_EINVAL, nothing launched
            rc, dw, db = call(ws, nws)
            assert rc == -1, rc
            torch.cuda.synchronize()
            assert_equal(dw, inp["dw0"], cid + " refused call: dw untouched")
            return
        runs = []
        for i in range(2):
            rc, dw, db = call(ws, nws)
            exact(rc, dw, db, "deterministic run %d" % i)
            runs.append((dw, db))
        assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)) and torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
    finally:
        L.danhip_set_option(b"deterministic", 0)


def run_concat2(api, cid, shp, family, extra):
    N, H, W, Cin, Cout, kh, kw, s = shp
    c1, pitch = extra["c1"], extra["pitch"]
    c2 = Cin - c1
    inp = forward_inputs(shp)
    check_forward_inputs(inp, relu=True)
    d, L, ptr, vptr = api.desc(shp), api.L, api.ptr, api.ops._vptr
    dp = ctypes.byref(d)
    assert L.danhip_conv2d_fwd_concat2_supported(dp, c1, pitch) == 1
    # two separate buffers `pitch` wide: the first source in channels 0 : c1, the second right-aligned in pitch - c2 : pitch
    abuf, av = view_buffer(api, (N, H, W, c1), pitch, 0, inp["x"][..., :c1])
    fbuf, fv = view_buffer(api, (N, H, W, c2), pitch, pitch - c2, inp["x"][..., c1:])
    wf, _ = api.ops.pack_conv_weight(d, api.f32(inp["w"]), need_bwd=False)
    b = api.f32(inp["b"])
    for relu in (0, 1):
        y = torch.full((N, H, W, Cout), float("nan"), dtype=api.act, device=api.dev)
        api.ok(L.danhip_conv2d_fwd_concat2(dp, vptr(av), vptr(fv), c1, pitch, ptr(wf), ptr(b), ptr(y), relu, api.stream()))
        api.launched(cid, "relu=%d" % relu, family)
        assert_equal(y, forward_outputs(inp, relu, False), "%s relu=%d" % (cid, relu))


RUNNERS = dict(fwd=run_fwd, dgrad=run_dgrad, wgrad=run_wgrad, pool=run_pool, fold=run_fold, vfwd=run_vfwd, vdgrad=run_vdgrad, vwgrad=run_vwgrad,
               concat2=run_concat2)


def run_case(case, dev):
    cid, kind, shp, family, extra = case
    RUNNERS[kind](_Api(dev), cid, shp, family, extra)

"""Exact dyadic cases for the deformable sampling kernels (csrc/deform_conv.hip, csrc/deform_fused.hip): generators, float64 reference,
census of the knife-edge samples and the case table tests/test_deform_exact_cpu.py and tests/test_deform_exact_gpu.py share.

Why equality is the right check.  Offsets are multiples of 1/4 with |offset| <= 8 (exact in a 16-bit float), so every bilinear weight is a
multiple of 1/16 and every coordinate-gradient weight (a_w, b_w, a_h, b_h) a multiple of 1/4.  x holds small integers: a sample is k / 16 and
the fp32 fma chain that blends it is exact.  dS holds {-1, 0, 1}: dOffset is a sum of multiples of 1/4 and dX a sum of multiples of 1/16,
exact in fp32 in ANY order (atomics, shuffle trees, packed dot products, the fp32 side buffer of the far corners), and exact in the 16-bit
output while |4 dOffset| <= 256 and |16 dX| <= 256.  So every kernel form must return the float64 reference bit for bit; a term counted zero
times or twice, a corner weight from the wrong branch or a tap given to the wrong window shows as a difference of at least 1/16.
check_exact() asserts these preconditions on the reference, on the CPU, before any device result is looked at.

Nothing here needs a GPU or the library."""
import collections
import functools

import torch

from oracle import deform as OD

F64 = torch.float64
LIMIT16 = 256                  # largest |value / unit| a 16-bit output may hold
MIN_PER_CLASS = 4              # every knife-edge class of census() occurs at least this often in every case
KNIFE = (-2.0, -1.75, -1.0, -0.75, 0.75, 1.0, 1.75, 2.0)      # the window edges of both gather forms ([-R, R), R = 1, 2) and their last inner step
EDGE_NAMES = ("-0.25", "0", "L-1", "L-0.25", "L", "L+0.25")   # sample coordinates put exactly there, per axis (L = H or W)
SHARES = (0.45, 0.15, 0.30, 0.10)                              # bulk inside [-1, 1) | KNIFE values | edge coordinates | far outside

Case = collections.namedtuple("Case", "name N H W C dg dil seed density")


def _edge_targets(L):
    return torch.tensor([-0.25, 0.0, L - 1.0, L - 0.25, float(L), L + 0.25], dtype=F64)


def nominal(H, W, dil):
    """Nominal sampling position of (output pixel, tap) for a 3 x 3 kernel, stride 1, SAME padding from the undilated kernel (pad 1):
    -> (nom_h [H,1,9], nom_w [1,W,9]) float64."""
    t = torch.arange(9)
    nh = (torch.arange(H).view(H, 1, 1) - 1 + (t // 3 * dil).view(1, 1, 9)).to(F64)
    nw = (torch.arange(W).view(1, W, 1) - 1 + (t % 3 * dil).view(1, 1, 9)).to(F64)
    return nh, nw


def gen_offsets(N, H, W, dg, dil, seed, shares=SHARES):
    """Offsets [N,H,W,dg*18] float64 (channel (g*9 + t)*2 + {0: dh, 1: dw}), multiples of 1/4 with |offset| <= 8, each component drawn from
    the mixture `shares`; half of the pairs use one class for both components, so that corner cases (both axes on an edge) occur."""
    g = torch.Generator().manual_seed(seed)
    shape = (N, H, W, dg, 9)
    nh, nw = nominal(H, W, dil)
    nom = torch.stack([nh.view(1, H, 1, 1, 9).expand(shape), nw.view(1, 1, W, 1, 9).expand(shape)], dim=-1)       # [N,H,W,dg,9,2]
    cls = torch.multinomial(torch.tensor(shares, dtype=F64), 2 * nom[..., 0].numel(), True, generator=g).view(shape + (2,))
    same = torch.rand(shape, generator=g) < 0.5
    cls[..., 1] = torch.where(same, cls[..., 0], cls[..., 1])
    full = shape + (2,)
    bulk = torch.randint(-4, 4, full, generator=g).to(F64) / 4
    knife = torch.tensor(KNIFE, dtype=F64)[torch.randint(0, len(KNIFE), full, generator=g)]
    which = torch.randint(0, 6, full, generator=g)
    targ = torch.stack([_edge_targets(H)[which[..., 0]], _edge_targets(W)[which[..., 1]]], dim=-1)
    edge = targ - nom
    edge = torch.where(edge.abs() <= 8, edge, bulk)                       # (an edge the tap cannot reach with |offset| <= 8: bulk instead)
    far = (torch.randint(12, 33, full, generator=g).to(F64) / 4) * (torch.randint(0, 2, full, generator=g) * 2 - 1).to(F64)
    off = torch.where(cls == 0, bulk, torch.where(cls == 1, knife, torch.where(cls == 2, edge, far)))
    assert torch.equal(off * 4, (off * 4).round()) and off.abs().max().item() <= 8
    return off.reshape(N, H, W, dg * 18)


def bulk_offsets(N, H, W, dg, seed):
    """Offsets of the bulk class only: every component a multiple of 1/4 inside [-1, 1)."""
    return gen_offsets(N, H, W, dg, 1, seed, shares=(1.0, 0.0, 0.0, 0.0))


def gen_x(N, H, W, C, seed):
    """Integers in [-3, 3], float64 [N,H,W,C]."""
    return torch.randint(-3, 4, (N, H, W, C), generator=torch.Generator().manual_seed(seed)).to(F64)


def gen_ternary(shape, density, seed):
    """{-1, 0, 1} float64: non-zero with probability `density`, either sign equally likely."""
    g = torch.Generator().manual_seed(seed)
    nz = torch.rand(shape, generator=g) < density
    sign = (torch.randint(0, 2, shape, generator=g) * 2 - 1).to(F64)
    return torch.where(nz, sign, torch.zeros(shape, dtype=F64))


def gen_small_ints(shape, seed, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).to(F64)


def gen_filter(C, Cout, nnz, seed):
    """Ternary filter OIHW [Cout, C, 3, 3] float64 with exactly `nnz` non-zeros (+-1) per output channel: |y| <= 3 nnz whatever the samples are."""
    g = torch.Generator().manual_seed(seed)
    w = torch.zeros((Cout, C * 9), dtype=F64)
    for co in range(Cout):
        idx = torch.randperm(C * 9, generator=g)[:nnz]
        w[co, idx] = (torch.randint(0, 2, (nnz,), generator=g) * 2 - 1).to(F64)
    return w.reshape(Cout, C, 3, 3)


def filter_hwio(w_oihw):
    """OIHW [Cout,C,3,3] -> the GEMM operand [1,1,9C,Cout], k = tap * C + c."""
    co, c = w_oihw.shape[0], w_oihw.shape[1]
    return w_oihw.permute(2, 3, 1, 0).reshape(1, 1, 9 * c, co).contiguous()


# ================================================================================================================ reference (float64, CPU)
def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def col_ref(x, off, dg, dil, dtype=F64):
    """The deformable im2col in `dtype`: x [N,H,W,C], off [N,H,W,dg*18] -> S [N,H,W,9C], k = tap * C + c (the kernels' column buffer)."""
    N, H, W, C = x.shape
    col = OD.deform_im2col(_nchw(x.to(dtype)), _nchw(off.to(dtype)), 3, 3, 1, dil, dg)               # [N,C,9,H,W]
    return col.permute(0, 3, 4, 2, 1).reshape(N, H, W, 9 * C).contiguous()


def sample_bwd_ref(x, off, dS, dg, dil, dtype=F64):
    """x [N,H,W,C], off [N,H,W,dg*18], dS [N*H*W, 9C] (k = tap * C + c) -> (dX [N,H,W,C], dOffset [N,H,W,dg*18]) in `dtype`."""
    N, H, W, C = x.shape
    cg = dS.to(dtype).reshape(N, H, W, 9, C).permute(0, 4, 3, 1, 2).contiguous()                      # [N,C,9,H,W]
    dx, doff = OD.deform_sample_backward(_nchw(x.to(dtype)), _nchw(off.to(dtype)), cg, 3, 3, 1, dil, dg)
    return dx.permute(0, 2, 3, 1).contiguous(), doff.permute(0, 2, 3, 1).contiguous()


def conv_ref(x, w_oihw, off, dg, dil, bias=None):
    """DeformConvOp in float64 -> y [N,H,W,Cout]."""
    y = OD.deform_conv_forward(_nchw(x), w_oihw, _nchw(off), 1, dil, dg).permute(0, 2, 3, 1)
    return (y + bias if bias is not None else y).contiguous()


def conv_bwd_ref(x, w_oihw, off, dy, dg, dil):
    """DeformConvBackpropOp in float64: dy [N,H,W,Cout] -> (dX [N,H,W,C], dW OIHW, dOffset [N,H,W,dg*18], dS [N*H*W, 9C])."""
    N, H, W, C = x.shape
    dx, dw, doff = OD.deform_conv_backward(_nchw(x), w_oihw, _nchw(off), _nchw(dy), 1, dil, dg)
    dS = dy.reshape(N * H * W, -1) @ filter_hwio(w_oihw).reshape(9 * C, -1).t()
    return dx.permute(0, 2, 3, 1).contiguous(), dw, doff.permute(0, 2, 3, 1).contiguous(), dS


def check_exact(ref, unit, limit16):
    """The exactness preconditions of one reference tensor: every value a whole multiple of `unit`; with limit16 (an output stored in
    16 bits) no multiple beyond LIMIT16.  Called on every reference of every case before a device result is compared with it."""
    assert ref.dtype == F64
    q = ref / unit
    assert torch.equal(q, q.round()), "reference is not a multiple of %g" % unit
    if limit16:
        big = q.abs().max().item() if q.numel() else 0.0
        assert big <= LIMIT16, "|reference / %g| reaches %g > %d: not exact in 16 bits" % (unit, big, LIMIT16)
    return ref


# ================================================================================================================ census
def far_counts(off):
    """What deform_far_stat_kernel counts: the (dh, dw) pairs with a component outside [-2, 2) and outside [-1, 1)."""
    p = off.reshape(-1, 2)
    out = lambda R: int((((p < -R) | (p >= R)).any(dim=1)).sum().item())
    return out(2.0), out(1.0)


def census_of(off, H, W, dg, dil):
    """Number of samples (offset pairs) in each knife-edge class -> dict.
      h=<e> / w=<e>   that coordinate exactly on edge e of EDGE_NAMES while the other coordinate lies inside [0, L): the sample's fate is
                      decided by this coordinate's range test alone (`>= H` of dOffset and the forward against `> H` of dX, `< 0`, the clamp)
      floor!=trunc    inside the image with a negative fractional coordinate RELATIVE to the window origin: the forward's floorf and an
                      (int) truncation differ there
      clamp_h / clamp_w / clamp_hw   inside the image with only the row, only the column, both on the high-edge clamp (coordinate >= L - 1):
                      the duplicate-corner flags dup = {cw, ch, ch || cw}
      off=<v>         a component exactly v of KNIFE: the far tests `offset outside [-R, R)` at -R, R and one step inside
      far2 / far1     pairs with a component outside [-2, 2) / [-1, 1): the statistic"""
    N = off.shape[0]
    o = off.reshape(N, H, W, dg, 9, 2)
    nh, nw = nominal(H, W, dil)
    ch = nh.view(1, H, 1, 1, 9) + o[..., 0]
    cw = nw.view(1, 1, W, 1, 9) + o[..., 1]
    in_h, in_w = (ch >= 0) & (ch < H), (cw >= 0) & (cw < W)
    out = collections.OrderedDict()
    for name, th, tw in zip(EDGE_NAMES, _edge_targets(H).tolist(), _edge_targets(W).tolist()):
        out["h=" + name] = int(((ch == th) & in_w).sum().item())
        out["w=" + name] = int(((cw == tw) & in_h).sum().item())
    inside = in_h & in_w
    t = torch.arange(9)
    mh = (t // 3 * dil).view(1, 1, 1, 1, 9).to(F64) + o[..., 0]
    mw = (t % 3 * dil).view(1, 1, 1, 1, 9).to(F64) + o[..., 1]
    out["floor!=trunc"] = int((inside & (((mh < 0) & (mh != mh.floor())) | ((mw < 0) & (mw != mw.floor())))).sum().item())
    kh, kw = ch >= H - 1, cw >= W - 1
    out["clamp_h"] = int((inside & kh & ~kw).sum().item())
    out["clamp_w"] = int((inside & ~kh & kw).sum().item())
    out["clamp_hw"] = int((inside & kh & kw).sum().item())
    for v in KNIFE:
        out["off=%g" % v] = int((o == v).any(dim=-1).sum().item())
    out["far2"], out["far1"] = far_counts(off)
    return out


# ================================================================================================================ cases
# Tiles are 8 x 16; the c64 item and tile kernels need C / dg == 64; the forward's blocks own 8 output pixels of a row.
#   5 x 5: tile larger than the map     8 x 16: exactly one tile     9 x 17: one ragged row and column     17 x 33: 3 x 3 tiles, interior seams
# N = 2 throughout (a read of the neighbour image shows).  Density of dS: 16 expected non-zeros per deformable group, so that the 64-, 32-
# and 128-channel reductions of dOffset stay within the 16-bit exact range.
def _cases():
    out = []
    seed = 100
    for (H, W) in ((5, 5), (8, 16), (9, 17), (17, 33)):
        for (C, dg) in ((64, 1), (128, 2), (256, 4)):
            out.append(Case("c64_%dx%d_c%d_dg%d" % (H, W, C, dg), 2, H, W, C, dg, 1, seed, 0.25))
            seed += 1
    for (H, W) in ((5, 5), (9, 17)):
        for (C, dg, dens) in ((128, 4, 0.5), (256, 2, 0.125)):
            out.append(Case("generic_%dx%d_c%d_dg%d" % (H, W, C, dg), 2, H, W, C, dg, 1, seed, dens))
            seed += 1
    out.append(Case("dil2_9x17_c128_dg2", 2, 9, 17, 128, 2, 2, seed, 0.25))
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
Data = collections.namedtuple("Data", "x off dS dx0 col dx doff")


@functools.lru_cache(maxsize=None)
def data(name):
    """Inputs and float64 references of a case, computed once and shared (treat as read-only): x, off, dS, dx0 (what dX accumulates onto),
    col = im2col, dx / doff = the sampling gradients of dS."""
    c = CASE_BY_NAME[name]
    x = gen_x(c.N, c.H, c.W, c.C, c.seed)
    off = gen_offsets(c.N, c.H, c.W, c.dg, c.dil, c.seed + 1000)
    dS = gen_ternary((c.N * c.H * c.W, 9 * c.C), c.density, c.seed + 2000)
    dx0 = gen_small_ints((c.N, c.H, c.W, c.C), c.seed + 3000)
    col = col_ref(x, off, c.dg, c.dil)
    dx, doff = sample_bwd_ref(x, off, dS, c.dg, c.dil)
    return Data(x, off, dS, dx0, col, dx, doff)


def census(case):
    return census_of(data(case.name).off, case.H, case.W, case.dg, case.dil)


def check_case(case):
    """Every exactness precondition of a case, on its references: samples in 1/16 within the 16-bit range, dOffset in 1/4, dX in 1/16 -
    alone and on top of dx0."""
    d = data(case.name)
    check_exact(d.x, 1.0, True)
    check_exact(d.off, 0.25, True)
    check_exact(d.dS, 1.0, True)
    check_exact(d.col, 1.0 / 16, True)
    check_exact(d.doff, 0.25, True)
    check_exact(d.dx, 1.0 / 16, True)
    check_exact(d.dx + d.dx0, 1.0 / 16, True)
    return d


# ---- the convolution around the sampling: a ternary filter with 5 non-zeros per output channel (|y| <= 15 + |bias| <= 16: exact in 16 bits
# whatever the samples are) and a ternary dY; dS = dY W^T then holds small integers and the gradients' limits are asserted on the references.
CONV_CASES = ("c64_9x17_c128_dg2", "c64_17x33_c64_dg1", "c64_5x5_c256_dg4")
Conv = collections.namedtuple("Conv", "w bias y dy dS dx dw doff")


FwdConv = collections.namedtuple("FwdConv", "w bias y")


@functools.lru_cache(maxsize=None)
def fwd_conv_data(name):
    """Filter (Cout = C), bias in {-1, 0, 1} and y of a case; the limit |16 y| <= 256 is asserted here, on the reference."""
    c = CASE_BY_NAME[name]
    d = data(name)
    w = gen_filter(c.C, c.C, 5, c.seed + 4000)
    bias = gen_small_ints((c.C,), c.seed + 5000, -1, 1)
    y = check_exact(conv_ref(d.x, w, d.off, c.dg, c.dil, bias), 1.0 / 16, True)
    return FwdConv(w, bias, y)


@functools.lru_cache(maxsize=None)
def conv_data(name):
    """Cout = C: the three cases run the fused forward's three output widths (128, 64, 256)."""
    c = CASE_BY_NAME[name]
    d = data(name)
    w, bias, y = fwd_conv_data(name)
    dy = gen_ternary((c.N, c.H, c.W, c.C), 0.25, c.seed + 6000)
    dx, dw, doff, dS = conv_bwd_ref(d.x, w, d.off, dy, c.dg, c.dil)
    return Conv(w, bias, y, dy, dS, dx, dw, doff)


def check_conv(name):
    cv = conv_data(name)
    check_exact(cv.y, 1.0 / 16, True)
    check_exact(cv.dS, 1.0, True)
    check_exact(cv.doff, 0.25, True)
    check_exact(cv.dx, 1.0 / 16, True)
    check_exact(cv.dw, 1.0 / 16, False)
    assert (cv.dw * 16).abs().max().item() < 2 ** 24
    return cv


# ---- offsets that put the statistic just below, on and just above a threshold: bulk offsets (nothing outside [-1, 1)) with exactly `count`
# pairs, chosen by a fixed permutation, whose dh is set to `value`.
def planted_offsets(N, H, W, dg, seed, count, value):
    off = bulk_offsets(N, H, W, dg, seed).reshape(-1, 2).clone()
    idx = torch.randperm(off.shape[0], generator=torch.Generator().manual_seed(seed + 1))[:count]
    off[idx, 0] = value
    return off.reshape(N, H, W, dg * 18)

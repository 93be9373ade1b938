"""Exact cases for the two forward-only inference paths (csrc/split_infer.hip with the fp16 build's convolution epilogues, csrc/f32_infer.hip):
operand builders, float64 references, the restated kernel selection of a split-operand call, case tables and the runners
tests/test_infer_exact_gpu.py uses.  tests/test_infer_exact_cpu.py pins everything here that needs no GPU.

Why equality is the right check for the split-operand convolution.  A value is carried as two IEEE-half limbs, v = hi + lo; the kernel sums the
three half products hi.hi + lo.hi + hi.lo in fp32.  With
    x = 16 a + 2^-8 b |a|        (a, b ternary; a limb map holds x 2^-2, so hi = 4 a, lo = 2^-10 b)
    w = 16 a' + 2^-8 b' |a'|     (packed as w 2^9: hi = 2^13 a', lo = 2 b')
every limb is a normal half or zero, hi + lo is the value exactly, a main product is 2^15 and a cross product 2^3 in the accumulator: every
partial sum is a multiple of 2^3 below 2^27, exact in fp32 in any order, under any split of K.  So the device result must EQUAL float64
conv(x, w) when only one operand carries lo limbs (classes A and B), and float64 conv(x, w) - conv(x_lo, w_lo) when both do (class C: the
dropped lo.lo term, itself computed in float64).  A cross term dropped or doubled in one K chunk is a whole-quantum difference.

Nothing before the runners needs a GPU or the library; the runners import dan_amd lazily."""
import ctypes
import functools
import math

import torch
import torch.nn.functional as F

import conv_exact as CE

F64 = CE.F64
LIMB_EXP = 2            # dan_amd.ops.LIMB_EXP restated: the maps the split path writes hold v * 2^-2
CLASSES = ("A", "B", "C")


# ================================================================================================================ limbs (float64 tensors of halves)
def half(t):
    """Round to IEEE half (nearest even), as float64.  Through fp32: the callers assert their values are fp32 values, so nothing rounds twice."""
    return t.to(torch.float32).to(torch.float16).to(F64)


def is_f32(t):
    return bool(torch.equal(t.to(torch.float32).to(F64), t))


def limbs(v):
    """(hi, lo) = (half(v), half(v - hi)) of the STORED value v (the exponent already applied)."""
    hi = half(v)
    return hi, half(v - hi)


def limb_map(v):
    """[.., C] stored values -> [.., 3C] = [hi | lo | hi] as torch.float16 (the raw halves the device must write)."""
    hi, lo = limbs(v)
    return torch.cat([hi, lo, hi], dim=-1).to(torch.float16)


def normal_or_zero(t):
    a = t.abs()
    return bool(((a == 0) | ((a >= 2.0 ** -14) & (a <= 65504))).all())


def weight_exp(w):
    """ops._weight_exp restated: e with max|w 2^e| in [2^13, 2^14)."""
    m = float(w.abs().max())
    return 0 if m == 0.0 else 14 - math.frexp(m)[1]


def quantum(*ts):
    """The largest power of two that divides every element of the tensors (values are multiples of 2^-40 below 2^22)."""
    q = None
    for t in ts:
        i = (t * 2.0 ** 40).to(torch.int64)
        assert torch.equal(i.to(F64) * 2.0 ** -40, t)
        i = i[i != 0]
        if i.numel():
            low = int((i & -i).min())
            q = low if q is None else min(q, low)
    return (q or 2 ** 40) * 2.0 ** -40


# ================================================================================================================ references (float64, CPU)
def conv_ref(x, w, b=None, stride=1, padding="same"):
    if padding == "same":
        return CE.conv_ref(x, w, b, stride)
    return F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), b, stride=stride).permute(0, 2, 3, 1).contiguous()


def out_hw(H, W, kh, kw, s, padding):
    if padding == "valid":
        return (H - kh) // s + 1, (W - kw) // s + 1
    return -(-H // s), -(-W // s)


def operand(shape, p, g, lo):
    """16 a + 2^-8 b |a|: a ternary with density p, b ternary with density 0.5 (only where lo is asked for); lo is non-zero only where hi is."""
    a = CE.ternary(shape, p, g)
    b = CE.ternary(shape, 0.5, g)
    return 16.0 * a + (2.0 ** -8 * b * a.abs() if lo else 0.0)


def split_density(K):
    return min(1.0, math.sqrt(64.0 / K))


@functools.lru_cache(maxsize=4)
def split_inputs(shape, cls, padding="same", seed=11):
    """Operands of one class for the logical shape (N,H,W,C,Cout,kh,kw,s): x, w, a bias and a residual of multiples of the output quantum 2^-4,
    pre = the float64 value the device must produce before bias / ReLU, lolo = the dropped term (class C; zero otherwise), and the stored limbs."""
    N, H, W, C, Cout, kh, kw, s = shape
    g = CE.gen(seed + sum(shape) + 1000 * CLASSES.index(cls))
    p = split_density(kh * kw * C)
    x = operand((N, H, W, C), p, g, cls in "AC")
    w = operand((kh, kw, C, Cout), p, g, cls in "BC")
    b = CE.small((Cout,), g, -64, 64) * 2.0 ** -4
    xh, xl = limbs(x * 2.0 ** -LIMB_EXP)
    we = weight_exp(w)
    wh, wl = limbs(w * 2.0 ** we)
    full = conv_ref(x, w, None, s, padding)
    lolo = conv_ref(xl * 2.0 ** LIMB_EXP, wl * 2.0 ** -we, None, s, padding) if cls == "C" else torch.zeros_like(full)
    res = CE.small(tuple(full.shape), g, -64, 64) * 2.0 ** -4
    # an upper bound of the accumulator's abs-sum (it also counts the lo.lo products the kernel never forms), in stored units
    abs_acc = conv_ref(xh.abs() + xl.abs(), wh.abs() + wl.abs(), None, s, padding)
    return dict(x=x, w=w, b=b, res=res, pre=full - lolo, full=full, lolo=lolo, xh=xh, xl=xl, wh=wh, wl=wl, we=we, xe=LIMB_EXP, abs_acc=abs_acc, cls=cls)


def check_stage(xh, xl, wh, wl, abs_acc, acc_exp, bias_stored, v_stored):
    """What makes a split-operand stage exact, from reference-side data only: every limb normal or zero; every product a multiple of the
    accumulator quantum q = quantum(x limbs) quantum(w limbs); abs-sum + |bias| below 2^24 q; the epilogue's value an fp32 value."""
    assert normal_or_zero(xh) and normal_or_zero(xl) and normal_or_zero(wh) and normal_or_zero(wl), "a limb is subnormal or out of range"
    # the products the kernel forms: hi.hi, lo.hi, hi.lo (never lo.lo)
    qs = [quantum(a) * quantum(b) for a, b in ((xh, wh), (xl, wh), (xh, wl)) if a.any() and b.any()]
    q = min(qs)
    sc = 2.0 ** acc_exp
    bmax = 0.0 if bias_stored is None else bias_stored.abs().max().item()
    quanta = (abs_acc.max().item() * sc + bmax) / (q * sc)
    assert quanta < 2 ** 24, ("the accumulator leaves fp32's exact range", quanta)
    if bias_stored is not None:
        assert torch.equal(torch.round(bias_stored / (q * sc)) * (q * sc), bias_stored), "bias is no multiple of the output quantum"
    assert is_f32(v_stored), "the epilogue value is no fp32 value"
    return quanta


def check_split_inputs(inp, relu=True):
    """The preconditions of a split-operand case (ISSUE section A), all from the reference side; returns figures for the log."""
    x, w, cls = inp["x"], inp["w"], inp["cls"]
    xs, ws = x * 2.0 ** -LIMB_EXP, w * 2.0 ** inp["we"]
    assert torch.equal(inp["xh"] + inp["xl"], xs) and torch.equal(inp["wh"] + inp["wl"], ws), "hi + lo is not the value"
    assert is_f32(x) and is_f32(w)
    figs = dict(we=inp["we"])
    for limbs_out in (True, False):
        ye = LIMB_EXP if limbs_out else 0
        v = inp["pre"] + inp["b"]
        figs["quanta"] = check_stage(inp["xh"], inp["xl"], inp["wh"], inp["wl"], inp["abs_acc"], inp["xe"] - inp["we"] - ye, inp["b"] * 2.0 ** -ye, v * 2.0 ** -ye)
        assert is_f32(inp["pre"] * 2.0 ** -ye) and is_f32((v + inp["res"]))
    assert inp["pre"].abs().max().item() * 2.0 ** -LIMB_EXP < 65504
    lo_x, lo_w = (inp["xl"] != 0).double().mean().item(), (inp["wl"] != 0).double().mean().item()
    if cls in "AC":
        assert lo_x >= 0.05, ("fewer than 5 % of the activations carry a lo limb", lo_x)
    else:
        assert lo_x == 0
    if cls in "BC":
        assert lo_w >= 0.05, ("fewer than 5 % of the weights carry a lo limb", lo_w)
    else:
        assert lo_w == 0
    if cls == "C":
        figs["lolo"] = (inp["lolo"] != 0).double().mean().item()
        assert figs["lolo"] > 0.5, ("the dropped lo.lo term is zero for most outputs", figs["lolo"])
    else:
        assert not inp["lolo"].any()
    if relu:
        v = inp["pre"] + inp["b"]
        assert int((v < 0).sum()) >= 1 and int((v > 0).sum()) >= 1, "ReLU clips everything or nothing"
    figs.update(lo_x=lo_x, lo_w=lo_w, max=inp["pre"].abs().max().item())
    return figs


def split_expected(inp, bias, relu, residual, limbs_out):
    """The float64 value and (limbs_out) the raw half map [N,Ho,Wo,3 Cout] the device must write."""
    v = inp["pre"] + (inp["b"] if bias else 0.0)
    if relu:
        v = torch.relu(v)
    if residual:
        v = v + inp["res"]
    return limb_map(v * 2.0 ** -LIMB_EXP) if limbs_out else v


# ================================================================================================================ kernel selection, restated
def ceil8(c):
    return (c + 7) // 8 * 8


def pick_bn(co):
    return 128 if co % 128 == 0 else 64 if co % 64 == 0 else 16 if co <= 16 else 32 if co <= 32 else 64


def plan_split_call(shape, limbs_out, padding="same", cus=256, use_splitk=True):
    """What ops._conv2d_split launches for the logical shape: conv_igemm.hip select_conv / plan_splitk and conv_halo.hip plan_halo over 3C
    (rounded up to 8) channels, with the scratch rule of ops._conv2d_split.  -> dict(label, splits, ws_bytes, limb_shape, M)."""
    N, H, W, C, Cout, kh, kw, s = shape
    C3 = ceil8(3 * C)
    Ho, Wo = out_hw(H, W, kh, kw, s, padding)
    M = N * Ho * Wo
    ktiles = CE.cdiv(kh * kw * C3, 64)
    bn = pick_bn(Cout)
    bm = 128 if bn == 128 else (64 if M <= 256 * 128 else 256) if bn == 16 else 256
    # plan_splitk
    tiles = CE.cdiv(M, bm) * CE.cdiv(Cout, bn)
    target = (8 if bn == 16 else 2) * cus
    splits = 1
    if not (tiles * 2 > target or ktiles < 8):
        sp = min(CE.cdiv(target, tiles), ktiles // 4, 36)
        if sp >= 2:
            splits = CE.cdiv(ktiles, CE.cdiv(ktiles, sp))
    ws_bytes = query = splits * M * Cout * 4 if splits >= 2 else 0          # danhip_conv2d_workspace_bytes of the limb descriptor
    if CE.cdiv(M, 128) * CE.cdiv(Cout, 128) > 160 or not use_splitk:          # ops._conv2d_split: only small problems ask for scratch
        ws_bytes = 0
    prefer = ws_bytes > 0 and CE.cdiv(M, 128) * CE.cdiv(Cout, 128) * 2 <= cus
    out = dict(limb_shape=(N, H, W, C3, Cout, kh, kw, s), M=M, ktiles=ktiles, splits=splits if ws_bytes else 1, ws_bytes=ws_bytes, query_bytes=query)
    assert C3 not in (8, 64), "the first-layer / 64 -> 64 kernels are not restated here"
    if not prefer:
        same3 = kh == 3 and kw == 3 and s == 1 and padding == "same"
        head = Cout <= 16
        co_ok = Cout % 64 == 0 or head or (Cout % 8 == 0 and Cout > 32)
        if same3 and C3 >= 64 and C3 <= 2048 and co_ok and Cout <= 2048 and not (limbs_out and head):
            util = lambda th, tw: H * W / float(CE.cdiv(H, th) * th * CE.cdiv(W, tw) * tw)
            u1, u2 = util(8, 32), util(16, 16)
            if max(u1, u2) >= 0.78:
                tile = "8, 32" if u1 >= u2 else "16, 16"
                if head:
                    cfg = "64, 8, 1, 3, 3, false, 1, false"
                elif CE.cdiv(Cout, 64) * 64 % 128 == 0:
                    cfg = "128, 4, 2, 1, 4, false, 0, false"
                else:
                    cfg = "64, 8, 1, 1, 4, false, 0, false"
                out["label"] = "conv3x3_halo_kernel<%s, %s>" % (tile, cfg)
                out["splits"] = 1
                return out
    wn = 2 if bn == 128 else 1
    out["label"] = "conv_igemm_kernel<%d, %d, %d, %s>" % (bm, bn, wn, "true" if C3 % 64 == 0 else "false")
    return out


# ================================================================================================================ case tables
S = CE.S
HALO, FLAT = CE.HALO, CE.FLAT
# (id, logical shape, options, family of the launched instance, "splitk" where the case is there for a split K).
# options: f32 (out_f32=True), valid (padding='valid'), res (a residual: fp32 output).  The halo kernels take a split call only where it does
# not prefer to split K: select_conv asks prefer_splitk first, and ops._conv2d_split hands scratch over for up to 160 tiles of 128 x 128 - so
# a halo case needs more than 16384 output pixels (cdiv(M, 128) cdiv(Cout, 128) 2 > 256 CUs).  The shapes the issue sketched for the halo rows
# (16 x 32 and 15 x 31 maps) split K on the flat-M kernel instead; they moved to the smallest maps that reach the halo kernels.
SPLIT_CASES = [
    ("halo8x32_128", S(1, 104, 160, 64, 128), "", HALO + "8, 32, 128, * false, 0, false>", ""),
    ("halo8x32_128_f32", S(1, 104, 160, 64, 128), "f32", HALO + "8, 32, 128, * false, 0, false>", ""),
    ("halo16x16_64", S(1, 130, 130, 64, 64), "", HALO + "16, 16, 64, * false, 0, false>", ""),               # ragged 16 x 16 edges: 130 = 8 * 16 + 2
    ("halo_ragged_cin72_cout40", S(2, 91, 93, 72, 40), "", HALO + "8, 32, 64, 8, 1, 1, 4, false, 0, false>", ""),   # 216 % 64 != 0, 40 % 64 != 0
    ("halo_head6_f32", S(1, 104, 160, 64, 6), "f32", HALO + "8, 32, 64, * false, 1, false>", ""),
    ("halo_head8_f32", S(1, 104, 160, 64, 8), "f32", HALO + "8, 32, 64, * false, 1, false>", ""),
    ("small_map_splits_k", S(1, 16, 32, 64, 128), "", FLAT + "128, 128, 2, true>", "splitk"),                 # the issue's halo shape: flat-M, split K
    ("limbs_exclude_head8", S(1, 16, 32, 64, 8), "", FLAT + "64, 16, 1, true>", "splitk"),
    ("pointwise_256_splitk", S(1, 20, 20, 256, 256, 1), "", FLAT + "128, 128, 2, true>", "splitk"),
    ("pointwise_no_scratch", S(4, 52, 52, 64, 256, 1), "", FLAT + "128, 128, 2, true>", ""),                  # 85 x 2 = 170 tiles > 160
    ("stride2_odd", S(2, 33, 31, 128, 256, 3, 2), "", FLAT + "128, 128, 2, true>", "splitk"),
    ("pointwise_cin72", S(1, 12, 12, 72, 64, 1), "", FLAT + "256, 64, 1, false>", ""),
    ("cin5_pad_column", S(2, 9, 11, 5, 16), "", FLAT + "64, 16, 1, false>", ""),
    ("taps_3x1", S(1, 12, 12, 64, 32, (3, 1)), "", FLAT + "256, 32, 1, true>", "splitk"),
    ("taps_1x3", S(1, 12, 12, 64, 32, (1, 3)), "", FLAT + "256, 32, 1, true>", "splitk"),
    ("valid_9x10", S(1, 9, 10, 64, 64), "valid", FLAT + "256, 64, 1, true>", "splitk"),
    ("head6_small_map_f32", S(1, 10, 10, 512, 6), "f32", FLAT + "64, 16, 1, true>", "splitk"),
    ("deform_gemm_k1728", S(1, 8, 8, 1728, 64, 1), "", FLAT + "256, 64, 1, true>", "splitk"),
    ("residual_f32", S(1, 16, 32, 64, 64), "res", FLAT + "256, 64, 1, true>", "splitk"),
]
# the variants every case and class runs: (bias, relu)
SPLIT_VARIANTS = ((True, True), (False, False))


def case_opts(case):
    cid, shp, opts, family, extra = case
    return dict(f32="f32" in opts or "res" in opts, padding="valid" if "valid" in opts else "same", res="res" in opts)


def check_split_case(case, cus=256):
    """Preconditions of every class of one case and the restated launch; returns figures for the log."""
    cid, shp, opts, family, extra = case
    o = case_opts(case)
    plan = plan_split_call(shp, not o["f32"], o["padding"], cus)
    from test_conv_dispatch_gpu import in_family
    assert in_family(plan["label"], family), (cid, plan["label"], family)
    if extra == "splitk":
        assert plan["splits"] >= 2 and plan["ws_bytes"] > 0, (cid, plan)
        if o["padding"] == "same":
            assert CE.plan_splitk(plan["limb_shape"], 0, cus)[0] == plan["splits"] >= 2
    figs = dict(label=plan["label"], splits=plan["splits"])
    for cls in CLASSES:
        figs[cls] = check_split_inputs(split_inputs(shp, cls, o["padding"]))
    return figs


# ---- the chained case: conv -> conv -> max-pool -> head conv, every intermediate a limb view.  Later stages multiply a many-bit activation
# (hi and lo limbs) with exactly representable sparse weights, so that nothing is dropped and every stage stays exact.
CHAIN_SHAPE = (1, 12, 12, 16)      # N, H, W, C of the fp32 input; 16 -> 16 -> 16 -> pool -> 6
CHAIN_CLASSES = ("A", "B")


@functools.lru_cache(maxsize=2)
def chain_inputs(cls, seed=23):
    N, H, W, C = CHAIN_SHAPE
    g = CE.gen(seed + CLASSES.index(cls))
    x = operand((N, H, W, C), 1 / 3, g, cls == "A")
    w1 = operand((3, 3, C, 16), 1 / 3, g, cls == "B")
    w2 = CE.ternary((3, 3, 16, 16), 1 / 12, g) * 2.0 ** -4
    w3 = CE.ternary((3, 3, 16, 6), 1 / 24, g)
    b1, b2, b3 = (CE.small((n,), g, -8, 8) for n in (16, 16, 6))
    stages = []
    # stage 1 (fp32 input, split here), 2 (limb view in), pool, 3 (limb view in, fp32 out)
    v0 = x
    xh, xl = limbs(v0 * 2.0 ** -LIMB_EXP)
    for w, b, relu, ye in ((w1, b1, True, LIMB_EXP), (w2, b2, True, LIMB_EXP), (w3, b3, False, 0)):
        if len(stages) == 2:                                   # the pool between stage 2 and the head
            v0 = CE.pool_ref(v0)[0]
            xh, xl = limbs(v0 * 2.0 ** -LIMB_EXP)
        we = weight_exp(w)
        wh, wl = limbs(w * 2.0 ** we)
        v = conv_ref(v0, w, b, 1)
        v = torch.relu(v) if relu else v
        stages.append(dict(xh=xh, xl=xl, wh=wh, wl=wl, we=we, ye=ye, b=b, v=v, carried=xh + xl, v_in=v0 * 2.0 ** -LIMB_EXP,
                           abs_acc=conv_ref(xh.abs() + xl.abs(), wh.abs() + wl.abs(), None, 1), pre=conv_ref(v0, w, b, 1)))
        v0 = v
        xh, xl = limbs(v0 * 2.0 ** -LIMB_EXP)
    return dict(x=x, ws=(w1, w2, w3), bs=(b1, b2, b3), stages=stages)


def check_chain_inputs(inp):
    figs = []
    for i, st in enumerate(inp["stages"]):
        assert torch.equal(st["carried"], st["v_in"]), "stage %d: the limbs do not carry the value exactly" % (i + 1)
        assert torch.equal(st["wh"] + st["wl"], inp["ws"][i] * 2.0 ** st["we"])
        if i > 0:
            assert not st["wl"].any(), "a later stage's weights must be exact halves (nothing may be dropped)"
        q = check_stage(st["xh"], st["xl"], st["wh"], st["wl"], st["abs_acc"], LIMB_EXP - st["we"] - st["ye"], st["b"] * 2.0 ** -st["ye"], st["pre"] * 2.0 ** -st["ye"])
        if st["ye"]:
            assert st["v"].abs().max().item() * 2.0 ** -LIMB_EXP < 65504
            assert int((st["pre"] < 0).sum()) >= 1 and int((st["pre"] > 0).sum()) >= 1
        figs.append(dict(quanta=q, lo=(st["xl"] != 0).double().mean().item(), max=st["v"].abs().max().item()))
    assert figs[1]["lo"] >= 0.05 and figs[2]["lo"] >= 0.05 and inp["stages"][2]["v"].abs().max().item() > 0
    return figs


# ================================================================================================================ B: the first layer
FIRST_SHAPES = [(2, 1, 1), (1, 2, 3), (2, 3, 5), (1, 7, 6), (2, 5, 167), (1, 3, 45)]      # (1,3,45): 3 * 12 * 8 = 288 threads = one block + 32


@functools.lru_cache(maxsize=2)
def first_inputs(nhw, seed=31):
    N, H, W = nhw
    g = CE.gen(seed + N + 7 * H + 13 * W)
    x = CE.small((N, H, W, 3), g, -128, 127)
    w = CE.small((3, 3, 3, 64), g)
    # integers of 14 bits: v / 4 then spans more than hi's 11 bits for most outputs, whatever the image size
    b = (8192 + CE.small((64,), g, 0, 4096)) * CE.signs((64,), g)
    return dict(x=x, w=w, b=b, pre=conv_ref(x, w, None, 1))


def first_expected(inp, bias, relu):
    v = inp["pre"] + (inp["b"] if bias else 0.0)
    return limb_map((torch.relu(v) if relu else v) * 2.0 ** -LIMB_EXP)


def check_first_inputs(inp):
    v = inp["pre"] + inp["b"]
    assert v.abs().max().item() <= 27648 + 12288 and conv_ref(inp["x"].abs(), inp["w"].abs(), None, 1).max().item() + 12288 < 2 ** 22      # quarters below 2^24
    hi, lo = limbs(v * 2.0 ** -LIMB_EXP)
    assert torch.equal(hi + lo, v * 2.0 ** -LIMB_EXP) and normal_or_zero(hi) and normal_or_zero(lo)
    need_lo = (lo != 0).double().mean().item()
    assert need_lo > 0.5, ("most outputs should need a lo limb", need_lo)
    return dict(max=v.abs().max().item(), need_lo=need_lo)


# ================================================================================================================ C: max-pool on the limb layout
POOL_SHAPES = [(1, 1, 1, 8), (2, 1, 7, 8), (1, 7, 1, 16), (2, 33, 47, 72), (1, 6, 6, 128)]
POOL_HI = (-3.0, -1.5, -0.0, 0.0, 1.0, 2.5)
POOL_LO = (-3 * 2.0 ** -13, -2.0 ** -13, 0.0, 2.0 ** -13, 3 * 2.0 ** -13)


@functools.lru_cache(maxsize=8)
def pool_inputs(shape, seed=41):
    """Limb maps built limb by limb (not from a split): in even channels every element of a window shares its hi limb, so only lo decides; odd
    channels draw hi per element.  Channels 0 and 1 are negative everywhere, channel 2 is -0 only (hi and lo), channel 3 is +-0 only."""
    N, H, W, C = shape
    g = CE.gen(seed + sum(shape))
    pick = lambda vals, shp: torch.tensor(vals, dtype=F64)[torch.randint(0, len(vals), shp, generator=g)]
    Hp, Wp = (H + 1) // 2, (W + 1) // 2
    shared = pick(POOL_HI, (N, Hp, Wp, C)).repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W]
    hi = pick(POOL_HI, (N, H, W, C))
    hi[..., 0::2] = shared[..., 0::2]
    lo = pick(POOL_LO, (N, H, W, C))
    hi[..., 0:2] = -hi[..., 0:2].abs() - 1.0                 # all-negative windows (the odd border must not see a zero)
    hi[..., 3] = torch.where(hi[..., 3] > 0, 0.0, -0.0)
    lo[..., 3] = hi[..., 3]                                  # (-0) + (-0) = -0, (+0) + (+0) = +0
    hi[..., 2], lo[..., 2] = -0.0, -0.0
    return dict(hi=hi, lo=lo, x3=torch.cat([hi, lo, hi], dim=-1).to(torch.float16))


def pool_expected(inp):
    """The fp32 maximum of hi + lo over the window, re-split; also `loose`: outputs whose window holds +0 and -0 as its maximum (IEEE 754
    leaves the sign of max(-0, +0) open: compared by value)."""
    s = (inp["hi"].to(torch.float32) + inp["lo"].to(torch.float32)).to(F64)          # exact: spans fewer than 24 bits (asserted)
    m = CE.pool_ref(s)[0]
    N, H, W, C = s.shape
    sp = torch.full((N, H + H % 2, W + W % 2, C), float("nan"), dtype=F64)
    sp[:, :H, :W] = s
    wins = torch.stack([sp[:, dh::2, dw::2] for dh in (0, 1) for dw in (0, 1)])
    neg0 = ((wins == 0) & torch.signbit(wins)).any(0)
    pos0 = ((wins == 0) & ~torch.signbit(wins)).any(0)
    loose = (m == 0) & neg0 & pos0
    m = torch.where(m == 0, torch.where(pos0, 0.0, -0.0).to(F64), m)       # a zero maximum is -0 only where the window holds no +0
    return limb_map(m), loose, s


def check_pool_inputs(inp):
    hi, lo = inp["hi"], inp["lo"]
    s64 = hi + lo
    assert is_f32(s64) and normal_or_zero(hi) and normal_or_zero(lo)
    N, H, W, C = hi.shape
    figs = dict(shared_pos=0, shared_neg=0, ties=0, negative=0, zeros=0)
    if H >= 2 and W >= 2:
        h2, w2 = H // 2 * 2, W // 2 * 2
        win = lambda t: torch.stack([t[:, dh:h2:2, dw:w2:2] for dh in (0, 1) for dw in (0, 1)])
        wh, wl, ws = win(hi), win(lo), win(s64)
        same_hi = (wh == wh[0]).all(0) & (wl.max(0)[0] != wl.min(0)[0])
        figs["shared_pos"] = int((same_hi & (wl.max(0)[0] > 0)).sum())
        figs["shared_neg"] = int((same_hi & (wl.max(0)[0] < 0)).sum())
        figs["ties"] = int(((ws == ws.max(0)[0]).sum(0) > 1).sum())
        figs["negative"] = int((ws.max(0)[0] < 0).sum())
        figs["zeros"] = int((ws.max(0)[0] == 0).sum())
    return figs


# ================================================================================================================ D: l2norm
L2_CS = (8, 64, 72, 512, 1024)
U = 2.0 ** -24          # fp32 unit roundoff


def l2_bound(C, limbs_out):
    """Relative bound of the l2norm kernels against float64 on the carried values, composed from the formats:
      input      (float)hi + (float)lo spans fewer than 24 bits: exact (asserted on the inputs); ldexp is exact.  [The limbs' own 2^-22 is the
                 distance of hi + lo from the value they were split from; the reference starts from hi + lo, so it does not enter.]
      sum        a lane adds n = ceil(C / 64) rounded squares in sequence, six shuffle levels follow: s (all terms >= 0) is within (n + 6) U;
                 inv = rsqrt(s) takes half of that
      rsqrt      v_rsq_f32: 1 ulp = 2 U
      multiplies (x inv) gamma: 2 U
      limbs out  hi = half(t) leaves r = t - hi exactly, |r| <= 2^-11 |t|; lo = half(r) is within 2^-11 |r| = 2^-22 |t| = 4 U while lo is
                 normal, within half of half's subnormal step (2^-25, absolute) below
    -> ((n + 6) / 2 + 4 [+ 4]) U relative [+ 2^-25 absolute]: 7.5 U at C = 8 (fp32 output) ... 19 U at C = 1024 (limb output).  The issue caps
    the relative part at 2^-20 = 16 U, so min(composed, 16 U) is asserted: only the limb kernel at C = 1024 (19 U by this worst-case count)
    is held to the cap instead of its own sum."""
    n = -(-C // 64)
    rel = ((n + 6) / 2.0 + 4.0 + (4.0 if limbs_out else 0.0)) * U
    return min(rel, 2.0 ** -20), (2.0 ** -25 if limbs_out else 0.0)


@functools.lru_cache(maxsize=4)
def l2_inputs(M, C, in_exp, seed=51):
    """x of 20 significant bits spread over five binades, its limbs at exponent in_exp, gamma around 10."""
    g = CE.gen(seed + M % 1000 + C + in_exp)
    x = torch.randn((M, C), generator=g, dtype=F64) * torch.logspace(-1, 1.5, C, dtype=F64)
    x = x.to(torch.float32).to(F64)
    gamma = (10 + torch.randn((C,), generator=g, dtype=F64)).to(torch.float32).to(F64)
    hi, lo = limbs(x * 2.0 ** -in_exp)
    carried = (hi + lo) * 2.0 ** in_exp
    return dict(x=x, gamma=gamma, hi=hi, lo=lo, carried=carried)


def l2_ref(v, gamma):
    s = (v * v).sum(-1, keepdim=True).clamp_min(float(torch.tensor(1e-10, dtype=torch.float32)))
    return v / s.sqrt() * gamma


def check_l2_inputs(inp):
    assert is_f32(inp["carried"]) and is_f32(inp["hi"] + inp["lo"])
    assert (inp["carried"] ** 2).sum(-1).min().item() > 1e-6


# ================================================================================================================ E: the fp32 path
F32_CONV_CASES = [
    ("valid_7x9", S(1, 7, 9, 16, 64), "valid"),
    ("taps_3x1_cin20_cout65", S(1, 12, 12, 20, 65, (3, 1)), "same"),
    ("taps_1x3_cin20_cout65", S(1, 12, 12, 20, 65, (1, 3)), "same"),
    ("tile_spans_three_images", S(4, 5, 5, 3, 6), "same"),
    ("m_below_64", S(1, 3, 3, 5, 70), "same"),
    ("stride2_odd", S(2, 9, 7, 24, 64, 3, 2), "same"),
    ("stride2_even", S(2, 10, 8, 24, 64, 3, 2), "same"),
    ("taps_5x5", S(1, 8, 8, 64, 64, 5), "same"),
    ("m_65", S(1, 65, 1, 16, 16, 1), "same"),
]
F32_CONV_VARIANTS = ((True, True, False), (False, False, True), (True, True, True))      # (bias, relu, residual)


@functools.lru_cache(maxsize=2)
def f32_conv_inputs(shape, padding, seed=61):
    N, H, W, Cin, Cout, kh, kw, s = shape
    g = CE.gen(seed + sum(shape))
    x, w, b = CE.small((N, H, W, Cin), g), CE.small((kh, kw, Cin, Cout), g), CE.small((Cout,), g)
    pre = conv_ref(x, w, None, s, padding)
    res = CE.small(tuple(pre.shape), g)
    return dict(x=x, w=w, b=b, res=res, pre=pre, abs=conv_ref(x.abs(), w.abs(), None, s, padding))


def check_f32_conv_inputs(inp):
    assert inp["abs"].max().item() + 16 < 2 ** 24
    v = inp["pre"] + inp["b"]
    assert int((v < 0).sum()) >= 1 and int((v > 0).sum()) >= 1
    return dict(abs=inp["abs"].max().item())


def f32_conv_expected(inp, bias, relu, residual):
    v = inp["pre"] + (inp["b"] if bias else 0.0)
    v = torch.relu(v) if relu else v
    return v + inp["res"] if residual else v


LAYER_SHAPES = [(1, 1, 1, 3), (2, 7, 5, 5), (1, 33, 47, 64)]
LOOP_CAP = 16384 * 256          # outputs one trip of a layer kernel's grid-stride loop covers (f32_blocks)
MAXPOOL_LOOP = (1, 513, 513, 64)       # 257 * 257 * 64 = 4 227 136 outputs
AVGPOOL_LOOP = (1, 257, 257, 64)
RESIZE_LOOP = ((1, 129, 129, 64), 2)   # -> 258 x 258 x 64 = 4 260 096 outputs


def maxpool_inputs(shape, seed=71):
    """Small integers; channel 0 negative everywhere: at an odd border the window's missing elements must not count as 0."""
    x = CE.small(shape, CE.gen(seed + sum(shape))).to(torch.float32)
    x[..., 0] = -x[..., 0].abs() - 1
    return x


def avgpool_inputs(shape, seed=73):
    """Multiples of 1/4 up to +-64: a sum of 1, 2 or 4 taps and its division by 1, 2 or 4 are exact."""
    return (CE.small(shape, CE.gen(seed + sum(shape)), -256, 256) / 4).to(torch.float32)


def avgpool_ref(x):
    """tf.layers.average_pooling2d((2,2), 1, 'same'): pad (0, 1), divisor = number of valid taps."""
    N, H, W, C = x.shape
    xp = torch.zeros((N, H + 1, W + 1, C), dtype=x.dtype)
    xp[:, :H, :W] = x
    ones = torch.zeros((1, H + 1, W + 1, 1), dtype=x.dtype)
    ones[:, :H, :W] = 1
    tap = lambda t: t[:, :-1, :-1] + t[:, :-1, 1:] + t[:, 1:, :-1] + t[:, 1:, 1:]
    return tap(xp) / tap(ones)


def resize_coords(n_in, n_out):
    """The kernel's own source coordinates in fp32: f = (float)i * ((float)in / (float)out), i0 = floor, i1 = min(i0 + 1, in - 1), l = f - i0."""
    sc = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    f = torch.arange(n_out, dtype=torch.float32) * sc
    i0 = torch.floor(f)
    return i0.long(), torch.clamp(i0.long() + 1, max=n_in - 1), (f - i0).to(F64)


def resize_ref(up, Ho, Wo, lat=None):
    """TF1 legacy bilinear resize in float64 at those coordinates, rows blended along x first; also the largest corner magnitude per output."""
    up = up.to(F64)
    y0, y1, ly = resize_coords(up.shape[1], Ho)
    x0, x1, lx = resize_coords(up.shape[2], Wo)
    lx, ly = lx.view(1, 1, -1, 1), ly.view(1, -1, 1, 1)
    tl, tr, bl, br = up[:, y0][:, :, x0], up[:, y0][:, :, x1], up[:, y1][:, :, x0], up[:, y1][:, :, x1]
    top, bot = tl + (tr - tl) * lx, bl + (br - bl) * lx
    v = top + (bot - top) * ly
    scale = torch.stack([tl.abs(), tr.abs(), bl.abs(), br.abs()]).max(0)[0]
    return (v if lat is None else lat.to(F64) + v), scale


def resize_inputs(shape, seed=79):
    """Multiples of 1/8 up to +-32: with weights in quarters (ratios 2 and 4) every product and sum is exact in fp32."""
    return (CE.small(shape, CE.gen(seed + sum(shape)), -256, 256) / 8).to(torch.float32)


# ================================================================================================================ runners (GPU)
assert_equal = CE.assert_equal


def assert_same_halves(got, want, what, loose=None):
    """Bit for bit on the raw halves (so that -0 and +0 differ); loose: elements compared by value instead."""
    got = got.detach().cpu().contiguous()
    want = want.reshape(got.shape).contiguous()
    g, w = got.view(torch.int16), want.view(torch.int16)
    bad = g != w
    if loose is not None:
        bad &= ~(loose & (got == want))
    if not bad.any():
        return
    idx = bad.nonzero()
    first = [(tuple(i.tolist()), got[tuple(i)].item(), want[tuple(i)].item()) for i in idx[:6]]
    raise AssertionError("%s: %d of %d halves differ, first (index, got, want): %s" % (what, idx.shape[0], got.numel(), first))


class Api:
    def __init__(self, dev):
        from dan_amd import _lib, ops
        from test_conv_dispatch_gpu import in_family
        self.dev, self.lib, self.ops, self.in_family = dev, _lib, ops, in_family
        self.L16 = _lib.lib_f16()
        self.cus = torch.cuda.get_device_properties(dev).multi_processor_count
        ops._range_flag(dev)
        ops.split_range_reset()          # (a flag an earlier, failed test left raised is not this test's)

    def last_label(self):
        return self.L16.danhip_conv_last_launch_label().decode()

    def f32(self, t):
        return None if t is None else t.to(torch.float32).to(self.dev).contiguous()

    def range_ok(self):
        self.ops.split_range_check()


def run_split_case(api, case):
    """Every class and variant of one case through ops.conv2d under SPLIT_EVAL; returns the set of (label, splits) launched."""
    cid, shp, opts, family, extra = case
    o = case_opts(case)
    N, H, W, C, Cout, kh, kw, s = shp
    ops = api.ops
    plan = plan_split_call(shp, not o["f32"], o["padding"], api.cus)
    if extra == "splitk":
        assert plan["splits"] >= 2 and plan["ws_bytes"] > 0, (cid, plan)
        if o["padding"] == "same":
            assert CE.plan_splitk(plan["limb_shape"], 0, api.cus)[0] >= 2
    d3 = ops._desc(*plan["limb_shape"], o["padding"] == "valid")
    nws = api.L16.danhip_conv2d_workspace_bytes(ctypes.byref(d3), 0)
    assert nws == plan["query_bytes"], (cid, nws, plan)
    launched = set()
    for cls in CLASSES:
        inp = split_inputs(shp, cls, o["padding"])
        check_split_inputs(inp)
        x, w, b, res = api.f32(inp["x"]), api.f32(inp["w"]), api.f32(inp["b"]), api.f32(inp["res"])
        for bias, relu in SPLIT_VARIANTS:
            what = "%s class %s bias=%d relu=%d" % (cid, cls, bias, relu)
            with ops.use_context(ops.OpsContext(SPLIT_EVAL=True)), torch.no_grad():
                y = ops.conv2d(x, w, b if bias else None, stride=s, relu=relu, out_f32=o["f32"] and not o["res"], residual=res if o["res"] else None,
                               padding=o["padding"])
            torch.cuda.synchronize()
            got = api.last_label()
            assert got == plan["label"] and api.in_family(got, family), "%s: launched %s, restated %s, listed %s" % (what, got, plan["label"], family)
            launched.add((got, plan["splits"]))
            want = split_expected(inp, bias, relu, o["res"], not o["f32"])
            if o["f32"]:
                assert y.dtype == torch.float32 and not ops._is_limbs(y)
                assert_equal(y, want, what)
            else:
                assert ops._is_limbs(y) and y._dh_exp == LIMB_EXP and y.dtype == torch.float16 and tuple(y.shape) == tuple(want.shape[:-1]) + (Cout,)
                assert_same_halves(y._dh_split3, want, what)
            api.range_ok()
    return launched


def run_chain(api, cls):
    inp = chain_inputs(cls)
    check_chain_inputs(inp)
    ops = api.ops
    st = inp["stages"]
    ws, bs = [api.f32(w) for w in inp["ws"]], [api.f32(b) for b in inp["bs"]]
    with ops.use_context(ops.OpsContext(SPLIT_EVAL=True)), torch.no_grad():
        y1 = ops.conv2d(api.f32(inp["x"]), ws[0], bs[0], relu=True)
        assert ops._is_limbs(y1) and y1._dh_exp == LIMB_EXP
        assert_same_halves(y1._dh_split3, limb_map(st[0]["v"] * 2.0 ** -LIMB_EXP), "chain %s stage 1" % cls)
        y2 = ops.conv2d(y1, ws[1], bs[1], relu=True)
        assert ops._is_limbs(y2) and y2._dh_exp == LIMB_EXP
        assert_same_halves(y2._dh_split3, limb_map(st[1]["v"] * 2.0 ** -LIMB_EXP), "chain %s stage 2" % cls)
        p = ops.max_pool_2x2(y2)
        assert ops._is_limbs(p) and p._dh_exp == LIMB_EXP
        assert_same_halves(p._dh_split3, limb_map(CE.pool_ref(st[1]["v"])[0] * 2.0 ** -LIMB_EXP), "chain %s pool" % cls)
        y3 = ops.conv2d(p, ws[2], bs[2], relu=False, out_f32=True)
    assert y3.dtype == torch.float32
    assert_equal(y3, st[2]["v"], "chain %s head" % cls)
    api.range_ok()

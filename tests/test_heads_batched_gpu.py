"""danhip_heads_split_fwd / danhip_heads_grad_pad (all pyramid levels of the detection heads in one launch each way) against the per-level
entry points they replace, on the same inputs: danhip_head_split_fwd, and danhip_head_split_bwd -> danhip_cast_pad_f32_to_bf16.  The
reference is never the new code, every comparison is torch.equal (16-bit tensors by their bit patterns), in the bf16 and the fp16 build.

Level sets: four levels whose row counts are no multiple of 64 (A = 55), a single 1 x 1 level, a full table of eight levels handed over
in another order than their anchor offsets (rows of 6, 7, 8 and 10 channels, co_pad 8 and 16: every load form of the gradient kernel),
and one set whose row count makes the capped grid take a second, partial trip (the cap is read from loss.hip).  Inputs: random floats;
small integers, so that every combination of tied maxima occurs in every group; +-inf, values beyond the fp16 range and values on the
16-bit rounding boundaries in dloc / dcls.  Pad columns are zero, canaries around every destination stay untouched, malformed tables are
refused with DANHIP_EINVAL, and one training step of S3FD, PyramidBox and DAN gives the same head dY bits with the switch on and off."""
import ctypes
import functools
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gradcheck as GC  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
GUARD = 64                      # canary elements on either side of a destination (keeps it 16-byte aligned)
CANARY32, CANARY16 = 12345.0, 0x7B7B

# (H, W, nneg, npos, co_pad) per level
FOUR = (2, [(5, 7, 3, 1, 8), (3, 3, 1, 1, 8), (1, 1, 1, 1, 8), (2, 5, 1, 3, 8)])
ONE = (1, [(1, 1, 1, 1, 8)])
EIGHT = (2, [(5, 7, 3, 1, 8), (3, 3, 1, 1, 8), (1, 1, 1, 1, 8), (2, 5, 1, 3, 8), (4, 4, 2, 1, 8), (3, 5, 3, 3, 16), (2, 2, 1, 1, 16), (6, 1, 2, 2, 8)])
SETS = {"four": FOUR, "one": ONE, "eight": EIGHT}


def _trip():
    src = open(os.path.join(ROOT, "dan_amd", "csrc", "loss.hip")).read()
    cap = int(re.search(r"heads_grad_pad_kernel, dim3\(dh_grid_for\(rows, 256, (\d+)\)\), dim3\(256\)", src).group(1))
    assert "heads_split_fwd_kernel, dim3(dh_grid_for(rows, 256, %d)), dim3(256)" % cap in src
    return cap * 256


def _build(name):
    """-> (library, 16-bit torch dtype) of the bf16 / fp16 build; both load into one process."""
    from dan_amd import _lib
    bf = _lib.ACT_NAME == "bf16"
    if name == "bf16":
        return (_lib.lib() if bf else _lib._load(os.path.join(os.path.dirname(_lib.SO_PATH), "libdanhip.so"), "bf16")), torch.bfloat16
    return _lib.lib_f16(), torch.float16


def _ptr(t, elems=0):
    return ctypes.c_void_p(t.data_ptr() + t.element_size() * elems)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(L, rc):
    assert rc == 0, L.danhip_last_error().decode()


@functools.lru_cache(maxsize=None)
def _inputs(set_name, kind):
    """CPU inputs of one case: ([h per level], dloc [B,A,4], dcls [B,A,2], offsets, permutation of the table)."""
    if set_name == "two-trips":
        trip = _trip()
        B, specs = 33, [(160, 160, 3, 1, 8), (79, 81, 1, 1, 8)]
        rows = B * sum(s[0] * s[1] for s in specs)
        assert trip < rows < 2 * trip and (rows - trip) % 256 != 0, (rows, trip)
    else:
        B, specs = SETS[set_name]
    g = torch.Generator().manual_seed(len(specs) * 7 + {"random": 0, "ties": 1, "edges": 2}[kind])
    A = sum(s[0] * s[1] for s in specs)
    hs = []
    for H, W, nneg, npos, _ in specs:
        shape = (B, H, W, 4 + nneg + npos)
        if kind == "random":
            h = torch.randn(shape, generator=g)
        else:                   # values from {-1, 0, 1}: every pattern of tied maxima in groups of up to three channels, -0.0 among them
            h = torch.randint(-1, 2, shape, generator=g).float()
            h = torch.where((h == 0) & (torch.rand(shape, generator=g) < 0.3), torch.tensor(-0.0), h)
        hs.append(h)
    dloc, dcls = torch.randn((B, A, 4), generator=g), torch.randn((B, A, 2), generator=g)
    if kind == "edges":
        inf = float("inf")
        # +-inf, the largest floats, beyond the fp16 range (65504) and its rounding boundary 65520, bf16 ties (1 + 2^-8: round to even,
        # 1 + 3 * 2^-8), the fp16 tie 1 + 2^-11, fp16 subnormals and values that divide by a tie count of 2 or 3 onto a boundary
        vals = torch.tensor([inf, -inf, 3.4028234663852886e38, -3.4028234663852886e38, 3.3e38, 65504.0, 65519.99, 65520.0, -65520.0, 70000.0, 1e30, -1e30,
                             1.00390625, 1.01171875, 1.00048828125, 2.0 * 1.00390625, 3.0 * 1.00390625, 6e-8, 2.98e-8, -5.96e-8, 1e-40, -0.0, 0.0, 1e-45])
        pick = lambda shape: vals[torch.randint(0, len(vals), shape, generator=g)]
        dloc = torch.where(torch.rand(dloc.shape, generator=g) < 0.7, pick(dloc.shape), dloc)
        dcls = torch.where(torch.rand(dcls.shape, generator=g) < 0.7, pick(dcls.shape), dcls)
    n = len(specs)
    perm = list(range(n)) if set_name != "eight" else [5, 2, 7, 0, 3, 6, 1, 4]       # table order != anchor order
    offs, off = [], 0
    for s in specs:
        offs.append(off)
        off += s[0] * s[1]
    return B, A, specs, hs, dloc, dcls, offs, perm


def _guarded(shape, dtype, dev, skew=0):
    """A destination of `shape` inside a buffer with GUARD (+ skew) canary elements in front and GUARD behind, the destination itself
    canary-filled too.  skew = 2 (fp32): a destination that is 8-byte but not 16-byte aligned, as a batch slice of cls [B, A, 2] is."""
    n = 1
    for s in shape:
        n *= s
    if dtype == torch.float32:
        buf = torch.full((n + 2 * GUARD + skew,), CANARY32, dtype=torch.float32, device=dev)
    else:
        buf = torch.full((n + 2 * GUARD + skew,), CANARY16, dtype=torch.int16, device=dev).view(dtype)
    return buf, buf[GUARD + skew:GUARD + skew + n].view(shape)


def _guards_intact(buf):
    raw = buf if buf.dtype == torch.float32 else buf.view(torch.int16)
    want = CANARY32 if buf.dtype == torch.float32 else CANARY16
    return bool((raw[:GUARD] == want).all()) and bool((raw[-GUARD:] == want).all())


def _table(specs, hs, dys, offs, perm):
    from dan_amd import _lib
    tab = (_lib.HeadLevel * len(perm))()
    for e, i in zip(tab, perm):
        H, W, nneg, npos, co_pad = specs[i]
        e.h, e.dy = hs[i].data_ptr(), (dys[i].data_ptr() if dys is not None else None)
        e.HW, e.Ch, e.nneg, e.npos, e.off, e.co_pad = H * W, 4 + nneg + npos, nneg, npos, offs[i], co_pad
    return tab


def _run_case(build, set_name, kind, dev):
    L, dt = _build(build)
    B, A, specs, hs, dloc, dcls, offs, perm = _inputs(set_name, kind)
    hs = [h.to(dev) for h in hs]
    dloc = dloc.to(dev)
    dcls_buf = torch.zeros(dcls.numel() + 2, dtype=torch.float32, device=dev)              # dcls 8-byte aligned only
    dcls_buf[2:].copy_(dcls.reshape(-1))
    dcls = dcls_buf[2:].view(dcls.shape)
    assert dcls.data_ptr() % 16 == 8 and dcls.is_contiguous()
    s = _stream()
    # ---- reference: the per-level entry points
    loc_ref = torch.zeros((B, A, 4), dtype=torch.float32, device=dev)
    cls_ref = torch.zeros((B, A, 2), dtype=torch.float32, device=dev)
    dy_ref = []
    for (H, W, nneg, npos, co_pad), h, off in zip(specs, hs, offs):
        Ch = 4 + nneg + npos
        _ok(L, L.danhip_head_split_fwd(_ptr(h), _ptr(loc_ref), _ptr(cls_ref), B, H * W, Ch, nneg, npos, A, off, s))
        dy32 = torch.empty((B * H * W, Ch), dtype=torch.float32, device=dev)
        _ok(L, L.danhip_head_split_bwd(_ptr(h), _ptr(dloc), _ptr(dcls), _ptr(dy32), B, H * W, Ch, nneg, npos, A, off, s))
        d16 = torch.full((B * H * W, co_pad), CANARY16, dtype=torch.int16, device=dev).view(dt)
        _ok(L, L.danhip_cast_pad_f32_to_bf16(_ptr(dy32), None, _ptr(d16), B * H * W, Ch, co_pad, s))
        dy_ref.append(d16)
    # ---- the batched kernels, every destination between canaries
    loc_buf, loc = _guarded((B, A, 4), torch.float32, dev)
    cls_buf, cls = _guarded((B, A, 2), torch.float32, dev, skew=2)
    assert cls.data_ptr() % 16 == 8
    dy_bufs, dys = zip(*[_guarded((B * sp[0] * sp[1], sp[4]), dt, dev) for sp in specs])
    tab = _table(specs, hs, dys, offs, perm)
    _ok(L, L.danhip_heads_split_fwd(tab, len(perm), _ptr(loc), _ptr(cls), B, A, s))
    _ok(L, L.danhip_heads_grad_pad(tab, len(perm), _ptr(dloc), _ptr(dcls), B, A, s))
    torch.cuda.synchronize()
    assert torch.equal(loc, loc_ref) and torch.equal(cls, cls_ref), (build, set_name, kind)
    assert _guards_intact(loc_buf) and _guards_intact(cls_buf)
    for i, (sp, got, want, buf) in enumerate(zip(specs, dys, dy_ref, dy_bufs)):
        Ch = 4 + sp[2] + sp[3]
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (build, set_name, kind, "level %d" % i)
        assert bool((got.view(torch.int16)[:, Ch:] == 0).all()), "pad columns of level %d" % i
        assert _guards_intact(buf), "canaries of level %d" % i
    return dys, specs


@pytest.mark.parametrize("build", ["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["random", "ties", "edges"])
@pytest.mark.parametrize("set_name", ["four", "one", "eight"])
def test_batched_heads_are_the_per_level_kernels(set_name, kind, build, dev):
    dys, specs = _run_case(build, set_name, kind, dev)
    if kind == "edges" and set_name != "one":      # the edge values reached the 16-bit rounding: infinities among the outputs
        assert any(bool(torch.isinf(d.float()).any()) for d in dys)


def test_tie_inputs_hold_every_tie_count():
    """(no kernel: the 'ties' inputs) each group of two and three channels meets every count of tied maxima."""
    B, A, specs, hs, _, _, _, _ = _inputs("eight", "ties")
    seen = set()
    for (H, W, nneg, npos, _), h in zip(specs, hs):
        for s, n in ((4, nneg), (4 + nneg, npos)):
            grp = h[..., s:s + n]
            cnt = (grp == grp.amax(-1, keepdim=True)).sum(-1)
            seen |= {(n, int(c)) for c in cnt.unique()}
    assert {(2, 1), (2, 2), (3, 1), (3, 2), (3, 3)} <= seen, seen


@pytest.mark.parametrize("build", ["bf16", "fp16"])
def test_batched_heads_past_the_launch_cap(build, dev):
    _run_case(build, "two-trips", "ties", dev)


def test_malformed_tables_are_refused(dev):
    from dan_amd import _lib
    L = _lib.lib()
    B, A, specs, hs, dloc, dcls, offs, perm = _inputs("four", "random")
    hs = [h.to(dev) for h in hs]
    dloc, dcls = dloc.to(dev), dcls.to(dev)
    loc, cls = torch.zeros((B, A, 4), device=dev), torch.zeros((B, A, 2), device=dev)
    dys = [torch.zeros((B * sp[0] * sp[1], 16), dtype=torch.int16, device=dev) for sp in specs]
    s = _stream()

    def both(tab, n, fwd_too=True, what=b""):
        rcs = [L.danhip_heads_grad_pad(tab, n, _ptr(dloc), _ptr(dcls), B, A, s)]
        msg = L.danhip_last_error()
        if fwd_too:
            rcs.append(L.danhip_heads_split_fwd(tab, n, _ptr(loc), _ptr(cls), B, A, s))
        assert all(rc == EINVAL for rc in rcs) and what in msg, (rcs, msg)

    good = lambda: _table(specs, hs, dys, offs, perm)
    tab = good()
    _ok(L, L.danhip_heads_grad_pad(tab, 4, _ptr(dloc), _ptr(dcls), B, A, s))               # the well-formed table passes
    for d in dys:
        d.zero_()
    nine = (_lib.HeadLevel * 9)()
    for i in range(9):                                                                     # nine 1 x 1 levels tiling [0, 9)
        nine[i].h, nine[i].dy = hs[2].data_ptr(), dys[2].data_ptr()
        nine[i].HW, nine[i].Ch, nine[i].nneg, nine[i].npos, nine[i].off, nine[i].co_pad = 1, 6, 1, 1, i, 8
    rc = L.danhip_heads_grad_pad(nine, 9, _ptr(dloc), _ptr(dcls), B, 9, s)
    assert rc == EINVAL and b"levels" in L.danhip_last_error()
    assert L.danhip_heads_split_fwd(nine, 9, _ptr(loc), _ptr(cls), B, 9, s) == EINVAL
    both(tab, 0, what=b"levels")
    tab = good(); tab[1].Ch = 7
    both(tab, 4, what=b"4 + nneg + npos")
    tab = good(); tab[0].co_pad = 0                                                          # co_pad < Ch
    both(tab, 4, fwd_too=False, what=b"co_pad")
    tab = good(); tab[0].co_pad = 12                                                         # not a multiple of 8
    both(tab, 4, fwd_too=False, what=b"co_pad")
    tab = good(); tab[1].off -= 1                                                            # overlaps level 0
    both(tab, 4, what=b"tile")
    tab = good(); tab[3].off += 1                                                            # a gap (and past A)
    both(tab, 4)
    tab = good(); tab[1].off, tab[3].off = tab[3].off, tab[1].off                            # swapped offsets of levels of unequal size
    both(tab, 4, what=b"tile")
    both(good(), 3)                                                                         # the levels end before A
    tab = good(); tab[2].h = None
    both(tab, 4, what=b"null")
    tab = good(); tab[2].dy = None
    both(tab, 4, fwd_too=False, what=b"null")
    tab = good()
    assert L.danhip_heads_grad_pad(tab, 4, None, _ptr(dcls), B, A, s) == EINVAL and L.danhip_heads_grad_pad(tab, 4, _ptr(dloc), None, B, A, s) == EINVAL
    assert L.danhip_heads_split_fwd(tab, 4, None, _ptr(cls), B, A, s) == EINVAL and L.danhip_heads_split_fwd(tab, 4, _ptr(loc), None, B, A, s) == EINVAL
    assert L.danhip_heads_grad_pad(None, 4, _ptr(dloc), _ptr(dcls), B, A, s) == EINVAL
    assert L.danhip_heads_grad_pad(tab, 4, _ptr(dloc, 2), _ptr(dcls), B, A, s) == EINVAL and b"aligned" in L.danhip_last_error()     # dloc at 8 bytes
    assert L.danhip_heads_grad_pad(tab, 4, _ptr(dloc), _ptr(dcls, 1), B, A, s) == EINVAL and L.danhip_heads_split_fwd(tab, 4, _ptr(loc), _ptr(cls, 1), B, A, s) == EINVAL
    torch.cuda.synchronize()
    assert all(bool((d == 0).all()) for d in dys) and bool((loc == 0).all()) and bool((cls == 0).all()), "a refused call wrote something"


def _one_step(which, batched, dev):
    """One training step of `which` (64 x 64, B = 2) from the seeded state -> (head dY tensors in backward order, gradients per variable)."""
    from dan_amd import ops, synthetic
    H = W = 64
    model, flat, ofwd, P, imgs, x = GC.setup(which, H, W, 2, dev, torch.bfloat16, seed=11)
    gts = synthetic.make_gt_boxes(2, H, W, seed=2, max_faces=4)
    prev = ops.HEADS_BATCHED
    ops.HEADS_BATCHED = batched
    try:
        if which == "pb":
            from dan_amd.train_pb import PBAnchorTargets, PBTrainer
            tr = PBTrainer(model, world=1)
            args = (imgs.to(dev), PBAnchorTargets(H, W, dev).encode_batch(gts))
        elif which == "sfd":
            from dan_amd.train_sfd import AnchorConfig, SFDTrainer
            tr = SFDTrainer(model, world=1)
            loc_t, cls_t, _ = AnchorConfig(H, W, dev).encode_batch(gts)
            args = (imgs.to(dev), loc_t, cls_t)
        else:
            from dan_amd.train_dan import DANTrainer, dan_anchor_config, encode_batch_dan
            anchors = dan_anchor_config(H, W, dev)
            tr = DANTrainer(model, anchors, world=1)
            args = (imgs.to(dev),) + tuple(encode_batch_dan(anchors, gts))
        tr.ops_ctx.HEADS_BATCHED = batched
        ops.TRACE = {}
        try:
            tr.train_step(*args)
            rec = ops.TRACE
        finally:
            ops.TRACE = None
        torch.cuda.synchronize()
    finally:
        ops.HEADS_BATCHED = prev
    grads = {n: (p.grad.detach().float().cpu() if p.grad is not None else None) for n, p in model.vs.named()}
    return [t.clone() for t in rec.get("head_dy", [])], grads


@pytest.mark.parametrize("which", ["sfd", "dan", "pb"])
def test_train_step_head_gradients_do_not_depend_on_the_switch(which, dev):
    dy_on, g_on = _one_step(which, True, dev)
    dy_off, g_off = _one_step(which, False, dev)
    assert len(dy_on) == len(dy_off) >= 6, (len(dy_on), len(dy_off))
    for i, (a, b) in enumerate(zip(dy_on, dy_off)):
        assert a.dtype == b.dtype and a.dtype != torch.float32 and a.shape == b.shape and a.shape[-1] % 8 == 0
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (which, "head dY %d" % i)
    assert any(bool((a != 0).any()) for a in dy_on)
    # the flat gradients hold atomically summed weight gradients: the bound tests/test_grad_parity_gpu.py sets between two routes through the
    # same kernels
    bad, checked = GC.compare(g_on, g_off, 0.03)
    assert checked > 30 and not bad, (which, checked, bad[:10])

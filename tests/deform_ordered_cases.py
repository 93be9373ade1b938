"""Cases and references for the ordered far-corner path of the deformable backward (csrc/deform_far.hip, csrc/deform_far.h; the order contract is
in include/danhip.h).  Shared by tests/test_deform_ordered_cpu.py and tests/test_deform_ordered_gpu.py.  Nothing here needs a GPU.

Two families of cases:
  * the dyadic cases of tests/deform_exact.py that belong to the ordered shape class (3 x 3, dilation 1, C / dg == 64): every sum is exact in
    fp32 in any order, so they show that every term is counted once - not in which order;
  * ORDER cases (below): L sources sent onto one interior destination by INTEGER offsets of at least 3 px.  The sample then sits on the
    destination pixel: corner 0 has weight exactly 1, the other three are rejected by corner_set's |position - corner| < 1 guard, so a source
    is exactly one record (k = 0) whatever the window is, and the destination's fp32 sum is the plain sequential sum of the sources' dS rows
    in ascending (m, t).  Every other offset is 0 and every other dS row is 0: the gather part of dX is exactly 0 and dX = round16(0 + F).
    dS values are +-(1 + j / 128) 2^e (exact in bf16 and in fp16), e in [-8, 8]: large ones come in +- pairs that cancel, so the rounding an
    fp32 partial sum suffers near 2^9 survives into a result near 2^-7, where it is worth half a 16-bit ulp - ascending and descending order
    give different 16-bit outputs, which order_expected() lets a test assert before it looks at a device.
"""
import collections
import ctypes
import functools

import numpy as np
import torch

import deform_exact as DE

# ---- the dyadic cases inside the ordered shape class; 8 x 16 is exactly one tile, 9 x 17 one past it in each direction, with dg 1 and 4, N = 2
EXACT_NAMES = [c.name for c in DE.CASES if c.C // c.dg == 64 and c.dil == 1]
assert {"c64_8x16_c64_dg1", "c64_8x16_c256_dg4", "c64_9x17_c64_dg1", "c64_9x17_c256_dg4"} <= set(EXACT_NAMES)
assert all(DE.CASE_BY_NAME[n].N == 2 for n in EXACT_NAMES)

# ---- order cases
LANES = 8                                     # DH_FAR_LANES: the stride of the sum kernel's key search, the one chunk size along a segment
ORDER_L = (1, 2, 7, 8, 9, 64, 65, 300)        # the issue's lengths + one below, at and one above LANES
OH, OW, ODG = 36, 60, 2                       # 4320 destinations: three workgroups of the prefix sum (2048 each), the last one partial
OC = 64 * ODG
DESTS = ((5, 7), (20, 31), (33, 50), (20, 32))          # interior pixels spread over the prefix sum's workgroups; the last is the second's neighbour
OrderCase = collections.namedtuple("OrderCase", "L off dS records shared")


def _values(rng, n):
    """n values +-(1 + j / 128) 2^e for the 64 channels of one destination -> float32 [n, 64]: n // 3 cancelling +- pairs and small values,
    in shuffled positions per channel.  Even channels are SPREAD (pairs with e in [0, 8] and either sign, small values with e in [-8, -3]);
    odd channels are TIGHT (every pair +(..) 2^8 and its negative, small values with e in {-8, -7} and odd j): two of the large values
    lift the partial sum to 2^9, where fp32 drops the 2^-15 bit of a small value that arrives then - and keeps it when the small value
    arrives before or after the large ones, as it does in the opposite order."""
    out = np.zeros((n, 64), np.float32)
    pairs, ns = n // 3, n - 2 * (n // 3)
    for ch in range(64):
        if ch % 2:
            big = (1.0 + rng.integers(0, 128, pairs) / 128.0) * 256.0
            small = (1.0 + (2 * rng.integers(0, 64, ns) + 1) / 128.0) * np.exp2(rng.integers(-8, -6, ns)) * rng.choice([-1.0, 1.0], ns)
        else:
            big = (1.0 + rng.integers(0, 128, pairs) / 128.0) * np.exp2(rng.integers(0, 9, pairs)) * rng.choice([-1.0, 1.0], pairs)
            small = (1.0 + rng.integers(0, 128, ns) / 128.0) * np.exp2(rng.integers(-8, -2, ns)) * rng.choice([-1.0, 1.0], ns)
        v = np.concatenate([big, -big, small]).astype(np.float32)
        out[:, ch] = v[rng.permutation(n)]
    return out


@functools.lru_cache(maxsize=None)
def order_case(L):
    """N = 1, 36 x 60, C = 128, dg = 2.  Destinations (per group): DESTS[0] receives exactly L sources, DESTS[1] max(1, L // 2), DESTS[2] min(L, 3), DESTS[3] 1.
    The first pixel drawn sends tap 0 to DESTS[0] and tap 1 to DESTS[1] (two destinations that share a source pixel; asserted).
    -> off float32 [1,H,W,dg*18], dS float32 [H*W, 9*C], records {(h, w, grp): [(m, t, k), ...] ascending}, shared (bool)."""
    rng = np.random.default_rng(7000 + L)
    H, W, dg, C = OH, OW, ODG, OC
    off = np.zeros((H * W, dg, 9, 2), np.float32)
    dS = np.zeros((H * W, 9, C), np.float32)
    records = {}
    lens = (L, max(1, L // 2), min(L, 3), 1)
    shared = False
    for grp in range(dg):
        order = rng.permutation(H * W * 9)
        p0 = int(order[0]) // 9
        head = [p0 * 9 + 0, p0 * 9 + 1]                                   # the same pixel's taps 0 and 1 open the lists of DESTS[0] and DESTS[1]
        rest = [int(s) for s in order if int(s) not in head]
        used = 0
        for di, ((dh, dw), n) in enumerate(zip(DESTS, lens)):
            cand = [head[di]] if di < 2 else []
            kept = []
            while len(kept) < n:
                if cand:
                    s = cand.pop()
                else:
                    s = rest[used]
                    used += 1
                m, t = divmod(s, 9)
                nh, nw = m // W - 1 + t // 3, m % W - 1 + t % 3
                oh, ow = dh - nh, dw - nw
                if max(abs(oh), abs(ow)) < 3:                               # not far in the +-2 window: leave the tap alone (its offset stays 0)
                    continue
                assert off[m, grp, t, 0] == 0 and off[m, grp, t, 1] == 0
                off[m, grp, t] = (oh, ow)
                kept.append((m, t, 0))
            kept.sort()
            vals = _values(rng, len(kept))
            for i, (m, t, _) in enumerate(kept):
                dS[m, t, grp * 64:(grp + 1) * 64] = vals[i]
            records[(dh, dw, grp)] = kept
        a = {m for m, _, _ in records[(DESTS[0][0], DESTS[0][1], grp)]}
        b = {m for m, _, _ in records[(DESTS[1][0], DESTS[1][1], grp)]}
        shared = shared or bool(a & b)
    assert np.abs(off).max() < 256 and np.array_equal(off, np.round(off))
    return OrderCase(L, off.reshape(1, H, W, dg * 18), dS.reshape(H * W, 9 * C), records, shared)


def order_far_dx(case, descending=False):
    """The contract's F for every element of far_dx, by a plain loop over the records with an np.float32 running sum -> float32 [1,H,W,C]."""
    F = np.zeros((1, OH, OW, OC), np.float32)
    dS = case.dS.reshape(OH * OW, 9, OC)
    for (h, w, grp), recs in case.records.items():
        acc = np.zeros(64, np.float32)
        for (m, t, _k) in (reversed(recs) if descending else recs):
            acc = (acc + np.float32(1.0) * dS[m, t, grp * 64:(grp + 1) * 64]).astype(np.float32)       # (weight exactly 1: product and fma agree)
        F[0, h, w, grp * 64:(grp + 1) * 64] = acc
    return F


def order_expected(case, dtype, descending=False):
    """dX of the case in the 16-bit type `dtype`: round(0 + F) (the gather sum is exactly 0: every dS row of a near source is 0)."""
    return torch.from_numpy(np.float32(0.0) + order_far_dx(case, descending)).to(dtype)


# ---- far records of ANY offsets, by corner_set restated in numpy float32 (for counting records in the dyadic cases)
def far_record_count(off, H, W, dg, R):
    """Number of far records under window R: off float [N,H,W,dg*18]."""
    o = np.asarray(off, np.float32).reshape(-1, H, W, dg, 9, 2)
    t = np.arange(9)
    nh = (np.arange(H).reshape(1, H, 1, 1, 1) - 1 + (t // 3).reshape(1, 1, 1, 1, 9)).astype(np.int64)
    nw = (np.arange(W).reshape(1, 1, W, 1, 1) - 1 + (t % 3).reshape(1, 1, 1, 1, 9)).astype(np.int64)
    ih = (nh.astype(np.float32) + o[..., 0]).astype(np.float32)
    iw = (nw.astype(np.float32) + o[..., 1]).astype(np.float32)
    inside = ~((ih < 0) | (ih > H) | (iw < 0) | (iw > W))
    ah, aw = np.where(inside, np.maximum(ih, 0), 0), np.where(inside, np.maximum(iw, 0), 0)
    hl, wl = ah.astype(np.int64), aw.astype(np.int64)
    ch, cw = hl >= H - 1, wl >= W - 1
    hl, wl = np.where(ch, H - 1, hl), np.where(cw, W - 1, wl)
    hh, wh = np.where(ch, hl, hl + 1), np.where(cw, wl, wl + 1)
    total = 0
    for rh, rw, dup in ((hl, wl, np.zeros_like(ch)), (hl, wh, cw), (hh, wl, ch), (hh, wh, ch | cw)):
        ok = inside & ~dup & (np.abs(ih - rh) < 1) & (np.abs(iw - rw) < 1) & (rh >= 0) & (rh < H) & (rw >= 0) & (rw < W)
        far = (np.abs(rh - nh) > R) | (np.abs(rw - nw) > R)
        total += int((ok & far).sum())
    return total


def window_of(off, dg):
    """The gather window deterministic mode picks: +-1 while at most pairs / 128 offset pairs leave [-1, 1), else +-2."""
    p = np.asarray(off, np.float32).reshape(-1, 2)
    stat1 = int(((p < -1) | (p >= 1)).any(axis=1).sum())
    return 1 if stat1 <= p.shape[0] // 128 else 2


# ---- the host emulation (needs the library, no GPU)
GUARD = 64


def act_dtype():
    from dan_amd import _lib
    return torch.float16 if _lib.ACT_NAME == "fp16" else torch.bfloat16


def emulate16(off16, dS16, N, H, W, C, dg, window=0):
    """danhip_deform_far_ordered_emulate on CPU tensors of the build's 16-bit type -> (far_dx float32 [N,H,W,C], records, range_errors).
    far_dx sits between GUARD-word guards, which must come back untouched."""
    from dan_amd import _lib
    L = _lib.lib()
    assert off16.dtype == act_dtype() and dS16.dtype == act_dtype() and off16.is_contiguous() and dS16.is_contiguous()
    n = N * H * W * C
    buf = np.full(n + 2 * GUARD, np.float32(-777.25), np.float32)
    rec, err = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = L.danhip_deform_far_ordered_emulate(off16.data_ptr(), dS16.data_ptr(), buf.ctypes.data + 4 * GUARD, n, N, H, W, C, dg, window,
                                            ctypes.addressof(rec), ctypes.addressof(err))
    assert rc == 0, L.danhip_last_error()
    assert np.all(buf[:GUARD] == np.float32(-777.25)) and np.all(buf[-GUARD:] == np.float32(-777.25)), "guard words around far_dx were written"
    return buf[GUARD:-GUARD].reshape(N, H, W, C).copy(), rec.value, err.value


def emulate(off, dS, N, H, W, C, dg, window=0):
    """The same from float arrays (values exact in the 16-bit type)."""
    act = act_dtype()
    return emulate16(torch.as_tensor(np.asarray(off, np.float32)).to(act).contiguous(), torch.as_tensor(np.asarray(dS, np.float32)).to(act).contiguous(),
                     N, H, W, C, dg, window)

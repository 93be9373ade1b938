"""Host side of the test-time pipeline for images of different sizes (csrc/evalpipe_ragged_exact.hip): the new entry points resolve with
their argument types, danhip_resize_item_init and the batched call refuse on the host what include/danhip.h says they refuse (nothing is
launched: every call here fails its validation or never reaches a launch), and the workspace query and the scale lists behave."""
import ctypes

import pytest

from dan_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def test_symbols_resolve_with_argument_types(lib):
    assert lib.danhip_version() >= 12
    for name in ("danhip_resize_item_init", "danhip_resize_u8_linear_batch", "danhip_detect_select"):
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name] and fn.restype is ctypes.c_int
    assert lib.danhip_resize_item_bytes() == ctypes.sizeof(_lib.ResizeItem) == 80
    assert lib.danhip_detect_select_workspace_bytes.restype is ctypes.c_size_t
    assert _lib.DETECT_SELECT_LAUNCHES == 7


def _init(lib, item, src_offset=0, H=10, W=20, pitch=60, dst_offset=0, Ho=5, Wo=10, fx=0.5, fy=0.5, mirror=0, first=0):
    nt = ctypes.c_int32(-1)
    rc = lib.danhip_resize_item_init(ctypes.byref(item), src_offset, H, W, pitch, dst_offset, Ho, Wo, fx, fy, mirror, first, ctypes.byref(nt))
    return rc, nt.value


def test_item_init_accepts_a_good_item_and_refuses_the_bad_ones(lib):
    item = _lib.ResizeItem()
    rc, nt = _init(lib, item)
    assert rc == 0 and nt == 1 and (item.H, item.W, item.Ho, item.Wo, item.tiles) == (10, 20, 5, 10, 1)
    assert item.scale_x == 2.0 and item.scale_y == 2.0
    rc, nt = _init(lib, item, H=768, W=1024, pitch=4096, Ho=1344, Wo=1792, fx=1.75, fy=1.75, mirror=1, first=7)
    assert rc == 0 and nt == (1344 * 1792 + 1023) // 1024 and item.first_tile == 7
    assert _init(lib, item, H=203, W=331, pitch=993, Ho=203, Wo=331, fx=1.0, fy=1.0, mirror=1)[0] == 0      # the plain mirrored copy
    assert _init(lib, item, H=5, W=5, pitch=15, Ho=2, Wo=2, fx=0.5, fy=0.5)[0] == 0                      # rint(2.5) = 2: half to even
    for bad in (dict(H=0), dict(W=-1), dict(Ho=0), dict(Wo=0)):                                             # non-positive sizes
        assert _init(lib, item, **bad)[0] == -1 and b"non-positive" in lib.danhip_last_error(), bad
    for bad in (dict(Ho=6), dict(Wo=9), dict(H=5, W=5, pitch=15, Ho=3, Wo=3)):                              # not rint(H * fy) / rint(W * fx)
        assert _init(lib, item, **bad)[0] == -1 and b"rint" in lib.danhip_last_error(), bad
    assert _init(lib, item, pitch=59)[0] == -1 and b"pitch" in lib.danhip_last_error()
    assert _init(lib, item, mirror=2)[0] == -1 and b"mirror" in lib.danhip_last_error()
    assert _init(lib, item, fx=0.0, Wo=0)[0] == -1 and _init(lib, item, fy=-0.5)[0] == -1
    assert _init(lib, item, src_offset=-1)[0] == -1 and _init(lib, item, first=-1)[0] == -1


def test_batch_call_checks_the_host_table_before_any_launch(lib):
    """Every call here is refused on the host: no launch is attempted (the pointers are host addresses that are never dereferenced)."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    tab = (_lib.ResizeItem * 2)()
    rc, n0 = _init(lib, tab[0], dst_offset=0)
    assert rc == 0
    assert _init(lib, tab[1], dst_offset=149, first=n0)[0] == 0          # item 0 writes bytes [0, 150)
    batch = lambda n=2, src_bytes=600, dst_bytes=4096: lib.danhip_resize_u8_linear_batch(ctypes.addressof(tab), p, n, p, src_bytes, p, dst_bytes, None)
    assert batch() == -1 and b"overlap" in lib.danhip_last_error()
    assert _init(lib, tab[1], dst_offset=150, first=n0)[0] == 0
    assert batch(src_bytes=599) == -1 and b"source" in lib.danhip_last_error()
    assert batch(dst_bytes=299) == -1 and b"destination" in lib.danhip_last_error()
    assert batch(n=0) == -1
    assert _init(lib, tab[1], dst_offset=150, first=n0 + 1)[0] == 0
    assert batch() == -1 and b"first_tile" in lib.danhip_last_error()
    assert _init(lib, tab[1], dst_offset=150, first=n0)[0] == 0
    tab[1].Wo = 11                                                        # edited after init
    assert batch() == -1 and b"item 1" in lib.danhip_last_error()
    assert lib.danhip_resize_u8_linear_batch(None, p, 2, p, 600, p, 4096, None) == -1


def test_select_workspace_query_and_argument_checks(lib):
    q = lib.danhip_detect_select_workspace_bytes
    sizes = [q(a) for a in (1, 2, 1126, 1127, 5000, 70001, 600000, 1 << 24)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert q(0) == 0
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    n = ctypes.c_int32(-1)
    sel = lambda A, K, shrink=1.0, filt=0, ws=1 << 20: lib.danhip_detect_select(p, p, A, K, shrink, filt, -1.0, p, p, p, ws, ctypes.byref(n), None)
    assert sel(10, 11) == -1 and sel(0, 0) == -1 and sel(5000, 2049) == -1 and sel(10, -1) == -1
    assert sel(10, 5, filt=3) == -1 and sel(10, 5, shrink=0.0) == -1
    assert sel(70001, 1125, ws=16) == -3 and n.value == 0
    assert sel(1, 0) == 0 and n.value == 0                                 # A = 1: the reference's K = A - 1 = 0 rows, nothing to launch


def test_scale_passes_are_those_detect_image_walks():
    """scale_passes against a trace of the serial functions, driven by a stub net that records the sizes it is shown."""
    from dan_amd import eval_dan as P
    for (h, w) in [(240, 320), (203, 331), (400, 300), (120, 160), (768, 1024), (1536, 1024)]:
        for pyramid in (False, True):
            shrink, max_shrink = P.get_shrink(h, w)
            expected = [shrink, shrink]
            st = 0.5 if max_shrink >= 0.75 else 0.5 * max_shrink
            expected.append(st)
            bt = min(2, max_shrink) if max_shrink > 1 else (st + max_shrink) / 2
            expected.append(bt)
            if max_shrink > 2:
                bt *= 2
                while bt < max_shrink:
                    expected.append(bt)
                    bt *= 2
                expected.append(max_shrink)
            if pyramid:
                expected += [0.25] + [s for s in (0.75, 1.25, 1.5, 1.75) if s <= max_shrink]
            got = P.scale_passes(h, w, pyramid)
            assert [s for s, _, _ in got] == expected
            assert [m for _, m, _ in got] == [0, 1] + [0] * (len(got) - 2)
            assert got[0][2] == got[1][2] == P.FILTER_NONE and got[2][2] == P.FILTER_BIG
    assert len(P.scale_passes(120, 160, False)) > 4                          # max_shrink > 2: the loop branch of multi_scale_test


FORM_LIMITS = (577, 40000, 80000, 115000, 150000)
FORM_SIZES = ((120, 160), (96, 136))
FORM_MAX_SHRINK = {(120, 160): (11.22, 1.37, 0.88, 0.68, 0.56), (96, 136): (13.78, 1.62, 1.13, 0.89, 0.74)}


def test_scale_passes_is_origin_flip_and_the_two_pass_lists():
    """The ten (size, memory_limit) pairs tests/test_evalpipe_forms_gpu.py runs: between them every branch of multi_scale_test's schedule.
    scale_passes equals the two private pass lists composed by hand, and each branch's list is spelled out once."""
    from dan_amd import eval_dan as P
    N, BIG, SMALL = P.FILTER_NONE, P.FILTER_BIG, P.FILTER_SMALL
    for size in FORM_SIZES:
        for ml, want in zip(FORM_LIMITS, FORM_MAX_SHRINK[size]):
            shrink, m = P.get_shrink(size[0], size[1], ml)
            assert round(m, 2) == want and shrink == min(m, 1), (size, ml, m)
            head = [(shrink, 0, N), (shrink, 1, N)]
            assert P.scale_passes(size[0], size[1], False, ml) == head + P._multi_scale_passes(m)
            assert P.scale_passes(size[0], size[1], True, ml) == head + P._multi_scale_passes(m) + P._pyramid_passes(m)
    m = P.get_shrink(120, 160, 577)[1]                                       # the loop: 2, 4, 8 and max_shrink itself, all small-filtered
    assert P._multi_scale_passes(m) == [(0.5, 0, BIG), (2, 0, SMALL), (4, 0, SMALL), (8, 0, SMALL), (m, 0, SMALL)]
    m = P.get_shrink(120, 160, 40000)[1]                                     # 1 < m <= 2
    assert P._multi_scale_passes(m) == [(0.5, 0, BIG), (m, 0, SMALL)]
    m = P.get_shrink(120, 160, 80000)[1]                                     # 0.75 <= m <= 1: bt = (0.5 + m) / 2 <= 1, the BIG filter
    assert P._multi_scale_passes(m) == [(0.5, 0, BIG), ((0.5 + m) / 2, 0, BIG)] and P.scale_passes(120, 160, True, 80000)[1] == (m, 1, N)
    m = P.get_shrink(120, 160, 115000)[1]                                    # m < 0.75: st = 0.5 m
    assert P._multi_scale_passes(m) == [(0.5 * m, 0, BIG), ((0.5 * m + m) / 2, 0, BIG)]
    assert P._pyramid_passes(0.74) == [(0.25, 0, BIG)] and P._pyramid_passes(0.75) == [(0.25, 0, BIG), (0.75, 0, BIG)]
    assert P._pyramid_passes(1.62) == [(0.25, 0, BIG), (0.75, 0, BIG), (1.25, 0, SMALL), (1.5, 0, SMALL)]

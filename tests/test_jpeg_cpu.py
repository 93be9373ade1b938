"""Host half of the JPEG decoder (csrc/jpeg_entropy.cpp) without a GPU: the library's coefficients and descriptors, run through the numpy
restatement of the device arithmetic (tests/jpeg_protocol.py), must equal Pillow's pixels bit for bit - for the recorded fixtures
(tests/golden/jpeg_golden.npz) and, where Pillow is importable, for live encodes; refused streams give their reason code on the host."""
import ctypes
import io
import os

import numpy as np
import pytest

import jpeg_protocol as JP
from dan_amd import _lib

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_golden.npz"))
ACCEPTED = [(str(n), GOLDEN["a%d_jpeg" % i].tobytes(), GOLDEN["a%d_rgb" % i]) for i, n in enumerate(GOLDEN["a_names"])]
REFUSED = [(str(n), GOLDEN["r%d_jpeg" % i].tobytes(), int(GOLDEN["r_reasons"][i])) for i, n in enumerate(GOLDEN["r_names"])]


def _decode(datas, **kw):
    return JP.entropy_decode(_lib.lib(), _lib.JpegDesc, datas, **kw)


def test_fixture_coverage():
    names = [n for n, _, _ in ACCEPTED]
    for mode in ("grey", "444", "422", "420"):
        for size in ("1x1", "7x9", "17x33", "40x56", "65x47", "136x50"):
            assert any(n.startswith("%s_%s_" % (mode, size)) for n in names), (mode, size)
        for extra in ("optimize", "rst_rows1", "rst_blocks3"):
            assert "%s_65x47_%s" % (mode, extra) in names
    for q in (30, 75, 95, 100):
        assert any(n.endswith("_q%d" % q) for n in names), q
    assert sorted(n for n, _, _ in REFUSED) == ["cmyk", "cut_mid_scan", "header_65535x65535", "noise_after_soi", "progressive"]


@pytest.mark.parametrize("name,data,want", ACCEPTED, ids=[a[0] for a in ACCEPTED])
def test_protocol_on_library_coefficients_equals_recorded_pillow(name, data, want):
    L = _lib.lib()
    info = _lib.JpegInfo()
    assert L.danhip_jpeg_inspect(data, len(data), ctypes.byref(info)) == 0
    assert (info.height, info.width) == want.shape[:2] and info.coef_count > 0 and info.coef_count % 64 == 0
    coef, descs, status = _decode([data])
    assert status == [0] and descs[0].status == 0 and descs[0].coef_count == info.coef_count
    assert descs[0].mode == {"grey": 0, "444": 1, "422": 2, "420": 3}[name.split("_")[0]]
    assert np.array_equal(JP.reconstruct(coef, descs[0]), want)


def _synthetic(h, w, seed):
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), ((xx + yy) * 5) % 256], 2).astype(np.float64)
    img[h // 4: h // 2 + 1, w // 3: 2 * w // 3 + 1] = r.randint(0, 256, 3)
    img += r.randn(h, w, 3) * r.choice([4, 20, 45])
    return np.clip(img, 0, 255).astype(np.uint8)


def test_protocol_equals_live_pillow_on_seeded_random_images():
    Image = pytest.importorskip("PIL.Image")
    r = np.random.RandomState(2024)
    cases = [(768, 1024, m, 90, {}) for m in (None, 0, 1, 2)]
    cases += [(h, w, m, 85, {}) for m in (None, 0, 1, 2) for h, w in ((1, 2), (2, 1), (3, 3), (8, 2), (2, 5), (5, 6), (100, 2), (16, 16))]
    while len(cases) < 76:
        kw = [{}, dict(optimize=True), dict(restart_marker_rows=1), dict(restart_marker_blocks=int(r.randint(1, 9)))][int(r.randint(4))]
        cases.append((int(r.randint(1, 200)), int(r.randint(1, 200)), [None, 0, 1, 2][int(r.randint(4))], int(r.randint(5, 101)), kw))
    refused = []
    for k, (h, w, sub, q, kw) in enumerate(cases):
        img = _synthetic(h, w, k)
        b = io.BytesIO()
        if sub is None:
            Image.fromarray(img[:, :, 0]).save(b, format="JPEG", quality=q, **kw)
        else:
            Image.fromarray(img).save(b, format="JPEG", quality=q, subsampling=sub, **kw)
        data = b.getvalue()
        want = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        coef, descs, status = _decode([data])
        if status[0] != 0:
            refused.append((k, h, w, sub, q, status[0]))
            continue
        assert np.array_equal(JP.reconstruct(coef, descs[0]), want), (k, h, w, sub, q, kw)
    assert refused == []                                                  # baseline encodes, every one: none may fall back


def test_one_thread_and_four_threads_give_identical_buffers():
    datas = [d for _, d, _ in ACCEPTED] + [d for _, d, _ in REFUSED]
    c1, d1, s1 = _decode(datas, threads=1, fill=-21846)
    c4, d4, s4 = _decode(datas, threads=4, fill=-21846)
    c99, d99, s99 = _decode(datas, threads=99, fill=-21846)               # clamped to DANHIP_JPEG_MAX_THREADS
    assert s1 == s4 == s99 and np.array_equal(c1, c4) and np.array_equal(c1, c99)
    assert bytes(d1) == bytes(d4) == bytes(d99)
    assert s1[:len(ACCEPTED)] == [0] * len(ACCEPTED)
    # batch offsets: coefficient slots in order, planes and images disjoint and aligned
    next_coef = 0
    for d in list(d1)[:len(ACCEPTED)]:
        assert d.coef_offset == next_coef and d.out_offset % 256 == 0 and all(o % 256 == 0 for o in d.plane_offset)
        next_coef += d.coef_count
    L = _lib.lib()
    assert L.danhip_jpeg_output_bytes(d1, len(datas)) == max(d.out_offset + (d.width * d.height * 3 + 255) // 256 * 256 for d in d1 if d.status == 0)
    assert L.danhip_jpeg_workspace_bytes(d1, len(datas)) > 0


@pytest.mark.parametrize("name,data,reason", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_stream_gives_its_reason_and_stays_in_its_slot(name, data, reason):
    L = _lib.lib()
    info = _lib.JpegInfo()
    header_reason = L.danhip_jpeg_inspect(data, len(data), ctypes.byref(info))
    assert header_reason == info.reason and header_reason in (0, reason)
    good = ACCEPTED[5][1]
    coef, descs, status = _decode([good, data, good], fill=-21846)
    assert status == [0, reason, 0] and descs[1].status == reason
    d = descs[1]
    assert (d.width, d.height, d.idct_groups, d.rgb_groups, d.coef_count, d.out_offset) == (0, 0, 0, 0, 0, 0)
    alone, da, _ = _decode([good])
    n = da[0].coef_count
    slot = info.coef_count if header_reason == 0 else 0                   # a stream refused at its header owns nothing
    assert descs[0].coef_offset == 0 and descs[2].coef_offset == n + slot
    assert np.array_equal(coef[:n], alone[:n]) and np.array_equal(coef[n + slot:2 * n + slot], alone[:n])
    assert len(coef) == 2 * n + slot
    assert np.array_equal(JP.reconstruct(coef, descs[2]), ACCEPTED[5][2])
    # the device entry point launches nothing for it (no GPU here: had it tried, the call would fail)
    launches = ctypes.c_int32(7)
    one = (_lib.JpegDesc * 1)()
    ctypes.memmove(one, ctypes.byref(descs[1]), ctypes.sizeof(_lib.JpegDesc))
    assert L.danhip_jpeg_reconstruct_batch(None, 0, one, one, 1, None, 0, None, 0, ctypes.byref(launches), None) == 0 and launches.value == 0


def test_reconstruct_refuses_descriptors_that_leave_their_buffers():
    """Every check comes before a launch: the device pointers are never dereferenced (and there is no GPU in this process)."""
    L = _lib.lib()
    coef, descs, status = _decode([ACCEPTED[9][1]])
    d = descs[0]
    ws, out = L.danhip_jpeg_workspace_bytes(descs, 1), L.danhip_jpeg_output_bytes(descs, 1)
    fake = ctypes.c_void_p(4096)

    def run(desc, coef_count=d.coef_count, out_bytes=out, ws_bytes=ws):
        one = (_lib.JpegDesc * 1)()
        ctypes.memmove(one, ctypes.byref(desc), ctypes.sizeof(_lib.JpegDesc))
        return L.danhip_jpeg_reconstruct_batch(fake, coef_count, one, fake, 1, fake, out_bytes, fake, ws_bytes, None, None)

    assert run(d, coef_count=d.coef_count - 1) == -1 and b"coefficients" in L.danhip_last_error()
    assert run(d, out_bytes=out - 256) == -1 and b"output" in L.danhip_last_error()
    assert run(d, ws_bytes=ws - 1) == -3
    for field, value in (("width", d.width + 8), ("height", 1 << 20), ("mode", 9), ("coef_offset", 64), ("out_offset", 256), ("idct_groups", d.idct_groups + 1),
                         ("rgb_groups", 1 << 30), ("ncomp", 1)):
        bad = _lib.JpegDesc()
        ctypes.memmove(ctypes.byref(bad), ctypes.byref(d), ctypes.sizeof(_lib.JpegDesc))
        setattr(bad, field, value)
        assert run(bad) == -1, field
    for index_field in ("blocks_w", "comp_w", "quant_index", "plane_offset"):
        bad = _lib.JpegDesc()
        ctypes.memmove(ctypes.byref(bad), ctypes.byref(d), ctypes.sizeof(_lib.JpegDesc))
        getattr(bad, index_field)[0] = 1 << 20
        assert run(bad) in (-1, -3), index_field

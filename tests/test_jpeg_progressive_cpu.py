"""Progressive streams through the host entropy stage (csrc/jpeg_entropy.cpp, DANHIP_JPEG_ALLOW_PROGRESSIVE) without a GPU: the library's
coefficients and descriptors, run through the numpy restatement of the device arithmetic (tests/jpeg_protocol.py), must equal Pillow's
pixels bit for bit - for the recorded fixtures (tests/golden/jpeg_progressive_golden.npz) and, where Pillow is importable, for live
encodes; without the flag every one of them stays reason 3; the refused set gives its derived reason and leaves the words around its slot
alone; and a stand-alone sanitizer build of the stage survives the fixtures and a seeded set of mutations of them."""
import ctypes
import io
import os
import shutil
import struct
import subprocess
import warnings

import numpy as np
import pytest

import jpeg_protocol as JP
from dan_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "jpeg_progressive_golden.npz"))
ACCEPTED = [(str(n), GOLDEN["a%d_jpeg" % i].tobytes(), GOLDEN["a%d_rgb" % i]) for i, n in enumerate(GOLDEN["a_names"])]
REFUSED = [(str(n), GOLDEN["r%d_jpeg" % i].tobytes(), int(GOLDEN["r_reasons"][i])) for i, n in enumerate(GOLDEN["r_names"])]
BASE = np.load(os.path.join(HERE, "golden", "jpeg_golden.npz"))
BASELINE = [(str(n), BASE["a%d_jpeg" % i].tobytes(), BASE["a%d_rgb" % i]) for i, n in enumerate(BASE["a_names"])]
PROGRESSIVE, EPROGRESSIVE, EPROGRESSION, HOSTONLY = 1, 3, 18, -1
CANARY, GUARD = -21846, 192


def inspect(data, flags):
    info = _lib.JpegInfo()
    rc = _lib.lib().danhip_jpeg_inspect_ex(data, len(data), flags, ctypes.byref(info))
    assert rc == info.reason or rc < 0
    return rc, info


def tables(datas):
    bufs = [ctypes.create_string_buffer(d, len(d)) for d in datas]
    ptrs = (ctypes.c_void_p * len(datas))(*[ctypes.addressof(b) for b in bufs])
    return bufs, ptrs, (ctypes.c_int64 * len(datas))(*[len(d) for d in datas])


def decode(datas, flags=PROGRESSIVE, threads=1):
    """danhip_jpeg_entropy_decode_batch_ex into a buffer with GUARD canary words on either side of the capacity the inspections add up to
    -> (coef of that capacity, descs, statuses); the canaries are checked here."""
    L, B = _lib.lib(), len(datas)
    capacity = sum(info.coef_count for rc, info in (inspect(d, flags) for d in datas) if rc == 0)
    buf = np.full(capacity + 2 * GUARD, CANARY, dtype=np.int16)
    descs, status = (_lib.JpegDesc * B)(), (ctypes.c_int32 * B)()
    bufs, ptrs, sizes = tables(datas)
    rc = L.danhip_jpeg_entropy_decode_batch_ex(ptrs, sizes, B, threads, flags, ctypes.c_void_p(buf.ctypes.data + 2 * GUARD), capacity, descs, status)
    assert rc == 0, L.danhip_last_error()
    assert (buf[:GUARD] == CANARY).all() and (buf[GUARD + capacity:] == CANARY).all()
    return buf[GUARD:GUARD + capacity], descs, list(status)


def prepare(datas, flags):
    L, B = _lib.lib(), len(datas)
    capacity = sum(info.coef_count for rc, info in (inspect(d, flags) for d in datas) if rc == 0)
    bufs, ptrs, sizes = tables(datas)
    need = L.danhip_jpeg_scan_staging_bytes(ptrs, sizes, B)
    staging = np.zeros(need + 16, np.uint8)
    at = (staging.ctypes.data + 15) & ~15
    descs, status = (_lib.JpegDesc * B)(), (ctypes.c_int32 * B)()
    rc = L.danhip_jpeg_scan_prepare_batch_ex(ptrs, sizes, B, flags, ctypes.c_void_p(at), need, capacity, descs, status)
    assert rc == 0, L.danhip_last_error()
    return descs, list(status)


def test_abi_version_and_fixture_coverage():
    assert _lib.lib().danhip_version() >= 8
    names = [n for n, _, _ in ACCEPTED]
    for mode in ("grey", "444", "422", "420"):
        for size in ("1x1", "17x9"):
            assert "%s_%s_q75" % (mode, size) in names
    for n in ("420_56x40_q75", "422_56x40_q75", "420_33x47_q75", "420_56x40_rst_blocks3", "420_56x40_q30", "420_48x32_flat"):
        assert n in names
    assert sorted((n, r) for n, _, r in REFUSED) == [("ac_scan_ss0", 18), ("ah_not_previous_al", 18), ("cut_after_scan5", 18),
                                                     ("cut_mid_refinement", 2), ("last_scan_removed", 18)]
    assert all(b"\xff\xc2" in d for _, d, _ in ACCEPTED) and b"\xff\xdd" in dict((n, d) for n, d, _ in ACCEPTED)["420_56x40_rst_blocks3"]


@pytest.mark.parametrize("name,data,want", ACCEPTED, ids=[a[0] for a in ACCEPTED])
def test_protocol_on_library_coefficients_equals_recorded_pillow(name, data, want):
    rc, info = inspect(data, PROGRESSIVE)
    assert rc == 0 and (info.height, info.width) == want.shape[:2] and info.coef_count > 0 and info.coef_count % 64 == 0
    coef, descs, status = decode([data])
    d = descs[0]
    assert status == [0] and d.status == 0
    # the inspection agrees with the batch call, and the geometry is the baseline geometry of the same size and sampling
    mode = {"grey": 0, "444": 1, "422": 2, "420": 3}[name.split("_")[0]]
    assert (d.width, d.height, d.mode, d.coef_count) == (info.width, info.height, info.mode, info.coef_count) and d.mode == mode
    hs, vs = (2 if mode >= 2 else 1), (2 if mode == 3 else 1)
    mx, my = -(-d.width // (8 * hs)), -(-d.height // (8 * vs))
    assert d.coef_count == 64 * mx * my * (hs * vs + 2 if mode else 1) and list(d.blocks_w)[:1] == [mx * hs] and list(d.blocks_h)[:1] == [my * vs]
    assert np.array_equal(JP.reconstruct(coef, d), want)


def test_a_batch_that_interleaves_baseline_and_progressive_streams():
    mixed = [x + (k,) for pair in zip(BASELINE[3::4], ACCEPTED) for k, x in enumerate(pair)]          # (name, stream, pixels, progressive)
    assert len(mixed) >= 16
    datas = [m[1] for m in mixed]
    coef1, descs1, status1 = decode(datas, threads=1)
    coef4, descs4, status4 = decode(datas, threads=4)
    assert status1 == status4 == [0] * len(mixed) and np.array_equal(coef1, coef4) and bytes(descs1) == bytes(descs4)
    next_coef = 0
    for (name, data, want, progressive), d in zip(mixed, descs1):
        assert d.coef_offset == next_coef, name                              # offsets in order ...
        next_coef += d.coef_count
        assert d.reserved[0] == progressive, name
        assert np.array_equal(JP.reconstruct(coef1, d), want), name           # ... and every slot holds its own image
    assert next_coef == len(coef1)


def test_without_the_flag_every_progressive_stream_keeps_reason_3():
    L = _lib.lib()
    for name, data, _ in ACCEPTED + REFUSED:
        rc, info = inspect(data, 0)
        assert rc == EPROGRESSIVE and info.coef_count == 0, name
        old = _lib.JpegInfo()
        assert L.danhip_jpeg_inspect(data, len(data), ctypes.byref(old)) == EPROGRESSIVE and bytes(old) == bytes(info)
        coef, descs, status = decode([data], flags=0)
        assert status == [EPROGRESSIVE] and descs[0].status == EPROGRESSIVE and len(coef) == 0, name
        _, pstatus = prepare([data], 0)
        assert pstatus == [EPROGRESSIVE], name
    # flags == 0 on baseline streams: the old entry points, byte for byte
    datas = [d for _, d, _ in BASELINE[:8]]
    coef, descs, status = decode(datas, flags=0)
    old_coef, old_descs, old_status = JP.entropy_decode(L, _lib.JpegDesc, datas)
    assert status == old_status and np.array_equal(coef, old_coef) and bytes(descs) == bytes(old_descs)


def test_unknown_flag_bits_are_refused():
    L = _lib.lib()
    data = ACCEPTED[0][1]
    info = _lib.JpegInfo()
    assert L.danhip_jpeg_inspect_ex(data, len(data), 2, ctypes.byref(info)) == -1 and b"flags" in L.danhip_last_error()
    bufs, ptrs, sizes = tables([data])
    descs, status, coef = (_lib.JpegDesc * 1)(), (ctypes.c_int32 * 1)(), np.zeros(4096, np.int16)
    assert L.danhip_jpeg_entropy_decode_batch_ex(ptrs, sizes, 1, 1, 0x80000001, ctypes.c_void_p(coef.ctypes.data), 4096, descs, status) == -1
    staging = np.zeros(1 << 16, np.uint8)
    at = (staging.ctypes.data + 15) & ~15
    assert L.danhip_jpeg_scan_prepare_batch_ex(ptrs, sizes, 1, 3, ctypes.c_void_p(at), (1 << 16) - 16, 4096, descs, status) == -1
    assert not coef.any()


@pytest.mark.parametrize("name,data,reason", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_stream_gives_its_reason_and_leaves_its_neighbours_alone(name, data, reason):
    rc, info = inspect(data, PROGRESSIVE)
    assert rc == reason and (info.width, info.height, info.coef_count) == (0, 0, 0)     # the scan script is the header: refused there, it owns nothing
    good, want = ACCEPTED[9][1], ACCEPTED[9][2]
    coef, descs, status = decode([good, data, good])                          # (decode checks the canaries around the buffer)
    assert status == [0, reason, 0] and descs[1].status == reason
    d = descs[1]
    assert (d.width, d.height, d.idct_groups, d.rgb_groups, d.coef_count, d.out_offset) == (0, 0, 0, 0, 0, 0)
    n = descs[0].coef_count
    assert descs[2].coef_offset == n and len(coef) == 2 * n and np.array_equal(coef[:n], coef[n:])
    assert np.array_equal(JP.reconstruct(coef, descs[2]), want)
    _, pstatus = prepare([good, data, BASELINE[5][1]], PROGRESSIVE)
    assert pstatus == [HOSTONLY, reason, 0]


def _corrupt_scan(data, which, value):
    """`data` with one byte in the middle of the entropy-coded data of its scan number `which` set to `value`."""
    at, sos = [], 0
    p = 2
    while data[p + 1] != 0xD9:
        q = p + 2 + ((data[p + 2] << 8) | data[p + 3])
        if data[p + 1] == 0xDA:
            a = q
            while not (data[q] == 0xFF and data[q + 1] != 0 and not 0xD0 <= data[q + 1] <= 0xD7):
                q += 1
            at.append((a + q) // 2)
        p = q
    out = bytearray(data)
    out[at[which]] = value
    return bytes(out)


def test_a_stream_refused_behind_its_header_keeps_its_slot_and_writes_nothing_outside_it():
    """A marker in the middle of a scan's data passes the walk over the markers (the scan just ends early) and fails in the entropy stage:
    truncated, with the slot kept, as the baseline path does it."""
    good, want = ACCEPTED[9][1], ACCEPTED[9][2]
    seen = []
    for which in range(10):
        for value in (0xFF, 0x00, 0xA5):                                      # FF + what follows: a marker, or FF00 = other data
            bad = _corrupt_scan(good, which, value)
            rc, info = inspect(bad, PROGRESSIVE)
            if rc != 0:
                continue
            coef, descs, status = decode([good, bad, good])
            n = descs[0].coef_count
            assert info.coef_count == n
            assert status[0] == 0 and status[2] == 0 and descs[2].coef_offset == 2 * n and len(coef) == 3 * n
            assert np.array_equal(coef[:n], coef[2 * n:]) and np.array_equal(JP.reconstruct(coef, descs[2]), want)
            if status[1]:
                assert status[1] in (2, 11, 15, 16) and descs[1].coef_count == 0 and descs[1].width == 0
                seen.append(status[1])
    assert 2 in seen and len(seen) >= 5


def test_prepare_hands_an_accepted_progressive_header_its_slot_and_no_device_work():
    datas = [BASELINE[5][1], ACCEPTED[9][1], BASELINE[20][1], ACCEPTED[0][1]]
    descs, status = prepare(datas, PROGRESSIVE)
    assert status == [0, HOSTONLY, 0, HOSTONLY]
    _, host_descs, _ = decode(datas)
    assert descs[0].coef_offset == 0 and descs[2].coef_offset == host_descs[2].coef_offset == descs[0].coef_count + host_descs[1].coef_count
    for i in (1, 3):
        assert (descs[i].status, descs[i].width, descs[i].coef_count, descs[i].idct_groups, descs[i].out_offset) == (HOSTONLY, 0, 0, 0, 0)
    assert _lib.lib().danhip_jpeg_output_bytes(descs, 4) == descs[2].out_offset + (descs[2].width * descs[2].height * 3 + 255) // 256 * 256


def test_protocol_equals_live_pillow_on_seeded_random_progressive_images():
    Image = pytest.importorskip("PIL.Image")
    r = np.random.RandomState(77)
    cases = [(h, w, m, 75, {}) for m in (None, 0, 1, 2) for h, w in ((1, 2), (2, 1), (8, 8), (9, 17), (16, 16), (2, 100))]
    cases += [(96, 128, 2, 90, {}), (96, 128, 1, 30, dict(restart_marker_rows=1)), (40, 56, 2, 95, dict(optimize=True))]
    while len(cases) < 48:
        kw = [{}, dict(restart_marker_rows=1), dict(restart_marker_blocks=int(r.randint(1, 9)))][int(r.randint(3))]
        cases.append((int(r.randint(1, 120)), int(r.randint(1, 120)), [None, 0, 1, 2][int(r.randint(4))], int(r.randint(5, 101)), kw))
    for k, (h, w, sub, q, kw) in enumerate(cases):
        rr = np.random.RandomState(k)
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), ((xx + yy) * 5) % 256], 2).astype(np.float64)
        img = np.clip(img + rr.randn(h, w, 3) * rr.choice([0, 4, 20, 45]), 0, 255).astype(np.uint8)
        b = io.BytesIO()
        if sub is None:
            Image.fromarray(img[:, :, 0]).save(b, format="JPEG", quality=q, progressive=True, **kw)
        else:
            Image.fromarray(img).save(b, format="JPEG", quality=q, subsampling=sub, progressive=True, **kw)
        data = b.getvalue()
        want = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        coef, descs, status = decode([data])
        assert status == [0], (k, h, w, sub, q, kw, status)
        assert np.array_equal(JP.reconstruct(coef, descs[0]), want), (k, h, w, sub, q, kw)


def test_sanitizer_build_survives_the_fixtures_and_seeded_mutations(tmp_path):
    """A stand-alone program (tests/jpeg_progressive_fuzz.cpp, its own main) compiled with the host compiler together with
    jpeg_entropy.cpp under -fsanitize=address,undefined, the sanitizer runtimes linked statically so that the program does not depend on
    what else the loader brings in: CPU only, nothing loaded into this interpreter, the environment handed on as it is.  Where the host
    compiler cannot make that link the same program is built without sanitizers (its own consistency checks remain) and the test says so
    with a warning; the program reports which build it is, and that is asserted."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler (g++, c++, clang++): the box that built libdanhip has one"
    root = os.path.dirname(HERE)
    srcs = [os.path.join(HERE, "jpeg_progressive_fuzz.cpp"), os.path.join(root, "dan_amd", "csrc", "jpeg_entropy.cpp")]
    exe = str(tmp_path / "jpeg_progressive_fuzz")
    base = [cxx, "-std=c++17", "-O0", "-g", "-pthread"]                    # -O0: the compile is most of this test's time
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = [] if is_clang else ["-static-libasan", "-static-libubsan"]   # clang links its sanitizer runtimes statically by default
    r = subprocess.run(base + san + static + srcs + ["-o", exe], capture_output=True, text=True)
    sanitized = r.returncode == 0
    if not sanitized:
        warnings.warn("%s cannot link the sanitizer runtimes statically; jpeg_progressive_fuzz runs WITHOUT sanitizers: %s" % (cxx, r.stderr[-300:]))
        r = subprocess.run(base + srcs + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    streams = [d for _, d, _ in ACCEPTED + REFUSED] + [d for _, d, _ in BASELINE[:3]]
    with open(str(tmp_path / "streams.bin"), "wb") as f:
        f.write(struct.pack("<i", len(streams)))
        for d in streams:
            f.write(struct.pack("<i", len(d)) + d)
    r = subprocess.run([exe, str(tmp_path / "streams.bin"), "32"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-500:])
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert ("sanitizers: address" in r.stdout) == sanitized, r.stdout[-500:]

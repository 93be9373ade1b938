"""The JPEG encoder's optimize=True without a GPU (include/danhip.h, "JPEG encode: optimised Huffman tables"): the table rule of
csrc/jpeg_encode.h against a plain-Python restatement of its six steps, the host stage's files against Pillow's save(optimize=True) byte
for byte, the default path against Pillow without the flag, and the evaluation commands' --encode_optimize.  No tolerance: equality."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_encode_cases as C  # noqa: E402
import jpeg_encode_huffman_cases as H  # noqa: E402
import jpeg_optimal_table as T  # noqa: E402


@pytest.fixture(scope="module")
def L():
    return C.host_lib()


def test_abi_version_and_constants(L):
    from dan_amd import _lib
    assert L.danhip_version() >= 20
    assert _lib.JPEG_ENCODE_OPTIMIZE_LAUNCHES == 3 and _lib.JPEG_ENC_OPTIMIZE == 1
    out = (ctypes.c_int32 * 8)()
    stride = L.danhip_jpeg_encode_optimize_layout(out)
    assert stride == out[0] and stride % 16 == 0
    assert out[1] + 4 * 257 * 4 <= out[2] and out[2] + 4 * 256 * 4 <= out[3] and out[3] + 4 * 273 <= out[4] and out[4] + 16 <= out[5]
    assert out[5] + out[7] <= stride and out[7] >= 177 + 4 * (21 + 256) + 14 and out[6] % 256 == 0


@pytest.mark.parametrize("name", list(T.count_sets()))
def test_table_rule_equals_its_restatement(name, L):
    counts = T.count_sets()[name]
    bits, vals, info = T.optimal_table(counts)
    rc, got_bits, got_vals = T.host_table(L, counts)
    assert rc == 0 and got_bits == bits and got_vals == vals
    used = sum(1 for c in counts if c)
    assert sum(bits) == used and bits[0] == 0 and sorted(vals[:used]) == [s for s in range(256) if counts[s]]
    assert sum(n / 2.0 ** l for l, n in enumerate(bits) if l) < 1                # a prefix code with the all-ones code left free
    if name == "one_symbol":
        assert bits[1] == 1 and vals[0] == 5                                      # one bit, not none: the reserved symbol takes the other code
    if name == "two_equal":
        assert bits[1:3] == [1, 1] and vals[:2] == [3, 200]                       # the larger symbol met the reserved one first: the longer code
    if name == "all_equal":
        # the reserved symbol (count 1) is merged with the LARGEST symbol of count 9, which so gets the one code of 9 bits and stands last
        assert bits[8] == 255 and bits[9] == 1 and vals == list(range(256))
    if name == "fibonacci_40":
        assert info["longest"] > 16 and info["direct"] > 0 and info["walked"] > 0 and bits[16] > 0
    if name == "capped_fibonacci":
        assert info["longest"] == 17


def test_table_rule_on_the_counts_of_real_images(L):
    """The statistics of noise at three qualities and of a smooth image, every table: the rule and its restatement agree."""
    for a, q in ((H.noise(48, 64, 81), 100), (H.noise(48, 64, 82), 50), (H.noise(40, 56, 83), 1), (C.image(100, 131, "smooth"), 75)):
        coef, descs, totals = H.pixels_host(L, [a], 3, q)
        counts = T.symbol_counts(coef, descs[0])
        assert counts[:, 256].sum() == 0 and counts[0].sum() + 2 * counts[2].sum() >= 3
        for t in range(4):
            bits, vals, _ = T.optimal_table(counts[t])
            assert T.host_table(L, counts[t]) == (0, bits, vals), (q, t)


def test_table_rule_refuses_what_it_cannot_take(L):
    big = [0] * 256
    big[0] = big[1] = 2 ** 30
    assert T.host_table(L, big)[0] != 0                                          # the sum leaves int32
    bits = (ctypes.c_uint8 * 17)()
    vals = (ctypes.c_uint8 * 256)()
    assert L.danhip_jpeg_optimal_table_host(None, bits, vals) != 0
    none = T.host_table(L, [0] * 256)                                            # no symbol at all: an empty table, not a crash
    assert none[0] == 0 and sum(none[1]) == 0


@pytest.mark.parametrize("sub,mode", T.MODES)
@pytest.mark.parametrize("q", T.QUALITIES)
def test_host_stage_equals_pillow_optimize(sub, mode, q):
    """JpegEncoder(optimize=True) on host images = Image.save(quality=q, subsampling=s, optimize=True), for constant grey (DC symbols and
    EOB only), a ramp and noise (many symbols and long codes at quality 100, ZRL runs at quality 1) at 1x1, 8x8, 16x16, 17x23, 64x48; one
    at a time and as one batch.  Pillow's own file is a baseline SOF0 file with four DHT segments in the order DC 0, AC 0, DC 1, AC 1."""
    pytest.importorskip("PIL.Image")
    from dan_amd.dataset.jpeg import JpegEncoder
    enc = JpegEncoder(quality=q, subsampling=sub, threads=3, optimize=True)
    named = T.images()
    want = [T.pillow_optimized(a, q, sub) for _, a in named]
    for w in want:
        m = T.markers(w)
        assert [k for k, _ in m] == [0xe0, 0xdb, 0xdb, 0xc0, 0xc4, 0xc4, 0xc4, 0xc4, 0xda]
        assert [p[0] for k, p in m if k == 0xc4] == [0x00, 0x10, 0x01, 0x11]
    got = enc.encode_batch([a for _, a in named])
    assert [n for (n, _), g, w in zip(named, got, want) if g != w] == []
    assert enc.encode(named[-1][1]) == want[-1] and enc.encode(named[0][1]) == want[0]
    plain = JpegEncoder(quality=q, subsampling=sub).encode_batch([a for _, a in named])
    assert all(len(g) <= len(p) for g, p in zip(got, plain))                      # never longer than with the standard tables


def test_zrl_and_long_codes_are_among_the_cases(L):
    """What the byte comparison above rests on: noise at quality 1 holds runs of 16 and more; noise at quality 100 has AC values of every
    category up to 8 bits and beyond and codes of 12 bits and more (the cut to 16 is the Fibonacci set's to exercise: a 64 x 48 image
    does not reach it)."""
    coef, descs, totals = H.pixels_host(L, [H.noise(48, 64, 74)], 3, 1)
    assert T.symbol_counts(coef, descs[0])[[1, 3], 0xf0].sum() > 0
    coef, descs, totals = H.pixels_host(L, [H.noise(48, 64, 74)], 1, 100)
    counts = T.symbol_counts(coef, descs[0])
    bits = [T.optimal_table(row)[0] for row in counts]
    assert np.count_nonzero(counts[1]) >= 10 and np.count_nonzero(counts[3]) >= 10 and counts[1][1:9].min() > 0
    assert max(l for b in bits for l in range(17) if b[l]) >= 12


@pytest.mark.parametrize("sub,mode", T.MODES)
def test_default_is_untouched(sub, mode, L):
    """optimize=False, and no keyword at all: Pillow's bytes without the flag, as before; the _ex calls with flags 0 are the plain calls."""
    pytest.importorskip("PIL.Image")
    from dan_amd.dataset.jpeg import JpegEncoder
    arrays = [a for _, a in T.images()]
    for q in (25, 95):
        want = [C.pillow_bytes(a, q, sub) for a in arrays]
        assert JpegEncoder(quality=q, subsampling=sub).encode_batch(arrays) == want
        assert JpegEncoder(quality=q, subsampling=sub, optimize=False).encode_batch(arrays) == want
        coef, descs, totals = H.pixels_host(L, arrays, mode, q)
        B = len(arrays)
        out = np.empty(totals[2], np.uint8)
        sizes = (ctypes.c_int64 * B)()
        assert L.danhip_jpeg_encode_entropy_batch_ex(H.vp(coef), coef.size, descs, B, 2, 0, H.vp(out), totals[2], sizes) == 0
        assert H.files_of(out, descs, list(sizes)) == want
        assert L.danhip_jpeg_encode_entropy_batch_ex(H.vp(coef), coef.size, descs, B, 2, 2, H.vp(out), totals[2], sizes) != 0      # an unknown flag
    st, _ = H.staging(L, descs, totals)
    again = np.zeros_like(st)
    status = (ctypes.c_int32 * B)()
    assert L.danhip_jpeg_encode_scan_prepare_ex(descs, B, totals[0], totals[2], 0, H.vp(again), again.size, status) == 0
    assert np.array_equal(st, again)


def test_staging_with_optimize_grows_the_workspace_by_a_region_per_image(L):
    coef, descs, totals = H.pixels_host(L, [H.noise(16, 24, 31), H.noise(9, 9, 32)], 3, 75)
    st, _ = H.staging(L, descs, totals)
    opt = np.zeros_like(st)
    status = (ctypes.c_int32 * 2)()
    assert L.danhip_jpeg_encode_scan_prepare_ex(descs, 2, totals[0], totals[2], 1, H.vp(opt), opt.size, status) == 0 and list(status) == [0, 0]
    stride = L.danhip_jpeg_encode_optimize_layout(None)
    assert L.danhip_jpeg_encode_scan_workspace_bytes(H.vp(opt)) == L.danhip_jpeg_encode_scan_workspace_bytes(H.vp(st)) + 2 * stride
    assert L.danhip_jpeg_encode_scan_prepare_ex(descs, 2, totals[0], totals[2], 4, H.vp(opt), opt.size, status) != 0
    out = np.empty(totals[2], np.uint8)
    sizes = (ctypes.c_int64 * 2)()
    rc = L.danhip_jpeg_encode_entropy_emulate_batch(H.vp(opt), opt.size, descs, 2, H.vp(coef), coef.size, H.vp(out), totals[2], sizes, status, None)
    assert rc != 0 and b"OPTIMIZE" in L.danhip_last_error()


def test_a_value_without_a_baseline_code_is_refused_with_optimize_too(L):
    coef, descs, totals = H.pixels_host(L, [H.noise(24, 40, 21)], 3, 90)
    bad = coef.copy()
    bad[64 * 3 + 9] = 32767
    out = np.empty(totals[2], np.uint8)
    sizes = (ctypes.c_int64 * 1)()
    assert L.danhip_jpeg_encode_entropy_batch_ex(H.vp(bad), bad.size, descs, 1, 1, 1, H.vp(out), totals[2], sizes) != 0
    assert b"baseline" in L.danhip_last_error()


def test_parser_takes_encode_optimize_and_defaults_to_off():
    from dan_amd import eval_cli
    for model in ("sfd", "pb", "dan", "dan_deform"):
        p = eval_cli.build_parser(model)
        assert p.parse_args([]).encode_optimize is False
        assert p.parse_args(["--encode_optimize"]).encode_optimize is True
        assert p.parse_args(["--encode_optimize", "--encode_entropy", "device"]).encode_entropy == "device"

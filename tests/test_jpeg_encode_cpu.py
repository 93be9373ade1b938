"""Baseline JPEG encode on the host (include/danhip.h, "Baseline JPEG encode"; csrc/jpeg_encode.cpp + csrc/jpeg_encode.h): the file
danhip_jpeg_encode_host writes is byte for byte Pillow's over the matrix of tests/jpeg_encode_cases.py - pinned by a committed fixture and,
whenever Pillow imports, compared live; the two stages are checked against the existing DEcoder's entropy stage; a stand-alone program
drives the encoder over odd sizes under the host sanitizers.  No tolerance anywhere."""
import ctypes
import os
import shutil
import subprocess
import sys
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jpeg_encode_cases as C  # noqa: E402

CASES = C.cases()


@pytest.fixture(scope="module")
def L():
    return C.host_lib()


@pytest.fixture(scope="module")
def golden():
    return C.load_golden()


def test_abi_version_and_descriptor_size(L):
    from dan_amd import _lib
    assert L.danhip_version() >= 15
    assert L.danhip_jpeg_enc_desc_bytes() == ctypes.sizeof(_lib.JpegEncDesc)
    assert L.danhip_draw_item_bytes() == ctypes.sizeof(_lib.DrawItem)


def test_fixture_holds_the_whole_matrix(golden):
    files, inputs = golden
    assert len(CASES) == 280 and sorted(files) == sorted(c[0] for c in CASES)
    for (h, w, c), a in inputs.items():
        assert np.array_equal(a, C.image(h, w, c)), (h, w, c)            # the generator still makes the fixture's inputs


@pytest.mark.parametrize("size", C.SIZES, ids=lambda s: "%dx%d" % s)
def test_host_encoder_equals_the_pinned_pillow_bytes(size, L, golden):
    files, inputs = golden
    n = 0
    for key, h, w, content, sub, mode, q in CASES:
        if (h, w) != size:
            continue
        got = C.encode_host(L, inputs[(h, w, content)], q, mode)
        assert got == files[key], key
        n += 1
    assert n == 40


@pytest.mark.parametrize("size", C.SIZES, ids=lambda s: "%dx%d" % s)
def test_host_encoder_equals_pillow_live(size, L):
    pytest.importorskip("PIL.Image")
    for key, h, w, content, sub, mode, q in CASES:
        if (h, w) != size:
            continue
        a = C.image(h, w, content)
        assert C.encode_host(L, a, q, mode) == C.pillow_bytes(a, q, sub), key
    a = C.image(*size, "noise")
    for q in (1, 2, 49, 50, 51):                                          # the quality scaling's two branches and the clamp to 255
        assert C.encode_host(L, a, q, 3) == C.pillow_bytes(a, q, "4:2:0"), (size, q)


def _prepare(L, arrays, mode, quality):
    from dan_amd._lib import JpegEncDesc
    B = len(arrays)
    descs = (JpegEncDesc * B)()
    widths = (ctypes.c_int32 * B)(*[a.shape[1] for a in arrays])
    heights = (ctypes.c_int32 * B)(*[a.shape[0] for a in arrays])
    srcs = (ctypes.c_void_p * B)(*[a.ctypes.data for a in arrays])
    totals = (ctypes.c_int64 * 3)()
    assert L.danhip_jpeg_encode_prepare(widths, heights, srcs, B, mode, quality, descs, totals) == 0
    return descs, totals


def _decode_coefficients(L, datas):
    """The existing decoder's entropy stage: streams -> (int16 coefficients, descriptors)."""
    from dan_amd._lib import JpegDesc, JpegInfo
    B = len(datas)
    info = JpegInfo()
    cap = 0
    for d in datas:
        assert L.danhip_jpeg_inspect(d, len(d), ctypes.byref(info)) == 0
        cap += info.coef_count
    coef = np.zeros(cap, np.int16)
    descs = (JpegDesc * B)()
    status = (ctypes.c_int32 * B)()
    ptrs = (ctypes.c_char_p * B)(*datas)
    sizes = (ctypes.c_int64 * B)(*[len(d) for d in datas])
    assert L.danhip_jpeg_entropy_decode_batch(ptrs, sizes, B, 2, ctypes.c_void_p(coef.ctypes.data), cap, descs, status) == 0
    assert list(status) == [0] * B
    return coef, descs


@pytest.mark.parametrize("sub,mode", C.MODES)
@pytest.mark.parametrize("q", [10, 75, 100])
def test_stages_against_the_decoder(sub, mode, q, L, golden):
    """Pillow's stream through danhip_jpeg_entropy_decode_batch gives the host pixel stage's coefficients, element for element (dummy
    blocks included: the layouts are the same), and danhip_jpeg_encode_entropy_batch on the DEcoded coefficients gives Pillow's file back."""
    files, inputs = golden
    arrays = [inputs[(h, w, "noise" if k % 2 else "smooth")] for k, (h, w) in enumerate(C.SIZES)]
    want = [files["%dx%d_%s_%s_q%d" % (a.shape[0], a.shape[1], "noise" if k % 2 else "smooth", sub.replace(":", ""), q)] for k, a in enumerate(arrays)]
    B = len(arrays)
    dec_coef, dec_descs = _decode_coefficients(L, want)
    descs, totals = _prepare(L, arrays, mode, q)
    assert totals[0] == dec_coef.size
    for i in range(B):
        assert (descs[i].coef_offset, descs[i].coef_count) == (dec_descs[i].coef_offset, dec_descs[i].coef_count)
        assert list(descs[i].blocks_w) == list(dec_descs[i].blocks_w) and list(descs[i].blocks_h) == list(dec_descs[i].blocks_h)
    coef = np.full(totals[0], 12345, np.int16)
    assert L.danhip_jpeg_encode_pixels_host(descs, B, ctypes.c_void_p(coef.ctypes.data), totals[0]) == 0, L.danhip_last_error()
    for i in range(B):
        a, b = descs[i].coef_offset, descs[i].coef_offset + descs[i].coef_count
        assert np.array_equal(coef[a:b], dec_coef[a:b]), (i, arrays[i].shape)
    out = np.empty(totals[2], np.uint8)
    sizes = (ctypes.c_int64 * B)()
    rc = L.danhip_jpeg_encode_entropy_batch(ctypes.c_void_p(dec_coef.ctypes.data), dec_coef.size, descs, B, 3, ctypes.c_void_p(out.ctypes.data),
                                            totals[2], sizes)
    assert rc == 0, L.danhip_last_error()
    for i in range(B):
        assert out[descs[i].file_offset:descs[i].file_offset + sizes[i]].tobytes() == want[i], i


def test_bad_arguments_are_refused(L):
    a = C.image(8, 8, "noise")
    out = np.empty(4096, np.uint8)
    n = ctypes.c_int64(0)
    args = lambda w, h, mode, q, cap: (ctypes.c_void_p(a.ctypes.data), w, h, mode, q, ctypes.c_void_p(out.ctypes.data), cap, ctypes.byref(n))
    assert L.danhip_jpeg_encode_host(*args(8, 8, 2, 75, 4096)) != 0             # 4:2:2 is not made
    assert L.danhip_jpeg_encode_host(*args(8, 8, 0, 75, 4096)) != 0             # grey neither
    assert L.danhip_jpeg_encode_host(*args(8, 8, 3, 0, 4096)) != 0 and L.danhip_jpeg_encode_host(*args(8, 8, 3, 101, 4096)) != 0
    assert L.danhip_jpeg_encode_host(*args(0, 8, 3, 75, 4096)) != 0 and L.danhip_jpeg_encode_host(*args(8, 16385, 3, 75, 4096)) != 0
    assert L.danhip_jpeg_encode_host(*args(8, 8, 3, 75, 100)) != 0 and n.value > 100          # too small: the size is still reported
    assert L.danhip_jpeg_encode_host(*args(8, 8, 3, 75, 4096)) == 0
    descs, totals = _prepare(L, [a], 3, 75)
    coef = np.zeros(totals[0], np.int16)
    coef[0] = 32767                                                              # a DC difference of 16 bits: no baseline code
    sizes = (ctypes.c_int64 * 1)()
    big = np.empty(totals[2], np.uint8)
    assert L.danhip_jpeg_encode_entropy_batch(ctypes.c_void_p(coef.ctypes.data), totals[0], descs, 1, 1, ctypes.c_void_p(big.ctypes.data), totals[2], sizes) != 0
    descs[0].real_bw = 7                                                         # a descriptor that no longer follows from its size
    coef[0] = 0
    assert L.danhip_jpeg_encode_entropy_batch(ctypes.c_void_p(coef.ctypes.data), totals[0], descs, 1, 1, ctypes.c_void_p(big.ctypes.data), totals[2], sizes) != 0


def test_encoder_class_takes_host_images_without_a_gpu():
    import torch
    from dan_amd.dataset.jpeg import JpegEncoder
    files, inputs = C.load_golden()
    arrays = [inputs[(17, 33, "noise")], torch.from_numpy(inputs[(100, 131, "smooth")])]
    enc = JpegEncoder(quality=95, subsampling="4:4:4")
    got = enc.encode_batch(arrays)
    assert got == [files["17x33_noise_444_q95"], files["100x131_smooth_444_q95"]] and enc.stats["host"] == 2 and enc.stats["launches"] == 0
    assert JpegEncoder().encode(arrays[0]) == files["17x33_noise_420_q75"]
    with pytest.raises(ValueError):
        JpegEncoder(subsampling="4:2:2")


def test_sanitizer_build_encodes_odd_sizes(tmp_path):
    """tests/jpeg_encode_fuzz.cpp (its own main) compiled with the host compiler together with jpeg_encode.cpp and jpeg_entropy.cpp under
    -fsanitize=address,undefined, the runtimes linked statically: CPU only, nothing loaded into this interpreter.  Where the host compiler
    cannot make that link the program is built without sanitizers (its own checks remain) and the test says so with a warning."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler (g++, c++, clang++): the box that built libdanhip has one"
    csrc = os.path.join(os.path.dirname(HERE), "dan_amd", "csrc")
    srcs = [os.path.join(HERE, "jpeg_encode_fuzz.cpp"), os.path.join(csrc, "jpeg_encode.cpp"), os.path.join(csrc, "jpeg_entropy.cpp")]
    exe = str(tmp_path / "jpeg_encode_fuzz")
    base = [cxx, "-std=c++17", "-O1", "-g", "-pthread"]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    r = subprocess.run(base + san + static + srcs + ["-o", exe], capture_output=True, text=True)
    sanitized = r.returncode == 0
    if not sanitized:
        warnings.warn("%s cannot link the sanitizer runtimes statically; jpeg_encode_fuzz runs WITHOUT sanitizers: %s" % (cxx, r.stderr[-300:]))
        r = subprocess.run(base + srcs + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, "40"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-500:])
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert ("sanitizers: address" in r.stdout) == sanitized, r.stdout[-500:]

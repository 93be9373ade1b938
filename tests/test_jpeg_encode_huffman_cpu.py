"""The JPEG encoder's device Huffman stage, emulated on the host (include/danhip.h, "JPEG encode: Huffman stage on the device";
csrc/jpeg_encode_huffman.h through danhip_jpeg_encode_entropy_emulate_batch): the phases the kernels run, over the same staging buffer,
give the bytes of danhip_jpeg_encode_entropy_batch - the host stage, which is Pillow's byte for byte - on the committed fixture, on live
Pillow encodes and on coefficients no baseline stream carries.  No tolerance anywhere."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jpeg_encode_cases as C  # noqa: E402
import jpeg_encode_huffman_cases as H  # noqa: E402

LIVE_QUALITIES = [1, 50, 75, 95, 100]


@pytest.fixture(scope="module")
def L():
    return C.host_lib()


@pytest.fixture(scope="module")
def golden():
    return C.load_golden()


def test_abi_version_and_constants(L):
    from dan_amd import _lib
    assert L.danhip_version() >= 16
    assert _lib.JPEG_ENCODE_ENTROPY_LAUNCHES == 6 and _lib.JPEG_HOSTONLY == -1
    assert L.danhip_jpeg_encode_scan_staging_bytes(0) == 0 and L.danhip_jpeg_encode_scan_staging_bytes(65536) == 0
    assert L.danhip_jpeg_encode_scan_staging_bytes(3) > 3 * 623 + 4096


@pytest.mark.parametrize("sub,mode", C.MODES)
@pytest.mark.parametrize("q", C.QUALITIES)
def test_fixture_files_singly_and_in_one_batch(sub, mode, q, L, golden):
    """Every case of the fixture with this (mode, quality): coefficients of the host pixel stage -> the emulation's file equals the host
    stage's and the pinned Pillow bytes, image by image and all 35 in one batch."""
    files, inputs = golden
    cases = [c for c in C.cases() if c[5] == mode and c[6] == q]
    assert len(cases) == 35
    arrays = [inputs[(h, w, content)] for _, h, w, content, _, _, _ in cases]
    want = [files[c[0]] for c in cases]
    for a, w in zip(arrays, want):
        coef, descs, totals = H.pixels_host(L, [a], mode, q)
        out, sizes, status, errors = H.emulate(L, coef, descs, totals)
        assert status == [0] and errors == 0
        assert H.files_of(out, descs, sizes) == [w] == H.host_entropy(L, coef, descs, totals)
        assert np.all(out[sizes[0]:] == H.GUARD)
    coef, descs, totals = H.pixels_host(L, arrays, mode, q)
    out, sizes, status, errors = H.emulate(L, coef, descs, totals)
    assert status == [0] * 35 and errors == 0
    assert H.files_of(out, descs, sizes) == want == H.host_entropy(L, coef, descs, totals)


@pytest.mark.parametrize("sub,mode", C.MODES)
@pytest.mark.parametrize("q", LIVE_QUALITIES)
def test_live_pillow_encodes_and_the_chain_to_pillow(sub, mode, q, L):
    """Host pixel stage + emulation = Image.save(quality=q, subsampling=s), and = the host stage from the same coefficients; images with
    several workgroups of blocks (more than 256) and several stuffing chunks among them."""
    pytest.importorskip("PIL.Image")
    arrays = [H.noise(64, 48, 11), H.noise(17, 9, 12), H.noise(9, 17, 13), H.flat_grey(40, 24), H.sparse_high_frequency(), H.noise(1, 1, 14),
              C.image(100, 131, "smooth"), H.noise(128, 160, 15)]
    coef, descs, totals = H.pixels_host(L, arrays, mode, q)
    out, sizes, status, errors = H.emulate(L, coef, descs, totals)
    assert errors == 0 and status == [0] * len(arrays)
    got = H.files_of(out, descs, sizes)
    assert got == H.host_entropy(L, coef, descs, totals)
    for a, g in zip(arrays, got):
        assert g == H.pillow(a, q, sub), (a.shape, q, sub)
    for i, d in enumerate(descs):                                            # nothing beyond a file inside its slot
        assert np.all(out[d.file_offset + sizes[i]:d.file_offset + d.file_capacity] == H.GUARD)


def test_pinned_padding_seeds_and_the_zrl_image(L):
    """The images the GPU test takes for its padding and ZRL cases are what it says they are: a scan that ends on a byte boundary, one that
    ends one bit past one, and one with runs of 16 and more zeros in front of a value."""
    tabs = None
    for seed, want in ((H.PAD0_SEED, 0), (H.PAD1_SEED, 1)):
        coef, descs, totals = H.pixels_host(L, [H.noise(16, 16, seed)], 3, 75)
        tabs = tabs or H.tables(H.staging(L, descs, totals)[0])
        assert H.scan_bits(tabs, coef, descs[0])[0] % 8 == want, seed
        out, sizes, status, errors = H.emulate(L, coef, descs, totals)
        assert status == [0] and errors == 0 and H.files_of(out, descs, sizes) == H.host_entropy(L, coef, descs, totals)
    coef, descs, totals = H.pixels_host(L, [H.sparse_high_frequency()], 3, 30)
    assert H.scan_bits(tabs, coef, descs[0])[1] >= 16
    out, sizes, status, errors = H.emulate(L, coef, descs, totals)
    assert status == [0] and errors == 0 and H.files_of(out, descs, sizes) == H.host_entropy(L, coef, descs, totals)


@pytest.mark.parametrize("where", ["dc", "ac", "dc_min", "ac_min", "last_block"])
def test_values_without_a_baseline_code_flag_their_image_and_stay_in_their_slot(where, L):
    arrays = [H.noise(24, 40, 21), H.noise(17, 33, 22), H.noise(16, 16, 23)]
    coef, descs, totals = H.pixels_host(L, arrays, 3, 90)
    clean = H.host_entropy(L, coef, descs, totals)
    bad = coef.copy()
    d = descs[1]
    if where == "last_block":
        bad[d.coef_offset + d.coef_count - 64 + 5] = 32767
    else:
        bad[d.coef_offset + 64 * 3 + (0 if where.startswith("dc") else 9)] = -32768 if where.endswith("min") else 32767
    out, sizes, status, errors = H.emulate(L, bad, descs, totals)
    assert status[0] == 0 and status[2] == 0 and status[1] != 0 and sizes[1] == 0 and errors == 0
    assert out[descs[0].file_offset:descs[0].file_offset + sizes[0]].tobytes() == clean[0]
    assert out[descs[2].file_offset:descs[2].file_offset + sizes[2]].tobytes() == clean[2]
    assert np.all(out[descs[0].file_offset + sizes[0]:descs[1].file_offset] == H.GUARD)          # image 0's slot beyond its file
    assert np.all(out[descs[2].file_offset + sizes[2]:] == H.GUARD)
    # the host stage has the last word on such a value: it refuses the batch
    buf = np.empty(totals[2], np.uint8)
    n = (ctypes.c_int64 * 3)()
    assert L.danhip_jpeg_encode_entropy_batch(H.vp(bad), bad.size, descs, 3, 1, H.vp(buf), totals[2], n) != 0


def test_every_block_at_its_longest_stays_inside_the_file_bound(L):
    """1023 / -1023 in every AC position and DC values that jump by 2046: blocks at (or a few bits below) the 1658 bits that
    danhip_jpeg_encode_file_bound is made for.  The emulation agrees with the host stage and both stay inside the slot."""
    descs, totals = H.prepare(L, [(24, 24), (8, 8)], 3, 50)
    coef = np.zeros(totals[0], np.int16)
    coef[:] = 1023
    coef[1::2] = -1023
    coef[0::128] = -1023
    out, sizes, status, errors = H.emulate(L, coef, descs, totals)
    assert status == [0, 0] and errors == 0
    assert H.files_of(out, descs, sizes) == H.host_entropy(L, coef, descs, totals)
    assert all(sizes[i] <= descs[i].file_capacity for i in range(2))


def test_bad_arguments_are_refused(L):
    a = H.noise(16, 24, 31)
    coef, descs, totals = H.pixels_host(L, [a], 3, 75)
    st, pstatus = H.staging(L, descs, totals)
    B, n = 1, st.size
    status = (ctypes.c_int32 * 1)()
    sizes = (ctypes.c_int64 * 1)()
    out = np.empty(totals[2], np.uint8)
    EINVAL = -1
    prep = L.danhip_jpeg_encode_scan_prepare
    assert prep(None, B, totals[0], totals[2], H.vp(st), n, status) == EINVAL
    assert prep(descs, 0, totals[0], totals[2], H.vp(st), n, status) == EINVAL
    assert prep(descs, B, totals[0], totals[2], None, n, status) == EINVAL
    assert prep(descs, B, totals[0], totals[2], H.vp(st), n - 1, status) == EINVAL               # staging too small
    assert prep(descs, B, totals[0], totals[2], ctypes.c_void_p(st.ctypes.data + 4), n, status) == EINVAL      # not aligned
    assert prep(descs, B, totals[0] - 1, totals[2], H.vp(st), n, status) == EINVAL               # coefficients leave the buffer
    assert prep(descs, B, totals[0], totals[2] - 1, H.vp(st), n, status) == EINVAL               # the file slot leaves the buffer
    assert prep(descs, B, totals[0], totals[2], H.vp(st), n, None) == EINVAL
    assert L.danhip_jpeg_encode_scan_workspace_bytes(H.vp(np.zeros(256, np.uint8))) == 0          # no staging buffer
    emu = L.danhip_jpeg_encode_entropy_emulate_batch
    good = lambda: (H.vp(st), n, descs, B, H.vp(coef), coef.size, H.vp(out), totals[2], sizes, status, None)
    assert emu(*good()) == 0
    for k, v in ((0, None), (2, None), (3, 0), (4, None), (6, None), (8, None), (9, None), (1, n - 16), (5, coef.size - 1), (7, totals[2] - 1)):
        args = list(good())
        args[k] = v
        assert emu(*args) == EINVAL, k
    tampered = st.copy()
    tampered[n - 700] ^= 1                                                    # a byte of the staged markers
    assert emu(H.vp(tampered), n, descs, B, H.vp(coef), coef.size, H.vp(out), totals[2], sizes, status, None) == EINVAL
    descs[0].real_bw += 1                                                     # a descriptor that no longer follows from its size
    assert emu(*good()) == EINVAL and prep(descs, B, totals[0], totals[2], H.vp(st), n, status) == EINVAL

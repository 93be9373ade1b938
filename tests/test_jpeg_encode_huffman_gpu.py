"""The JPEG encoder's Huffman stage on the GPU (csrc/jpeg_encode_huffman_exact.hip): the files danhip_jpeg_encode_huffman_batch leaves in
device memory equal danhip_jpeg_encode_entropy_batch's from the same coefficients and Pillow's Image.save from the same pixels, byte for
byte, at the smallest shapes at which each phase can go wrong; every status is 0, the launch count is the constant for B = 1 and B = 5,
and JpegEncoder(entropy="device") never takes its retry route, so no fallback hides a failure.  No tolerance: equality."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_encode_cases as C  # noqa: E402
import jpeg_encode_huffman_cases as H  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = {"4:2:0": 3, "4:4:4": 1}
RANGE = 1                                     # DANHIP_JPEG_ENC_DEV_RANGE


@pytest.fixture(scope="module")
def L():
    from dan_amd import _lib
    return _lib.lib()


def device_stage(L, dev, coef, descs, totals):
    """danhip_jpeg_encode_huffman_batch on host coefficients -> (files buffer pre-filled with GUARD, sizes, status, launches)."""
    from dan_amd._lib import ptr, stream
    B = len(descs)
    st, pstatus = H.staging(L, descs, totals)
    assert pstatus == [0] * B
    with torch.cuda.device(dev):
        st_dev = torch.from_numpy(st.copy()).to(dev)
        coef_dev = torch.from_numpy(coef).to(dev)
        files = torch.full((totals[2],), H.GUARD, dtype=torch.uint8, device=dev)
        sizes = torch.full((B,), -7, dtype=torch.int64, device=dev)
        status = torch.full((B,), -7, dtype=torch.int32, device=dev)
        nws = L.danhip_jpeg_encode_scan_workspace_bytes(H.vp(st))
        ws = torch.full((nws,), 0x5A, dtype=torch.uint8, device=dev)           # exactly the queried size, not zeroed
        launches = ctypes.c_int32(-1)
        rc = L.danhip_jpeg_encode_huffman_batch(H.vp(st), ptr(st_dev), st.size, descs, B, ptr(coef_dev), coef.size, ptr(files), totals[2],
                                                ptr(sizes), ptr(status), ptr(ws), nws, ctypes.byref(launches), stream())
        assert rc == 0, L.danhip_last_error()
        return files.cpu().numpy(), sizes.cpu().tolist(), status.cpu().tolist(), launches.value


def check_images(L, dev, arrays, sub, q):
    """Host pixel stage -> device Huffman stage, against the host stage and Image.save.  Returns the files."""
    from dan_amd import _lib
    coef, descs, totals = H.pixels_host(L, arrays, MODES[sub], q)
    out, sizes, status, launches = device_stage(L, dev, coef, descs, totals)
    assert status == [0] * len(arrays), status
    assert launches == _lib.JPEG_ENCODE_ENTROPY_LAUNCHES == 6
    got = H.files_of(out, descs, sizes)
    want = H.host_entropy(L, coef, descs, totals)
    assert got == want, [i for i in range(len(arrays)) if got[i] != want[i]]
    for a, g in zip(arrays, got):
        assert g == H.pillow(a, q, sub), (a.shape, sub, q)
    for i, d in enumerate(descs):                                               # nothing beyond a file inside its slot
        assert np.all(out[d.file_offset + sizes[i]:d.file_offset + d.file_capacity] == H.GUARD), i
    return got, coef, descs


CASES = {
    "one_mcu_444": (lambda: [H.noise(8, 8, 41)], "4:4:4", 75),
    "one_mcu_420": (lambda: [H.noise(16, 16, 42)], "4:2:0", 75),
    "one_pixel_444": (lambda: [H.noise(1, 1, 43)], "4:4:4", 75),
    "one_pixel_420": (lambda: [H.noise(1, 1, 43)], "4:2:0", 75),
    "dummy_blocks_17x9_420": (lambda: [H.noise(9, 17, 44)], "4:2:0", 90),       # H x W
    "dummy_blocks_9x17_420": (lambda: [H.noise(17, 9, 45)], "4:2:0", 90),
    "edges_17x9_444": (lambda: [H.noise(9, 17, 44)], "4:4:4", 90),
    "edges_9x17_444": (lambda: [H.noise(17, 9, 45)], "4:4:4", 90),
    "eob_only_flat_grey_420": (lambda: [H.flat_grey(48, 64)], "4:2:0", 75),
    "eob_only_flat_grey_444": (lambda: [H.flat_grey(48, 64)], "4:4:4", 75),
    "long_codes_and_stuffing_q100_420": (lambda: [H.harsh_noise(48, 64, 46)], "4:2:0", 100),
    "long_codes_and_stuffing_q100_444": (lambda: [H.harsh_noise(48, 64, 46)], "4:4:4", 100),
    "seams_256x192_420": (lambda: [H.noise(192, 256, 47)], "4:2:0", 95),
    "seams_256x192_444": (lambda: [H.noise(192, 256, 47)], "4:4:4", 95),
}


@pytest.mark.parametrize("name", list(CASES))
def test_device_files_equal_the_host_stage_and_pillow(name, L, dev):
    make, sub, q = CASES[name]
    got, coef, descs = check_images(L, dev, make(), sub, q)
    if name.startswith("long_codes"):
        scan = got[0][623:]
        assert scan.count(b"\xff\x00") > 20 and np.abs(coef.reshape(-1, 64)[:, 1:]).max() >= 512      # stuffing, category-10 AC magnitudes
    if name.startswith("seams"):
        nblocks = descs[0].coef_count // 64
        assert nblocks > 3 * 256 and len(got[0]) - 623 > 3 * 256 * 16             # more than three workgroups of the write and of the stuff launches
    if name.startswith("eob_only"):
        assert np.count_nonzero(coef) <= 3                                       # at most the first DC value of each component


def test_zrl_runs(L, dev):
    a = H.sparse_high_frequency()
    _, coef, descs = check_images(L, dev, [a], "4:2:0", 30)
    tabs = H.tables(H.staging(L, *H.prepare(L, [a.shape[:2]], 3, 30))[0])
    assert H.scan_bits(tabs, coef, descs[0])[1] >= 16                            # the coefficients hold a run that needs ZRL


@pytest.mark.parametrize("seed,rest", [(H.PAD0_SEED, 0), (H.PAD1_SEED, 1)])
def test_padding_at_and_one_bit_past_a_byte_boundary(seed, rest, L, dev):
    a = H.noise(16, 16, seed)
    _, coef, descs = check_images(L, dev, [a], "4:2:0", 75)
    tabs = H.tables(H.staging(L, *H.prepare(L, [a.shape[:2]], 3, 75))[0])
    assert H.scan_bits(tabs, coef, descs[0])[0] % 8 == rest


@pytest.mark.parametrize("sub", list(MODES))
def test_mixed_batch_of_five_equals_the_images_singly(sub, L, dev):
    arrays = [H.noise(192, 256, 47), H.noise(1, 1, 43), H.flat_grey(48, 64), H.noise(9, 17, 44), H.harsh_noise(48, 64, 46)]
    together, _, _ = check_images(L, dev, arrays, sub, 95)                        # B = 5: launches == 6 inside
    for a, t in zip(arrays, together):
        assert check_images(L, dev, [a], sub, 95)[0] == [t]                       # B = 1: launches == 6 inside


@pytest.mark.parametrize("sub", list(MODES))
def test_the_decoder_coefficients_of_a_pillow_file_reproduce_its_scan(sub, L, dev):
    """Arbitrary coefficients: the decoder's buffer of Pillow files, descriptors with srcs = NULL, straight into the device stage."""
    from dan_amd._lib import JpegDesc, JpegInfo
    arrays = [H.noise(40, 56, 51), C.image(100, 131, "smooth"), H.noise(17, 33, 52)]
    datas = [H.pillow(a, 85, sub) for a in arrays]
    B = len(datas)
    info = JpegInfo()
    cap = 0
    for d in datas:
        assert L.danhip_jpeg_inspect(d, len(d), ctypes.byref(info)) == 0
        cap += info.coef_count
    coef = np.zeros(cap, np.int16)
    ddescs = (JpegDesc * B)()
    dstatus = (ctypes.c_int32 * B)()
    ptrs = (ctypes.c_char_p * B)(*datas)
    lens = (ctypes.c_int64 * B)(*[len(d) for d in datas])
    assert L.danhip_jpeg_entropy_decode_batch(ptrs, lens, B, 2, H.vp(coef), cap, ddescs, dstatus) == 0 and list(dstatus) == [0] * B
    descs, totals = H.prepare(L, [a.shape[:2] for a in arrays], MODES[sub], 85)
    assert totals[0] == cap
    out, sizes, status, launches = device_stage(L, dev, coef, descs, totals)
    assert status == [0] * B and launches == 6
    assert H.files_of(out, descs, sizes) == datas


def test_encoder_class_end_to_end_against_the_host_route(L, dev):
    from dan_amd import _lib
    from dan_amd.dataset.jpeg import JpegEncoder
    arrays = [H.noise(192, 256, 47), H.noise(9, 17, 44), H.flat_grey(48, 64), H.sparse_high_frequency(), H.noise(1, 1, 43)]
    tensors = [torch.from_numpy(a).to(dev) for a in arrays]
    for sub, q in (("4:2:0", 75), ("4:4:4", 100), ("4:2:0", 30)):
        host = JpegEncoder(quality=q, subsampling=sub, entropy="host")
        device = JpegEncoder(quality=q, subsampling=sub, entropy="device")
        want = host.encode_batch(tensors)
        assert device.encode_batch(tensors) == want
        assert device.stats["download_bytes"] == 12 * 5 + sum(len(w) for w in want) < host.stats["download_bytes"]      # one batch against one batch
        assert device.encode_batch(tensors) == want                              # the second call runs in the kept buffers
        assert device.encode_batch(tensors[1:2]) == want[1:2]                    # a smaller batch in the same buffers
        assert want == [H.pillow(a, q, sub) for a in arrays]
        s = device.stats
        assert s["entropy_retry"] == 0 and s["entropy_device"] == 11 and s["device"] == 11 and s["host"] == 0
        assert s["entropy_launches"] == 3 * _lib.JPEG_ENCODE_ENTROPY_LAUNCHES and s["launches"] == 3 * _lib.JPEG_ENCODE_LAUNCHES
        assert s["download_bytes"] == 12 * 11 + 2 * sum(len(w) for w in want) + len(want[1])       # sizes, status and the files: no coefficient
        assert device.coef is None
    with pytest.raises(ValueError):
        JpegEncoder(entropy="gpu")


def test_flagged_image_stays_in_its_slot_and_equals_the_emulation(L, dev):
    """A coefficient no baseline code carries: the device flags that image alone and writes nothing outside its slot; the other image's file
    is whole."""
    arrays = [H.noise(24, 40, 21), H.noise(17, 33, 22)]
    coef, descs, totals = H.pixels_host(L, arrays, 3, 90)
    clean = H.host_entropy(L, coef, descs, totals)
    bad = coef.copy()
    bad[descs[0].coef_offset + 64 * 2 + 9] = -32768
    bad[descs[0].coef_offset + 64 * 5] = 32767
    out, sizes, status, launches = device_stage(L, dev, bad, descs, totals)
    assert status[0] == RANGE and sizes[0] == 0 and status[1] == 0 and launches == 6
    assert out[descs[1].file_offset:descs[1].file_offset + sizes[1]].tobytes() == clean[1]
    assert np.all(out[descs[1].file_offset + sizes[1]:] == H.GUARD)
    eout, esizes, estatus, errors = H.emulate(L, bad, descs, totals)
    assert estatus == status and esizes == sizes and errors == 0 and np.array_equal(eout, out)   # the emulation is the kernels' text, slot bytes included


def test_bad_arguments_launch_nothing(L, dev):
    from dan_amd._lib import ptr
    coef, descs, totals = H.pixels_host(L, [H.noise(16, 24, 31)], 3, 75)
    st, _ = H.staging(L, descs, totals)
    with torch.cuda.device(dev):
        buf = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
        launches = ctypes.c_int32(-1)
        args = [H.vp(st), ptr(buf), st.size, descs, 1, ptr(buf), coef.size, ptr(buf), totals[2], ptr(buf), ptr(buf), ptr(buf), 16, ctypes.byref(launches), None]
        assert L.danhip_jpeg_encode_huffman_batch(*args) == -1 and launches.value == 0      # the workspace is too small
        args[12] = buf.numel()
        args[8] = totals[2] - 1
        assert L.danhip_jpeg_encode_huffman_batch(*args) == -1 and launches.value == 0      # not the sizes the staging buffer was made for
        args[8] = totals[2]
        args[1] = None
        assert L.danhip_jpeg_encode_huffman_batch(*args) == -1 and launches.value == 0
        torch.cuda.synchronize()

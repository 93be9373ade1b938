"""The device pixel stage of the JPEG encoder (csrc/jpeg_encode_exact.hip) on the GPU: coefficients equal the host pixel stage's, files
equal the pinned Pillow bytes, over the whole matrix of tests/jpeg_encode_cases.py - all sizes in ONE batched call and once singly, with
the same number of launches; views into the decoder's output buffer as input; the round trip through JpegDecoder.  No tolerance: equality."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_encode_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return C.load_golden()


def _host_coefficients(L, arrays, mode, q):
    from dan_amd._lib import JpegEncDesc
    B = len(arrays)
    descs = (JpegEncDesc * B)()
    widths = (ctypes.c_int32 * B)(*[a.shape[1] for a in arrays])
    heights = (ctypes.c_int32 * B)(*[a.shape[0] for a in arrays])
    srcs = (ctypes.c_void_p * B)(*[a.ctypes.data for a in arrays])
    totals = (ctypes.c_int64 * 3)()
    assert L.danhip_jpeg_encode_prepare(widths, heights, srcs, B, mode, q, descs, totals) == 0
    coef = np.zeros(totals[0], np.int16)
    assert L.danhip_jpeg_encode_pixels_host(descs, B, ctypes.c_void_p(coef.ctypes.data), totals[0]) == 0
    return coef


@pytest.mark.parametrize("sub,mode", C.MODES)
@pytest.mark.parametrize("q", C.QUALITIES)
def test_device_equals_host_and_golden_batched_and_singly(sub, mode, q, dev, golden):
    from dan_amd import _lib
    from dan_amd.dataset.jpeg import JpegEncoder
    files, inputs = golden
    L = _lib.lib()
    for content in C.CONTENTS:
        arrays = [inputs[(h, w, content)] for (h, w) in C.SIZES]
        want = [files["%dx%d_%s_%s_q%d" % (h, w, content, sub.replace(":", ""), q)] for (h, w) in C.SIZES]
        tensors = [torch.from_numpy(a).to(dev) for a in arrays]
        enc = JpegEncoder(quality=q, subsampling=sub)
        got = enc.encode_batch(tensors)                                       # B = 7, mixed sizes, ONE call
        assert enc.stats["launches"] == _lib.JPEG_ENCODE_LAUNCHES == 2 and enc.stats["device"] == 7
        assert np.array_equal(enc.coef.numpy(), _host_coefficients(L, arrays, mode, q)), (content, "coefficients")
        assert got == want, (content, [i for i in range(7) if got[i] != want[i]])
        for i, t in enumerate(tensors):                                        # B = 1: the same launches
            one = JpegEncoder(quality=q, subsampling=sub)
            assert one.encode(t) == want[i], (content, C.SIZES[i])
            assert one.stats["launches"] == 2
            assert np.array_equal(one.coef.numpy(), _host_coefficients(L, [arrays[i]], mode, q)), (content, C.SIZES[i])


def test_round_trip_and_views_into_the_decoder_buffer(dev, golden):
    """Encode on the device, decode with JpegDecoder: the Pillow decode of the Pillow encode.  The decoder's outputs are views into one
    buffer at 256-byte offsets: encoded from where they lie, they give the host encoder's files."""
    Image = pytest.importorskip("PIL.Image")
    from dan_amd.dataset.jpeg import JpegDecoder, JpegEncoder
    files, inputs = golden
    arrays = [inputs[(h, w, "smooth")] for (h, w) in C.SIZES[2:]] + [inputs[(100, 131, "noise")]]
    tensors = [torch.from_numpy(a).to(dev) for a in arrays]
    datas = JpegEncoder(quality=75).encode_batch(tensors)
    dec = JpegDecoder(dev)
    decoded = dec.decode_batch(datas)
    assert dec.stats["device"] == len(datas) and dec.stats["fallback"] == {}
    for a, d in zip(arrays, decoded):
        want = np.asarray(Image.open(io.BytesIO(C.pillow_bytes(a, 75, "4:2:0"))).convert("RGB"))
        assert np.array_equal(d.cpu().numpy(), want), a.shape
    assert len(set(d.untyped_storage().data_ptr() for d in decoded)) == 1          # views of one allocation
    again = JpegEncoder(quality=95, subsampling="4:4:4").encode_batch(decoded)
    L = C.host_lib()
    for d, data in zip(decoded, again):
        assert data == C.encode_host(L, np.ascontiguousarray(d.cpu().numpy()), 95, 1), tuple(d.shape)


def test_launcher_refuses_descriptors_that_do_not_fit(dev):
    from dan_amd import _lib
    from dan_amd._lib import JpegEncDesc
    L = _lib.lib()
    img = torch.zeros((24, 40, 3), dtype=torch.uint8, device=dev)
    descs = (JpegEncDesc * 1)()
    totals = (ctypes.c_int64 * 3)()
    assert L.danhip_jpeg_encode_prepare((ctypes.c_int32 * 1)(40), (ctypes.c_int32 * 1)(24), (ctypes.c_void_p * 1)(img.data_ptr()), 1, 3, 75, descs, totals) == 0
    table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
    coef = torch.empty(totals[0], dtype=torch.int16, device=dev)
    ws = torch.empty(totals[1], dtype=torch.uint8, device=dev)
    n = ctypes.c_int32(-1)
    args = lambda cc, wsb: (descs, _lib.ptr(table), 1, _lib.ptr(coef), cc, _lib.ptr(ws), wsb, ctypes.byref(n), _lib.stream())
    assert L.danhip_jpeg_encode_pixels_batch(*args(totals[0] - 64, totals[1])) != 0 and n.value == 0          # coefficients leave the buffer
    assert L.danhip_jpeg_encode_pixels_batch(*args(totals[0], totals[1] - 256)) != 0 and n.value == 0         # a plane leaves the workspace
    descs[0].fdct_groups += 1
    assert L.danhip_jpeg_encode_pixels_batch(*args(totals[0], totals[1])) != 0 and n.value == 0               # re-derived, not trusted
    descs[0].fdct_groups -= 1
    assert L.danhip_jpeg_encode_pixels_batch(*args(totals[0], totals[1])) == 0 and n.value == 2
    torch.cuda.synchronize()

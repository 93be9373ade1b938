"""Baseline JPEG records decoded on the device, bit for bit what Pillow (libjpeg-turbo, JDCT_ISLOW, fancy upsampling) gives.

The serial half (markers, Huffman) runs in libdanhip on a few host threads (csrc/jpeg_entropy.cpp) and leaves quantised coefficients in a
pinned buffer; dequantisation, inverse DCT, chroma upsampling and colour conversion are two launches per BATCH (csrc/jpeg_exact.hip).
A stream the host validator refuses (progressive, CMYK, 4:1:1, truncated, ... - include/danhip.h lists the reason codes) never reaches
the device: it goes through dataset_common.decode_image (Pillow) and is counted in `stats`.

    dec = JpegDecoder(torch.device("cuda:0"))
    images = dec.decode_batch([record_bytes, ...])        # uint8 [H,W,3] device tensors: what preprocess_for_train takes"""
import ctypes
import time

import torch

from .._lib import JpegDesc, JpegInfo, call, lib, ptr, stream
from . import dataset_common

MAX_THREADS = 16                                          # DANHIP_JPEG_MAX_THREADS
REASONS = {1: "not_jpeg", 2: "truncated", 3: "progressive", 4: "arithmetic", 5: "precision", 6: "multiscan", 7: "components", 8: "adobe",
           9: "rgb_ids", 10: "sampling", 11: "huffman", 12: "too_large", 13: "table", 14: "unsupported", 15: "restart", 16: "coef_range",
           17: "capacity"}
_DESC_BYTES = ctypes.sizeof(JpegDesc)


def _align(v, a=256):
    return (v + a - 1) // a * a


class JpegDecoder(object):
    def __init__(self, device, threads=4):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("JpegDecoder decodes on the GPU; use dataset_common.decode_image on the host")
        self.threads = max(1, min(int(threads), MAX_THREADS))
        self.stats = {"device": 0, "fallback": {}, "launches": 0, "entropy_seconds": 0.0}
        self._pinned = None                               # [descriptors | coefficients] of the batch in flight
        self._uploaded = None                             # event after the upload that reads _pinned

    def decode(self, encoded):
        return self.decode_batch([encoded])[0]

    def _staging(self, nbytes):
        if self._uploaded is not None:                    # the previous batch's upload still reads the buffer
            self._uploaded.synchronize()
            self._uploaded = None
        if self._pinned is None or self._pinned.numel() < nbytes:
            self._pinned = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8).pin_memory()
        return self._pinned

    def decode_batch(self, encoded_list):
        """list of bytes -> list of uint8 [H,W,3] device tensors (views of one allocation for the device-decoded ones)."""
        datas = [bytes(e) for e in encoded_list]
        B = len(datas)
        if B == 0:
            return []
        if B > 65535:
            return self.decode_batch(datas[:65535]) + self.decode_batch(datas[65535:])
        L = lib()
        info = JpegInfo()
        capacity = 0
        for d in datas:                                   # headers only: the size of the coefficient buffer
            if L.danhip_jpeg_inspect(d, len(d), ctypes.byref(info)) == 0:
                capacity += info.coef_count
        head = _align(B * _DESC_BYTES)
        pinned = self._staging(head + 2 * capacity)
        base = pinned.data_ptr()
        descs = (JpegDesc * B).from_address(base)
        status = (ctypes.c_int32 * B)()
        ptrs = (ctypes.c_char_p * B)(*datas)
        sizes = (ctypes.c_int64 * B)(*[len(d) for d in datas])
        t0 = time.perf_counter()
        call("danhip_jpeg_entropy_decode_batch", ptrs, sizes, B, self.threads, ctypes.c_void_p(base + head), capacity, descs, status)
        self.stats["entropy_seconds"] += time.perf_counter() - t0
        out_bytes = L.danhip_jpeg_output_bytes(descs, B)
        results = [None] * B
        if out_bytes > 0:                                 # at least one image for the device
            with torch.cuda.device(self.device):
                dev_in = torch.empty(head + 2 * capacity, dtype=torch.uint8, device=self.device)
                dev_in.copy_(pinned[:head + 2 * capacity], non_blocking=True)          # descriptors and coefficients: one upload
                self._uploaded = torch.cuda.Event()
                self._uploaded.record()
                ws_bytes = L.danhip_jpeg_workspace_bytes(descs, B)
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
                out = torch.empty(out_bytes, dtype=torch.uint8, device=self.device)
                launches = ctypes.c_int32(0)
                call("danhip_jpeg_reconstruct_batch", ctypes.c_void_p(dev_in.data_ptr() + head), capacity, descs, ptr(dev_in), B, ptr(out),
                     out_bytes, ptr(ws), ws_bytes, ctypes.byref(launches), stream())
            self.stats["launches"] += launches.value
            for i in range(B):
                if status[i] == 0:
                    d = descs[i]
                    results[i] = out[d.out_offset:d.out_offset + d.height * d.width * 3].view(d.height, d.width, 3)
                    self.stats["device"] += 1
        for i in range(B):
            if status[i] != 0:
                name = REASONS.get(status[i], str(status[i]))
                self.stats["fallback"][name] = self.stats["fallback"].get(name, 0) + 1
                results[i] = torch.from_numpy(dataset_common.decode_image(datas[i]).copy()).to(self.device)
        return results

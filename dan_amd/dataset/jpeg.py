"""Baseline - and, opt-in, complete progressive - JPEG records decoded on the device, bit for bit what Pillow (libjpeg-turbo, JDCT_ISLOW,
fancy upsampling) gives.

By default the serial half (markers, Huffman) runs in libdanhip on a few host threads (csrc/jpeg_entropy.cpp) and leaves quantised
coefficients in a pinned buffer; dequantisation, inverse DCT, chroma upsampling and colour conversion are two launches per BATCH
(csrc/jpeg_exact.hip).  With entropy="device" the host keeps the markers alone: one pass over the scan that looks for FF only, then the
stuffed stream itself is uploaded and a self-synchronising parallel Huffman decoder (csrc/jpeg_huffman_exact.hip, a fixed number of
launches per BATCH) writes the same coefficient buffer, bit for bit, on the device.  One copy of a status word per image comes back; an
image the device stage gave up on goes through the host stage, which stays the authority (stats["entropy_retry"]).
A stream the host validator refuses (progressive, CMYK, 4:1:1, truncated, ... - include/danhip.h lists the reason codes) never reaches
the device: it goes through dataset_common.decode_image (Pillow) and is counted in `stats`.

progressive=True also takes SOF2 frames (stats["progressive"] counts them): 8 bit, Huffman, the same component counts and sampling modes,
any number of scans whose script obeys T.81 G.1.1.1.1 (Ss = 0 implies Se = 0; AC scans carry one component; Al <= 13; Ah = 0 on a
coefficient's first scan, afterwards Ah = its previous Al and Al = Ah - 1; DC before AC; nothing twice at the same precision), DHT and DRI
between scans - and COMPLETE at EOI: every coefficient of every component sent down to Al = 0.  Their entropy stage is the host's whatever
`entropy` says (with entropy="device" they are counted in stats["entropy_retry"], as any host-only image); behind the coefficient buffer
the same two launches run, unchanged.  The completion rule exists because libjpeg decodes an incomplete progression through another path
(inter-block smoothing, coarse coefficients left as they are) that the kernels have no counterpart for: such a file, like any other
script the validator does not take, is refused with reason "progression" and goes to Pillow.  The default stays False: a progressive
record then takes the fallback as before (reason "progressive").

    dec = JpegDecoder(torch.device("cuda:0"))
    images = dec.decode_batch([record_bytes, ...])        # uint8 [H,W,3] device tensors: what preprocess_for_train takes

JpegEncoder is the mirror: uint8 [H,W,3] RGB images -> baseline JFIF files, byte for byte what Pillow writes with
save(f, "JPEG", quality=q, subsampling=s) and, with optimize=True, save(..., optimize=True) (no progressive).  Colour conversion, chroma downsampling, forward DCT and quantisation
are two launches per BATCH on the device (csrc/jpeg_encode_exact.hip); the quantised coefficients come back in one download - in the layout the
decoder's entropy stage produces - and host threads write the Huffman scan and the markers (csrc/jpeg_encode.cpp).  Images in host memory
(numpy arrays, CPU tensors) run the same integer code on the host, which is also what a process without a GPU gets.

    enc = JpegEncoder(quality=75, subsampling="4:2:0")
    files = enc.encode_batch(images)                      # list of bytes; the images may be views into the decoder's output buffer

With entropy="device" (opt-in; device images only) the Huffman stage runs on the device as well (csrc/jpeg_encode_huffman_exact.hip, six
launches per BATCH): block lengths, prefix sums, the codes written at their bit offsets, FF stuffing, markers and EOI.  The files are the
same bytes.  No coefficient comes back: one download brings sizes and status words, one more the files themselves, packed back to back on
the device first.  An image the device stage flags, or leaves to the host for its size, goes through the host stage, which stays the
authority (stats["entropy_retry"]).

optimize=True (off by default) gives the same pixels in a smaller file, as Pillow's flag of that name does: each image's Huffman tables are
made from its own symbol statistics by libjpeg's rule (csrc/jpeg_encode.h) and the four DHT segments carry them.  The host stage counts
and builds on its threads; the device stage puts three launches in front of its six - clear, a histogram of the coefficient blocks'
symbols, the tables - so that still no coefficient comes back.  Both stages give Pillow's bytes."""
import ctypes
import time

import numpy as np
import torch

from .._lib import JPEG_ENC_OPTIMIZE, JpegDesc, JpegEncDesc, JpegInfo, call, lib, ptr, stream
from . import dataset_common

MAX_THREADS = 16                                          # DANHIP_JPEG_MAX_THREADS
REASONS = {1: "not_jpeg", 2: "truncated", 3: "progressive", 4: "arithmetic", 5: "precision", 6: "multiscan", 7: "components", 8: "adobe",
           9: "rgb_ids", 10: "sampling", 11: "huffman", 12: "too_large", 13: "table", 14: "unsupported", 15: "restart", 16: "coef_range",
           17: "capacity", 18: "progression"}
ALLOW_PROGRESSIVE = 1                                     # DANHIP_JPEG_ALLOW_PROGRESSIVE
_DESC_BYTES = ctypes.sizeof(JpegDesc)


def _align(v, a=256):
    return (v + a - 1) // a * a


class JpegDecoder(object):
    def __init__(self, device, threads=4, entropy="host", progressive=False):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("JpegDecoder decodes on the GPU; use dataset_common.decode_image on the host")
        if entropy not in ("host", "device"):
            raise ValueError("entropy must be 'host' or 'device', got %r" % (entropy,))
        self.entropy = entropy
        self.threads = max(1, min(int(threads), MAX_THREADS))
        self.flags = ALLOW_PROGRESSIVE if progressive else 0
        # entropy_device: images whose coefficients came from the device; entropy_retry: images the device stage handed back to the host stage;
        # progressive: progressive images the host stage decoded (progressive=True)
        self.stats = {"device": 0, "fallback": {}, "launches": 0, "entropy_seconds": 0.0, "entropy_device": 0, "entropy_retry": 0,
                      "upload_bytes": 0, "huffman_ms": None, "progressive": 0}
        self.time_huffman = False                         # diagnosis (tools/bench_jpeg_entropy.py): device-event time of the Huffman launches
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
        return self._decode_device_entropy(datas) if self.entropy == "device" else self._decode_host_entropy(datas)

    def _fallback(self, datas, status, results):
        for i in range(len(datas)):
            if status[i] > 0:
                name = REASONS.get(status[i], str(status[i]))
                self.stats["fallback"][name] = self.stats["fallback"].get(name, 0) + 1
                results[i] = torch.from_numpy(dataset_common.decode_image(datas[i]).copy()).to(self.device)
        return results

    def _decode_host_entropy(self, datas):
        B = len(datas)
        L = lib()
        info = JpegInfo()
        capacity = 0
        # headers only: the size of the coefficient buffer.  A progressive stream's header is its scan script, so with progressive=True its
        # markers are walked to EOI here and again in the batch call's serial header loop (and once more by the prepare call with
        # entropy="device") before the threaded decode: memchr passes, small next to the entropy stage, but serial work per image that a
        # baseline stream does not have.  A batch call that reports the capacity itself would save them.
        for d in datas:
            if L.danhip_jpeg_inspect_ex(d, len(d), self.flags, ctypes.byref(info)) == 0:
                capacity += info.coef_count
        head = _align(B * _DESC_BYTES)
        pinned = self._staging(head + 2 * capacity)
        base = pinned.data_ptr()
        descs = (JpegDesc * B).from_address(base)
        status = (ctypes.c_int32 * B)()
        ptrs = (ctypes.c_char_p * B)(*datas)
        sizes = (ctypes.c_int64 * B)(*[len(d) for d in datas])
        t0 = time.perf_counter()
        call("danhip_jpeg_entropy_decode_batch_ex", ptrs, sizes, B, self.threads, self.flags, ctypes.c_void_p(base + head), capacity, descs, status)
        self.stats["entropy_seconds"] += time.perf_counter() - t0
        out_bytes = L.danhip_jpeg_output_bytes(descs, B)
        results = [None] * B
        if out_bytes > 0:                                 # at least one image for the device
            with torch.cuda.device(self.device):
                dev_in = torch.empty(head + 2 * capacity, dtype=torch.uint8, device=self.device)
                dev_in.copy_(pinned[:head + 2 * capacity], non_blocking=True)          # descriptors and coefficients: one upload
                self.stats["upload_bytes"] += head + 2 * capacity
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
                    self.stats["progressive"] += d.reserved[0]            # 1: a progressive frame
        return self._fallback(datas, status, results)

    def _decode_device_entropy(self, datas):
        """Markers on the host, Huffman on the device; the images whose device status is not 0 go through _decode_host_entropy."""
        B = len(datas)
        L = lib()
        info = JpegInfo()
        capacity = 0
        for d in datas:
            if L.danhip_jpeg_inspect_ex(d, len(d), self.flags, ctypes.byref(info)) == 0:
                capacity += info.coef_count
        ptrs = (ctypes.c_char_p * B)(*datas)
        sizes = (ctypes.c_int64 * B)(*[len(d) for d in datas])
        need = L.danhip_jpeg_scan_staging_bytes(ptrs, sizes, B)
        head = _align(B * _DESC_BYTES)
        pinned = self._staging(head + need)
        base = pinned.data_ptr()
        descs = (JpegDesc * B).from_address(base)
        status = (ctypes.c_int32 * B)()
        staging = ctypes.c_void_p(base + head)
        t0 = time.perf_counter()
        call("danhip_jpeg_scan_prepare_batch_ex", ptrs, sizes, B, self.flags, staging, need, capacity, descs, status)
        self.stats["entropy_seconds"] += time.perf_counter() - t0
        used = L.danhip_jpeg_scan_device_bytes(staging)
        out_bytes = L.danhip_jpeg_output_bytes(descs, B)
        results = [None] * B
        retry = [i for i in range(B) if status[i] < 0]    # DANHIP_JPEG_HOSTONLY (a progressive frame among them)
        if out_bytes > 0:                                 # at least one image for the device
            with torch.cuda.device(self.device):
                dev_in = torch.empty(head + used, dtype=torch.uint8, device=self.device)
                dev_in.copy_(pinned[:head + used], non_blocking=True)                  # descriptors, tables and the stuffed streams: one upload
                self.stats["upload_bytes"] += head + used
                self._uploaded = torch.cuda.Event()
                self._uploaded.record()
                coef = torch.empty(max(capacity, 8), dtype=torch.int16, device=self.device)
                hws_bytes = L.danhip_jpeg_scan_workspace_bytes(staging)
                hws = torch.empty(hws_bytes, dtype=torch.uint8, device=self.device)
                dev_status = torch.empty(B, dtype=torch.int32, device=self.device)
                ws_bytes = L.danhip_jpeg_workspace_bytes(descs, B)
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
                out = torch.empty(out_bytes, dtype=torch.uint8, device=self.device)
                n_huff, n_rec = ctypes.c_int32(0), ctypes.c_int32(0)
                if self.time_huffman:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                call("danhip_jpeg_huffman_decode_batch", staging, ctypes.c_void_p(dev_in.data_ptr() + head), used, B, ptr(coef), capacity, descs,
                     ptr(dev_in), ptr(hws), hws_bytes, ptr(dev_status), ctypes.byref(n_huff), stream())
                if self.time_huffman:
                    e1.record()
                # the geometry comes from the header: the pair can be enqueued before any status is known
                call("danhip_jpeg_reconstruct_batch", ptr(coef), capacity, descs, ptr(dev_in), B, ptr(out), out_bytes, ptr(ws), ws_bytes,
                     ctypes.byref(n_rec), stream())
                host_status = dev_status.cpu().tolist()   # the one synchronisation this path adds
                if self.time_huffman:
                    self.stats["huffman_ms"] = (self.stats["huffman_ms"] or 0.0) + e0.elapsed_time(e1)
            self.coef = coef                              # the last batch's coefficient buffer (tests compare it with the host stage's)
            self.stats["launches"] += n_huff.value + n_rec.value
            for i in range(B):
                if status[i] != 0:
                    continue
                if host_status[i] != 0:
                    retry.append(i)
                    continue
                d = descs[i]
                results[i] = out[d.out_offset:d.out_offset + d.height * d.width * 3].view(d.height, d.width, 3)
                self.stats["device"] += 1
                self.stats["entropy_device"] += 1
        refused = [int(v) for v in status]
        if retry:                                         # the host stage decodes them, or names the reason and they take the Pillow fallback
            retry.sort()
            self.stats["entropy_retry"] += len(retry)
            again = self._decode_host_entropy([datas[i] for i in retry])
            for i, image in zip(retry, again):
                results[i] = image
        return self._fallback(datas, refused, results)


MODE_444, MODE_420 = 1, 3                                 # DANHIP_JPEG_444, DANHIP_JPEG_420
_SUBSAMPLING = {0: MODE_444, "4:4:4": MODE_444, 2: MODE_420, "4:2:0": MODE_420}      # Pillow's names for them


class JpegEncoder(object):
    def __init__(self, quality=75, subsampling="4:2:0", threads=4, entropy="host", optimize=False):
        if entropy not in ("host", "device"):
            raise ValueError("entropy must be 'host' or 'device', got %r" % (entropy,))
        if subsampling not in _SUBSAMPLING:
            raise ValueError("subsampling must be '4:2:0' (2) or '4:4:4' (0), got %r" % (subsampling,))
        if not 1 <= int(quality) <= 100:
            raise ValueError("quality must be 1 .. 100, got %r" % (quality,))
        self.quality = int(quality)
        self.mode = _SUBSAMPLING[subsampling]
        self.threads = max(1, min(int(threads), MAX_THREADS))
        self.entropy = entropy
        self.optimize = bool(optimize)
        self.stats = {"device": 0, "host": 0, "launches": 0, "entropy_seconds": 0.0, "download_bytes": 0, "entropy_device": 0,
                      "entropy_launches": 0, "entropy_retry": 0}
        self.coef = None                                  # the last device batch's coefficients on the host (tests compare them)
        self._buffers = {}                                # entropy="device": workspace, files and result words, kept and grown across calls

    def encode(self, image):
        return self.encode_batch([image])[0]

    def encode_batch(self, images):
        """list of uint8 [H,W,3] RGB images -> list of bytes.  Device tensors (separate, or views into one buffer) take the device pixel
        stage in one batch; numpy arrays and CPU tensors take the host's.  The two may be mixed."""
        images = list(images)
        results = [None] * len(images)
        on_device = [i for i, im in enumerate(images) if torch.is_tensor(im) and im.is_cuda]
        on_host = [i for i in range(len(images)) if i not in set(on_device)]
        for at in range(0, len(on_device), 65535):
            part = on_device[at:at + 65535]
            for i, data in zip(part, self._encode([images[i] for i in part], True, self.entropy == "device")):
                results[i] = data
        for at in range(0, len(on_host), 65535):
            part = on_host[at:at + 65535]
            host = [np.ascontiguousarray(im.numpy() if torch.is_tensor(im) else im) for im in (images[i] for i in part)]
            for i, data in zip(part, self._encode(host, False)):
                results[i] = data
        return results

    def _buffer(self, name, nbytes, dev):
        """A device byte buffer of at least nbytes, kept across calls and grown by half as much again when it is too small."""
        t = self._buffers.get(name)
        if t is None or t.device != dev or t.numel() < nbytes:
            t = torch.empty(max(nbytes + nbytes // 2, 256), dtype=torch.uint8, device=dev)
            self._buffers[name] = t
        return t

    def _entropy_device(self, images, descs, totals, coef_dev, dev):
        """The device Huffman stage behind the pixel stage (called under torch.cuda.device(dev)) -> list of bytes."""
        L = lib()
        B, ncoef, nfile = len(images), totals[0], totals[2]
        nstaging = L.danhip_jpeg_encode_scan_staging_bytes(B)
        staging = torch.empty(nstaging, dtype=torch.uint8, pin_memory=True)
        prepared = (ctypes.c_int32 * B)()
        if self.optimize:
            call("danhip_jpeg_encode_scan_prepare_ex", descs, B, ncoef, nfile, JPEG_ENC_OPTIMIZE, ctypes.c_void_p(staging.data_ptr()), nstaging,
                 prepared)
        else:
            call("danhip_jpeg_encode_scan_prepare", descs, B, ncoef, nfile, ctypes.c_void_p(staging.data_ptr()), nstaging, prepared)
        staging_dev = staging.to(dev, non_blocking=True)
        ws = self._buffer("workspace", max(L.danhip_jpeg_encode_scan_workspace_bytes(ctypes.c_void_p(staging.data_ptr())), 16), dev)
        files = self._buffer("files", nfile, dev)
        words = self._buffer("words", 12 * B, dev)        # int64 sizes[B], then int32 status[B]
        launches = ctypes.c_int32(0)
        call("danhip_jpeg_encode_huffman_batch", ctypes.c_void_p(staging.data_ptr()), ptr(staging_dev), nstaging, descs, B, ptr(coef_dev), ncoef,
             ptr(files), nfile, ctypes.c_void_p(words.data_ptr()), ctypes.c_void_p(words.data_ptr() + 8 * B), ptr(ws), ws.numel(),
             ctypes.byref(launches), stream())
        self.stats["entropy_launches"] += launches.value
        if launches.value:
            host_words = words[:12 * B].cpu()             # download 1: sizes and status
            self.stats["download_bytes"] += 12 * B
            sizes = host_words[:8 * B].view(torch.int64).tolist()
            status = host_words[8 * B:].view(torch.int32).tolist()
        else:                                             # nothing was prepared: every status is the prepare call's
            sizes, status = [0] * B, list(prepared)
        good = [i for i in range(B) if status[i] == 0]
        results = [None] * B
        if good:
            packed = torch.cat([files[descs[i].file_offset:descs[i].file_offset + sizes[i]] for i in good]).cpu()     # download 2: the files
            self.stats["download_bytes"] += packed.numel()
            data = packed.numpy().tobytes()
            at = 0
            for i in good:
                results[i] = data[at:at + sizes[i]]
                at += sizes[i]
        self.stats["entropy_device"] += len(good)
        retry = [i for i in range(B) if status[i] != 0]
        if retry:                                         # the host stage has the last word (and raises for a value no baseline code carries)
            self.stats["entropy_retry"] += len(retry)
            self.stats["device"] -= len(retry)            # _encode counts them again
            for i, data in zip(retry, self._encode([images[i] for i in retry], True, False)):
                results[i] = data
        return results

    def _encode(self, images, device, entropy_device=False):
        B = len(images)
        for im in images:
            if tuple(im.shape[2:]) != (3,) or len(im.shape) != 3 or str(im.dtype) not in ("torch.uint8", "uint8"):
                raise ValueError("JpegEncoder takes uint8 [H,W,3] images, got %s %s" % (im.dtype, tuple(im.shape)))
        if device:
            images = [im.contiguous() for im in images]
            if len(set(im.device for im in images)) != 1:
                raise ValueError("JpegEncoder: the images of a batch lie on one device")
        L = lib()
        nbytes = B * ctypes.sizeof(JpegEncDesc)
        table = torch.empty(max(nbytes, 1), dtype=torch.uint8, pin_memory=device)
        descs = (JpegEncDesc * B).from_address(table.data_ptr())
        widths = (ctypes.c_int32 * B)(*[int(im.shape[1]) for im in images])
        heights = (ctypes.c_int32 * B)(*[int(im.shape[0]) for im in images])
        srcs = (ctypes.c_void_p * B)(*[im.data_ptr() if device else im.ctypes.data for im in images])
        totals = (ctypes.c_int64 * 3)()
        call("danhip_jpeg_encode_prepare", widths, heights, srcs, B, self.mode, self.quality, descs, totals)
        ncoef = totals[0]
        if device:
            dev = images[0].device
            with torch.cuda.device(dev):
                table_dev = table.to(dev, non_blocking=True)
                coef_dev = torch.empty(ncoef, dtype=torch.int16, device=dev)
                ws = torch.empty(max(totals[1], 16), dtype=torch.uint8, device=dev)
                launches = ctypes.c_int32(0)
                call("danhip_jpeg_encode_pixels_batch", descs, ptr(table_dev), B, ptr(coef_dev), ncoef, ptr(ws), ws.numel(), ctypes.byref(launches),
                     stream())
                self.stats["launches"] += launches.value
                self.stats["device"] += B
                if entropy_device:
                    t0 = time.perf_counter()
                    results = self._entropy_device(images, descs, totals, coef_dev, dev)
                    self.stats["entropy_seconds"] += time.perf_counter() - t0
                    return results
                coef = coef_dev.cpu()                     # the one download
            self.coef = coef
            self.stats["download_bytes"] += 2 * ncoef
        else:
            coef = torch.empty(ncoef, dtype=torch.int16)
            call("danhip_jpeg_encode_pixels_host", descs, B, ctypes.c_void_p(coef.data_ptr()), ncoef)
            self.stats["host"] += B
        files = np.empty(totals[2], dtype=np.uint8)       # the bound of every file; pages a file does not reach are never touched
        sizes = (ctypes.c_int64 * B)()
        t0 = time.perf_counter()
        if self.optimize:
            call("danhip_jpeg_encode_entropy_batch_ex", ctypes.c_void_p(coef.data_ptr()), ncoef, descs, B, self.threads, JPEG_ENC_OPTIMIZE,
                 ctypes.c_void_p(files.ctypes.data), totals[2], sizes)
        else:
            call("danhip_jpeg_encode_entropy_batch", ctypes.c_void_p(coef.data_ptr()), ncoef, descs, B, self.threads,
                 ctypes.c_void_p(files.ctypes.data), totals[2], sizes)
        self.stats["entropy_seconds"] += time.perf_counter() - t0
        return [files[descs[i].file_offset:descs[i].file_offset + sizes[i]].tobytes() for i in range(B)]

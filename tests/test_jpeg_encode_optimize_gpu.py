"""The JPEG encoder's optimize=True on the GPU (csrc/jpeg_encode_huffman_exact.hip: the clear, histogram and tables launches in front of
the six of the Huffman stage): the device's symbol counts equal a plain count of the same blocks, its tables the host rule's, its files the
host stage's and Pillow's save(optimize=True) byte for byte - whatever the order of the batch - the launch count is the sum of the three
constants, no optimised file is longer than the standard-table one, and a flagged image stays in its slot.  No tolerance: equality."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_encode_huffman_cases as H  # noqa: E402
import jpeg_optimal_table as T  # noqa: E402

pytestmark = pytest.mark.gpu

RANGE = 1                                     # DANHIP_JPEG_ENC_DEV_RANGE


@pytest.fixture(scope="module")
def L():
    from dan_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def layout(L):
    out = (ctypes.c_int32 * 8)()
    L.danhip_jpeg_encode_optimize_layout(out)
    return dict(zip(("stride", "counts", "tabs", "bitsvals", "words", "header", "item_blocks", "header_max"), out))


def device_stage(L, dev, coef, descs, totals, guard=0):
    """danhip_jpeg_encode_huffman_batch over a staging buffer prepared with DANHIP_JPEG_ENC_OPTIMIZE -> (files buffer with `guard` bytes of
    GUARD on either side, sizes, status, launches, workspace)."""
    from dan_amd._lib import ptr, stream
    B = len(descs)
    n = L.danhip_jpeg_encode_scan_staging_bytes(B)
    raw = np.zeros(n + 16, np.uint8)
    at = (-raw.ctypes.data) % 16
    st = raw[at:at + n]
    pstatus = (ctypes.c_int32 * B)()
    assert L.danhip_jpeg_encode_scan_prepare_ex(descs, B, totals[0], totals[2], 1, H.vp(st), n, pstatus) == 0, L.danhip_last_error()
    assert list(pstatus) == [0] * B
    with torch.cuda.device(dev):
        st_dev = torch.from_numpy(st.copy()).to(dev)
        coef_dev = torch.from_numpy(coef).to(dev)
        files = torch.full((totals[2] + 2 * guard,), H.GUARD, dtype=torch.uint8, device=dev)
        sizes = torch.full((B,), -7, dtype=torch.int64, device=dev)
        status = torch.full((B,), -7, dtype=torch.int32, device=dev)
        nws = L.danhip_jpeg_encode_scan_workspace_bytes(H.vp(st))
        ws = torch.full((nws,), 0x5A, dtype=torch.uint8, device=dev)           # exactly the queried size, not zeroed
        launches = ctypes.c_int32(-1)
        rc = L.danhip_jpeg_encode_huffman_batch(H.vp(st), ptr(st_dev), st.size, descs, B, ptr(coef_dev), coef.size,
                                                ctypes.c_void_p(files.data_ptr() + guard), totals[2], ptr(sizes), ptr(status), ptr(ws), nws,
                                                ctypes.byref(launches), stream())
        assert rc == 0, L.danhip_last_error()
        return files.cpu().numpy(), sizes.cpu().tolist(), status.cpu().tolist(), launches.value, ws.cpu().numpy()


def region_counts(ws, layout, i):
    at = i * layout["stride"] + layout["counts"]
    return torch.from_numpy(ws[at:at + 4 * 257 * 4].view(np.uint32).astype(np.int64).reshape(4, 257))


def region_bits_vals(ws, layout, i, t):
    at = i * layout["stride"] + layout["bitsvals"] + t * 273
    return ws[at:at + 17].tolist(), ws[at + 17:at + 273].tolist()


@pytest.fixture(scope="module")
def batch(L, dev):
    """The image set of the CPU test as ONE batch of different sizes, 4:2:0 at quality 75, through the device stage once: shared, unchanged."""
    named = T.images()
    arrays = [a for _, a in named]
    coef, descs, totals = H.pixels_host(L, arrays, 3, 75)
    out, sizes, status, launches, ws = device_stage(L, dev, coef, descs, totals)
    return {"arrays": arrays, "names": [n for n, _ in named], "coef": coef, "descs": descs, "totals": totals, "out": out, "sizes": sizes,
            "status": status, "launches": launches, "ws": ws}


def test_histogram_of_a_batch_of_different_sizes(batch, layout):
    assert batch["status"] == [0] * len(batch["arrays"])
    for i, name in enumerate(batch["names"]):
        want = torch.from_numpy(T.symbol_counts(batch["coef"], batch["descs"][i]))
        assert torch.equal(region_counts(batch["ws"], layout, i), want), name


@pytest.mark.parametrize("sub,mode,h,w", [("4:2:0", 3, 336, 336), ("4:4:4", 1, 232, 240)])
def test_histogram_where_the_kernel_loops_and_workgroups_share_a_table(sub, mode, h, w, L, dev, layout):
    """About 2.5 work items of blocks: two workgroups run every round of the loop, a third a partial one, all add into one table."""
    a = H.noise(h, w, 91)
    coef, descs, totals = H.pixels_host(L, [a], mode, 60)
    nblocks = descs[0].coef_count // 64
    assert 2.2 * layout["item_blocks"] < nblocks < 3 * layout["item_blocks"] and nblocks % layout["item_blocks"] % 256 != 0
    out, sizes, status, launches, ws = device_stage(L, dev, coef, descs, totals)
    assert status == [0]
    assert torch.equal(region_counts(ws, layout, 0), torch.from_numpy(T.symbol_counts(coef, descs[0])))
    assert H.files_of(out, descs, sizes) == [T.pillow_optimized(a, 60, sub)]


def test_tables_launch_equals_the_host_rule(batch, layout, L, dev):
    """bits / vals of every image and table of the batch, and of count sets fed to the tables launch directly (the Fibonacci set among
    them: the cut to 16 bits), against danhip_jpeg_optimal_table_host."""
    from dan_amd._lib import ptr, stream
    for i in range(len(batch["arrays"])):
        counts = region_counts(batch["ws"], layout, i).numpy()
        for t in range(4):
            rc, bits, vals = T.host_table(L, counts[t])
            assert rc == 0 and region_bits_vals(batch["ws"], layout, i, t) == (bits, vals), (batch["names"][i], t)
    sets = T.count_sets()
    names = list(sets)
    groups = [names[k:k + 4] for k in range(0, len(names), 4)]
    regions = np.full(len(groups) * layout["stride"], 0x5A, np.uint8)
    for g, group in enumerate(groups):
        table = np.zeros((4, 257), np.uint32)
        for t, name in enumerate(group):
            table[t, :256] = sets[name]
        at = g * layout["stride"] + layout["counts"]
        regions[at:at + table.nbytes] = table.view(np.uint8).reshape(-1)
    with torch.cuda.device(dev):
        r = torch.from_numpy(regions).to(dev)
        assert L.danhip_jpeg_optimal_tables_device(ptr(r), len(groups), stream()) == 0, L.danhip_last_error()
        got = r.cpu().numpy()
    for g, group in enumerate(groups):
        for t, name in enumerate(group):
            rc, bits, vals = T.host_table(L, sets[name])
            assert rc == 0 and region_bits_vals(got, layout, g, t) == (bits, vals), name
            words = got[g * layout["stride"] + layout["tabs"] + t * 1024:][:1024].view(np.uint32)
            lengths = [int(x) >> 16 for x in words]
            assert sorted(l for l in lengths if l) == [l for l in range(17) for _ in range(bits[l])]       # a code for the counted symbols only
            assert all((lengths[s] > 0) == (sets[name][s] > 0) for s in range(256))
    assert np.all(got[layout["header"]:layout["stride"]] == 0x5A)                 # the direct call leaves the markers alone


def test_files_equal_the_host_stage_and_pillow(batch, L):
    got = H.files_of(batch["out"], batch["descs"], batch["sizes"])
    assert got == T.host_entropy_optimized(L, batch["coef"], batch["descs"], batch["totals"])
    for name, a, g in zip(batch["names"], batch["arrays"], got):
        assert g == T.pillow_optimized(a, 75, "4:2:0"), name
    for i, d in enumerate(batch["descs"]):                                       # nothing beyond a file inside its slot
        assert np.all(batch["out"][d.file_offset + batch["sizes"][i]:d.file_offset + d.file_capacity] == H.GUARD), i


@pytest.mark.parametrize("sub,q", [("4:2:0", 1), ("4:4:4", 100), ("4:4:4", 25), ("4:2:0", 95)])
def test_encoder_class_both_stages_permuted_and_singly(sub, q, dev):
    """JpegEncoder(entropy="device", optimize=True) = the host stage = Pillow, in batch order, in a permuted order (the tables are each
    image's own) and for a batch of one; never through the retry route; launches as the constants say."""
    from dan_amd import _lib
    from dan_amd.dataset.jpeg import JpegEncoder
    arrays = [a for _, a in T.images()]
    tensors = [torch.from_numpy(a).to(dev) for a in arrays]
    want = [T.pillow_optimized(a, q, sub) for a in arrays]
    host = JpegEncoder(quality=q, subsampling=sub, entropy="host", optimize=True)
    device = JpegEncoder(quality=q, subsampling=sub, entropy="device", optimize=True)
    assert host.encode_batch(tensors) == want
    assert device.encode_batch(tensors) == want
    order = np.random.RandomState(5).permutation(len(arrays)).tolist()
    assert device.encode_batch([tensors[i] for i in order]) == [want[i] for i in order]
    assert device.encode_batch(tensors[-1:]) == want[-1:] and device.encode_batch(tensors[:1]) == want[:1]
    s = device.stats
    per_call = _lib.JPEG_ENCODE_OPTIMIZE_LAUNCHES + _lib.JPEG_ENCODE_ENTROPY_LAUNCHES
    assert s["entropy_retry"] == 0 and s["host"] == 0 and s["entropy_launches"] == 4 * per_call and s["launches"] == 4 * _lib.JPEG_ENCODE_LAUNCHES


@pytest.mark.parametrize("B", [1, 5])
def test_launch_counts(B, dev):
    """Through the launches out-parameters (JpegEncoder adds them up): pixel stage + optimize + Huffman stage for B = 1 and B = 5; without
    optimize what it was."""
    from dan_amd import _lib
    from dan_amd.dataset.jpeg import JpegEncoder
    tensors = [torch.from_numpy(a).to(dev) for _, a in T.images()[4:4 + B]]
    for optimize, extra in ((True, _lib.JPEG_ENCODE_OPTIMIZE_LAUNCHES), (False, 0)):
        enc = JpegEncoder(entropy="device", optimize=optimize)
        enc.encode_batch(tensors)
        assert enc.stats["launches"] == _lib.JPEG_ENCODE_LAUNCHES == 2
        assert enc.stats["entropy_launches"] == extra + _lib.JPEG_ENCODE_ENTROPY_LAUNCHES == extra + 6


def test_launches_out_parameter(batch):
    from dan_amd import _lib
    assert batch["launches"] == _lib.JPEG_ENCODE_OPTIMIZE_LAUNCHES + _lib.JPEG_ENCODE_ENTROPY_LAUNCHES == 9


def test_no_optimised_file_is_longer_and_the_pixels_are_the_same(batch, L):
    """Against the standard-table files of the same coefficients: never longer (a valid but poor table would be), the same pixels when
    Pillow opens both (the tables changed, the coefficients did not)."""
    from PIL import Image
    plain = H.host_entropy(L, batch["coef"], batch["descs"], batch["totals"])
    got = H.files_of(batch["out"], batch["descs"], batch["sizes"])
    shorter = 0
    for name, g, p in zip(batch["names"], got, plain):
        assert len(g) <= len(p), name
        shorter += len(g) < len(p)
        a, b = np.asarray(Image.open(io.BytesIO(g)).convert("RGB")), np.asarray(Image.open(io.BytesIO(p)).convert("RGB"))
        assert np.array_equal(a, b), name
    assert shorter >= len(got) - 1


def test_flagged_image_stays_in_its_slot(L, dev):
    """A coefficient no baseline code carries, with optimize: that image alone is flagged, sizes 0; the others' files are whole; nothing
    is written outside the file buffer (guard bytes on either side) nor beyond the other images' files."""
    arrays = [H.noise(24, 40, 21), H.noise(17, 33, 22), H.noise(16, 16, 23)]
    coef, descs, totals = H.pixels_host(L, arrays, 3, 90)
    clean = T.host_entropy_optimized(L, coef, descs, totals)
    bad = coef.copy()
    bad[descs[1].coef_offset + 64 * 2 + 9] = -32768
    bad[descs[1].coef_offset + 64 * 5] = 32767
    guard = 4096
    out, sizes, status, launches, ws = device_stage(L, dev, bad, descs, totals, guard=guard)
    assert status == [0, RANGE, 0] and sizes[1] == 0 and launches == 9
    assert np.all(out[:guard] == H.GUARD) and np.all(out[guard + totals[2]:] == H.GUARD)
    slots = out[guard:guard + totals[2]]
    for i in (0, 2):
        d = descs[i]
        assert slots[d.file_offset:d.file_offset + sizes[i]].tobytes() == clean[i]
        assert np.all(slots[d.file_offset + sizes[i]:d.file_offset + d.file_capacity] == H.GUARD)
    # the host stage has the last word: it refuses the value
    buf = np.empty(totals[2], np.uint8)
    n = (ctypes.c_int64 * 3)()
    assert L.danhip_jpeg_encode_entropy_batch_ex(H.vp(bad), bad.size, descs, 3, 1, 1, H.vp(buf), totals[2], n) != 0

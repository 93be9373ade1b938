"""danhip_crc32c_batch (csrc/crc32c_exact.hip) against the byte-wise Python loop: every length at which the kernel changes path (lines,
chunks, windows), every start alignment class, both walk forms, masked and not; nothing read outside a range; a fixed number of launches."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

OFFSETS = (0, 1, 2, 3, 13)


def _geometry():
    from dan_amd import _lib
    L = _lib.lib()
    return L.danhip_crc32c_chunk_bytes(), L.danhip_crc32c_group_bytes()


def _lengths():
    C, G = _geometry()
    return [0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, C - 1, C, C + 1, 2 * C + 3, G - 1, G, G + 1, 3 * G + 5]


def _batch(image, ranges, masked, table_form=1):
    """One library call over [(offset, bytes)] of the uint8 device tensor `image` -> (uint32 numpy [n], launches)."""
    from dan_amd import _lib
    L = _lib.lib()
    n = len(ranges)
    tab = (_lib.CrcSegment * max(n, 1))()
    for i, (off, nb) in enumerate(ranges):
        tab[i].ptr, tab[i].bytes = image.data_ptr() + off, nb
    need = L.danhip_crc32c_batch_workspace_bytes(n, sum(nb for _, nb in ranges))
    ws = torch.zeros(max(need, 16), dtype=torch.uint8, device=image.device)
    out = torch.full((max(n, 1),), 0x5A5A5A5A, dtype=torch.int32, device=image.device)
    if n:
        host = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8)[:n * 16]
        ws[:n * 16].copy_(host)                                            # the table: one copy, to the front of the workspace
    default = L.danhip_get_option(b"crc_table")
    assert L.danhip_set_option(b"crc_table", table_form) == 0
    try:
        _lib.call("danhip_crc32c_batch", ctypes.addressof(tab), n, _lib.ptr(out), int(masked), _lib.ptr(ws), ws.numel(), _lib.stream())
    finally:
        L.danhip_set_option(b"crc_table", default)
    launches = L.danhip_crc32c_batch_last_launches()
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32), launches


@pytest.fixture(scope="module")
def cases():
    """Every length at every start offset, adjacent in one buffer with 3 guard bytes between two ranges; the Python loop's CRC of each,
    computed once (about 1.3 MB)."""
    from dan_amd.utility.checkpoint import _crc32c_py
    rng = np.random.RandomState(2024)
    ranges, at = [], 16
    for off in OFFSETS:
        for n in _lengths():
            at = (at + 15) // 16 * 16 + off                                # `off` bytes past a 16-byte aligned address
            ranges.append((at, n))
            at += n + 3
    data = rng.randint(0, 256, at + 64, dtype=np.uint8)
    want = np.array([_crc32c_py(data[o:o + n].tobytes()) for o, n in ranges], dtype=np.uint32)
    assert sum(n for _, n in ranges) < 1500000
    return data, ranges, want


def _mask(c):
    from dan_amd.utility.checkpoint import mask_crc
    return np.array([mask_crc(int(v)) for v in c], dtype=np.uint32)


@pytest.mark.parametrize("table_form", [0, 1])
def test_adjacent_ranges_and_their_surroundings(dev, cases, table_form):
    data, ranges, want = cases
    image = torch.from_numpy(data).to(dev)
    assert image.data_ptr() % 16 == 0
    got, launches = _batch(image, ranges, False, table_form)
    assert np.array_equal(got, want), [(r, hex(g), hex(w)) for r, g, w in zip(ranges, got, want) if g != w][:8]
    got_m, _ = _batch(image, ranges, True, table_form)
    assert np.array_equal(got_m, _mask(want))
    # every byte that belongs to no range changes (the guard bytes, the lead-in, the tail): no CRC moves, so nothing outside a range is read
    inside = np.zeros(data.size, dtype=bool)
    for o, n in ranges:
        inside[o:o + n] = True
    other = data.copy()
    other[~inside] ^= 0xA5
    again, _ = _batch(torch.from_numpy(other).to(dev), ranges, False, table_form)
    assert np.array_equal(again, want)


def test_shuffled_table(dev, cases):
    data, ranges, want = cases
    order = np.random.RandomState(5).permutation(len(ranges))
    image = torch.from_numpy(data).to(dev)
    for masked in (False, True):
        got, _ = _batch(image, [ranges[i] for i in order], masked)
        assert np.array_equal(got, (_mask(want) if masked else want)[order])


def test_launch_count_is_fixed_and_nothing_happens_for_no_ranges(dev, cases):
    from dan_amd import _lib
    data, ranges, want = cases
    image = torch.from_numpy(data).to(dev)
    one, l1 = _batch(image, ranges[-1:], False)                            # the largest range alone: many windows of one range
    sixty, l60 = _batch(image, ranges[:60], False)
    assert l1 == l60 == _lib.CRC32C_BATCH_LAUNCHES
    assert one[0] == want[-1] and np.array_equal(sixty, want[:60])
    none, l0 = _batch(image, [], False)
    assert l0 == 0 and none[0] == 0x5A5A5A5A                               # success, nothing launched, nothing written


def test_all_ranges_empty(dev):
    image = torch.zeros(64, dtype=torch.uint8, device=dev)
    got, launches = _batch(image, [(0, 0), (5, 0), (17, 0)], False)
    assert launches == 3 and list(got) == [0, 0, 0]


def test_one_large_range_against_the_host_entry(dev):
    """64 MiB + 5 bytes from an odd address: 2049 windows of one range XORed into one word, exponents far past a chunk table.  The host
    entry (pinned to the Python loop by tests/test_crc32c_cpu.py) is the reference."""
    from dan_amd import _lib
    n = (64 << 20) + 5
    g = torch.Generator(device="cpu").manual_seed(9)
    host = torch.randint(0, 256, (n + 32,), dtype=torch.uint8, generator=g)
    want = _lib.lib().danhip_crc32c_host(host.data_ptr() + 3, n, 0)
    image = host.to(dev)
    for form in (0, 1):
        got, _ = _batch(image, [(3, n)], False, form)
        assert int(got[0]) == want, (form, hex(int(got[0])), hex(want))

"""CRC-32C on the host (csrc/crc32c.cpp through the C ABI) against the byte-wise Python loop, the RFC 3720 B.4 vectors, the combine
arithmetic the device path is built on, and the Python routines that now go through the library.  Nothing here launches a kernel."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from dan_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def py():
    from dan_amd.utility import checkpoint
    return checkpoint._crc32c_py


def _host(L, data, crc=0, form=0):
    return L.danhip_crc32c_host_form(bytes(data), len(data), crc, form)


def test_abi_version_and_header(L):
    from dan_amd import _lib
    assert L.danhip_version() >= 14
    hdr = open(os.path.join(ROOT, "include", "danhip.h")).read()
    for text in ("uint32_t danhip_crc32c_host(const void* data, size_t n, uint32_t crc);",
                 "uint32_t danhip_crc32c_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);",
                 "size_t danhip_crc32c_batch_workspace_bytes(int32_t n, uint64_t total_bytes);",
                 "int danhip_crc32c_batch(const danhip_crc_segment* table_host, int32_t n, uint32_t* crc_out_dev, int32_t masked, void* ws, size_t ws_bytes,"):
        assert text in hdr, text
    assert L.danhip_crc_segment_bytes() == ctypes.sizeof(_lib.CrcSegment) == 16
    assert "#define DANHIP_CRC32C_BATCH_LAUNCHES %d" % _lib.CRC32C_BATCH_LAUNCHES in hdr


def test_rfc3720_vectors(L, py):
    vectors = [(bytes(32), 0x8A9136AA), (b"\xff" * 32, 0x62A8AB43), (bytes(range(32)), 0x46DD794E), (bytes(range(31, -1, -1)), 0x113FDB5C),
               (b"123456789", 0xE3069283)]
    for data, want in vectors:
        assert py(data) == want
        assert L.danhip_crc32c_host(data, len(data), 0) == want
        assert _host(L, data, form=1) == want                             # the portable tables, whatever the CPU has
    assert L.danhip_crc32c_host(None, 0, 0) == 0 and L.danhip_crc32c_host(b"", 0, 0) == 0
    assert L.danhip_crc32c_host(b"", 0, 0x1234ABCD) == 0x1234ABCD


def test_host_against_the_python_loop(L, py):
    rng = np.random.RandomState(7)
    buf = rng.randint(0, 256, 96, dtype=np.uint8)
    base = buf.ctypes.data
    for off in range(8):
        for n in range(71):
            want = py(buf[off:off + n].tobytes())
            for form in (0, 1):
                assert L.danhip_crc32c_host_form(base + off, n, 0, form) == want, (off, n, form)   # (the pointer itself is off alignment)
    big = rng.randint(0, 256, 100003, dtype=np.uint8).tobytes()
    want = py(big)
    assert _host(L, big) == want and _host(L, big, form=1) == want
    msg = rng.randint(0, 256, 40, dtype=np.uint8).tobytes()
    whole = py(msg)
    for cut in range(41):
        for form in (0, 1):
            assert _host(L, msg[cut:], _host(L, msg[:cut], 0, form), form) == whole, (cut, form)
        assert py(msg[cut:], py(msg[:cut])) == whole


def test_combine(L, py):
    rng = np.random.RandomState(11)
    lengths = list(range(71)) + [100003]
    data = rng.randint(0, 256, max(lengths) + 40, dtype=np.uint8).tobytes()
    a = data[:40]
    ca = py(a)
    for n in lengths:
        b = data[40:40 + n]
        assert L.danhip_crc32c_combine(ca, _host(L, b), n) == _host(L, a + b), n
    for n in range(71):                                                    # the same identity with the Python loop on both sides
        assert L.danhip_crc32c_combine(ca, py(data[40:40 + n]), n) == py(data[:40 + n]), n
    assert L.danhip_crc32c_combine(ca, py(b""), 0) == ca                   # B empty: crc_a ^ crc(b"") = crc_a
    assert L.danhip_crc32c_combine(0x12345678, 0x9ABCDEF0, 0) == 0x12345678 ^ 0x9ABCDEF0
    # associativity exercises the 64-bit exponent without allocating anything: (A B) C = A (B C)
    x, y, z = 0xDEADBEEF, 0x01234567, 0x89ABCDEF
    for lb in (1, 70, (1 << 31) + 1, (1 << 32) - 1, 1 << 32, (1 << 40) + 3):
        for lc in (0, 5, (1 << 33) + 7, (1 << 40) + 3):
            left = L.danhip_crc32c_combine(L.danhip_crc32c_combine(x, y, lb), z, lc)
            right = L.danhip_crc32c_combine(x, L.danhip_crc32c_combine(y, z, lc), lb + lc)
            assert left == right, (lb, lc)
    # and the exponent is not cut to 32 bits: appending 2^32 zero bytes is not appending none
    assert L.danhip_crc32c_combine(x, 0, 1 << 32) != L.danhip_crc32c_combine(x, 0, 0)
    assert L.danhip_crc32c_combine(x, 0, (1 << 32) + 5) == L.danhip_crc32c_combine(L.danhip_crc32c_combine(x, 0, 1 << 32), 0, 5)


def test_python_routines_go_through_the_library(py):
    from dan_amd.dataset import dataset_common as DC
    from dan_amd.utility import checkpoint as C
    assert C._native_crc() is not None                                     # the library loads here: the fast path is the one under test
    rng = np.random.RandomState(3)
    for n in (0, 1, 9, 4097):
        data = rng.randint(0, 256, n, dtype=np.uint8).tobytes()
        want = py(data)
        assert C.crc32c(data) == want and DC._crc32c(data) == want == DC._crc32c_py(data)
        assert C.crc32c(bytearray(data)) == want and C.crc32c(memoryview(data)) == want
        assert C.crc32c(np.frombuffer(data, dtype=np.uint8)) == want
        assert C.crc32c(data[n // 2:], C.crc32c(data[:n // 2])) == want
    a = np.arange(24, dtype=np.float32).reshape(4, 6)
    assert C.crc32c(a) == py(a.tobytes()) and C.crc32c(a[:, ::2]) == py(a[:, ::2].tobytes())     # a strided array: its C-order bytes
    assert DC.masked_crc32c(b"123456789") == C.mask_crc(0xE3069283)


def test_python_fallback_without_the_library(py, monkeypatch):
    from dan_amd.utility import checkpoint as C
    monkeypatch.setattr(C, "_NATIVE", None)
    assert C._native_crc() is None and C.crc32c(b"123456789") == 0xE3069283 and C.crc32c(b"6789", C.crc32c(b"12345")) == 0xE3069283


def test_record_payload_is_verified_at_library_speed(tmp_path):
    from dan_amd.dataset import dataset_common as DC
    rng = np.random.RandomState(5)
    payloads = [rng.randint(0, 256, n, dtype=np.uint8).tobytes() for n in (0, 1, 300, 70001)]
    path = str(tmp_path / "train-00000-of-00001")
    DC.write_tfrecord(path, payloads)
    assert list(DC.read_tfrecord(path, verify_payload=True)) == payloads
    raw = bytearray(open(path, "rb").read())
    at = len(raw) - 4 - 35000                                              # inside the last payload
    raw[at] ^= 0x10
    open(path, "wb").write(bytes(raw))
    assert len(list(DC.read_tfrecord(path))) == 4                          # (unverified, as before)
    with pytest.raises(IOError, match="corrupt record payload"):
        list(DC.read_tfrecord(path, verify_payload=True))


def test_batch_refuses_bad_arguments(L):
    from dan_amd import _lib
    EINVAL, EWORKSPACE = -1, -3
    tab = (_lib.CrcSegment * 2)()
    buf = (ctypes.c_char * 256)()
    p = (ctypes.addressof(buf) + 15) & ~15                                 # aligned host memory: every check comes before a launch
    tab[0].ptr, tab[0].bytes = p, 8
    tab[1].ptr, tab[1].bytes = None, 0
    t = ctypes.addressof(tab)
    need = L.danhip_crc32c_batch_workspace_bytes(2, 8)
    assert need >= 2 * 16 + 3 * 4 + 2 * 4 and L.danhip_crc32c_batch_workspace_bytes(0, 0) == 0
    assert L.danhip_crc32c_batch(t, 0, None, 1, None, 0, None) == 0 and L.danhip_crc32c_batch_last_launches() == 0      # n == 0: nothing to do
    assert L.danhip_crc32c_batch(t, -1, p, 1, p, need, None) == EINVAL and b"crc32c_batch" in L.danhip_last_error()
    assert L.danhip_crc32c_batch(None, 2, p, 1, p, need, None) == EINVAL and b"null" in L.danhip_last_error()
    assert L.danhip_crc32c_batch(t, 2, None, 1, p, need, None) == EINVAL
    assert L.danhip_crc32c_batch(t, 2, p, 1, None, need, None) == EINVAL
    assert L.danhip_crc32c_batch(t, 2, p, 1, p + 4, need, None) == EINVAL and b"aligned" in L.danhip_last_error()
    assert L.danhip_crc32c_batch(t, 2, p, 1, p, need - 1, None) == EWORKSPACE and b"workspace" in L.danhip_last_error()
    tab[1].bytes = 4                                                       # bytes behind a null pointer
    assert L.danhip_crc32c_batch(t, 2, p, 1, p, need, None) == EINVAL and b"segment 1" in L.danhip_last_error()
    assert L.danhip_crc32c_batch_last_launches() == 0
    assert L.danhip_crc32c_chunk_bytes() > 0 and L.danhip_crc32c_group_bytes() % L.danhip_crc32c_chunk_bytes() == 0

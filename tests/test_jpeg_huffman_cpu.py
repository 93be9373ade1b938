"""The Huffman stage of the device JPEG decoder without a GPU: danhip_jpeg_scan_prepare_batch (markers, segments, work items) and
danhip_jpeg_entropy_emulate_batch - the phases of csrc/jpeg_huffman_exact.hip run on the host through the same routines (csrc/jpeg_huffman.h)
with checked indexing - against the host entropy stage, danhip_jpeg_entropy_decode_batch, coefficient for coefficient."""
import ctypes
import io
import os

import numpy as np
import pytest

import jpeg_entropy_fixtures as F
from dan_amd import _lib

K = F.header_constants()
S, G, ROUNDS = K["DANHIP_JPEG_SUBSEQ_BYTES"], K["DANHIP_JPEG_SUBSEQ_PER_GROUP"], K["DANHIP_JPEG_SYNC_ROUNDS"]
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_golden.npz"))
ACCEPTED = [(str(n), GOLDEN["a%d_jpeg" % i].tobytes()) for i, n in enumerate(GOLDEN["a_names"])]
REFUSED = [(str(n), GOLDEN["r%d_jpeg" % i].tobytes(), int(GOLDEN["r_reasons"][i])) for i, n in enumerate(GOLDEN["r_names"])]
GOOD, BAD = F.load()
NOTSYNC, FILL = 1, -21846


class ScanHeader(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("magic", "B", "nseg", "nitems", "ngroups", "nchunks", "ntabs", "reserved")] + \
               [(n, ctypes.c_int64) for n in ("off_images", "off_segs", "off_items", "off_groups", "off_chunks", "off_tabs", "off_scan", "scan_bytes",
                                              "used_bytes", "coef_capacity")]


class ScanImage(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("prepared", "ncomp", "hs", "vs", "bpm", "mcus_x", "mcus", "restart")] + [("blocks_w", ctypes.c_int32 * 3)] + \
               [(n, ctypes.c_int32) for n in ("tab_first", "first_seg", "nseg", "first_item", "nitems", "first_group", "ngroups", "first_chunk", "nchunks")] + \
               [("plane", ctypes.c_int64 * 3)] + [(n, ctypes.c_int64) for n in ("total_blocks", "coef_offset", "scan_offset", "scan_len")]


class ScanSeg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("offset", "len", "data_len", "first_mcu", "mcu_count", "first_item", "nitems", "final")]


class ScanItem(ctypes.Structure):
    _fields_ = [("seg", ctypes.c_int32), ("sub", ctypes.c_int32)]


class ScanGroup(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("image", "first_item", "nitems", "carry_from")] + [("win_base", ctypes.c_int64), ("reserved", ctypes.c_int64)]


def prepare(datas):
    """-> (staging buffer, descs, statuses, capacity)"""
    L = _lib.lib()
    B = len(datas)
    capacity = 0
    for d in datas:
        info = _lib.JpegInfo()
        L.danhip_jpeg_inspect(d, len(d), ctypes.byref(info))
        capacity += info.coef_count
    ptrs = (ctypes.c_char_p * B)(*datas)
    sizes = (ctypes.c_int64 * B)(*[len(d) for d in datas])
    need = L.danhip_jpeg_scan_staging_bytes(ptrs, sizes, B)
    assert need > 0
    raw = np.zeros(need + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    staging = raw[off:off + need]
    descs = (_lib.JpegDesc * B)()
    status = (ctypes.c_int32 * B)()
    rc = L.danhip_jpeg_scan_prepare_batch(ptrs, sizes, B, staging.ctypes.data_as(ctypes.c_void_p), need, capacity, descs, status)
    assert rc == 0, L.danhip_last_error()
    assert 0 < L.danhip_jpeg_scan_device_bytes(staging.ctypes.data_as(ctypes.c_void_p)) <= need
    return staging, descs, list(status), capacity


def emulate(datas, rounds=-1, fill=FILL):
    """-> (coef, descs, prepare statuses, device statuses, range errors)"""
    L = _lib.lib()
    staging, descs, status, capacity = prepare(datas)
    coef = np.full(max(capacity, 1), fill, dtype=np.int16)
    dev = (ctypes.c_int32 * len(datas))()
    errors = ctypes.c_int64(-1)
    rc = L.danhip_jpeg_entropy_emulate_batch(staging.ctypes.data_as(ctypes.c_void_p), staging.nbytes, len(datas), descs,
                                             coef.ctypes.data_as(ctypes.c_void_p), capacity, rounds, dev, ctypes.byref(errors))
    assert rc == 0, L.danhip_last_error()
    return coef, descs, status, list(dev), errors.value


def host(datas, fill=FILL):
    return F.host_decode(_lib.lib(), _lib.JpegDesc, _lib.JpegInfo, datas, fill=fill)


def tables(staging):
    h = ScanHeader.from_buffer_copy(staging[:ctypes.sizeof(ScanHeader)].tobytes())

    def arr(T, off, n):
        return (T * n).from_buffer_copy(staging[off:off + n * ctypes.sizeof(T)].tobytes())

    return h, arr(ScanImage, h.off_images, h.B), arr(ScanSeg, h.off_segs, h.nseg), arr(ScanItem, h.off_items, h.nitems), arr(ScanGroup, h.off_groups, h.ngroups)


def test_abi_version_and_constants():
    assert _lib.lib().danhip_version() >= 7
    assert S * G == 32768 and ROUNDS >= 1


def test_every_accepted_stream_in_one_batch_equals_the_host_stage():
    datas = [d for _, d in ACCEPTED] + [d for _, d in GOOD]
    want, want_descs, want_status = host(datas)
    got, descs, status, dev, errors = emulate(datas)
    assert want_status == [0] * len(datas) and status == [0] * len(datas)
    assert dev == [0] * len(datas) and errors == 0
    assert np.array_equal(got, want)
    assert bytes(descs) == bytes(want_descs)                               # the descriptors of the reconstruct launches are the host stage's


@pytest.mark.parametrize("name,data", ACCEPTED + GOOD, ids=[a[0] for a in ACCEPTED + GOOD])
def test_every_accepted_stream_alone_equals_the_host_stage(name, data):
    want, _, want_status = host([data])
    got, _, status, dev, errors = emulate([data])
    assert want_status == [0] and status == [0] and dev == [0] and errors == 0
    assert np.array_equal(got, want)


def test_refused_streams_between_good_ones_leave_their_slots_alone():
    datas = [ACCEPTED[5][1]] + [d for _, d, _ in REFUSED] + [GOOD[2][1]]
    want, _, want_status = host(datas)
    got, _, status, dev, errors = emulate(datas)
    assert errors == 0 and dev[0] == 0 and dev[-1] == 0
    for i, (name, _, reason) in enumerate(REFUSED, 1):
        assert want_status[i] == reason
        assert status[i] == reason or (status[i] == 0 and dev[i] != 0), name      # refused at its header, or handed back by the device stage
    # whole buffers: the slots of the decoded images equal, the slot of the stream cut in mid-scan is the only place that may differ
    info = _lib.JpegInfo()
    ends = np.cumsum([_lib.lib().danhip_jpeg_inspect(d, len(d), ctypes.byref(info)) * 0 + info.coef_count for d in datas])
    for i in range(len(datas)):
        lo, hi = (0 if i == 0 else ends[i - 1]), ends[i]
        if want_status[i] == 0:
            assert np.array_equal(got[lo:hi], want[lo:hi])
    assert len(got) == len(want) == ends[-1]


def test_live_encodes_equal_the_host_stage():
    Image = pytest.importorskip("PIL.Image")
    from test_jpeg_cpu import _synthetic
    r = np.random.RandomState(2024)                                           # the live-encode set of tests/test_jpeg_cpu.py
    cases = [(768, 1024, m, 90, {}) for m in (None, 0, 1, 2)]
    cases += [(h, w, m, 85, {}) for m in (None, 0, 1, 2) for h, w in ((1, 2), (2, 1), (3, 3), (8, 2), (2, 5), (5, 6), (100, 2), (16, 16))]
    while len(cases) < 76:
        kw = [{}, dict(optimize=True), dict(restart_marker_rows=1), dict(restart_marker_blocks=int(r.randint(1, 9)))][int(r.randint(4))]
        cases.append((int(r.randint(1, 200)), int(r.randint(1, 200)), [None, 0, 1, 2][int(r.randint(4))], int(r.randint(5, 101)), kw))
    datas = []
    for k, (h, w, sub, q, kw) in enumerate(cases):
        img = _synthetic(h, w, k)
        b = io.BytesIO()
        if sub is None:
            Image.fromarray(img[:, :, 0]).save(b, format="JPEG", quality=q, **kw)
        else:
            Image.fromarray(img).save(b, format="JPEG", quality=q, subsampling=sub, **kw)
        datas.append(b.getvalue())
    want, _, want_status = host(datas)
    got, _, status, dev, errors = emulate(datas)
    assert want_status == [0] * len(datas) and status == want_status and dev == want_status and errors == 0
    assert np.array_equal(got, want)


def test_segment_and_work_item_tables():
    names = [n for n, _ in ACCEPTED + GOOD]
    datas = [d for _, d in ACCEPTED + GOOD]
    staging, descs, status, _ = prepare(datas)
    h, images, segs, items, groups = tables(staging)
    assert h.B == len(datas) and h.used_bytes <= staging.nbytes and h.off_scan % 16 == 0
    scan = staging[h.off_scan:h.off_scan + h.scan_bytes]
    for i, (name, data) in enumerate(zip(names, datas)):
        im = images[i]
        s, e = F.scan_start(data), F.scan_end(data)
        assert im.prepared == 1 and im.scan_offset % 16 == 0 and im.scan_len == e - s, name
        assert scan[im.scan_offset:im.scan_offset + im.scan_len].tobytes() == data[s:e], name      # the stream itself, left stuffed
        at, mcu = 0, 0
        for k in range(im.first_seg, im.first_seg + im.nseg):                  # segment + marker tile the scan exactly
            sg = segs[k]
            assert sg.offset == at and 0 <= sg.data_len <= sg.len, name
            if not sg.final:
                assert data[s + sg.offset + sg.len:s + sg.offset + sg.len + 2] == bytes([0xFF, 0xD0 + (k - im.first_seg) % 8]), name
            at = sg.offset + sg.len + 2
            assert sg.first_mcu == mcu and sg.mcu_count >= 1
            mcu += sg.mcu_count
            assert sg.nitems == max(1, -(-sg.data_len // S))
            for j in range(sg.nitems):                                         # every subsequence lies inside its segment
                it = items[sg.first_item + j]
                assert (it.seg, it.sub) == (k, j) and (j * S < sg.data_len or sg.data_len == 0)
        assert at - 2 == im.scan_len and mcu == im.mcus, name
        assert (im.nseg > 1) == ("rst" in name), name
        covered = 0
        for gi in range(im.first_group, im.first_group + im.ngroups):
            gr = groups[gi]
            assert gr.image == i and gr.first_item == im.first_item + covered and 1 <= gr.nitems <= G and gr.win_base % 16 == 0
            covered += gr.nitems
        assert covered == im.nitems
    # the fixture conditions, for the committed constants: two group seams inside one segment, and an FF 00 pair across a subsequence boundary
    big = images[len(ACCEPTED)]
    assert big.nseg == 1 and big.ngroups >= 3
    assert F.straddling_stuffed_pairs(GOOD[0][1], S)
    rst = images[len(ACCEPTED) + 1]
    assert rst.nseg > 1 and segs[rst.first_seg].data_len > S * G and rst.ngroups >= 3
    tiny = images[[n for n, _ in ACCEPTED].index("grey_1x1_q30")]
    assert tiny.nitems == 1 and segs[tiny.first_seg].data_len < S                # a scan shorter than one subsequence


def test_corrupted_scans_end_equal_to_the_host_or_with_a_status():
    bad = BAD + [("cut_mid_scan", [d for n, d, _ in REFUSED if n == "cut_mid_scan"][0], 2)]
    datas = []
    for _, data, _ in bad:
        datas += [ACCEPTED[7][1], data]
    datas.append(GOOD[3][1])
    want, _, want_status = host(datas)
    got, _, status, dev, errors = emulate(datas)
    assert errors == 0                                                         # the checked accessors refused no index
    info = _lib.JpegInfo()
    ends = np.cumsum([_lib.lib().danhip_jpeg_inspect(d, len(d), ctypes.byref(info)) * 0 + info.coef_count for d in datas])
    for i, d in enumerate(datas):
        lo, hi = (0 if i == 0 else ends[i - 1]), ends[i]
        if i % 2 == 0:                                                         # the good neighbours
            assert want_status[i] == 0 and status[i] == 0 and dev[i] == 0 and np.array_equal(got[lo:hi], want[lo:hi])
            continue
        name, _, outcome = bad[i // 2]
        assert want_status[i] == outcome, name                                 # the fixture's record of the host stage
        if status[i] != 0:
            assert status[i] == want_status[i], name                           # refused by the prepare pass: with the host stage's reason
        elif dev[i] == 0:
            assert want_status[i] == 0 and np.array_equal(got[lo:hi], want[lo:hi]), name
        assert not (want_status[i] != 0 and status[i] == 0 and dev[i] == 0), name
    for name, data, outcome in bad:                                            # and alone
        _, _, st, dv, err = emulate([data])
        assert err == 0 and (st[0] == outcome or (st[0] == 0 and (dv[0] != 0 or outcome == 0))), name


def test_without_cross_group_rounds_the_verify_step_flags_the_three_group_stream():
    data = GOOD[0][1]
    want, _, _ = host([data])
    got, _, status, dev, errors = emulate([data], rounds=0)
    assert status == [0] and errors == 0
    assert dev[0] & NOTSYNC                                                    # never passed with wrong coefficients
    for rounds in (1, ROUNDS):
        got, _, status, dev, errors = emulate([data], rounds=rounds)
        assert errors == 0 and (dev[0] == 0 or dev[0] & NOTSYNC)
        if dev[0] == 0:
            assert np.array_equal(got, want)
    assert dev == [0]                                                          # the committed constant is enough for the fixtures


def test_checks_of_the_staging_buffer_come_before_any_decoding():
    L = _lib.lib()
    datas = [ACCEPTED[9][1], GOOD[2][1]]
    staging, descs, status, capacity = prepare(datas)
    h, images, segs, items, groups = tables(staging)
    coef = np.zeros(capacity, np.int16)
    dev = (ctypes.c_int32 * 2)()

    def run(buf, cap=capacity, n=None):
        return L.danhip_jpeg_entropy_emulate_batch(buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes if n is None else n, 2, descs,
                                                   coef.ctypes.data_as(ctypes.c_void_p), cap, -1, dev, None)

    assert run(staging) == 0
    assert run(staging, cap=capacity - 64) == -1 and b"coefficients" in L.danhip_last_error()
    assert run(staging, n=h.used_bytes - 16) == -1
    for T, off, index, field, value in ((ScanSeg, h.off_segs, 0, "data_len", 1 << 29), (ScanSeg, h.off_segs, 0, "mcu_count", 1 << 20),
                                        (ScanItem, h.off_items, 1, "sub", 7), (ScanGroup, h.off_groups, 0, "nitems", G + 1),
                                        (ScanGroup, h.off_groups, 0, "win_base", 1 << 40), (ScanImage, h.off_images, 1, "scan_offset", 1 << 33),
                                        (ScanImage, h.off_images, 0, "tab_first", 100), (ScanImage, h.off_images, 0, "mcus_x", 3)):
        bad = staging.copy()
        raw = np.zeros(bad.nbytes + 16, np.uint8)
        o = (-raw.ctypes.data) % 16
        raw[o:o + bad.nbytes] = bad
        bad = raw[o:o + bad.nbytes]
        at = off + index * ctypes.sizeof(T)
        entry = T.from_buffer_copy(bad[at:at + ctypes.sizeof(T)].tobytes())
        setattr(entry, field, value)
        bad[at:at + ctypes.sizeof(T)] = np.frombuffer(bytes(entry), np.uint8)
        assert run(bad) == -1, field
    # the device launcher runs the same check first (no GPU here: had it launched, the call would fail otherwise)
    fake = ctypes.c_void_p(4096)
    launches = ctypes.c_int32(7)
    rc = L.danhip_jpeg_huffman_decode_batch(staging.ctypes.data_as(ctypes.c_void_p), fake, staging.nbytes, 2, fake, capacity - 64, descs, fake, fake, 1 << 30,
                                            fake, ctypes.byref(launches), None)
    assert rc == -1 and launches.value == 0 and b"coefficients" in L.danhip_last_error()

"""TensorFlow V2 checkpoint ("tensor bundle") reader / writer and the reference's warm-start rules.

The reference restores `vgg16_reducedfc.ckpt` / its own checkpoints through tf.train.Saver (utility/scaffolds.py:24-88, called from
train_sfd.py:159-163, train_dan.py, train_pb.py with name_remap {'/conv2d/kernel': '/weights', '/conv2d/bias': '/biases'}).
TensorFlow is not available here, so the on-disk format is read directly:

  <prefix>.index                 an SSTable (TF's port of the LevelDB table format): 48-byte footer with the metaindex and
                                 index block handles + magic 0xdb4775248b80fb57; blocks = prefix-compressed entries + restart
                                 array, followed by a 1-byte compression tag (0 none, 1 snappy) and a masked crc32c.
                                 key ""      -> BundleHeaderProto  {1: num_shards, 2: endianness, 3: version}
                                 key <name>  -> BundleEntryProto   {1: dtype, 2: shape{2: dim{1: size}}, 3: shard_id, 4: offset,
                                                                    5: size, 6: crc32c (fixed32), 7: slices}
  <prefix>.data-0000i-of-0000N   raw little-endian tensor bytes.

`CheckpointReader` mirrors tf.train.NewCheckpointReader (has_tensor / get_tensor / get_variable_to_shape_map), `latest_checkpoint`
mirrors tf.train.latest_checkpoint, and `init_from_checkpoint` applies scaffolds.get_init_fn_for_scaffold's scope / exclusion /
remap / missing-variable rules to a VariableStore.  Kernel layouts need no conversion: conv kernels are HWIO in both, the
deformable-conv kernel is OIHW in both (custom_op.py:134).  Host-side code (numpy), except the opt-in device path: DeviceCheckpointIO /
write_checkpoint_device (save_checkpoint(checksums="device")) assemble and checksum the data shard on the GPU, and
restore_checkpoint(verify=True) checks every tensor CRC there before a variable is written (csrc/crc32c_exact.hip).
"""
import os
import struct

import numpy as np

TABLE_MAGIC = 0xdb4775248b80fb57
# tensorflow/core/framework/types.proto
DTYPES = {1: np.float32, 2: np.float64, 3: np.int32, 4: np.uint8, 5: np.int16, 6: np.int8, 9: np.int64, 10: np.bool_, 17: np.uint16,
          19: np.float16, 22: np.uint32, 23: np.uint64}
DTYPE_ENUM = {np.dtype(v): k for k, v in DTYPES.items()}


class CheckpointError(ValueError):
    pass


# ------------------------------------------------------------------------------------------------------------ crc32c
_CRC_TABLE = None


def _crc_table():
    global _CRC_TABLE
    if _CRC_TABLE is None:
        t = []
        for i in range(256):
            c = i
            for _ in range(8):
                c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
            t.append(c)
        _CRC_TABLE = t
    return _CRC_TABLE


def _crc32c_py(data, crc=0):
    """The byte-wise table loop in plain Python (~1 MB/s): the fallback when libdanhip.so does not load, and the tests' reference."""
    t = _crc_table()
    c = crc ^ 0xFFFFFFFF
    for b in bytes(data):
        c = t[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


_NATIVE = False           # False: not asked yet; None: libdanhip.so does not load in this process


def _native_crc():
    global _NATIVE
    if _NATIVE is False:
        try:
            from .. import _lib
            _NATIVE = _lib.lib().danhip_crc32c_host
        except (ImportError, OSError, AttributeError, RuntimeError):
            _NATIVE = None
    return _NATIVE


def crc32c(data, crc=0):
    """CRC-32C (Castagnoli), as used by the table blocks and the bundle entries: danhip_crc32c_host (csrc/crc32c.cpp) when the library
    loads, the Python loop otherwise - same bits."""
    fn = _native_crc()
    if fn is None:
        return _crc32c_py(data, crc)
    if isinstance(data, bytes):
        return fn(data, len(data), crc)
    try:
        a = np.frombuffer(data, dtype=np.uint8)           # any contiguous buffer, not copied
    except (TypeError, ValueError, BufferError):
        a = np.frombuffer(bytes(data), dtype=np.uint8)
    return fn(a.ctypes.data, a.size, crc)


def mask_crc(c):
    return (((c >> 15) | (c << 17)) + 0xa282ead8) & 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------ varints / protobuf
def _varint(buf, pos):
    shift = result = 0
    while True:
        if pos >= len(buf):
            raise CheckpointError("truncated varint")
        b = buf[pos]
        pos += 1
        result |= (b & 0x7F) << shift
        if not b & 0x80:
            return result, pos
        shift += 7


def _put_varint(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _proto_fields(buf):
    """Yields (field number, wire type, value) of one protobuf message (value: int for varint/fixed, bytes for length-delimited)."""
    pos = 0
    while pos < len(buf):
        tag, pos = _varint(buf, pos)
        f, wt = tag >> 3, tag & 7
        if wt == 0:
            v, pos = _varint(buf, pos)
        elif wt == 1:
            v = struct.unpack_from("<Q", buf, pos)[0]
            pos += 8
        elif wt == 2:
            n, pos = _varint(buf, pos)
            v = bytes(buf[pos:pos + n])
            pos += n
        elif wt == 5:
            v = struct.unpack_from("<I", buf, pos)[0]
            pos += 4
        else:
            raise CheckpointError("unsupported protobuf wire type %d" % wt)
        yield f, wt, v


def _parse_shape(buf):
    dims = []
    for f, _, v in _proto_fields(buf):
        if f == 2:                                        # Dim
            size = 0
            for g, _, w in _proto_fields(v):
                if g == 1:
                    size = w if w < (1 << 63) else w - (1 << 64)
            dims.append(size)
        elif f == 3 and v:
            raise CheckpointError("tensor of unknown rank in checkpoint")
    return tuple(dims)


# ------------------------------------------------------------------------------------------------------------ snappy (blocks may be compressed)
def snappy_decompress(buf):
    n, pos = _varint(buf, 0)
    out = bytearray()
    while pos < len(buf):
        tag = buf[pos]
        pos += 1
        kind = tag & 3
        if kind == 0:                                     # literal
            ln = tag >> 2
            if ln >= 60:
                nb = ln - 59
                ln = int.from_bytes(buf[pos:pos + nb], "little")
                pos += nb
            ln += 1
            out += buf[pos:pos + ln]
            pos += ln
            continue
        if kind == 1:
            ln = ((tag >> 2) & 7) + 4
            off = ((tag >> 5) << 8) | buf[pos]
            pos += 1
        elif kind == 2:
            ln = (tag >> 2) + 1
            off = buf[pos] | (buf[pos + 1] << 8)
            pos += 2
        else:
            ln = (tag >> 2) + 1
            off = int.from_bytes(buf[pos:pos + 4], "little")
            pos += 4
        if off == 0 or off > len(out):
            raise CheckpointError("corrupt snappy stream")
        for _ in range(ln):                               # copies may overlap their own output
            out.append(out[-off])
    if len(out) != n:
        raise CheckpointError("snappy length mismatch")
    return bytes(out)


# ------------------------------------------------------------------------------------------------------------ table (index file)
def _read_block(data, offset, size, verify=True):
    raw = data[offset:offset + size]
    trailer = data[offset + size:offset + size + 5]
    if len(raw) != size or len(trailer) != 5:
        raise CheckpointError("block handle beyond the end of the index file")
    if verify:
        want = struct.unpack("<I", trailer[1:])[0]
        if mask_crc(crc32c(raw + trailer[:1])) != want:
            raise CheckpointError("index block checksum mismatch")
    if trailer[0] == 0:
        return raw
    if trailer[0] == 1:
        return snappy_decompress(raw)
    raise CheckpointError("unknown block compression %d" % trailer[0])


def _block_entries(block):
    if len(block) < 4:
        raise CheckpointError("short block")
    nrestart = struct.unpack_from("<I", block, len(block) - 4)[0]
    end = len(block) - 4 - 4 * nrestart
    pos, key = 0, b""
    while pos < end:
        shared, pos = _varint(block, pos)
        non_shared, pos = _varint(block, pos)
        vlen, pos = _varint(block, pos)
        key = key[:shared] + bytes(block[pos:pos + non_shared])
        pos += non_shared
        yield key, bytes(block[pos:pos + vlen])
        pos += vlen


def read_table(path, verify=True):
    """-> list of (key bytes, value bytes) of an SSTable file, in key order."""
    data = open(path, "rb").read()
    if len(data) < 48:
        raise CheckpointError("%s: too short for a table footer" % path)
    footer = data[-48:]
    if struct.unpack("<Q", footer[40:])[0] != TABLE_MAGIC:
        raise CheckpointError("%s: bad table magic (not a TF V2 checkpoint index)" % path)
    p = 0
    _, p = _varint(footer, p)                             # metaindex handle (unused)
    _, p = _varint(footer, p)
    ioff, p = _varint(footer, p)
    isize, p = _varint(footer, p)
    out = []
    for _, handle in _block_entries(_read_block(data, ioff, isize, verify)):
        off, q = _varint(handle, 0)
        size, q = _varint(handle, q)
        out.extend(_block_entries(_read_block(data, off, size, verify)))
    return out


# ------------------------------------------------------------------------------------------------------------ reader
class CheckpointReader(object):
    """tf.train.NewCheckpointReader for V2 checkpoints given by their prefix (e.g. './model/vgg16_reducedfc.ckpt')."""

    def __init__(self, prefix, verify_index=True):
        self.prefix = prefix
        index = prefix + ".index"
        if not os.path.exists(index):
            raise CheckpointError("%s not found (V1 single-file checkpoints are not supported)" % index)
        self.num_shards, self.entries = 1, {}
        for key, val in read_table(index, verify_index):
            if key == b"":
                for f, _, v in _proto_fields(val):
                    if f == 1:
                        self.num_shards = v
                    elif f == 2 and v != 0:
                        raise CheckpointError("big-endian checkpoint")
                continue
            e = {"dtype": 0, "shape": (), "shard": 0, "offset": 0, "size": 0, "crc": None, "sliced": False}
            for f, _, v in _proto_fields(val):
                if f == 1:
                    e["dtype"] = v
                elif f == 2:
                    e["shape"] = _parse_shape(v)
                elif f == 3:
                    e["shard"] = v
                elif f == 4:
                    e["offset"] = v
                elif f == 5:
                    e["size"] = v
                elif f == 6:
                    e["crc"] = v
                elif f == 7:
                    e["sliced"] = True
            self.entries[key.decode("utf-8")] = e

    def has_tensor(self, name):
        return name in self.entries

    def get_variable_to_shape_map(self):
        return {n: list(e["shape"]) for n, e in self.entries.items()}

    def get_variable_to_dtype_map(self):
        return {n: DTYPES.get(e["dtype"]) for n, e in self.entries.items()}

    def get_tensor(self, name, verify=False):
        if name not in self.entries:
            raise KeyError("tensor %r not found in checkpoint %s" % (name, self.prefix))
        e = self.entries[name]
        if e["sliced"]:
            raise CheckpointError("%s is a partitioned variable (slices are not supported)" % name)
        if e["dtype"] not in DTYPES:
            raise CheckpointError("%s: unsupported dtype enum %d" % (name, e["dtype"]))
        with open(self.shard_path(e["shard"]), "rb") as f:
            f.seek(e["offset"])
            raw = f.read(e["size"])
        return self._decode(name, e, raw, verify)

    def shard_path(self, shard):
        return "%s.data-%05d-of-%05d" % (self.prefix, shard, self.num_shards)

    def _decode(self, name, e, raw, verify=False):
        dt = np.dtype(DTYPES[e["dtype"]])
        count = int(np.prod(e["shape"], dtype=np.int64)) if e["shape"] else 1
        if len(raw) != e["size"] or count * dt.itemsize != e["size"]:
            raise CheckpointError("%s: %d bytes on disk for shape %s %s" % (name, len(raw), e["shape"], dt))
        if verify and e["crc"] is not None and mask_crc(crc32c(raw)) != e["crc"]:
            raise CheckpointError("%s: data checksum mismatch" % name)
        return np.frombuffer(raw, dtype=dt.newbyteorder("<")).reshape(e["shape"]).astype(dt)

    def get_tensor_from(self, name, shard_bytes):
        """get_tensor out of a shard already in memory (a buffer of the whole data file)."""
        e = self.entries[name]
        if e["sliced"] or e["dtype"] not in DTYPES:
            return self.get_tensor(name)                   # (raises the fitting error)
        return self._decode(name, e, bytes(shard_bytes[e["offset"]:e["offset"] + e["size"]]))

    def checked_entries(self, shard, shard_bytes):
        """[(name, entry)] of the entries of `shard` that carry a CRC, each inside the shard's shard_bytes bytes (else CheckpointError)."""
        out = []
        for n, e in self.entries.items():
            if e["shard"] != shard or e["crc"] is None or e["sliced"]:
                continue
            if e["offset"] + e["size"] > shard_bytes:
                raise CheckpointError("%s: data shard truncated (%d bytes, the tensor ends at %d)" % (n, shard_bytes, e["offset"] + e["size"]))
            out.append((n, e))
        return out

    def verify_all(self):
        """Checks every entry that carries a CRC against its bytes, each shard read once (host CRC); entries without one are accepted.
        CheckpointError naming the first tensor that does not match."""
        for shard in sorted({e["shard"] for e in self.entries.values()}):
            data = np.fromfile(self.shard_path(shard), dtype=np.uint8)
            for n, e in self.checked_entries(shard, data.size):
                if mask_crc(crc32c(data[e["offset"]:e["offset"] + e["size"]])) != e["crc"]:
                    raise CheckpointError("%s: data checksum mismatch" % n)


def latest_checkpoint(checkpoint_dir):
    """tf.train.latest_checkpoint: the prefix named by the 'checkpoint' state file, or None."""
    state = os.path.join(checkpoint_dir, "checkpoint")
    if not os.path.exists(state):
        return None
    for line in open(state):
        line = line.strip()
        if line.startswith("model_checkpoint_path:"):
            p = line.split(":", 1)[1].strip().strip('"')
            p = p if os.path.isabs(p) else os.path.join(checkpoint_dir, p)
            return p if os.path.exists(p + ".index") else None
    return None


# ------------------------------------------------------------------------------------------------------------ writer
def _pb_varint_field(f, v):
    return _put_varint((f << 3) | 0) + _put_varint(v)


def _pb_bytes_field(f, b):
    return _put_varint((f << 3) | 2) + _put_varint(len(b)) + b


def _table_block(entries, restart_interval=16):
    out, restarts, prev = bytearray(), [], b""
    for i, (k, v) in enumerate(entries):
        if i % restart_interval == 0:
            restarts.append(len(out))
            shared = 0
        else:
            shared = 0
            while shared < min(len(prev), len(k)) and prev[shared] == k[shared]:
                shared += 1
        out += _put_varint(shared) + _put_varint(len(k) - shared) + _put_varint(len(v)) + k[shared:] + v
        prev = k
    for r in restarts or [0]:
        out += struct.pack("<I", r)
    out += struct.pack("<I", max(len(restarts), 1))
    return bytes(out)


def _bundle_entry(dtype, shape, offset, size, masked_crc=None):
    """BundleEntryProto of one tensor of shard 0 (masked_crc None: the crc32c field is left out)."""
    dims = b"".join(_pb_bytes_field(2, _pb_varint_field(1, int(d))) for d in shape)
    e = _pb_varint_field(1, DTYPE_ENUM[np.dtype(dtype)]) + _pb_bytes_field(2, dims)
    if offset:
        e += _pb_varint_field(4, offset)
    e += _pb_varint_field(5, size)
    if masked_crc is not None:
        e += _put_varint((6 << 3) | 5) + struct.pack("<I", masked_crc)
    return e


def _write_index(prefix, entries, block_size=4096):
    """The .index table of a single-shard bundle from [(name, BundleEntryProto bytes)] in byte-sorted name order, and the 'checkpoint'
    state file beside it."""
    items = [(b"", _pb_varint_field(1, 1) + _pb_bytes_field(3, _pb_varint_field(1, 1)))]      # num_shards=1, version{producer=1}
    items += [(n.encode("utf-8"), e) for n, e in entries]
    out, index_entries, cur, cur_bytes = bytearray(), [], [], 0

    def flush():
        nonlocal cur, cur_bytes
        if not cur:
            return
        blk = _table_block(cur)
        handle = _put_varint(len(out)) + _put_varint(len(blk))
        out.extend(blk + b"\x00" + struct.pack("<I", mask_crc(crc32c(blk + b"\x00"))))
        index_entries.append((cur[-1][0], handle))
        cur, cur_bytes = [], 0

    for k, v in items:
        cur.append((k, v))
        cur_bytes += len(k) + len(v) + 8
        if cur_bytes >= block_size:
            flush()
    flush()
    meta = _table_block([])
    meta_handle = _put_varint(len(out)) + _put_varint(len(meta))
    out.extend(meta + b"\x00" + struct.pack("<I", mask_crc(crc32c(meta + b"\x00"))))
    idx = _table_block(index_entries, restart_interval=1)
    idx_handle = _put_varint(len(out)) + _put_varint(len(idx))
    out.extend(idx + b"\x00" + struct.pack("<I", mask_crc(crc32c(idx + b"\x00"))))
    footer = meta_handle + idx_handle
    out.extend(footer + b"\x00" * (40 - len(footer)) + struct.pack("<Q", TABLE_MAGIC))
    open(prefix + ".index", "wb").write(bytes(out))
    with open(os.path.join(os.path.dirname(os.path.abspath(prefix)), "checkpoint"), "w") as f:
        base = os.path.basename(prefix)
        f.write('model_checkpoint_path: "%s"\nall_model_checkpoint_paths: "%s"\n' % (base, base))


def write_checkpoint(prefix, tensors, block_size=4096, checksums=True):
    """Writes {name: numpy array} as a single-shard V2 checkpoint (uncompressed index blocks) + the 'checkpoint' state file.
    checksums=False leaves the per-tensor crc32c out; TensorFlow's reader checks that field, so a file for it is written with checksums
    (the CRC runs in libdanhip.so - danhip_crc32c_host - at memory-copy speed; in plain Python, ~1 MB/s, only when the library does not load)."""
    os.makedirs(os.path.dirname(os.path.abspath(prefix)), exist_ok=True)
    names = sorted(tensors, key=lambda s: s.encode("utf-8"))
    entries = []
    offset = 0
    with open(prefix + ".data-00000-of-00001", "wb") as f:
        for n in names:
            a = np.asarray(tensors[n])
            if not a.flags.c_contiguous:
                a = a.copy(order="C")
            if a.dtype not in DTYPE_ENUM:
                raise CheckpointError("%s: dtype %s not supported" % (n, a.dtype))
            raw = a.astype(a.dtype.newbyteorder("<")).tobytes()
            f.write(raw)
            entries.append((n, _bundle_entry(a.dtype, a.shape, offset, len(raw), mask_crc(crc32c(raw)) if checksums else None)))
            offset += len(raw)
    _write_index(prefix, entries, block_size)


# ------------------------------------------------------------------------------------------------------------ device path
class DeviceCheckpointIO(object):
    """The data shard as ONE device image: packed (save) or uploaded (verified restore) once, all tensor CRCs from one
    danhip_crc32c_batch call, one pinned host image.  Keeps its staging buffers between calls (a trainer owns one) and counts what it did
    in `stats`: batch calls and their kernel launches, host<->device copies (neither depends on the number of tensors) and their bytes,
    and the device-to-device packing copies (one per tensor, left to torch)."""

    def __init__(self, device):
        import torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise CheckpointError("DeviceCheckpointIO needs a GPU device, got %s" % self.device)
        self.stats = {"batch_calls": 0, "launches": 0, "h2d_copies": 0, "d2h_copies": 0, "h2d_bytes": 0, "d2h_bytes": 0, "crc_bytes": 0,
                      "pack_copies": 0}
        self._image = self._host = self._ws = self._table_pin = self._table_sent = self._crc = self._crc_pin = None

    @staticmethod
    def _grown(buf, n, make):
        return buf if buf is not None and buf.numel() >= n else make(max(n, 1))

    def image(self, nbytes):
        """uint8 device buffer of at least nbytes (16-byte aligned base: a fresh allocation)."""
        import torch
        self._image = self._grown(self._image, nbytes, lambda n: torch.empty(n, dtype=torch.uint8, device=self.device))
        return self._image

    def host(self, nbytes):
        import torch
        self._host = self._grown(self._host, nbytes, lambda n: torch.empty(n, dtype=torch.uint8, pin_memory=True))
        return self._host

    def pack(self, image, offset, t):
        """t (a device tensor, any strides) C-contiguous at image[offset:]."""
        import torch
        nb = t.numel() * t.element_size()
        if nb == 0:
            return
        dst = image[offset:offset + nb]
        if (image.data_ptr() + offset) % t.element_size() == 0:
            dst.view(t.dtype).view(t.shape).copy_(t)                       # a strided view is gathered by the copy itself
        else:
            dst.copy_(t.contiguous().reshape(-1).view(torch.uint8))
        self.stats["pack_copies"] += 1

    def crc_launch(self, image, ranges, masked=True):
        """One danhip_crc32c_batch over [(offset, bytes)] of `image`, on the current stream; -> device int32 [n] (the CRCs' bit patterns)."""
        import ctypes
        import torch
        from .. import _lib
        n = len(ranges)
        L = _lib.lib()
        table = (_lib.CrcSegment * max(n, 1))()
        base = image.data_ptr()
        total = 0
        for i, (off, nb) in enumerate(ranges):
            table[i].ptr, table[i].bytes = base + off, nb
            total += nb
        need = L.danhip_crc32c_batch_workspace_bytes(n, total)
        self._ws = self._grown(self._ws, need, lambda m: torch.empty(m, dtype=torch.uint8, device=self.device))
        self._crc = self._grown(self._crc, n, lambda m: torch.empty(m, dtype=torch.int32, device=self.device))
        tb = n * ctypes.sizeof(_lib.CrcSegment)
        if n:
            if self._table_sent is not None:
                self._table_sent.synchronize()                             # (the previous call's upload has left the pinned table)
            self._table_pin = self._grown(self._table_pin, tb, lambda m: torch.empty(m, dtype=torch.uint8, pin_memory=True))
            ctypes.memmove(self._table_pin.data_ptr(), ctypes.addressof(table), tb)
            self._ws[:tb].copy_(self._table_pin[:tb], non_blocking=True)   # the ONE table upload: to the front of the workspace
            self._table_sent = torch.cuda.Event()
            self._table_sent.record(torch.cuda.current_stream(self.device))
            self.stats["h2d_copies"] += 1
            self.stats["h2d_bytes"] += tb
        _lib.call("danhip_crc32c_batch", ctypes.addressof(table), n, _lib.ptr(self._crc), 1 if masked else 0, _lib.ptr(self._ws), self._ws.numel(),
                  _lib.stream())
        self.stats["batch_calls"] += 1
        self.stats["launches"] += L.danhip_crc32c_batch_last_launches()
        self.stats["crc_bytes"] += total
        return self._crc[:n]

    def fetch(self, image, nbytes, crcs):
        """The image and the CRC array to pinned host memory: two copies, ONE synchronisation.  -> (uint8 numpy view, uint32 numpy array)."""
        import torch
        host = self.host(nbytes)
        n = crcs.numel()
        self._crc_pin = self._grown(self._crc_pin, n, lambda m: torch.empty(m, dtype=torch.int32, pin_memory=True))
        if nbytes:
            host[:nbytes].copy_(image[:nbytes], non_blocking=True)
            self.stats["d2h_copies"] += 1
        if n:
            self._crc_pin[:n].copy_(crcs, non_blocking=True)
            self.stats["d2h_copies"] += 1
        self.stats["d2h_bytes"] += nbytes + 4 * n
        torch.cuda.current_stream(self.device).synchronize()
        return host.numpy()[:nbytes], self._crc_pin.numpy()[:n].view(np.uint32).copy()

    def upload(self, path):
        """A shard file read once into pinned memory and uploaded with one copy; -> (device image, host numpy view, bytes)."""
        nbytes = os.path.getsize(path)
        host = self.host(nbytes)
        view = host.numpy()[:nbytes]
        with open(path, "rb") as f:
            if f.readinto(memoryview(view)) != nbytes:
                raise CheckpointError("%s: short read" % path)
        image = self.image(nbytes)
        if nbytes:
            image[:nbytes].copy_(host[:nbytes], non_blocking=True)
            self.stats["h2d_copies"] += 1
            self.stats["h2d_bytes"] += nbytes
        return image, view, nbytes


def _torch_np_dtype(t):
    import torch
    table = {torch.float32: np.float32, torch.float64: np.float64, torch.int32: np.int32, torch.uint8: np.uint8, torch.int16: np.int16,
             torch.int8: np.int8, torch.int64: np.int64, torch.bool: np.bool_, torch.float16: np.float16}
    if t.dtype not in table:
        raise CheckpointError("dtype %s not supported" % t.dtype)
    return np.dtype(table[t.dtype])


def write_checkpoint_device(prefix, tensors, io, block_size=4096):
    """write_checkpoint(checksums=True) of {name: device tensor}, byte for byte, with the data shard assembled and checksummed on the
    device: the tensors are packed into one image in byte-sorted name order (C-contiguous, little-endian), ONE danhip_crc32c_batch call
    covers every tensor, the image and the CRC array come to pinned host memory behind one synchronisation, and the host writes the data
    file and - through the same _write_index as write_checkpoint - the index."""
    os.makedirs(os.path.dirname(os.path.abspath(prefix)), exist_ok=True)
    names = sorted(tensors, key=lambda s: s.encode("utf-8"))
    layout, offset = [], 0
    for n in names:
        t = tensors[n]
        try:
            dt = _torch_np_dtype(t)
        except CheckpointError as e:
            raise CheckpointError("%s: %s" % (n, e))
        nb = t.numel() * t.element_size()
        layout.append((n, dt, tuple(t.shape), offset, nb))
        offset += nb
    image = io.image(offset)
    for (n, _, _, off, _) in layout:
        io.pack(image, off, tensors[n].detach())
    crcs = io.crc_launch(image, [(off, nb) for (_, _, _, off, nb) in layout], masked=True)
    data, crc = io.fetch(image, offset, crcs)
    with open(prefix + ".data-00000-of-00001", "wb") as f:
        f.write(memoryview(data))
    _write_index(prefix, [(n, _bundle_entry(dt, shape, off, nb, int(c))) for (n, dt, shape, off, nb), c in zip(layout, crc)], block_size)


# ------------------------------------------------------------------------------------------------------------ warm start
def map_variable_names(var_names, model_scope, checkpoint_model_scope, checkpoint_exclude_scopes=None, name_remap=None):
    """scaffolds.get_init_fn_for_scaffold's name rules (utility/scaffolds.py:27-58): {checkpoint name: variable name}.
    var_names are full graph names ('<model_scope>/conv1/conv1_1/conv2d/kernel')."""
    exclusions = [s.strip() for s in checkpoint_exclude_scopes.split(",")] if checkpoint_exclude_scopes else []
    kept = [v for v in var_names if not any(ex in v for ex in exclusions)]           # substring match, as the reference (:38)
    if checkpoint_model_scope is None:
        return {v: v for v in kept}
    if checkpoint_model_scope.strip() == "":
        mapped = {v.replace(model_scope + "/", ""): v for v in kept}
    else:
        mapped = {v.replace(model_scope, checkpoint_model_scope.strip()): v for v in kept}
    if name_remap is not None:
        renamed = {}
        for ck, v in mapped.items():
            for k, r in name_remap.items():
                if k in ck:
                    renamed[ck.replace(k, r)] = v
                    break
            else:
                renamed[ck] = v
        mapped = renamed
    return mapped


def init_from_checkpoint(variables, checkpoint_path, model_scope, checkpoint_model_scope, checkpoint_exclude_scopes=None,
                         ignore_missing_vars=False, name_remap=None, verify=False):
    """Restores a VariableStore the way the reference's scaffold init_fn does (utility/scaffolds.py:24-88); returns the list of
    restored variable names.  `checkpoint_path` is a prefix or a directory holding a 'checkpoint' state file.  verify: every tensor of the
    checkpoint that carries a CRC is checked on the host (CheckpointReader.verify_all) before any variable is written."""
    import torch
    if os.path.isdir(checkpoint_path):
        found = latest_checkpoint(checkpoint_path)
        if found is None:
            raise CheckpointError("no checkpoint in %s" % checkpoint_path)
        checkpoint_path = found
    reader = CheckpointReader(checkpoint_path)
    if verify:
        reader.verify_all()
    store_names = [n for n, _ in variables.named()]
    full = {model_scope + "/" + n: n for n in store_names}
    mapping = map_variable_names(list(full), model_scope, checkpoint_model_scope, checkpoint_exclude_scopes, name_remap)
    if not mapping:
        raise ValueError("variables_to_restore cannot be empty")                       # scaffolds.py:62-63
    restored, params = [], dict(variables.named())
    for ck_name, var_name in mapping.items():
        if not reader.has_tensor(ck_name):
            if ignore_missing_vars or _optional(ck_name):
                continue
            raise CheckpointError("variable %s missing in checkpoint %s" % (ck_name, checkpoint_path))
        p = params[full[var_name]]
        t = reader.get_tensor(ck_name)
        if tuple(t.shape) != tuple(p.shape):                                           # Saver(reshape=False)
            raise CheckpointError("%s: checkpoint shape %s != variable shape %s" % (ck_name, tuple(t.shape), tuple(p.shape)))
        with torch.no_grad():
            p.copy_(torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(p.device))
        restored.append(full[var_name])
    _bump_weight_epoch()
    return restored


# Variables of this port's own options (the LFPN's transposed convolution, lfpn_upsample="transposed"): a checkpoint written without the
# option lacks them and their Momentum slots, and restores or warm-starts with ignore_missing_vars semantics whatever the caller asked for -
# they keep their initialiser (zero momentum).
OPTIONAL_VARIABLE_SCOPES = ("/upsample_deconv/",)


def _optional(ck_name):
    return any(s in ck_name for s in OPTIONAL_VARIABLE_SCOPES)


def _bump_weight_epoch():
    """Parameters were written through views (members of fused blocks keep their own version counters): the cached 16-bit packings of
    ops.packed_weights key on (WEIGHT_EPOCH, block version, pointer) and must be refreshed."""
    from .. import ops
    ops.WEIGHT_EPOCH += 1


def _momentum_views(trainer):
    """{variable name: view of the flat momentum buffer} — tf.train.MomentumOptimizer keeps one 'Momentum' slot per variable."""
    flat = trainer.flat
    out = {}
    for n, p in trainer.model.vs.named():
        off = p.data.data_ptr() - flat.w.data_ptr()
        assert off >= 0 and off % 4 == 0
        out[n] = flat.v.as_strided(p.data.shape, p.data.stride(), off // 4)
    return out


def _device_io(trainer, device, device_io=None):
    """The DeviceCheckpointIO of a call: the one passed in, else the trainer's (made on first use and kept: its staging buffers are reused)."""
    if device_io is not None:
        return device_io
    if trainer is None:
        return DeviceCheckpointIO(device)
    if getattr(trainer, "checkpoint_io", None) is None:
        trainer.checkpoint_io = DeviceCheckpointIO(device)
    return trainer.checkpoint_io


def save_checkpoint(variables, prefix, model_scope, checksums=False, trainer=None, device_io=None):
    """Writes the VariableStore under the reference's graph names ('<model_scope>/<name>'): trainable variables AND the non-trainable
    state the Estimator's Saver writes — batch-norm moving_mean / moving_variance (VariableStore.bufs) — and, given the trainer, the
    optimizer slots ('<var>/Momentum', tf.train.MomentumOptimizer train_dan.py:521) and 'global_step' (int64), so that a run resumed
    from its own checkpoint continues the learning-rate schedule and the momenta (train_dan.py:549-556 keeps 5 such checkpoints).
    checksums: False no per-tensor CRC (TensorFlow's reader refuses such a file); True CRCs on the host (one .cpu() per tensor);
    "device" the same bytes as True with the shard assembled and checksummed on the GPU (write_checkpoint_device; variables on a GPU)."""
    if checksums == "device":
        named = variables.named()
        device = named[0][1].device if named else trainer.flat.w.device
        io = _device_io(trainer, device, device_io)
        tensors = {model_scope + "/" + n: p.detach() for n, p in named}
        for n, b in getattr(variables, "bufs", {}).items():
            tensors[model_scope + "/" + n] = b.detach()
        if trainer is not None:
            import torch
            for n, v in _momentum_views(trainer).items():
                tensors[model_scope + "/" + n + "/Momentum"] = v.detach()
            tensors["global_step"] = torch.full((), int(trainer.step_no), dtype=torch.int64, device=io.device)
            if getattr(trainer, "ls_state", None) is not None:
                tensors["danhip/loss_scale"] = trainer.ls_state[0:2].detach().to(torch.float32)
        for n, t in tensors.items():
            if t.device != io.device:
                raise CheckpointError('%s lives on %s: checksums="device" needs every tensor on %s' % (n, t.device, io.device))
        write_checkpoint_device(prefix, tensors, io)
        return
    if checksums not in (False, True):
        raise ValueError('checksums must be False, True or "device", got %r' % (checksums,))
    tensors = {model_scope + "/" + n: p.detach().cpu().numpy() for n, p in variables.named()}
    for n, b in getattr(variables, "bufs", {}).items():
        tensors[model_scope + "/" + n] = b.detach().cpu().numpy()
    if trainer is not None:
        for n, v in _momentum_views(trainer).items():
            tensors[model_scope + "/" + n + "/Momentum"] = v.detach().cpu().contiguous().numpy()
        tensors["global_step"] = np.asarray(int(trainer.step_no), dtype=np.int64)
        if getattr(trainer, "ls_state", None) is not None:       # fp16 build: dynamic loss scale {scale, clean steps} (not a reference variable)
            tensors["danhip/loss_scale"] = trainer.ls_state[0:2].detach().cpu().numpy().astype(np.float32)
    write_checkpoint(prefix, tensors, checksums=checksums)


class _VerifiedShard(object):
    """restore_checkpoint(verify=True) with the variables on a GPU: the single data shard read once into pinned memory and uploaded once,
    every entry that carries a CRC checked by ONE danhip_crc32c_batch call against the index (CheckpointError naming the tensor, before
    anything is written); the variables are then filled from the device image."""

    def __init__(self, reader, io):
        self.reader, self.io = reader, io
        self.image, self.host, nbytes = io.upload(reader.shard_path(0))
        checked = reader.checked_entries(0, nbytes)
        crcs = io.crc_launch(self.image, [(e["offset"], e["size"]) for _, e in checked], masked=True)
        _, got = io.fetch(self.image, 0, crcs)
        for (n, e), c in zip(checked, got):
            if int(c) != e["crc"]:
                raise CheckpointError("%s: data checksum mismatch" % n)
        self.nbytes = nbytes

    def host_tensor(self, name):
        return self.reader.get_tensor_from(name, self.host)

    def device_tensor(self, name):
        """The entry as a device tensor viewing the uploaded image (None: a dtype torch has no view for - the caller takes host_tensor)."""
        import torch
        e = self.reader.entries[name]
        to_torch = {np.float32: torch.float32, np.float64: torch.float64, np.int32: torch.int32, np.uint8: torch.uint8, np.int16: torch.int16,
                    np.int8: torch.int8, np.int64: torch.int64, np.bool_: torch.bool, np.float16: torch.float16}
        if e["sliced"] or DTYPES.get(e["dtype"]) not in to_torch:
            return None
        dt = to_torch[DTYPES[e["dtype"]]]
        item = np.dtype(DTYPES[e["dtype"]]).itemsize
        count = int(np.prod(e["shape"], dtype=np.int64)) if e["shape"] else 1
        if count * item != e["size"] or e["offset"] + e["size"] > self.nbytes:
            raise CheckpointError("%s: %d bytes in the index for shape %s" % (name, e["size"], e["shape"]))
        raw = self.image[e["offset"]:e["offset"] + e["size"]]
        if (self.image.data_ptr() + e["offset"]) % item:
            raw = raw.clone()
        return raw.view(dt).view(tuple(e["shape"]))


def restore_checkpoint(variables, checkpoint_path, model_scope, trainer=None, strict=True, verify=False, device_io=None):
    """tf.train.Saver().restore of a checkpoint written by save_checkpoint (the Estimator's resume path; eval_dan.py:406-411): every
    variable, the batch-norm moving statistics and — given the trainer — the Momentum slots and global_step.  Returns the restored
    names.  strict: a variable / slot missing in the checkpoint is an error (Saver semantics); global_step and slots are optional when
    strict is False (e.g. an inference-only checkpoint).
    verify: every entry of the checkpoint that carries a CRC is checked BEFORE anything is written - a mismatch raises CheckpointError
    naming the tensor and leaves variables, slots and global_step as they were; entries without a CRC (files written with
    checksums=False) are accepted.  With the variables on a GPU and a single-shard checkpoint the check runs on the device (_VerifiedShard:
    one read, one upload, one batch call), otherwise on the host (CheckpointReader.verify_all)."""
    import torch
    if os.path.isdir(checkpoint_path):
        found = latest_checkpoint(checkpoint_path)
        if found is None:
            raise CheckpointError("no checkpoint in %s" % checkpoint_path)
        checkpoint_path = found
    reader = CheckpointReader(checkpoint_path)
    restored = []
    shard = None
    if verify:
        named = variables.named()
        device = named[0][1].device if named else torch.device("cpu")
        if device.type == "cuda" and reader.num_shards == 1 and all(e["shard"] == 0 for e in reader.entries.values()):
            shard = _VerifiedShard(reader, _device_io(trainer, device, device_io))
        else:
            reader.verify_all()

    def get(ck_name):
        return reader.get_tensor(ck_name) if shard is None else shard.host_tensor(ck_name)

    def load(ck_name, dst):
        if not reader.has_tensor(ck_name):
            if strict and not _optional(ck_name):
                raise CheckpointError("variable %s missing in checkpoint %s" % (ck_name, checkpoint_path))
            return
        t = shard.device_tensor(ck_name) if shard is not None and dst.device == shard.image.device else None
        if t is None:
            t = torch.from_numpy(np.ascontiguousarray(get(ck_name), dtype=np.float32))
        if tuple(t.shape) != tuple(dst.shape):
            raise CheckpointError("%s: checkpoint shape %s != variable shape %s" % (ck_name, tuple(t.shape), tuple(dst.shape)))
        with torch.no_grad():
            dst.copy_(t.to(dst.device))
        restored.append(ck_name)

    for n, p in variables.named():
        load(model_scope + "/" + n, p)           # (under no_grad, on the Parameter itself: its version counter moves, as init_from_checkpoint does)
    for n, b in getattr(variables, "bufs", {}).items():
        load(model_scope + "/" + n, b)
    if trainer is not None:
        for n, v in _momentum_views(trainer).items():
            load(model_scope + "/" + n + "/Momentum", v)
        if reader.has_tensor("global_step"):
            trainer.step_no = int(get("global_step"))
            restored.append("global_step")
        elif strict:
            raise CheckpointError("global_step missing in checkpoint %s" % checkpoint_path)
        if getattr(trainer, "ls_state", None) is not None and reader.has_tensor("danhip/loss_scale"):      # optional: reference checkpoints lack it
            ls = np.asarray(get("danhip/loss_scale"), dtype=np.float32).reshape(-1)
            with torch.no_grad():
                trainer.ls_state[0:2].copy_(torch.from_numpy(ls[:2].copy()).to(trainer.ls_state.device))
            restored.append("danhip/loss_scale")
        if trainer._graph is not None:           # a captured step holds the old learning rate: the next train_step re-captures
            trainer._graph = None
            trainer._recapture = True
    if shard is not None:
        torch.cuda.current_stream(shard.image.device).synchronize()        # the copies out of the image are done before its buffer is reused
    _bump_weight_epoch()
    return restored

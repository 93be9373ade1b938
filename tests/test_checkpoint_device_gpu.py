"""Checkpoints assembled and checksummed on the device (save_checkpoint(checksums="device")) and verified on the way in
(restore_checkpoint(verify=True)): byte-equality with the host writer and with the second, independent encoder of the format
(tests/tf_bundle_encoder.py), restore bit for bit, refusal of a flipped byte before anything is written, acceptance of files without CRCs."""
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZE, BATCH = 64, 2                                                        # the smallest trainer the suite builds (test_train_cli_gpu.py)
SUFFIXES = (".index", ".data-00000-of-00001")


def _files(prefix):
    return [open(prefix + s, "rb").read() for s in SUFFIXES]


class _Store(object):
    """What save_checkpoint asks of a VariableStore."""

    def __init__(self, named, bufs):
        self._named, self.bufs = named, bufs

    def named(self):
        return list(self._named)


def test_hand_built_store(dev, tmp_path, monkeypatch):
    import tf_bundle_encoder
    from dan_amd.utility import checkpoint as C
    g = torch.Generator(device="cpu").manual_seed(1)
    block = torch.randn(6, 10, generator=g).to(dev)
    named = [("head/fused_view", block[:, 2:7]),                            # a strided view into a larger block
             ("conv/kernel", torch.randn(3, 3, 2, 5, generator=g).to(dev)),
             ("empty/kernel", torch.zeros(0, 4, device=dev)),               # a zero-element tensor
             ("odd/bias", torch.randn(7, generator=g).to(dev))]
    bufs = {"bn/moving_mean": torch.randn(5, generator=g).to(dev), "bn/moving_variance": torch.rand(5, generator=g).to(dev) + 0.5}
    store = _Store(named, bufs)
    assert not named[0][1].is_contiguous()
    io = C.DeviceCheckpointIO(dev)
    C.save_checkpoint(store, str(tmp_path / "dev"), "m", checksums="device", device_io=io)
    # the same values through the host writer with the CRC in plain Python
    values = {"m/" + n: t.cpu().numpy() for n, t in named}
    values.update({"m/" + n: t.cpu().numpy() for n, t in bufs.items()})
    monkeypatch.setattr(C, "_NATIVE", None)
    C.write_checkpoint(str(tmp_path / "host"), values, checksums=True)
    monkeypatch.undo()
    assert _files(str(tmp_path / "dev")) == _files(str(tmp_path / "host"))
    assert io.stats["batch_calls"] == 1 and io.stats["launches"] == 3 and io.stats["pack_copies"] == 5      # (the empty tensor needs no copy)
    assert (io.stats["h2d_copies"], io.stats["d2h_copies"]) == (1, 2)

    # a dict with a scalar int64 and an int32 vector besides, through write_checkpoint_device itself
    more = dict(values)
    more["global_step"] = np.asarray(123456789012, dtype=np.int64)
    more["m/ids"] = np.arange(-3, 8, dtype=np.int32)
    on_dev = {n: torch.from_numpy(np.ascontiguousarray(v)).reshape(v.shape).to(dev) for n, v in more.items()}
    on_dev["m/head/fused_view"] = block[:, 2:7]
    C.write_checkpoint_device(str(tmp_path / "dev2"), on_dev, io)
    monkeypatch.setattr(C, "_NATIVE", None)
    C.write_checkpoint(str(tmp_path / "host2"), more, checksums=True)
    monkeypatch.undo()
    assert _files(str(tmp_path / "dev2")) == _files(str(tmp_path / "host2"))
    # the independent encoder (two shards, other block sizes) computes the same tensor CRCs
    tf_bundle_encoder.write_bundle(str(tmp_path / "tf"), {n: np.ascontiguousarray(v).reshape(v.shape) for n, v in more.items()})
    ours, theirs = C.CheckpointReader(str(tmp_path / "dev2")), C.CheckpointReader(str(tmp_path / "tf"))
    assert set(ours.entries) == set(theirs.entries) == set(more)
    for n in more:
        assert ours.entries[n]["crc"] is not None and ours.entries[n]["crc"] == theirs.entries[n]["crc"], n
        got = ours.get_tensor(n, verify=True)
        assert got.dtype == more[n].dtype and got.shape == more[n].shape and np.array_equal(got, more[n])


def _trainer(dev, seed):
    from dan_amd import synthetic
    from dan_amd.train_sfd import AnchorConfig, SFDModel, SFDTrainer
    tr = SFDTrainer(SFDModel(device=dev, seed=seed))
    imgs = synthetic.make_images(BATCH, SIZE, SIZE, dev, seed=3)
    loc_t, cls_t, _ = AnchorConfig(SIZE, SIZE, dev).encode_batch(synthetic.make_gt_boxes(BATCH, SIZE, SIZE, seed=2, max_faces=3))
    return tr, (imgs, loc_t, cls_t)


@pytest.fixture(scope="module")
def trained(dev, tmp_path_factory):
    """A real SFDTrainer after two steps, saved three ways."""
    d = tmp_path_factory.mktemp("ckpt")
    tr, args = _trainer(dev, seed=9)
    for _ in range(2):
        tr.train_step(*args)
    tr.save(str(d / "device" / "model.ckpt-2"), "sfd", checksums="device")
    stats = dict(tr.checkpoint_io.stats)
    tr.save(str(d / "host" / "model.ckpt-2"), "sfd", checksums=True)
    tr.save(str(d / "plain" / "model.ckpt-2"), "sfd", checksums=False)
    yield tr, d, stats
    tr.close()


def _state(tr):
    from dan_amd.utility.checkpoint import _momentum_views
    out = {n: p.detach().clone() for n, p in tr.model.vs.named()}
    out.update({n + "/Momentum": v.clone() for n, v in _momentum_views(tr).items()})
    out.update({n: b.clone() for n, b in getattr(tr.model.vs, "bufs", {}).items()})
    return out


def _same(a, b):
    return set(a) == set(b) and all(a[n].dtype == b[n].dtype and torch.equal(a[n], b[n]) for n in a)


def test_trainer_save_on_the_device_equals_the_host_writer(trained):
    from dan_amd.utility.checkpoint import CheckpointReader
    tr, d, stats = trained
    assert _files(str(d / "device" / "model.ckpt-2")) == _files(str(d / "host" / "model.ckpt-2"))
    r = CheckpointReader(str(d / "device" / "model.ckpt-2"))
    names = list(r.entries)
    assert len(names) > 50 and "global_step" in names and any(n.endswith("/Momentum") for n in names)
    for n in names:
        assert r.entries[n]["crc"] is not None
        r.get_tensor(n, verify=True)
    r.verify_all()
    assert int(r.get_tensor("global_step")) == 2
    # one batch call, and a number of host<->device copies that does not depend on the number of variables (the same three as for the
    # six tensors of test_hand_built_store: the table up, the image and the CRC array down)
    assert stats["batch_calls"] == 1 and stats["launches"] == 3
    assert (stats["h2d_copies"], stats["d2h_copies"]) == (1, 2)
    assert stats["pack_copies"] >= len(names) - 1 and stats["crc_bytes"] == os.path.getsize(str(d / "device" / "model.ckpt-2") + SUFFIXES[1])


def test_verified_restore_is_bit_exact(dev, trained):
    tr, d, _ = trained
    other, _ = _trainer(dev, seed=4)
    assert not _same(_state(tr), _state(other))
    names = other.restore(str(d / "device"), "sfd", verify=True)            # (a directory: the state file names the prefix)
    assert "global_step" in names and other.step_no == tr.step_no == 2
    assert _same(_state(tr), _state(other))
    s = other.checkpoint_io.stats
    assert s["batch_calls"] == 1 and s["launches"] == 3 and (s["h2d_copies"], s["d2h_copies"]) == (2, 1)     # shard + table up, CRCs down
    other.close()


def test_flipped_byte_is_refused_before_anything_is_written(dev, trained, tmp_path):
    from dan_amd.utility.checkpoint import CheckpointError, CheckpointReader
    tr, d, _ = trained
    for s in SUFFIXES:
        shutil.copy(str(d / "device" / "model.ckpt-2") + s, str(tmp_path / "model.ckpt-2") + s)
    prefix = str(tmp_path / "model.ckpt-2")
    raw = bytearray(open(prefix + SUFFIXES[1], "rb").read())
    at = len(raw) // 2
    raw[at] ^= 0x04
    open(prefix + SUFFIXES[1], "wb").write(bytes(raw))
    owner = [n for n, e in CheckpointReader(prefix).entries.items() if e["offset"] <= at < e["offset"] + e["size"]]
    assert len(owner) == 1
    other, _ = _trainer(dev, seed=4)
    other.step_no = 77
    before, w, v = _state(other), other.flat.w.clone(), other.flat.v.clone()
    with pytest.raises(CheckpointError) as err:
        other.restore(prefix, "sfd", verify=True)
    assert owner[0] in str(err.value) and "checksum" in str(err.value)
    assert other.step_no == 77 and torch.equal(other.flat.w, w) and torch.equal(other.flat.v, v) and _same(before, _state(other))
    other.restore(prefix, "sfd", verify=False)                              # unverified, as before: the damaged shard becomes weights
    assert other.step_no == 2 and not _same(before, _state(other))
    other.close()


def test_files_without_checksums_restore_under_verify(dev, trained):
    from dan_amd.utility.checkpoint import CheckpointReader
    tr, d, _ = trained
    prefix = str(d / "plain" / "model.ckpt-2")
    assert all(e["crc"] is None for e in CheckpointReader(prefix).entries.values())
    assert open(prefix + SUFFIXES[1], "rb").read() == open(str(d / "device" / "model.ckpt-2") + SUFFIXES[1], "rb").read()
    other, _ = _trainer(dev, seed=4)
    other.restore(prefix, "sfd", verify=True)
    assert other.step_no == 2 and _same(_state(tr), _state(other))
    other.close()

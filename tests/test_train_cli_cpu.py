"""CPU suite of the training driver (dan_amd/train_cli.py) and of the metric entry point's argument checks: flags, log line, checkpoint
rotation, export and refusals - nothing here launches a kernel."""
import ctypes
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "train_flags.json")))
MODELS = ("sfd", "pb", "dan", "dan_deform")


def test_parser_defaults_are_the_reference_flag_blocks():
    """tests/golden/train_flags.json: names, order and default values of every tf.app.flags definition of the four training scripts."""
    from dan_amd import train_cli
    for m in MODELS:
        args = vars(train_cli.build_parser(m).parse_args([]))
        want = GOLDEN[m]
        assert list(train_cli.flag_defaults(m)) == list(want), m
        for name, value in want.items():
            assert args[name] == value and type(args[name]) is type(value), (m, name, args[name], value)
        assert (args["device"], args["deterministic"], args["decode_entropy"]) == ("cuda:0", False, "host")
        assert list(train_cli.LOG_KEYS[m]) == GOLDEN["log_keys"][m]
    # tf.app.flags spellings of a boolean, and the ignored flags are still parsed
    a = train_cli.build_parser("sfd").parse_args(["--ignore_missing_vars=false", "--multi_gpu", "--num_readers", "3", "--data_format", "channels_last"])
    assert a.ignore_missing_vars is False and a.multi_gpu is True and a.num_readers == 3
    text = train_cli.build_parser("dan").format_help()
    for name in ("num_readers", "num_preprocessing_threads", "num_cpu_threads", "gpu_memory_fraction", "data_format", "multi_gpu"):
        assert name in train_cli.IGNORED_FLAGS and ("--" + name) in text
    assert text.count("ignored") >= 6                                     # --help says so, flag by flag


def test_every_script_has_a_main():
    import importlib
    for m in MODELS:
        mod = importlib.import_module("dan_amd.train_" + m)
        assert callable(mod.main)
        src = open(mod.__file__).read()
        assert 'if __name__ == "__main__":' in src


def test_log_line_formatter_is_the_reference_formatter():
    import collections
    from dan_amd import train_cli
    d = collections.OrderedDict([("lr", 1e-4), ("ce", 2.5), ("loc", 1.0 / 3.0), ("loss", 12.3456789), ("l2", 0.0), ("acc", 1.0)])
    assert train_cli.format_log(d) == "lr=0.000100, ce=2.500000, loc=0.333333, loss=12.345679, l2=0.000000, acc=1.000000"
    assert train_cli.parse_comma_list("0.1, 1, 0.1, 0.01") == [0.1, 1.0, 0.1, 0.01]


def test_checkpoint_rotation_keeps_five_and_names_the_newest(tmp_path):
    from dan_amd import train_cli
    from dan_amd.utility import checkpoint
    keeper = train_cli.CheckpointKeeper(str(tmp_path))
    assert keeper.keep == 5

    def save(step):
        prefix = keeper.prefix(step)
        assert os.path.basename(prefix) == "model.ckpt-%d" % step
        for suffix in (".index", ".data-00000-of-00001"):
            open(prefix + suffix, "wb").write(b"x")
        keeper.register(prefix)

    for step in (1, 2, 3, 10, 11):
        save(step)
    assert sorted(os.listdir(str(tmp_path))) == sorted(["checkpoint"] + ["model.ckpt-%d%s" % (s, e) for s in (1, 2, 3, 10, 11)
                                                                         for e in (".index", ".data-00000-of-00001")])
    save(12)                                                              # the 6th: the oldest goes - and model.ckpt-10 / -11 / -12 stay
    left = sorted(f for f in os.listdir(str(tmp_path)) if f != "checkpoint")
    assert left == sorted("model.ckpt-%d%s" % (s, e) for s in (2, 3, 10, 11, 12) for e in (".index", ".data-00000-of-00001"))
    lines = open(str(tmp_path / "checkpoint")).read().splitlines()
    assert lines[0] == 'model_checkpoint_path: "model.ckpt-12"'
    assert lines[1:] == ['all_model_checkpoint_paths: "model.ckpt-%d"' % s for s in (2, 3, 10, 11, 12)]
    assert checkpoint.latest_checkpoint(str(tmp_path)) == str(tmp_path / "model.ckpt-12")
    # a new process continues the list it finds
    again = train_cli.CheckpointKeeper(str(tmp_path))
    assert again.kept == ["model.ckpt-%d" % s for s in (2, 3, 10, 11, 12)]
    for suffix in (".index", ".data-00000-of-00001"):
        open(again.prefix(13) + suffix, "wb").write(b"x")
    again.register(again.prefix(13))
    assert not os.path.exists(str(tmp_path / "model.ckpt-2.index")) and os.path.exists(str(tmp_path / "model.ckpt-3.index"))
    assert checkpoint.latest_checkpoint(str(tmp_path)) == str(tmp_path / "model.ckpt-13")


def test_more_than_one_rank_is_refused(monkeypatch, tmp_path):
    import pytest
    from dan_amd import train_cli
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        train_cli.main(["--model_dir", str(tmp_path)], model="sfd")
    assert "WORLD_SIZE" in str(e.value) and "bench.py" in str(e.value)


def test_library_exports_cls_accuracy_and_refuses_bad_arguments():
    from dan_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "danhip_cls_accuracy") and "danhip_cls_accuracy" in _lib.SIGNATURES
    assert L.danhip_version() >= 13
    hdr = open(os.path.join(ROOT, "include", "danhip.h")).read()
    assert "int danhip_cls_accuracy(const float* cls, const int32_t* labels, const uint8_t* sel, int64_t* counts" in hdr
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                                 # aligned host memory: every check comes before the launch
    assert L.danhip_cls_accuracy(p, p, p, None, 1, 8, None) == -1 and b"cls_accuracy" in L.danhip_last_error()
    assert L.danhip_cls_accuracy(None, p, p, p, 1, 8, None) == -1
    assert L.danhip_cls_accuracy(p, p, p, p, 0, 8, None) == -1
    assert L.danhip_cls_accuracy(p, p, p, p, 2, 1 << 30, None) == -1      # B * A = 2^31: one past the 32-bit index range
    msg = L.danhip_last_error()
    assert b"cls_accuracy" in msg and b"2147483648" in msg and b"index range" in msg
    assert L.danhip_cls_accuracy(p, p, p, p, 65536, 32768, None) == -1

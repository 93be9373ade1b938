"""The ordered far-corner path of the deformable backward without a GPU: the host emulation (danhip_deform_far_ordered_emulate, the
per-record routines of csrc/deform_far.h run over checked host arrays) against a plain Python loop with an np.float32 running sum in key
order, and the command-line route of `train_dan_deform --deterministic`."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deform_ordered_cases as OC  # noqa: E402

emulate = OC.emulate


@pytest.mark.parametrize("L", OC.ORDER_L)
def test_emulation_equals_the_python_loop_in_key_order(L):
    case = OC.order_case(L)
    assert case.shared, "no two destinations share a source pixel"
    want = OC.order_far_dx(case)
    if L >= 7:
        assert not np.array_equal(want, OC.order_far_dx(case, descending=True)), "the case cannot tell ascending from descending order"
    for window in (0, 1, 2):
        got, records, errors = emulate(case.off, case.dS, 1, OC.OH, OC.OW, OC.OC, OC.ODG, window)
        assert errors == 0
        assert records == sum(len(r) for r in case.records.values())
        assert got.tobytes() == want.tobytes(), "window %d" % window


def test_emulation_counts_the_records_of_the_dyadic_cases():
    """On the dyadic cases every sum is exact: the emulation's record count equals corner_set restated in numpy, for both windows."""
    import deform_exact as DE
    for name in ("c64_9x17_c64_dg1", "c64_8x16_c256_dg4"):
        c = DE.CASE_BY_NAME[name]
        d = DE.data(name)
        for R in (1, 2):
            _, records, errors = emulate(d.off.numpy(), d.dS.numpy(), c.N, c.H, c.W, c.C, c.dg, R)
            assert errors == 0 and records == OC.far_record_count(d.off.numpy(), c.H, c.W, c.dg, R) and records > 0


def test_emulation_refuses_other_shape_classes():
    from dan_amd import _lib
    L = _lib.lib()
    a = np.zeros(16, np.int16)
    f = np.zeros(16, np.float32)
    assert L.danhip_deform_far_ordered_emulate(a.ctypes.data, a.ctypes.data, f.ctypes.data, 16, 1, 1, 1, 32, 1, 0, None, None) == -1      # C / dg = 32
    assert L.danhip_version() >= 17
    assert L.danhip_deform_sample_bwd_ordered_workspace_bytes(2, 8, 16, 128, 4) == 0
    nx, nd = 16 * 160 * 160 * 256, 16 * 160 * 160 * 4
    want = (nx + 64) * 4 + 4 * ((2 * nd + 1 + (nd + 2047) // 2048 + 3) // 4 * 4 + 4 * 9 * nd)
    assert L.danhip_deform_sample_bwd_ordered_workspace_bytes(16, 160, 160, 256, 4) == want


# ---------------------------------------------------------------------------------------------------------------- flags
def test_deterministic_flag_of_dan_deform_takes_the_context_route(monkeypatch):
    from dan_amd import ops, train_cli, train_dan, train_sfd
    seen = {}

    class FakeTrainer(object):
        def __init__(self, model, anchors, **kw):
            seen.update(kw, model=model)

    monkeypatch.setattr(train_dan, "DANTrainer", FakeTrainer)
    monkeypatch.setattr(train_dan, "DANModel", lambda **kw: ("model", kw["deform"]))
    monkeypatch.setattr(train_sfd, "AnchorConfig", lambda *a, **kw: "anchors")
    args = train_cli.build_parser("dan_deform").parse_args(["--deterministic", "--train_image_size", "64"])
    assert args.deterministic is True
    train_cli._Setup("dan_deform", args, torch.device("cpu"), dict(deterministic=args.deterministic, metrics=True))
    assert seen["model"] == ("model", True)
    assert seen["deterministic"] is False and isinstance(seen["ops_ctx"], ops.OpsContext) and seen["ops_ctx"].deterministic is True
    assert seen["ops_ctx"] is not ops.context() and ops.context().deterministic is False
    # the VGG model keeps the trainer's own flag, and without --deterministic nothing changes for the deformable one
    seen.clear()
    train_cli._Setup("dan", args, torch.device("cpu"), dict(deterministic=True, metrics=True))
    assert seen["deterministic"] is True and "ops_ctx" not in seen
    seen.clear()
    train_cli._Setup("dan_deform", args, torch.device("cpu"), dict(deterministic=False, metrics=True))
    assert seen["deterministic"] is False and "ops_ctx" not in seen


def test_deterministic_context_copies_the_source_and_sets_the_switch():
    from dan_amd import ops
    src = ops.OpsContext(KEEP_DEFORM_COL=False, deterministic=False)
    ctx = ops.deterministic_context(src)
    assert ctx is not src and ctx.deterministic is True and ctx.KEEP_DEFORM_COL is False and src.deterministic is False
    assert ops.deterministic_context().deterministic is True

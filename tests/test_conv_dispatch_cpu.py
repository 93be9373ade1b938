"""The convolution dispatch (which kernel instance a call gets, what the capability and workspace queries answer) against the table
recorded from the parent of the commit that introduced the single selection: tests/golden/conv_dispatch.json, written by
tests/golden/make_conv_dispatch_golden.py (see its header).  Host code only: no GPU, no DANHIP_* variable."""
import ctypes
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_conv_dispatch_golden", os.path.join(GOLDEN, "make_conv_dispatch_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def golden():
    g = _generator()
    return g, g.load(os.path.join(GOLDEN, "conv_dispatch.json"))


def test_table_covers_every_instance_family(golden):
    _, table = golden
    seen = {v for cols in table.values() for c, vals in cols.items() if c.startswith("label_") or c == "wgrad_label" for v in vals}
    want = ["conv_igemm_kernel<%s, %s>" % (t, f) for t in ("128, 128, 2", "256, 64, 1", "256, 32, 1", "64, 16, 1", "256, 16, 1") for f in ("true", "false")]
    for tile in ("8, 32", "16, 16"):
        want += ["conv3x3_halo_kernel<%s, 128, 4, 2, 1, 4, %s>" % (tile, v) for v in ("false, 0, false", "true, 0, false", "false, 0, true")]
        want += ["conv3x3_halo_kernel<%s, 64, 8, 1, 1, 4, %s, 0, false>" % (tile, v) for v in ("false", "true")]
        want += ["conv3x3_halo_kernel<%s, 64, 8, 1, 3, 3, false, 1, false>" % tile]
    want += ["conv3x3_c64_kernel<false>", "conv3x3_c64_kernel<true>", "conv3x3_c8_kernel<true>", "conv_bwd_data_strided_kernel"]
    want += ["conv_pointwise_kernel<128, 4, false, true, false>", "conv_pointwise_kernel<128, 4, false, true, true>"]
    want += ["conv_wgrad_rows_kernel<128>", "conv_wgrad_rows_kernel<64>", "conv_wgrad_pw_kernel", "conv_wgrad_c8_kernel"]
    want += ["conv_wgrad_kernel<%s, 2>" % t for t in ("64, 64", "64, 128", "128, 64", "128, 128")]
    assert not [w for w in want if w not in seen]


@pytest.mark.parametrize("build", ["bf16", "fp16"])
def test_build_reproduces_recorded_dispatch(golden, build):
    g, table = golden
    from dan_amd import build as B
    B.build()
    got = g.sweep(g.bind(ctypes.CDLL(B.OUT if build == "bf16" else B.OUT_F16)))
    want = table[build]
    descs = g.descriptors()
    diffs = [(c, descs[i], want[c][i], got[c][i]) for c in want for i in range(len(descs)) if want[c][i] != got[c][i]]
    assert not diffs, "%d entries differ from the recorded dispatch (recorded with no DANHIP_* option set), the first: %r" % (len(diffs), diffs[:8])

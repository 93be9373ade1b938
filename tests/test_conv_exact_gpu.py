"""The convolution kernels against a float64 reference on integer-valued operands: every comparison is an equality (tests/conv_exact.py says
why), so a term counted zero times or twice, a ReLU mask taken with >= instead of >, or a pool tie sent to the wrong element fails with a
whole-number difference.  One case per row of test_conv_dispatch_gpu.CASES at that row's shape and call, plus the edge shapes of every family;
after each call the launched instance must be in the family the case is listed for."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_exact as CE  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = CE.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_convolution_equals_the_float64_reference(case, dev):
    CE.run_case(case, dev)


def test_exact_tables_cover_every_family_of_the_dispatch_table():
    import test_conv_dispatch_gpu as D
    listed = {c[3] for c in CASES}
    assert not [r for r in D.CASES if r[3] not in listed], "a kernel instance family without an exact case"
    rows = {c[0][4:]: c for c in CASES if c[4].get("row")}
    for name, shp, call, family in D.CASES:
        c = rows[name]
        assert c[2][:5] == shp[:5] and c[2][5] == shp[5] and c[2][7] == shp[6] and c[3] == family and c[4]["row"] == call

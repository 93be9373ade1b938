"""The DAN context block as ONE autograd node over channel-slice views (ops.context_block) against the unfused block in float64 - ten
convolutions, average pool, concat, residual add and their autograd, written in tests/conv_exact.py from the network's definition, not from
the fused node.  Sparse ternary kernels, a sparse integer input and an integer upstream gradient keep every value either route stores in
16 bits a multiple of 1/4 that bf16 and IEEE half hold exactly, and every fp32 sum exact (tests/test_conv_exact_cpu.py asserts that on the
reference): the output, the input gradient and all 20 variable gradients must EQUAL the reference.  A wrong mask slice, a dropped `accumulate`,
branch 2's bias at the map edge or a delivery into x's buffer counted twice shows as a whole-number (or quarter) difference.

The two "plus" kernels (a 3x1 and a 1x3 convolution packed into one 3x3) receive gradient in their structural zeros by design; the variables
here are plain autograd leaves, so autograd slices those taps away (VariableStore.build) exactly as it does outside the trainer: the 3x1 / 1x3
variables' gradients are compared, the zeros' are not."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_exact as CE  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CE.BLOCK_CASES, ids=[c[0] for c in CE.BLOCK_CASES])
def test_context_block_equals_the_unfused_float64_block(case, dev):
    from dan_amd import _lib, ops
    from dan_amd.net import danet
    from dan_amd.net.variables import VariableStore
    inp, ref = CE.block_reference(case)
    N, H, W, C = case[1]
    # the map is there for the path its name says: the block's 64 -> 64 3x3 convolutions (called with scratch) run on the register-resident
    # kernel on the large map and split K on the flat-M kernel on the small one
    d33 = ops._desc(N, H, W, 64, 64, 3, 3, 1)
    label = _lib.lib().danhip_conv_kernel_label(ctypes.byref(d33), 0).decode()
    if case[0].startswith("splitk"):
        assert label.startswith(CE.FLAT) and CE.plan_splitk(CE.S(N, H, W, 64, 64), 0, torch.cuda.get_device_properties(dev).multi_processor_count)[0] >= 2
    else:
        assert label == CE.C64F
    vs = VariableStore(device=dev, seed=1)
    bb = danet.VGG16Backbone("channels_last", variables=vs)
    bb.FUSED_CONTEXT_BLOCK = True
    x = inp["x"].to(ops.ACT).to(dev)
    with torch.no_grad():
        bb.se_inception_block(x, "blk")                   # creates the 20 variables under the reference's names
        names = [n for n, _ in vs.named()]
        assert sorted(names) == sorted("blk/" + n for n in inp["P"])
        for n, p in vs.named():
            p.copy_(inp["P"][n[4:]].to(torch.float32).to(dev))
    for _, p in vs.named():
        p.grad = None
    xin = x.clone().requires_grad_(True)
    out = bb.se_inception_block(xin, "blk")
    out.backward(inp["dy"].to(ops.ACT).to(dev))
    torch.cuda.synchronize()
    CE.assert_equal(out, ref["out"], case[0] + " out")
    CE.assert_equal(xin.grad, ref["dx"], case[0] + " dx")
    for n, p in vs.named():
        assert p.grad is not None, n
        CE.assert_equal(p.grad, ref["grads"][n[4:]], "%s gradient of %s" % (case[0], n))

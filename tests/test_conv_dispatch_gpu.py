"""Label equals launch: for one small shape per kernel-instance family the real call is made through the entry point dan_amd.ops uses
(with scratch where ops passes it), and the instance the library launched (danhip_conv_last_launch_label) must be the one the label
function names for the code ops._prof_end files that call under.  Identity only: the numbers are checked in test_conv_gpu.py."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# (id, (N, H, W, Cin, Cout, k, stride), call, family the case is there for: kernel name and the template arguments that tell its instances apart)
#   fwd / dgrad / dgrad_mask: the *_ws entry points with the scratch buffer danhip_conv2d_workspace_bytes asks for (codes 0 / 1 / 5), as
#   ops always calls them: a map has to be large enough that the split-K preference does not take it from the halo / streaming kernels;
#   fwd_pool: danhip_conv2d_fwd_pool_arg (code 4), which ops calls where the shape wants no scratch - fused pool or the pool kernel after it;
#   fwd_pool_bits / dgrad_bits: the bit-mask entry points, which go straight to their family (codes 4 / 5).
CASES = [
    ("c8", (1, 8, 32, 8, 64, 3, 1), "fwd", "conv3x3_c8_kernel<true>"),
    ("c64", (1, 8, 32, 64, 64, 3, 1), "fwd", "conv3x3_c64_kernel<false>"),
    ("c64_pool", (4, 136, 128, 64, 64, 3, 1), "fwd_pool", "conv3x3_c64_kernel<false>"),
    ("c64_dgrad_bits", (1, 8, 32, 64, 64, 3, 1), "dgrad_bits", "conv3x3_c64_kernel<true>"),
    ("halo128", (1, 136, 128, 64, 128, 3, 1), "fwd", "conv3x3_halo_kernel<8, 32, 128, * false, 0, false>"),
    ("halo128_pool_bits", (1, 8, 32, 64, 128, 3, 1), "fwd_pool_bits", "conv3x3_halo_kernel<8, 32, 128, * false, 0, true>"),
    ("halo72_pool_not_fused", (2, 136, 128, 64, 72, 3, 1), "fwd_pool", "conv3x3_halo_kernel<8, 32, 128, * false, 0, false>"),
    ("halo128_dgrad_bits", (1, 136, 128, 128, 128, 3, 1), "dgrad_bits", "conv3x3_halo_kernel<8, 32, 128, * true, 0, false>"),
    ("halo128_dgrad", (1, 136, 128, 128, 64, 3, 1), "dgrad", "conv3x3_halo_kernel<8, 32, 128, * true, 0, false>"),
    ("halo64", (1, 136, 128, 128, 64, 3, 1), "fwd", "conv3x3_halo_kernel<8, 32, 64, * 1, 4, false, 0, false>"),
    ("halo16x16", (8, 48, 48, 64, 128, 3, 1), "fwd", "conv3x3_halo_kernel<16, 16, 128, * false, 0, false>"),
    ("halo_head", (1, 136, 128, 64, 8, 3, 1), "fwd", "conv3x3_halo_kernel<8, 32, 64, * 3, 3, false, 1, false>"),
    ("pointwise", (1, 32, 64, 64, 64, 1, 1), "fwd", "conv_pointwise_kernel<64, 4, false, true, false>"),
    ("pointwise_pool_not_fused", (1, 32, 64, 64, 64, 1, 1), "fwd_pool", "conv_pointwise_kernel<64, 4, false, true, false>"),
    ("pointwise_dgrad_mask", (1, 32, 64, 64, 64, 1, 1), "dgrad_mask", "conv_pointwise_kernel<64, 4, true, true, false>"),
    ("pointwise_dgrad", (1, 32, 64, 64, 64, 1, 1), "dgrad", "conv_pointwise_kernel<64, 4, true, false, false>"),
    ("pointwise_taps", (12, 40, 40, 128, 64, 3, 1), "fwd", "conv_pointwise_kernel<64, 4, false, true, true>"),
    ("flat", (1, 8, 8, 64, 8, 3, 1), "fwd", "conv_igemm_kernel<64, 16, 1, true>"),
    ("flat_slow", (1, 8, 8, 72, 24, 3, 1), "fwd", "conv_igemm_kernel<256, 32, 1, false>"),
    ("splitk", (1, 10, 10, 512, 512, 3, 1), "fwd", "conv_igemm_kernel<128, 128, 2, true>"),
    ("splitk_dgrad_mask", (1, 10, 10, 512, 512, 3, 1), "dgrad_mask", "conv_igemm_kernel<128, 128, 2, true>"),
    ("direct_strided_dgrad", (1, 9, 9, 8, 8, 3, 3), "dgrad", "conv_bwd_data_strided_kernel"),
    ("wgrad_rows128", (2, 32, 64, 256, 72, 3, 1), "wgrad", "conv_wgrad_rows_kernel<128>"),
    ("wgrad_rows64", (1, 24, 32, 128, 40, 3, 1), "wgrad", "conv_wgrad_rows_kernel<64>"),
    ("wgrad_pw", (1, 64, 64, 128, 64, 1, 1), "wgrad", "conv_wgrad_pw_kernel"),
    ("wgrad_c8", (1, 8, 32, 8, 64, 3, 1), "wgrad", "conv_wgrad_c8_kernel"),
    ("wgrad_64_64", (1, 8, 8, 64, 64, 1, 1), "wgrad", "conv_wgrad_kernel<64, 64, 2>"),
    ("wgrad_64_128", (1, 8, 8, 64, 128, 1, 1), "wgrad", "conv_wgrad_kernel<64, 128, 2>"),
    ("wgrad_128_64", (1, 8, 8, 128, 64, 1, 1), "wgrad", "conv_wgrad_kernel<128, 64, 2>"),
    ("wgrad_128_128", (1, 8, 8, 128, 128, 1, 1), "wgrad", "conv_wgrad_kernel<128, 128, 2>"),
]
WHICH = {"fwd": 0, "fwd_pool": 4, "fwd_pool_bits": 4, "dgrad": 1, "dgrad_mask": 5, "dgrad_bits": 5}


def in_family(label, family):
    """family is the label with at most one ' * ' standing for the template arguments that the instances of the case do not differ in."""
    head, _, tail = family.partition(" * ")
    return label.startswith(head) and label.endswith(tail) if tail else label == family


def expected_label(L, d, call):
    if call == "wgrad":
        return L.danhip_conv_wgrad_kernel_label(ctypes.byref(d)).decode()
    return L.danhip_conv_kernel_label(ctypes.byref(d), WHICH[call]).decode()


@pytest.mark.parametrize("name,shape,call,family", CASES, ids=[c[0] for c in CASES])
def test_launched_instance_is_the_labelled_one(name, shape, call, family, dev):
    from dan_amd import ops
    from dan_amd._lib import ACT_DTYPE, BF16, lib, ptr, stream
    L = lib()
    N, H, W, Cin, Cout, k, s = shape
    d = ops._desc(N, H, W, Cin, Cout, k, k, s)
    dp = ctypes.byref(d)
    want = expected_label(L, d, call)
    assert in_family(want, family), "the case no longer covers the family it is there for: %s" % want
    co8 = (Cout + 7) // 8 * 8
    g = torch.Generator().manual_seed(3)

    def act(*dims):
        return (torch.randn(dims, generator=g) * 0.25).to(ACT_DTYPE).to(dev)

    def packed(which):
        r, c = ctypes.c_int64(), ctypes.c_int64()
        assert L.danhip_conv_packed_dims(dp, which, ctypes.byref(r), ctypes.byref(c)) == 0
        return act(r.value, c.value)

    def scratch(n):
        return (torch.empty(n, dtype=torch.uint8, device=dev), n) if n else (None, 0)

    def u8(*dims):
        return torch.zeros(dims, dtype=torch.uint8, device=dev)

    x, dy = act(N, H, W, Cin), act(N, d.Ho, d.Wo, co8)
    bias = torch.randn((Cout,), generator=g).to(dev)
    y, dx = torch.empty((N, d.Ho, d.Wo, Cout), dtype=ACT_DTYPE, device=dev), torch.empty_like(x)
    pooled = torch.empty((N, (d.Ho + 1) // 2, (d.Wo + 1) // 2, Cout), dtype=ACT_DTYPE, device=dev)
    parg = u8(pooled.numel() // Cout, max(Cout // 4, 1))
    if call == "fwd":
        ws, nws = scratch(L.danhip_conv2d_workspace_bytes(dp, 0))
        assert nws or not name.startswith("splitk")
        rc = L.danhip_conv2d_fwd_ws(dp, ptr(x), ptr(packed(0)), ptr(bias), ptr(y), BF16, 1, None, ptr(ws), nws, stream())
    elif call == "fwd_pool":
        assert L.danhip_conv2d_workspace_bytes(dp, 0) == 0      # (ops runs a shape that wants scratch through danhip_conv2d_fwd_ws and pools after it)
        rc = L.danhip_conv2d_fwd_pool_arg(dp, ptr(x), ptr(packed(0)), ptr(bias), ptr(y), ptr(pooled), ptr(parg), stream())
    elif call == "fwd_pool_bits":
        assert L.danhip_conv2d_fwd_emits_bits(dp, 1)
        rc = L.danhip_conv2d_fwd_relu_bits_arg(dp, ptr(x), ptr(packed(0)), ptr(bias), ptr(y), ptr(u8(N * d.Ho * d.Wo, Cout // 8)), ptr(pooled),
                                               ptr(u8(pooled.numel() // Cout, Cout // 8)), ptr(parg), stream())
    elif call in ("dgrad", "dgrad_mask"):
        ws, nws = scratch(L.danhip_conv2d_workspace_bytes(dp, 1))
        assert nws or not name.startswith("splitk")
        rc = L.danhip_conv2d_bwd_data_ws(dp, ptr(dy), ptr(packed(1)), ptr(x) if call == "dgrad_mask" else None, ptr(dx), 0, ptr(ws), nws, stream())
    elif call == "dgrad_bits":
        assert L.danhip_conv2d_bwd_data_takes_bits(dp)
        rc = L.danhip_conv2d_bwd_data_bits(dp, ptr(dy), ptr(packed(1)), ptr(u8(N * H * W, Cin // 8)), ptr(dx), 0, stream())
    else:
        cin_real = 3 if Cin == 8 else Cin
        dw = torch.zeros((k, k, cin_real, Cout), dtype=torch.float32, device=dev)
        db = torch.zeros((Cout,), dtype=torch.float32, device=dev)
        ws, nws = scratch(L.danhip_conv2d_bwd_weight_workspace_bytes(dp))
        rc = L.danhip_conv2d_bwd_weight_ws(dp, ptr(x), ptr(dy), ptr(dw), ptr(db), cin_real, ptr(ws), nws, stream())
    assert rc == 0, L.danhip_last_error().decode()
    torch.cuda.synchronize()
    assert L.danhip_conv_last_launch_label().decode() == want

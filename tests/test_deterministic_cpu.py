"""Deterministic mode, the parts that need no device: the option, the version, what the capability queries answer with the option on, and
that the new exports resolve with their argument types (dan_amd/_lib.py)."""
import ctypes

import pytest


@pytest.fixture
def L():
    from dan_amd import _lib
    lib = _lib.lib()
    old = lib.danhip_get_option(b"deterministic")
    yield lib
    lib.danhip_set_option(b"deterministic", old)


def test_option_and_version(L):
    assert L.danhip_version() >= 10
    assert L.danhip_set_option(b"deterministic", 1) == 0
    assert L.danhip_get_option(b"deterministic") == 1
    assert L.danhip_set_option(b"deterministic", 0) == 0
    assert L.danhip_get_option(b"deterministic") == 0


def test_weight_gradient_workspace_query_follows_the_option(L):
    from dan_amd import ops
    d = ops._desc(16, 160, 160, 256, 256, 3, 3, 1)            # conv3_2 at batch 16: a long launch, atomics by default
    L.danhip_set_option(b"deterministic", 0)
    assert L.danhip_conv2d_bwd_weight_workspace_bytes(ctypes.byref(d)) == 0
    L.danhip_set_option(b"deterministic", 1)
    assert L.danhip_conv2d_bwd_weight_workspace_bytes(ctypes.byref(d)) > 0
    # every family has a size: pointwise, stride 2 (generic tiles), the first layer, a thin head on a small map
    for shape in [(2, 48, 48, 128, 64, 1, 1, 1), (2, 10, 10, 256, 512, 3, 3, 2), (2, 64, 128, 8, 64, 3, 3, 1), (2, 5, 5, 256, 6, 3, 3, 1)]:
        assert L.danhip_conv2d_bwd_weight_workspace_bytes(ctypes.byref(ops._desc(*shape))) > 0, shape


def test_folded_first_layer_gradient_is_not_offered(L):
    from dan_amd import ops
    d = ops._desc(2, 128, 128, 64, 64, 3, 3, 1)                # conv1_2
    L.danhip_set_option(b"deterministic", 0)
    assert L.danhip_conv2d_bwd_data_first_supported(ctypes.byref(d)) == 1
    L.danhip_set_option(b"deterministic", 1)
    assert L.danhip_conv2d_bwd_data_first_supported(ctypes.byref(d)) == 0


def test_new_exports_resolve(L):
    for name in ("danhip_ordered_reduce_f32", "danhip_reduce_workspace_bytes", "danhip_relu_bwd_bias_grad_ws", "danhip_l2norm_bwd_ws",
                 "danhip_l2norm_bwd_pool_scatter_ws", "danhip_detection_loss_fwd_ws", "danhip_sgd_momentum_flat_ws"):
        assert getattr(L, name).argtypes is not None, name
    assert L.danhip_reduce_workspace_bytes(5000, 72) >= 2048 * 72 * 4
    assert L.danhip_reduce_workspace_bytes(3, 64) == 3 * 64 * 4
    assert L.danhip_loss_workspace_bytes() == 2048 and L.danhip_sgd_workspace_bytes() == 16640      # DANHIP_LOSS_WS_BYTES / DANHIP_SGD_WS_BYTES


def test_context_switch_sets_the_library_option(L):
    from dan_amd import ops
    assert ops.context().deterministic is False
    with ops.use_context(ops.OpsContext(deterministic=True)):
        assert L.danhip_get_option(b"deterministic") == 1
        with ops.use_context(ops.OpsContext()):
            assert L.danhip_get_option(b"deterministic") == 0
        assert L.danhip_get_option(b"deterministic") == 1
    assert L.danhip_get_option(b"deterministic") == 0


def test_trainers_outside_the_modes_scope_refuse_the_flag():
    """The deformable model (its backward's float atomics have no ordered form), a trainer class that does not declare the mode, more than
    one rank: refused at construction, before anything is built."""
    import types
    from dan_amd.train_dan import DANTrainer
    from dan_amd.train_sfd import DetectorTrainer, SFDTrainer
    with pytest.raises(NotImplementedError, match="deterministic"):
        DANTrainer(types.SimpleNamespace(deform=True), None, deterministic=True)
    with pytest.raises(NotImplementedError, match="deterministic"):
        DetectorTrainer(types.SimpleNamespace(), deterministic=True)
    with pytest.raises(NotImplementedError, match="one rank"):
        SFDTrainer(types.SimpleNamespace(), world=2, deterministic=True)

"""GradSlot's deferred delivery (the host side of the gradient junction): order of launches and accumulate flags, without a GPU."""
import torch


def _slot():
    from dan_amd import ops
    return ops, ops.GradSlot(torch.zeros((1, 2, 2, 8)), True)


def test_partner_pops_the_deferred_delivery():
    ops, s = _slot()
    log = []
    s.defer(ops.TAP_POOL, lambda buf, acc: log.append(("pool alone", acc)), "payload")
    assert s.pop_pending(ops.TAP_L2NORM) is None                 # not this kind: stays
    assert s.pop_pending(ops.TAP_POOL) == (0, "payload")         # first delivery of a fresh slot: written, not accumulated
    buf, acc = s.target()
    assert acc == 1 and log == []                                # the fused launch is the second delivery; nothing ran on its own
    assert s.take() is buf and log == []


def test_a_third_delivery_launches_the_deferred_one_first():
    ops, s = _slot()
    log = []
    _, acc0 = s.target()                                         # somebody wrote the slot before
    s.defer(ops.TAP_L2NORM, lambda buf, acc: log.append(("l2 alone", acc, buf is s.buf)), None)
    _, acc2 = s.target()                                         # a consumer that is not the partner
    assert (acc0, acc2) == (0, 1) and log == [("l2 alone", 1, True)]
    assert s.pop_pending(ops.TAP_L2NORM) is None


def test_take_launches_a_delivery_whose_partner_never_came():
    ops, s = _slot()
    log = []
    s.defer(ops.TAP_POOL, lambda buf, acc: log.append(acc), None)
    b = s.take()
    assert log == [0] and b is not None and s.pending is None and s.buf is None


def test_junction_switch_is_a_context_field(monkeypatch):
    from dan_amd import ops
    assert ops.OpsContext().USE_JUNCTION is True
    monkeypatch.setenv("DANHIP_JUNCTION", "0")
    assert ops.OpsContext().USE_JUNCTION is False
    s = ops.GradSlot(torch.zeros((1, 2, 2, 64)), True)
    s.taps = ops.TAP_L2NORM | ops.TAP_POOL
    assert ops._junction_ok(s, None, 64) and not ops._junction_ok(s, torch.zeros(1), 64) and not ops._junction_ok(s, None, 1024)
    with ops.use_context(ops.OpsContext()):
        assert not ops._junction_ok(s, None, 64)

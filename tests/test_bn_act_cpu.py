"""tests/bn_act_cases.py without a device: the exact cases are exact (every intermediate of the forward and of the frozen backward is
representable in fp32 in either association, every expected output is a bf16 AND an fp16 value, the parameter-gradient sums stay below 2^24),
some of their outputs land exactly on 0, the float64 restatement agrees with autograd, and the random cases are well conditioned."""
import numpy as np
import pytest
import torch

import bn_act_cases as BC

ACTS = ("bf16", "fp16")


def _f32_exact(a):
    return np.array_equal(np.asarray(a, np.float64).astype(np.float32).astype(np.float64), a)


def test_round16_and_neighbours():
    v = np.array([1.0, 1.00390625, 1.005859375, 255.5, -3.0000001, 0.0, 1e-3])
    for act, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        assert np.array_equal(BC.round16(v, act), torch.from_numpy(v).to(dt).double().numpy())           # (float64 -> 16 bits in one rounding both ways)
        assert BC.is16(BC.round16(v, act), act)
    assert BC.round16(np.array([1.005859375]), "bf16")[0] == 1.0078125 and BC.round16(np.array([1.00390625]), "bf16")[0] == 1.0     # ties to even
    one, up, up2 = 1.0, 1.0078125, 1.015625
    assert BC.neighbours(np.array([up]), np.array([one]), "bf16")[0] and not BC.neighbours(np.array([up2]), np.array([one]), "bf16")[0]
    assert BC.neighbours(np.array([0.99609375]), np.array([one]), "bf16")[0] and not BC.neighbours(np.array([0.9921875]), np.array([one]), "bf16")[0]


@pytest.mark.parametrize("shortcut", [False, True])
@pytest.mark.parametrize("C", BC.EXACT_C)
@pytest.mark.parametrize("M", BC.EXACT_M)
def test_exact_cases_are_exact(M, C, shortcut):
    c = BC.exact_case(M, C, shortcut)
    x, sc, gamma, beta, mean, rstd, dy = (c[k] for k in ("x", "shortcut", "gamma", "beta", "mean", "rstd", "dy"))
    for act in ACTS:
        assert BC.is16(x, act) and BC.is16(dy, act) and (sc is None or BC.is16(sc, act))
    assert all(_f32_exact(a) for a in (gamma, beta, mean, rstd))
    # the forward's intermediates, in fp32 step by step, against float64
    f = np.float32
    d = x.astype(f) - mean.astype(f)
    xh = d * rstd.astype(f)
    t = xh * gamma.astype(f)
    v = t + beta.astype(f)
    steps = [(d, x - mean), (xh, (x - mean) * rstd), (t, (x - mean) * rstd * gamma), (v, (x - mean) * rstd * gamma + beta)]
    if sc is not None:
        steps.append((v + sc.astype(f), (x - mean) * rstd * gamma + beta + sc))
    for got, want in steps:
        assert np.array_equal(got.astype(np.float64), want)
        assert np.array_equal(2 * want, np.rint(2 * want)) and np.abs(want).max() <= 256                     # x - mean: a multiple of 1/2 ...
    for got, want in steps[1:]:
        assert np.array_equal(want, np.rint(want))                                                           # ... then integers: FMA or not, any association
    for relu in (False, True):
        y = BC.fwd(x, sc, gamma, beta, mean, rstd, relu)
        assert np.abs(y).max() <= 256 and np.array_equal(y, np.rint(y)) and all(BC.is16(y, act) for act in ACTS)
    y = BC.fwd(x, sc, gamma, beta, mean, rstd, False)
    if M * C >= 40:
        assert (y == 0).sum() >= M * C // 40 and (y > 0).any() and (y < 0).any()                             # exact zeros: the mask is y > 0, not >=
    # frozen backward
    for mask in (None, np.maximum(y, 0.0)):
        dx, dsc, dgamma, dbeta = BC.bwd(x, dy, mask, gamma, mean, rstd, True)
        g = dsc
        assert all(BC.is16(dx, act) and BC.is16(dsc, act) for act in ACTS)
        assert np.array_equal((g.astype(f) * gamma.astype(f) * rstd.astype(f)).astype(np.float64), dx)
        assert np.array_equal(g * xh, np.rint(g * xh)) and np.abs(g * xh).sum(axis=0).max() < 2 ** 24 and np.abs(g).sum(axis=0).max() < 2 ** 24
        assert np.array_equal(dgamma, np.rint(dgamma)) and np.array_equal(dbeta, np.rint(dbeta))
    if M * C >= 40:                                                                                          # >= in place of > would change the result
        at0 = (y == 0) & (dy != 0)
        assert at0.any() and np.all(BC.bwd(x, dy, np.maximum(y, 0.0), gamma, mean, rstd, True)[1][at0] == 0)


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("relu,shortcut", [(False, False), (True, True)])
def test_float64_restatement_against_autograd(relu, shortcut, frozen):
    c = BC.train_case(33, 8, shortcut, "bf16")
    t = {k: (torch.from_numpy(v).requires_grad_(k in ("x", "shortcut", "gamma", "beta")) if v is not None else None) for k, v in c.items()}
    x = t["x"]
    if frozen:
        mean, var = t["moving_mean"], t["moving_var"]
    else:
        mean = x.mean(0)
        var = (x * x).mean(0) - mean * mean
    rstd = 1.0 / torch.sqrt(var + BC.EPS)
    v = (x - mean) * rstd * t["gamma"] + t["beta"]
    if shortcut:
        v = v + t["shortcut"]
    y = torch.relu(v) if relu else v
    y.backward(t["dy"])
    if frozen:
        m, r = c["moving_mean"], 1.0 / np.sqrt(c["moving_var"] + BC.EPS)
    else:
        m, _, r = BC.stats(c["x"])
    yn = BC.fwd(c["x"], c["shortcut"], c["gamma"], c["beta"], m, r, relu)
    dx, dsc, dgamma, dbeta = BC.bwd(c["x"], c["dy"], yn if relu else None, c["gamma"], m, r, frozen)
    assert np.allclose(yn, y.detach().numpy(), rtol=1e-12, atol=1e-12)
    for got, want in ((dx, x.grad), (dgamma, t["gamma"].grad), (dbeta, t["beta"].grad)) + (((dsc, t["shortcut"].grad),) if shortcut else ()):
        assert np.allclose(got, want.numpy(), rtol=1e-9, atol=1e-11)
    mm, mv = BC.moving(c["moving_mean"], c["moving_var"], m, BC.stats(c["x"])[1], 33)
    assert np.allclose(mv, c["moving_var"] * BC.MOMENTUM + c["x"].var(axis=0, ddof=1) * (1 - BC.MOMENTUM)) and mm.shape == (8,)


@pytest.mark.parametrize("act", ACTS)
def test_the_comparison_rule_sees_a_wrong_kernel(act):
    """fp32 evaluation of the training form (a stand-in for the device) passes `within` on every element; the same with the mask taken as
    y >= 0, with the shortcut's rounding doubled (sum rounded to 16 bits before the add) or with dx lacking its mean term does not."""
    M, C = 130, 256
    c = BC.train_case(M, C, True, act)
    f = np.float32
    x, sc, gamma, beta, dy = (c[k] for k in ("x", "shortcut", "gamma", "beta", "dy"))
    mean, _, rstd = BC.stats(x)
    mean, rstd = mean.astype(f).astype(np.float64), rstd.astype(f).astype(np.float64)                       # what a device saves
    want = BC.fwd(x, sc, gamma, beta, mean, rstd, True)
    slack = BC.fwd_slack(x, sc, gamma, beta, mean, rstd)
    v32 = np.maximum((x.astype(f) - mean.astype(f)) * rstd.astype(f) * gamma.astype(f) + beta.astype(f) + sc.astype(f), f(0))
    y = BC.round16(v32.astype(np.float64), act)
    assert BC.within(y, want, slack, act).all()
    twice = BC.round16(np.maximum(BC.round16(BC.fwd(x, None, gamma, beta, mean, rstd, False), act) + sc, 0.0), act)
    assert act == "fp16" or not BC.within(twice, want, slack, act).all()          # (bf16: two roundings show; fp16's finer step hides them here)
    dx = BC.bwd(x, dy, y, gamma, mean, rstd, False)[0]
    dslack = BC.bwd_slack(x, dy, y, gamma, mean, rstd)
    g = np.where(y > 0, dy, 0.0).astype(f)
    xh = (x.astype(f) - mean.astype(f)) * rstd.astype(f)
    a, b = g.sum(axis=0, dtype=f) / f(M), (g * xh).sum(axis=0, dtype=f) / f(M)
    dx32 = gamma.astype(f) * rstd.astype(f) * (g - a - xh * b)
    assert BC.within(BC.round16(dx32.astype(np.float64), act), dx, dslack, act).all()
    nomean = gamma.astype(f) * rstd.astype(f) * (g - xh * b)
    assert not BC.within(BC.round16(nomean.astype(np.float64), act), dx, dslack, act).all()
    ge = BC.bwd(x, dy, np.where(y >= 0, 1.0, 0.0), gamma, mean, rstd, False)[0]                              # mask y >= 0: every element passes
    assert not BC.within(BC.round16(ge, act), dx, dslack, act).all()

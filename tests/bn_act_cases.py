"""The fused batch-norm tails (csrc/bn_act.hip: danhip_bn_act_fwd_train / _fwd_infer / _bwd) restated in float64 numpy, the case generators of
tests/test_bn_act_gpu.py, and the 16-bit helpers both test files share.  tests/test_bn_act_cpu.py checks, without a device, that the exact
cases are exact, and checks the comparison rules themselves.

Exact cases.  xhat = (x - mean) rstd is an integer in [-5, 5] by construction (rstd in {1/2, 1, 2}, mean an integer, x = mean + xhat / rstd a
multiple of 1/2 of magnitude <= 14), gamma a non-zero integer in [-3, 3], beta an integer in [-8, 8], shortcut an integer in [-16, 16]:
every intermediate of y = act(xhat gamma + beta + shortcut) is an integer of magnitude <= 39 - exact in fp32 in any association, with or
without FMA contraction, and a bf16 and an fp16 value.  Every fifth element lands exactly on 0 (the shortcut, or x and beta, are chosen for
it): the mask is y > 0.  Backward, frozen form: dy an integer in [-4, 4]; dx = g gamma rstd is a multiple of 1/2 of magnitude <= 24;
dbeta = sum g and dgamma = sum g xhat are integer sums of magnitude <= 20 M <= 81980 < 2^24: exact in fp32 in any order of addition.

Random cases (training form).  The device rounds to 16 bits a value computed in fp32, the reference one computed in float64: where the
float64 value v lies next to a rounding boundary the two 16-bit values differ by one step - the neighbour rule, `neighbours`.  That rule
presumes |v| is of the size of its terms.  Where the terms cancel (|v| << |largest term| - some elements of any large random map), the
fp32 roundings of the TERMS, not of v, decide the result, and the neighbour rule is then replaced by their bound e: the device value must
lie in [round16(v - e), round16(v + e)] (`within`).  e comes from the formats alone:
  forward:  4 fp32 operations on the largest term (subtract, two products, up to two sums): e = 4 * 2^-24 |largest term| (`fwd_slack`);
  dx:       the same for its own terms, plus the error of the two fp32 sums a = sum g / M and b = sum g xhat / M, which any order of M additions
            keeps within (M - 1) 2^-24 times the mean magnitude of the addends (`bwd_slack`).
For an element whose 16-bit step exceeds e the interval is within the neighbour rule, so nothing is widened where the rule applies."""
import numpy as np

EPS = 1e-5
MOMENTUM = 0.997
EXACT_C = (8, 64, 256, 2048)
EXACT_M = (1, 7, 33, 4099)          # 4099 is prime: no lane or block count divides it; 4099 rows loop in the reduce kernels (grid cap 1024)
# (M, C) of the training-form comparisons: one row per block and many, a block of one row (C = 2048), a looping reduction
TRAIN_SHAPES = ((7, 64), (33, 8), (4099, 64), (130, 256), (9, 2048))


# ------------------------------------------------------------------------------------------------ 16-bit values
def round16(a, act):
    """float64 -> the nearest (ties to even) value of the 16-bit activation type `act` ("bf16" / "fp16"), as float64."""
    a = np.asarray(a, np.float64)
    if act == "fp16":
        return a.astype(np.float16).astype(np.float64)
    # float64 -> bf16 directly (through fp32 first would round twice): round the float64 to 8 significand bits
    m, e = np.frexp(a)                                   # a = m 2^e, 0.5 <= |m| < 1
    r = np.ldexp(np.rint(m * 256.0), e - 8)              # np.rint: ties to even
    return np.where(np.isfinite(a), r, a)


def is16(a, act):
    a = np.asarray(a, np.float64)
    return bool(np.array_equal(round16(a, act), a))


def step16(a, act):
    """the distance from |a| to the next larger 16-bit value (normal range)"""
    _, e = np.frexp(np.asarray(a, np.float64))
    return np.ldexp(1.0, e - (11 if act == "fp16" else 8))


def neighbours(got, want64, act):
    """got (16-bit values as float64) equals round16(want64) or the 16-bit value next to it on either side -> bool array"""
    r = round16(want64, act)
    small, big = np.minimum(np.abs(got), np.abs(r)), np.maximum(np.abs(got), np.abs(r))
    adjacent = (np.sign(got) == np.sign(r)) & (small > 0) & (big - small == step16(small, act))      # (the step up from the smaller one)
    return (got == r) | adjacent


# ------------------------------------------------------------------------------------------------ the three entry points in float64
def fwd(x, shortcut, gamma, beta, mean, rstd, relu):
    v = (x - mean) * rstd * gamma + beta
    if shortcut is not None:
        v = v + shortcut
    return np.maximum(v, 0.0) if relu else v


def stats(x, eps=EPS):
    """-> (mean, biased variance, rstd) over the rows of x [M, C]"""
    mean = x.mean(axis=0)
    var = np.maximum((x * x).mean(axis=0) - mean * mean, 0.0)
    return mean, var, 1.0 / np.sqrt(var + eps)


def moving(mm, mv, mean, var, M, momentum=MOMENTUM):
    """the reference's rule: moving = moving m + batch (1 - m), the variance Bessel-corrected (TF1's fused batch norm)"""
    unbiased = var * (M / (M - 1.0)) if M > 1 else var
    return mm * momentum + mean * (1.0 - momentum), mv * momentum + unbiased * (1.0 - momentum)


def bwd(x, dy, y, gamma, mean, rstd, frozen):
    """-> (dx, dshortcut, dgamma, dbeta); y None: no ReLU in the forward"""
    g = dy if y is None else np.where(y > 0, dy, 0.0)
    xhat = (x - mean) * rstd
    dbeta, dgamma = g.sum(axis=0), (g * xhat).sum(axis=0)
    if frozen:
        dx = g * gamma * rstd
    else:
        M = x.shape[0]
        dx = gamma * rstd * (g - dbeta / M - xhat * dgamma / M)
    return dx, g, dgamma, dbeta


def fwd_slack(x, shortcut, gamma, beta, mean, rstd):
    t = np.maximum(np.abs((x - mean) * rstd * gamma), np.abs(beta) + np.zeros_like(x))
    t = t if shortcut is None else np.maximum(t, np.abs(shortcut))
    return np.ldexp(t, -22)


def bwd_slack(x, dy, y, gamma, mean, rstd):
    g = dy if y is None else np.where(y > 0, dy, 0.0)
    xhat = (x - mean) * rstd
    M = x.shape[0]
    a, b = g.sum(axis=0) / M, (g * xhat).sum(axis=0) / M
    terms = np.maximum(np.maximum(np.abs(g), np.abs(a)), np.abs(xhat * b))
    sums = (M - 1) * 2.0 ** -24 * (np.abs(g).mean(axis=0) + np.abs(xhat) * np.abs(g * xhat).mean(axis=0))
    return np.abs(gamma * rstd) * (np.ldexp(terms, -22) + sums)


def within(got, want64, slack, act):
    """the neighbour rule, or inside the 16-bit roundings of want64 -+ slack (module docstring) -> bool array"""
    return neighbours(got, want64, act) | ((got >= round16(want64 - slack, act)) & (got <= round16(want64 + slack, act)))


# ------------------------------------------------------------------------------------------------ case generators
def exact_case(M, C, shortcut, seed=0):
    """-> dict of float64 arrays x [M,C], shortcut [M,C] or None, gamma, beta, mean, rstd [C], dy [M,C] (module docstring)"""
    r = np.random.RandomState(1000 * seed + 7 * M + C)
    rstd = np.ldexp(1.0, r.randint(-1, 2, size=C))
    mean = r.randint(-4, 5, size=C).astype(np.float64)
    gamma = r.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], size=C)
    beta = r.randint(-8, 9, size=C).astype(np.float64)
    xhat = r.randint(-5, 6, size=(M, C)).astype(np.float64)
    zero = (np.arange(M * C).reshape(M, C) % 5) == 0         # these land exactly on 0
    if shortcut:
        sc = r.randint(-16, 17, size=(M, C)).astype(np.float64)
        sc = np.where(zero, -(xhat * gamma + beta), sc)          # |.| <= 23
    else:
        sc = None
        beta[::3] = 0.0
        xhat = np.where(zero & (beta == 0.0), 0.0, xhat)
    x = mean + xhat / rstd
    dy = r.randint(-4, 5, size=(M, C)).astype(np.float64)
    return dict(x=x, shortcut=sc, gamma=gamma, beta=beta, mean=mean, rstd=rstd, dy=dy)


def train_case(M, C, shortcut, act, seed=0):
    """random 16-bit x (mean 0.5, std 2, as tests/test_layers2_gpu.py's), shortcut and dy, fp32 gamma in [0.5, 1.5) and beta ~ 0.1 N(0,1),
    non-trivial moving statistics"""
    r = np.random.RandomState(50021 * seed + 13 * M + C + (1 if shortcut else 0))
    x = round16(r.randn(M, C) * 2.0 + 0.5, act)
    sc = round16(r.randn(M, C), act) if shortcut else None
    gamma = (r.rand(C) + 0.5).astype(np.float32).astype(np.float64)
    beta = (r.randn(C) * 0.1).astype(np.float32).astype(np.float64)
    dy = round16(r.randn(M, C), act)
    mm = (r.randn(C) * 0.2).astype(np.float32).astype(np.float64)
    mv = (r.rand(C) + 0.5).astype(np.float32).astype(np.float64)
    return dict(x=x, shortcut=sc, gamma=gamma, beta=beta, dy=dy, moving_mean=mm, moving_var=mv)

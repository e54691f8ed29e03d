"""Host models of the two identities behind the division-free compact box test
(rt_kernel_common.h box_test_compact_q, option box_interior):

  * unit_quotients: inside face_interior's shared-reciprocal regime (|n| >= 2^-100, delta within
    [2^-60, 2^20] in magnitude) `0 <= RN(n / delta) <= 1` is decided from n and delta alone -- equal
    signs and |n| <= |delta| -- checked against numpy's correctly rounded float32 division over a
    few million seeded pairs and the edges; outside the regime (a zero or tiny numerator, whose
    quotient may be -0 or underflow to it) the kernel keeps the division, which the model shows
    is needed: the predicate alone is wrong exactly there;
  * planes: the opposite face's plane parameter from the shared reciprocal and the shared s*o_k
    equals the per-face expression, with every multiply, subtract and fma rounded to float32 from
    exact rational arithmetic (no float64 intermediate), for any odd reciprocal estimate.
"""
from fractions import Fraction

import numpy as np

F32 = np.float32
REGIME_N = F32(2.0 ** -100)
D_LO, D_HI = 2.0 ** -60, 2.0 ** 20


def unit_quotients(n, d):
    """The kernel's predicate for one numerator: no sign difference, |n| <= |delta|."""
    n, d = np.asarray(n, F32), np.asarray(d, F32)
    return ((n.view(np.int32) ^ d.view(np.int32)) >= 0) & (np.abs(n) <= np.abs(d))


def in_regime(n):
    return np.abs(np.asarray(n, F32)) >= REGIME_N   # false for zero, tiny and NaN


def by_division(n, d):
    with np.errstate(all="ignore"):
        q = np.asarray(n, F32) / np.asarray(d, F32)
    assert q.dtype == np.float32
    return (F32(0) <= q) & (q <= F32(1))


def decide(n, d):
    """What the kernel does: the predicate in the regime, the division outside it."""
    return np.where(in_regime(n), unit_quotients(n, d), by_division(n, d))


def _log_uniform(rng, lo, hi, size):
    mag = np.exp2(rng.uniform(np.log2(lo), np.log2(hi), size))
    return (mag * rng.choice([-1.0, 1.0], size)).astype(F32)


def _steps(x, k):
    """x moved k floats up (k < 0: down) in magnitude order."""
    x = np.asarray(x, F32)
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf) * np.sign(x) if k > 0 else F32(0))
    return x


def test_predicate_equals_division_seeded_pairs():
    rng = np.random.default_rng(20240607)
    N = 1_500_000
    d = np.clip(np.abs(_log_uniform(rng, D_LO, D_HI, N)), F32(D_LO), F32(D_HI)) * rng.choice([-1, 1], N).astype(F32)
    # numerators: a fraction of delta around [-1.5, 1.5]; any magnitude of the regime; within a few
    # floats of +-delta
    n1 = (d * rng.uniform(-1.5, 1.5, N).astype(F32)).astype(F32)
    n2 = _log_uniform(rng, 2.0 ** -100, 2.0 ** 40, N)
    k = rng.integers(-6, 7, N).astype(np.int32)
    n3 = (d.view(np.int32) + k).view(F32) * rng.choice([-1, 1], N).astype(F32)   # k floats from +-delta
    total = 0
    for n in (n1, n2, n3):
        ok = in_regime(n)
        total += int(ok.sum())
        bad = np.nonzero(ok & (unit_quotients(n, d) != by_division(n, d)))[0]
        assert bad.size == 0, (n[bad[:5]], d[bad[:5]])
    assert total > 4_000_000


def test_predicate_edges():
    ds = []
    for mag in (D_LO, D_HI, 1.0, 1.5, 2.0 - 2.0 ** -23, 1.0 + 2.0 ** -23, 3.0e-7, 12345.678):
        for s in (1.0, -1.0):
            ds.append(F32(s * mag))
    ds += [_steps(F32(D_LO), 1), _steps(F32(D_HI), -1), -_steps(F32(D_LO), 1), -_steps(F32(D_HI), -1)]
    for d in ds:
        ns = [d, -d]
        for k in range(1, 9):
            # delta (1 +- k 2^-24) rounded to float32, and the k-th float on either side of +-delta
            for sgn in (1.0, -1.0):
                ns.append(F32(sgn * float(d) * (1.0 + k * 2.0 ** -24)))
                ns.append(F32(sgn * float(d) * (1.0 - k * 2.0 ** -24)))
                ns.append(F32(sgn) * _steps(d, k))
                ns.append(F32(sgn) * _steps(d, -k))
        ns += [REGIME_N, -REGIME_N, _steps(REGIME_N, 1), -_steps(REGIME_N, 1), F32(np.inf), F32(-np.inf)]
        n = np.array(ns, F32)
        dd = np.full(n.shape, d, F32)
        assert in_regime(n).all()
        assert np.array_equal(unit_quotients(n, dd), by_division(n, dd)), (d, n[unit_quotients(n, dd) != by_division(n, dd)])
    # the quotients that round down to 1.0 are n = delta alone: the float above |delta| already
    # gives 1 + 2^-23 / m > the tie 1 + 2^-24
    for d in ds:
        up = _steps(d, 1)
        with np.errstate(all="ignore"):
            assert up / d > F32(1) and d / d == F32(1)


def test_outside_the_regime_the_division_decides():
    tiny = [F32(0.0), F32(-0.0), F32(2.0 ** -149), F32(-(2.0 ** -149)), F32(-(2.0 ** -140)), F32(2.0 ** -126),
            F32(-(2.0 ** -126)), _steps(REGIME_N, -1), -_steps(REGIME_N, -1), F32(np.nan)]
    wrong = 0
    for d in (F32(D_HI), F32(-D_HI), F32(D_LO), F32(-D_LO), F32(2.0), F32(-3.5)):
        n = np.array(tiny, F32)
        dd = np.full(n.shape, d, F32)
        assert not in_regime(n).any()
        assert np.array_equal(decide(n, dd), by_division(n, dd))
        wrong += int((unit_quotients(n, dd) != by_division(n, dd)).sum())
    # -0 / delta and a negative quotient that underflows are -0, which 0 <= q accepts: the
    # predicate alone would reject them, so the guard is not idle
    assert wrong > 0
    assert by_division(F32(-0.0), F32(1.0)) and not unit_quotients(F32(-0.0), F32(1.0))
    assert by_division(F32(-(2.0 ** -149)), F32(D_HI)) and not unit_quotients(F32(-(2.0 ** -149)), F32(D_HI))
    # and mixed: the whole decision equals the division on everything at once
    rng = np.random.default_rng(7)
    n = np.concatenate([_log_uniform(rng, 2.0 ** -149, 2.0 ** -90, 200_000), np.zeros(8, F32), -np.zeros(8, F32)])
    d = _log_uniform(rng, D_LO, D_HI, n.size)
    assert np.array_equal(decide(n, d), by_division(n, d))


# ---- planes: exact float32 steps from rational arithmetic ---------------------------------------

def rn32(x):
    """Fraction -> the nearest float32 (ties to even), as a Python float holding it exactly."""
    if x == 0:
        return 0.0
    s = -1.0 if x < 0 else 1.0
    x = abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    elif Fraction(2) ** (e + 1) <= x:
        e += 1
    e = max(e, -126)
    q = x / Fraction(2) ** (e - 23)
    m = q.numerator // q.denominator
    rem = q - m
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (m & 1)):
        m += 1
    return s * float(m) * 2.0 ** (e - 23)


def mul(a, b):
    return rn32(Fraction(a) * Fraction(b))


def sub(a, b):
    return rn32(Fraction(a) - Fraction(b))


def fma(a, b, c):
    return rn32(Fraction(a) * Fraction(b) + Fraction(c))


def rcp_est(x):
    """An odd reciprocal estimate a few float32 steps off 1/x (the hardware's is within 1 ulp)."""
    k = (int(abs(x) * 2.0 ** 40) % 5) - 2
    return rn32(Fraction(1) / Fraction(x) * (1 + Fraction(k, 2 ** 23)))


def rcp_nr(den):
    r0 = rcp_est(den)
    return fma(fma(-den, r0, 1.0), r0, r0)


def div_nr(num, den, r):
    q0 = mul(num, r)
    q1 = fma(fma(-den, q0, num), r, q0)
    return fma(fma(-den, q1, num), r, q1)


def test_rn32_matches_numpy():
    rng = np.random.default_rng(3)
    for a, b in rng.standard_normal((2000, 2)).astype(F32) * F32(37.0):
        assert mul(float(a), float(b)) == float(a * b)
        assert sub(float(a), float(b)) == float(a - b)
    assert rn32(Fraction(1) + Fraction(1, 2 ** 24)) == 1.0                       # a tie goes to even
    assert rn32(Fraction(1) + Fraction(3, 2 ** 24)) == 1.0 + 2.0 ** -22
    assert rn32(Fraction(1, 2 ** 149)) == 2.0 ** -149 and rn32(Fraction(1, 2 ** 151)) == 0.0


def test_opposite_face_plane_from_the_shared_reciprocal():
    rng = np.random.default_rng(11)
    f = lambda v: float(F32(v))   # noqa: E731
    n = 0
    for _ in range(3000):
        s = f(rng.choice([-1.0, 1.0]) * rng.choice([1.0, rng.uniform(0.1, 4.0)]))
        dk = f(rng.choice([-1.0, 1.0]) * np.exp2(rng.uniform(-20, 2)))
        ok = f(rng.uniform(-600, 600))
        q = f(rng.uniform(-600, 600))
        # today's opposite face: its own normal component -s, denominator, numerator and reciprocal
        den_o = mul(-s, dk)
        t_old = div_nr(sub(mul(-s, q), mul(-s, ok)), den_o, rcp_nr(den_o))
        # box_test_compact_q: the axis' denominator s d_k, its reciprocal and s o_k, shared
        den = mul(s, dk)
        t_new = div_nr(sub(mul(s, q), mul(s, ok)), den, rcp_nr(den))
        assert den_o == -den and abs(den) >= 1e-8
        assert t_old == t_new, (s, dk, ok, q, t_old, t_new)
        n += t_new != 0.0
    assert n > 2900

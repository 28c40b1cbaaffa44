"""detmath (the elementary-function library shared by the HIP kernels and the
oracle) against the host libm (glibc) and scipy."""
import numpy as np
import pytest

from tests import oracle_lib


def _ulps(a, b):
    a, b = np.asarray(a), np.asarray(b)
    sp = np.spacing(np.abs(b))
    return np.abs(a - b) / sp


@pytest.fixture(scope="module")
def libs():
    return oracle_lib.load("detmath"), oracle_lib.load("libm")


def _vec(f, *xs):
    return np.array([f(*v) for v in zip(*xs)])


def test_exp_log_pow_within_one_ulp_of_glibc(libs):
    dm, lm = libs
    rng = np.random.default_rng(7)
    x = rng.uniform(-745.0, 709.7, 20000)
    a, b = _vec(dm.oracle_exp, x), _vec(lm.oracle_exp, x)
    ok = b > 0
    assert _ulps(a[ok], b[ok]).max() <= 1.0
    y = np.exp(rng.uniform(-700, 700, 20000))
    assert _ulps(_vec(dm.oracle_log, y), _vec(lm.oracle_log, y)).max() <= 1.0
    px = np.exp(rng.uniform(-5, 6, 20000))
    py = rng.uniform(-20, 20, 20000)
    a, b = _vec(dm.oracle_pow, px, py), _vec(lm.oracle_pow, px, py)
    ok = np.isfinite(b) & (b > 0)
    assert _ulps(a[ok], b[ok]).max() <= 2.0
    # the exponents the method stacks use
    for xx, yy in ((273.15, 4.0), (2.0, -1.0 / 24 / 5.0), (0.85, 8.0), (0.3, 0.0687), (1.7, -1.0 / 3.0), (0.2, -0.2)):
        assert _ulps(dm.oracle_pow(xx, yy), lm.oracle_pow(xx, yy)) <= 1.0


def test_special_values(libs):
    dm, _ = libs
    assert dm.oracle_exp(0.0) == 1.0
    assert dm.oracle_log(1.0) == 0.0
    assert dm.oracle_exp(1000.0) == float("inf")
    assert dm.oracle_exp(-1000.0) == 0.0
    assert np.isnan(dm.oracle_log(-1.0))
    assert dm.oracle_log(0.0) == float("-inf")
    assert dm.oracle_pow(2.0, 0.0) == 1.0
    assert dm.oracle_pow(-2.0, 3.0) == -8.0
    assert np.isnan(dm.oracle_pow(-2.0, 0.5))
    assert dm.oracle_pow(0.0, -1.0) == float("inf")
    inf = float("inf")
    assert dm.oracle_exp(inf) == inf
    assert dm.oracle_exp(-inf) == 0.0 and not np.signbit(dm.oracle_exp(-inf))
    assert np.isnan(dm.oracle_exp(float("nan")))
    assert dm.oracle_log(inf) == inf
    assert np.isnan(dm.oracle_log(-inf))
    assert np.isnan(dm.oracle_log(float("nan")))
    assert dm.oracle_log(-0.0) == -inf


def _err_in_ulps(mp, got, true):
    """|got - true| in units of the last place of the true value (2^-1074 in the subnormal range); an infinite
    `got` counts as 2^1024, the value it rounds from."""
    if got != got:
        return float("inf"), False
    e = int(mp.floor(mp.log(abs(true), 2)))
    unit = mp.ldexp(1, max(e - 52, -1074))
    g = mp.mpf(got) if abs(got) != float("inf") else mp.ldexp(1 if got > 0 else -1, 1024)
    return float(abs(g - true) / unit), e < -1022


def test_edges_against_mpmath(libs):
    """detmath at the arguments where its branches change (tests/edge_sets.py) against mpmath at 200 bits, with the
    bounds detmath states for itself (detmath/detmath.h:8-9,131): exp and log within 1 ulp of the true value (1 unit of
    2^-1074 on subnormal results), pow within 2 ulp, lgamma within 4e-15 max(|lgamma|, 1). Where the true value is
    0, infinite, not a number or beyond the double range, detmath returns exactly that.
    Measured on these sets: log 0.763 ulp, exp 0.775 ulp (0.73 unit subnormal), pow 1.28 ulp (0.90 unit subnormal),
    lgamma 3.3e-15."""
    mpmath = pytest.importorskip("mpmath")
    from tests import edge_sets
    dm, _ = libs
    mp = mpmath.mp
    mp.prec = 200
    inf = float("inf")
    big = mp.ldexp(1, 1024)

    def check(name, args, got, true, bound, bound_sub):
        # true: an mpf, or a float for the exact cases (0, +-inf, nan, or an exactly representable value)
        if isinstance(true, float):
            assert (got != got) if true != true else (got == true), (name, args, got, true)
            return 0.0, 0.0
        if abs(true) >= big:
            assert got == (inf if true > 0 else -inf), (name, args, got)
            return 0.0, 0.0
        err, sub = _err_in_ulps(mp, got, true)
        assert err <= (bound_sub if sub else bound), (name, args, got, err)
        return (0.0, err) if sub else (err, 0.0)

    worst = {}

    def note(name, e):
        w = worst.setdefault(name, [0.0, 0.0])
        w[0], w[1] = max(w[0], e[0]), max(w[1], e[1])

    for x in edge_sets.exp_set():
        x = float(x)
        true = x if x != x else inf if x == inf else 0.0 if x == -inf else 1.0 if x == 0.0 else mp.exp(mp.mpf(x))
        note("exp", check("exp", x, dm.oracle_exp(x), true, 1.0, 1.0))
    for x in edge_sets.log_set():
        x = float(x)
        true = (x if x != x else float("nan") if x < 0 else -inf if x == 0.0 else inf if x == inf else
                0.0 if x == 1.0 else mp.log(mp.mpf(x)))
        note("log", check("log", x, dm.oracle_log(x), true, 1.0, 1.0))
    for x, y in zip(*edge_sets.pow_set()):
        x, y = float(x), float(y)
        if y == 0.0 or x == 1.0:
            true = 1.0
        elif x == 0.0:
            true = 0.0 if y > 0 else inf
        else:
            true = mp.power(mp.mpf(x), mp.mpf(y))
        note("pow", check("pow", (x, y), dm.oracle_pow(x, y), true, 2.0, 2.0))
    worst_lg = 0.0
    for x in edge_sets.lgamma_set():
        x = float(x)
        got, true = dm.oracle_lgamma_fn(x), mp.loggamma(mp.mpf(x))
        err = float(abs(mp.mpf(got) - true) / max(abs(true), 1))
        assert err <= 4e-15, ("lgamma", x, got, err)
        worst_lg = max(worst_lg, err)
    print(f"worst: exp {worst['exp']} log {worst['log']} pow {worst['pow']} (ulp normal, units subnormal); "
          f"lgamma {worst_lg:.3g}")


def test_gamma_pq_rescale_counter(libs):
    """oracle_gamma_pq_rescaled counts detmath's 2^-200 rescales. At gamma_snow's policy eps a rescale needs a shape
    near 1000: the series at a = 1000, x = 0.9 (a + 1) and the continued fraction at a = 4000, x = a + 1 rescale (a
    plain Python replay of the series agrees), no shape of the recorded January jobs (a in [0.1, 6.25]) does."""
    import ctypes as C
    dm, _ = libs
    dm.oracle_gamma_pq_rescaled.restype = C.c_int
    dm.oracle_gamma_pq_rescaled.argtypes = [C.c_double] * 3
    eps = 2.0 ** -18

    def series_replay(a, x):  # E and the rescale depend on the shape alone; the exit test on B to a few ulp
        ap, E, B, xn, count = a, 1.0, 0.0, 1.0, 0
        for _ in range(2000):
            ap += 1.0
            xn *= x
            E *= ap
            B = B * ap + xn
            if xn < eps * (B + E):
                break
            if E > 1e200:
                E *= 2.0 ** -200
                B *= 2.0 ** -200
                xn *= 2.0 ** -200
                count += 1
        return count

    n_series = dm.oracle_gamma_pq_rescaled(1000.0, 0.9 * 1001.0, eps)
    assert n_series > 0 and n_series == series_replay(1000.0, 0.9 * 1001.0)
    assert dm.oracle_gamma_pq_rescaled(4000.0, 4001.0, eps) > 0
    rng = np.random.default_rng(5)
    for a in rng.uniform(0.1, 6.25, 500):
        for m in (0.01, 0.5, 0.999, 1.0, 1.5, 3.0, 20.0):
            assert dm.oracle_gamma_pq_rescaled(a, (a + 1.0) * m, 2.0 ** -35 if a < 2 else eps) == 0
    for a, x in ((2.0, 0.0), (2.0, -1.0), (2.0, float("inf")), (2.0, float("nan"))):
        assert dm.oracle_gamma_pq_rescaled(a, x, eps) == 0


def test_lgamma_against_scipy(libs):
    sp = pytest.importorskip("scipy.special")
    dm, _ = libs
    x = np.concatenate([np.exp(np.linspace(np.log(1e-6), np.log(1e3), 4000)), [0.5, 1.0, 1.26, 2.0, 6.25, 7.25]])
    a = _vec(dm.oracle_lgamma_fn, x)
    b = sp.gammaln(x)
    assert (np.abs(a - b) / np.maximum(np.abs(b), 1.0)).max() < 5e-15


def test_gamma_pq_against_scipy(libs):
    import ctypes as C
    sp = pytest.importorskip("scipy.special")
    dm, _ = libs
    rng = np.random.default_rng(11)
    a = np.exp(rng.uniform(np.log(0.05), np.log(300.0), 6000))
    x = a * rng.uniform(0.0, 3.0, a.size)
    x[:50] = a[:50] + 1.0  # branch boundary
    p, p1, pre = C.c_double(), C.c_double(), C.c_double()
    worst = 0.0
    for ai, xi in zip(a, x):
        dm.oracle_gamma_pq(ai, xi, C.byref(p), C.byref(p1), C.byref(pre))
        for got, want in ((p.value, sp.gammainc(ai, xi)), (p1.value, sp.gammainc(ai + 1, xi))):
            err = abs(got - want) / max(abs(want), 1e-300)
            # relative 1e-12, or absolute 1e-14 where P is tiny / its complement dominates
            worst = max(worst, min(err, abs(got - want) / 1e-2))
            assert err < 1e-12 or abs(got - want) < 1e-14, (ai, xi, got, want)

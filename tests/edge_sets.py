"""Input sets for the elementary-function edge tests: the arguments at which exp / log / pow / lgamma change branch
(detmath/detmath.h) or at which the device restatements hand over to the general functions (device/fastmath.h,
device/special.h). Shared by tests/test_detmath.py (detmath against a 200-bit reference, CPU) and
tests/test_device_functions.py (the device code against detmath, GPU). Fixed lists and seeded generators only."""
import struct

import numpy as np

LN2 = 0.6931471805599453
MIN_NORMAL = 2.2250738585072014e-308
MAX_DOUBLE = 1.7976931348623157e308
INF = float("inf")
NAN = float("nan")


def neighbours(x, k=1):
    """x and its k nearest doubles on each side, ascending."""
    out = [float(x)]
    lo = hi = float(x)
    for _ in range(k):
        lo = float(np.nextafter(lo, -INF))
        hi = float(np.nextafter(hi, INF))
        out = [lo] + out + [hi]
    return out


def from_words(hi, lo):
    return struct.unpack("<d", struct.pack("<II", lo & 0xffffffff, hi & 0xffffffff))[0]


def exp_set():
    rng = np.random.default_rng(101)
    v = list(rng.uniform(-745.2, 709.8, 4000))
    v += neighbours(708.0, 2) + neighbours(-708.0, 2)  # the fast path's hand-over to exp_general
    v += [709.782712893384, -745.1332191019411, -745.2, 0.0, -0.0, 1e-300, -1e-300, 5e-324, INF, -INF, NAN, 1000.0, -1000.0]
    for k in range(-1075, 1025, 25):  # the reduction's rounding boundary k + 1/2
        v += neighbours((k + 0.5) * LN2, 1)
    j = rng.integers(0, 61, 2000)
    v += list(rng.choice([-1.0, 1.0], 2000) * rng.uniform(0.0, 1.0, 2000) * np.ldexp(1.0, -j))
    return np.array(v, dtype=np.float64)


def log_set():
    rng = np.random.default_rng(102)
    v = []
    for k in range(1, 53):  # 1 +- 2^-k and the next double away from 1
        up, dn = 1.0 + 2.0 ** -k, 1.0 - 2.0 ** -k
        v += [up, float(np.nextafter(up, INF)), dn, float(np.nextafter(dn, -INF))]
    v += list(rng.uniform(0.5, 2.0, 4000))
    for c in (1.0, 0.5, 2.0, 1.4142135623730951, 0.7071067811865476):
        v += neighbours(c, 4)
    # log_core's branch constants in the high word: the near-1 split (0x6147a, 0x6b851) and sqrt(2) (0x6a09e / 0x6a09f)
    for e in (0x3fe, 0x3ff, 0x400):
        for m in (0x6147a, 0x6b851, 0x6a09e, 0x6a09f):
            for d in (-1, 0, 1):
                for lo in (0, 0xffffffff):
                    v.append(from_words((e << 20) | (m + d), lo))
    v += neighbours(MIN_NORMAL, 1) + [5e-324, 1e-310, MAX_DOUBLE]
    v += [from_words(0, 0) + from_words(int(h), int(l)) for h, l in
          zip(rng.integers(0, 1 << 20, 50), rng.integers(0, 1 << 32, 50))]  # subnormals
    v += [0.0, -0.0, -1.0, INF, NAN]
    v += list(np.exp(rng.uniform(-700.0, 700.0, 2000)))
    return np.array(v, dtype=np.float64)


# the exponents the method stacks use (tests/test_detmath.py)
PHYSICS_POW = ((273.15, 4.0), (2.0, -1.0 / 24 / 5.0), (0.85, 8.0), (0.3, 0.0687), (1.7, -1.0 / 3.0), (0.2, -0.2))
POWR_Y = (0.0, 0.2, -0.2, -1.0 / 3.0, 0.0687)


def powr_x():
    return [0.0, MIN_NORMAL, 1.0] + neighbours(1.0, 2) + [1.0 - 2.0 ** -20, 1.0 + 2.0 ** -20, 0.999, 1.001]


def pow_set(with_powr_grid=True):
    """(x, y): the random set of the parity test, x near 1 with large |y|, the physics pairs, and (with_powr_grid)
    powr's grid with x = 0, the smallest normal and 1."""
    rng = np.random.default_rng(103)
    x = list(np.exp(rng.uniform(-5.0, 6.0, 4000)))
    y = list(rng.uniform(-20.0, 20.0, 4000))
    j = rng.integers(1, 40, 2000)
    x += list(1.0 + rng.choice([-1.0, 1.0], 2000) * rng.uniform(0.0, 1.0, 2000) * np.ldexp(1.0, -j))
    y += list(rng.uniform(-1e6, 1e6, 2000))
    for a, b in PHYSICS_POW:
        x.append(a)
        y.append(b)
    if with_powr_grid:
        for a in powr_x():
            for b in POWR_Y:
                x.append(a)
                y.append(b)
    return np.array(x, dtype=np.float64), np.array(y, dtype=np.float64)


def lgamma_set():
    v = list(np.exp(np.linspace(np.log(1e-6), np.log(1e3), 3000)))
    for c in (1.0, 2.0, 10.0, 1.4616321449683623):  # the zeros, the recurrence / Stirling hand-over, the minimum
        v += neighbours(c, 2)
    return np.array(v, dtype=np.float64)

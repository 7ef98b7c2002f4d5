"""The glossy lobe's power for an integer shininess, restated operation by operation in exact rational arithmetic.

drt_pow_shininess (csrc/drt_device.h) raises x in [0, 1] to an integer 0 <= n < 1024 by repeated squaring on double-double pairs:
the result (rh, rl) starts at (1, 0), the base (bh, bl) at (x, 0); for every bit of n from the lowest up, a set bit multiplies the
result by the base, and while bits remain above it the base is squared; the value is rh + rl. Each pair operation is six or seven
IEEE operations (a product, FMAs, sums), each rounded to nearest, ties to even. Here every one of them is formed exactly as a
Fraction and rounded once by float(Fraction): CPython's int / int true division rounds correctly, subnormals included, so each
step gives the bits an IEEE FMA unit gives -- no double rounding, whatever the platform's libm or FMA support.

Zeros. A Fraction has no -0. That changes nothing here:
  * no non-zero value depends on the sign of a zero operand, and the sums and FMAs of non-zero exact results are exact in the model;
  * the result is never -0. A sum is -0 only if both terms are -0, and a product p = rh * bh or bh * bh of two values that are not
    negative-signed is not -0; by induction rh and bh are never -0 (each is p + e with such a p), and rh + rl with rh not -0 is +0
    whenever it is zero. For x = -0 itself the first product gives p = -0, e = fma(1, -0, +0) = +0, and rh = p + e = +0: the device
    returns +0 for every n >= 1 (IEEE's pow gives -0 for odd n; tests/test_gpu_parity.py pins the +0), and 1 for n = 0.
So float(Fraction(0)) = +0.0 is the device's zero everywhere.

Pairs that drt_pow_shininess hands to the general pow() -- a non-integer exponent, one outside [0, 1024), a base outside [0, 1] or
a NaN -- are not this rule's business: on_integer_path says which pairs are.
"""
from fractions import Fraction


def on_integer_path(x, y):
    """drt_pow_shininess's guard: the pair goes through the double-double loop (True) or to pow() (False)"""
    return bool(0.0 <= y < 1024.0 and float(int(y)) == y and 0.0 <= x <= 1.0)


def _mul(a, b):
    return float(Fraction(a) * Fraction(b))


def _add(a, b):
    return float(Fraction(a) + Fraction(b))


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def dd_mul(rh, rl, bh, bl):
    """(rh + rl) * (bh + bl), the device's operations in the device's order"""
    p = _mul(rh, bh)
    e = _fma(rh, bh, -p)
    e = _fma(rh, bl, e)
    e = _fma(rl, bh, e)
    hi = _add(p, e)
    lo = _add(e, -_add(hi, -p))
    return hi, lo


def dd_sqr(bh, bl):
    """(bh + bl)^2"""
    p = _mul(bh, bh)
    e = _fma(bh, bh, -p)
    e = _fma(_add(bh, bh), bl, e)
    hi = _add(p, e)
    lo = _add(e, -_add(hi, -p))
    return hi, lo


def glossy_power(x, n):
    """x^n as drt_pow_shininess computes it, for a pair on the integer path"""
    x, n = float(x), int(n)
    assert on_integer_path(x, float(n)), (x, n)
    rh, rl, bh, bl = 1.0, 0.0, x, 0.0
    k = n
    while k != 0:
        if k & 1:
            rh, rl = dd_mul(rh, rl, bh, bl)
        if k > 1:
            bh, bl = dd_sqr(bh, bl)
        k >>= 1
    return _add(rh, rl)


def nearest_power(x, n):
    """x^n rounded once to the nearest double, from exact arithmetic (a zero comes out as +0)"""
    return float(Fraction(float(x)) ** int(n))

"""High-precision reference for bivariate-normal rectangle masses (mpmath).

TEST INFRASTRUCTURE ONLY.  Shares nothing with oracle/model.py or the library: no Gauss-Legendre
rule, no correlation classes, no second branch -- one integral, evaluated by adaptive tanh-sinh
quadrature at DPS digits:

    P(X > h, Y > k) = Phi(-h) Phi(-k)
                      + 1/(2 pi) int_0^{asin r} exp(-(h^2 + k^2 - 2 h k sin t) / (2 cos^2 t)) dt

(Plackett's identity dP/dr = density at (h, k), with r = sin t.)  Towards |r| = 1 the integrand
varies on the scale of cos t, so the interval is cut at points that halve the distance to pi/2.

Every input is taken as the exact value of the float64 it is given as; edges of cells are formed
exactly ((i - 1/2) cell), not in float64.
"""
import mpmath
from mpmath import mp, mpf

DPS = 34
CDF_EPS = mpf(1) / 1000          # the support rule's 1e-3, exact


def _phi(z):
    """standard normal cdf"""
    return mpmath.erfc(-z / mpmath.sqrt(2)) / 2


def bvu_mp(h, k, r):
    """P(X > h, Y > k) for the standard bivariate normal with correlation r, |r| < 1."""
    with mp.workdps(DPS):
        h, k, r = mpf(h), mpf(k), mpf(r)
        assert abs(r) < 1
        prod = _phi(-h) * _phi(-k)
        if r == 0:
            return prod
        a = mpmath.asin(abs(r))
        sgn = 1 if r > 0 else -1
        # with s = sin|t| and k' = sgn k:  h^2 + k^2 - 2 h k sin t = (h - k')^2 + 2 h k' (1 - s)
        d2 = (h - k * sgn) ** 2
        hk2 = 2 * h * k * sgn

        def f(t):                        # t = |theta|
            s = mpmath.sin(t)
            c = mpmath.cos(t)
            return mpmath.exp(-(d2 + hk2 * (1 - s)) / (2 * c * c))

        half_pi = mp.pi / 2
        pts = [mpf(0)]
        gap = half_pi / 2
        while half_pi - gap < a:         # cut points halving the distance to pi/2
            pts.append(half_pi - gap)
            gap = gap / 2
        pts.append(a)
        return prod + sgn * mpmath.quad(f, pts) / (2 * mp.pi)


def rect_mp(xl, xu, yl, yu, mu, sx, sy, rho, cache=None):
    """Mass of N(mu, S) on [xl, xu] x [yl, yu], S = [[sx^2, rho sx sy], [rho sx sy, sy^2]]: the limits
    standardised by the marginal standard deviations, then the four-corner difference
    bvu(l0, l1) - bvu(u0, l1) - bvu(l0, u1) + bvu(u0, u1), as mvnun forms it.  `cache`: a dict that
    keeps corner values between calls (neighbouring cells share corners)."""
    with mp.workdps(DPS):
        sx, sy, rho = mpf(sx), mpf(sy), mpf(rho)
        l0 = (mpf(xl) - mpf(mu[0])) / sx
        u0 = (mpf(xu) - mpf(mu[0])) / sx
        l1 = (mpf(yl) - mpf(mu[1])) / sy
        u1 = (mpf(yu) - mpf(mu[1])) / sy

        def corner(a, b):
            if cache is None:
                return bvu_mp(a, b, rho)
            key = (a, b)
            if key not in cache:
                cache[key] = bvu_mp(a, b, rho)
            return cache[key]

        return corner(l0, l1) - corner(u0, l1) - corner(l0, u1) + corner(u0, u1)


def square_deficit_mp(h, cell, mu, sx, sy, rho):
    """1 - P(square of half width (h + 1/2) cell around the origin)"""
    with mp.workdps(DPS):
        e = (mpf(h) + mpf(1) / 2) * mpf(cell)
        return 1 - rect_mp(-e, e, -e, e, mu, sx, sy, rho)


def support_mp(cell, mu, sx, sy, rho, hmax=64):
    """The square rule: smallest h with 1 - P(square of half width (h + 1/2) cell) < 1e-3.
    Returns (H, margin): margin = min |deficit - 1e-3| over h in {H - 1, H}."""
    with mp.workdps(DPS):
        prev = None
        for h in range(hmax + 1):
            d = square_deficit_mp(h, cell, mu, sx, sy, rho)
            if d < CDF_EPS:
                margin = abs(d - CDF_EPS)
                if prev is not None:
                    margin = min(margin, abs(prev - CDF_EPS))
                return h, margin
            prev = d
        raise ValueError('no support within %d cells' % hmax)


def stamp_mp(cell, mu, sx, sy, rho):
    """(H, masses, margin): the support half width of the square rule, the (2H+1)^2 cell masses in the
    orientation of get_mvn_cdf_values (row 0 is the largest y, column 0 the smallest x; cell (ii, jj)
    is [(ii - 1/2) cell, (ii + 1/2) cell] x [(jj - 1/2) cell, (jj + 1/2) cell]) as mpf, and the
    distance of the support decision from its threshold."""
    with mp.workdps(DPS):
        H, margin = support_mp(cell, mu, sx, sy, rho)
        c = mpf(cell)
        half = mpf(1) / 2
        cache = {}
        rows = []
        for jj in range(H, -H - 1, -1):
            row = []
            for ii in range(-H, H + 1):
                row.append(rect_mp((ii - half) * c, (ii + half) * c, (jj - half) * c, (jj + half) * c,
                                   mu, sx, sy, rho, cache))
            rows.append(row)
        return H, rows, margin

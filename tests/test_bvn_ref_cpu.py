"""The high-precision rectangle-mass reference (tests/bvn_ref.py, mpmath) against closed forms, the
committed fixture G10 against its generator, and the oracle's BVU restatement (oracle/model.py)
against G10 at every correlation class -- the prob_mass tests of tests/test_model_corr_gpu.py lean on
the oracle, this file pins the oracle to something exact."""
import numpy as np
from mpmath import mp, mpf
import mpmath

import bvn_ref
from oracle import model as OM

# worst |oracle - mpmath| over the 5797 cell masses of G10, measured (see the test's docstring)
ORACLE_WORST = 6.73e-16


def _phi(z):
    return mpmath.erfc(-mpf(z) / mpmath.sqrt(2)) / 2


def stamps(g):
    """(k, inputs, H, masses[2H+1, 2H+1]) of every case of G10"""
    for k in range(len(g['H'])):
        H = int(g['H'][k])
        m = g['masses'][int(g['offsets'][k]):int(g['offsets'][k + 1])].reshape(2 * H + 1, 2 * H + 1)
        yield k, g['inputs'][k], H, m


def test_reference_against_closed_forms():
    '''rho = 0: a product of Phi differences; h = k = 0: 1/4 + asin(rho)/2pi; (h, k) <-> (k, h);
    bvu(h, k, rho) + bvu(h, -k, -rho) = Phi(-h) -- to 1e-28 with the reference at 34 digits'''
    tol = mpf(10) ** -28
    with mp.workdps(bvn_ref.DPS):
        # rho = 0, a rectangle of N(mu, diag): product of the two marginal masses
        mu, sx, sy = (0.3, -1.1), 1.7, 0.6
        got = bvn_ref.rect_mp(-1.0, 2.5, -2.0, 0.25, mu, sx, sy, 0.0)
        want = ((_phi((mpf(2.5) - mpf(mu[0])) / mpf(sx)) - _phi((mpf(-1.0) - mpf(mu[0])) / mpf(sx))) *
                (_phi((mpf(0.25) - mpf(mu[1])) / mpf(sy)) - _phi((mpf(-2.0) - mpf(mu[1])) / mpf(sy))))
        assert abs(got - want) < tol
        for r in (0.2999, -0.3, 0.75, -0.9249, 0.925, -0.99, 0.999, -0.999):
            assert abs(bvn_ref.bvu_mp(0.0, 0.0, r) - (mpf(1) / 4 + mpmath.asin(mpf(r)) / (2 * mp.pi))) < tol
            for h, k in ((0.4, -1.3), (1.5, 1.45), (-2.0, 0.7)):
                v = bvn_ref.bvu_mp(h, k, r)
                assert abs(v - bvn_ref.bvu_mp(k, h, r)) < tol
                assert abs(v + bvn_ref.bvu_mp(h, -k, -r) - _phi(-mpf(h))) < tol
                assert 0 <= v <= min(_phi(-mpf(h)), _phi(-mpf(k))) + tol


def test_fixture_regenerates(golden):
    '''a random tenth of G10's stamps recomputed from bvn_ref: same H, same margin, masses equal to the
    file's float64 bit for bit; the generator's case list is the file's'''
    import importlib.util
    import os
    g = golden('g10_bvn_mp')
    spec = importlib.util.spec_from_file_location(
        'make_bvn_mp', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'make_bvn_mp.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    cs = gen.cases()
    assert len(cs) == len(g['H']) == 85 and int(g['dps']) == bvn_ref.DPS
    assert np.array_equal(np.array([c for _, c in cs]), g['inputs'])
    assert np.array_equal(np.array([ki for ki, _ in cs]), g['kind'])
    assert g['margin'].min() >= gen.MIN_MARGIN and g['H'].max() <= gen.MAX_H
    pick = set(np.random.default_rng(20261).choice(len(cs), size=(len(cs) + 9) // 10, replace=False).tolist())
    for k, c, H, m in stamps(g):
        if k not in pick:
            continue
        H2, m2, margin = gen.one(cs[k])
        assert H2 == H and margin == float(g['margin'][k])
        assert np.array_equal(m2, m), k


def test_oracle_against_mpmath(golden):
    '''oracle.model.get_mvn_cdf_values on all 85 stamps of G10 (17 correlations: 0, both sides of the
    0.3 / 0.75 / 0.925 class boundaries, 0.99, 0.999, both signs; 5 stamp shapes each): the same support
    half width H, and every cell mass within twice the measured worst distance.

    Measured (5797 cell masses): worst |oracle - mpmath| = 6.73e-16, by class 6.73e-16 (|rho| < 0.3),
    3.91e-16 (< 0.75), 4.39e-16 (< 0.925), 2.36e-16 (>= 0.925).  The largest figure is at |rho| = 0.2999, in the
    'fine' stamps: the three node pairs of BVU's smallest Gauss-Legendre rule stretched furthest before the
    next rule takes over.  At rho = 0 (the quadrature term vanishes) and in the second branch the distance
    is the 1 to 2e-16 round-off of a difference of O(1) corner values.  The bound asserted is 2 x 6.73e-16.'''
    g = golden('g10_bvn_mp')
    worst = {}
    for k, c, H, m in stamps(g):
        got = OM.get_mvn_cdf_values(c[0], np.array(c[1:3]), OM.Dmat(*c[3:6]))
        assert got.shape == m.shape, (k, c, got.shape, m.shape)
        cls = min(b for b in (0.3, 0.75, 0.925, 1.0) if abs(c[5]) < b)
        worst[cls] = max(worst.get(cls, 0.0), float(np.abs(got - m).max()))
    for cls in sorted(worst):
        print('|rho| < %-5g worst |oracle - mpmath| = %.3g' % (cls, worst[cls]))
    assert max(worst.values()) <= 2 * ORACLE_WORST

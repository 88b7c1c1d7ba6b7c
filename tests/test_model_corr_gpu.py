"""The day-kernel construction over the whole correlation range, every kernel instance.

The device picks its arithmetic by the diffusion correlation (ps_model.hip: make_rule, launch_pair_masses):
|rho| < 0.3 three Gauss-Legendre node pairs (k_pair_masses<false, 3>), [0.3, 0.75) six and [0.75, 0.925) ten
(<false, 0>), >= 0.925 Genz's second branch (<true, 0>) -- once for the in-flow and once for the
out-of-flow covariance.  tests/test_model_gpu.py stays below |rho| = 0.7; this file runs the rest:

* stamps (get_mvn_cdf_values) against the high-precision fixture G10 (tests/bvn_ref.py, mpmath), at every
  class and on both sides of every class boundary;
* prob_mass against the oracle (pinned to G10 by tests/test_bvn_ref_cpu.py) through every instance, both
  rules, both signs -- on 48-sample days at R = 40, where a day of the numpy oracle takes half a second
  and the flight stamps (H = 9, 19 cells) straddle the 16-cell tiles and fill corner tables of 17.
"""
import os
import warnings

import numpy as np
import pytest
from scipy import sparse

from oracle import model as OM
from helpers import HP

pytestmark = pytest.mark.gpu

VAL_ATOL = 5e-15            # the project's device bound (test_model_gpu.py)

SIG = (171.82, 144.58)      # in-flow sigmas (the defaults); H = 9 at 62.5 m cells
SIG_L = (70.0, 55.0)        # out-of-flow sigmas wide enough that lrule builds a real stamp (H = 4)
MU_R, NPER, RAD_DIST, R = 0.1, 6, 2500.0, 40
CELL = RAD_DIST / R

# (rho, rho_l): every class, both rules, both signs; the last two are controls in the lower classes
PAIRS = ((0.95, 0.0), (-0.97, 0.93), (0.253, -0.96), (0.8, -0.8), (-0.9249, 0.925), (0.999, -0.999),
         (0.2999, -0.3), (0.75, 0.7499))


@pytest.fixture(scope='module')
def PM():
    from parasitoids_amd import ParasitoidModel
    return ParasitoidModel


@pytest.fixture(scope='module')
def wind48(PM, golden_dir):
    '''the 30-minute samples themselves: 48 periods a day'''
    return PM.get_wind_data(os.path.join(golden_dir, 'data', 'kalbar'), 1, '00:00')


_oracle_cache = {}


def oracle_day(wd, day, rho, rho_l, mu_r=MU_R, start_time=None):
    '''OM.prob_mass with its trace and warning count; computed once per parameter set and shared'''
    key = (day, rho, rho_l, mu_r, start_time)
    if key not in _oracle_cache:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            ref, dbg = OM.prob_mass(day, wd, HP, SIG + (rho,), SIG_L + (rho_l,), mu_r, NPER, RAD_DIST, R,
                                    start_time, return_debug=True)
        _oracle_cache[key] = (ref, dbg, sum(issubclass(x.category, RuntimeWarning) for x in w))
    return _oracle_cache[key]


def rho_class(rho):
    return min(b for b in (0.3, 0.75, 0.925, 1.0) if abs(rho) < b)


def assert_same_kernel(got, ref, msg, tol=VAL_ATOL):
    '''identical shape and COO pattern, values to tol, sum 1'''
    assert got.shape == ref.shape, msg
    a, b = got.tocsr(), ref.tocsr()
    a.sort_indices(); b.sort_indices()
    assert a.nnz == got.nnz == b.nnz, msg            # (no duplicate entries folded by tocsr)
    assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices), msg
    err = float(np.abs(a.data - b.data).max())
    assert err < tol, (msg, err)
    assert abs(got.data.sum() - 1.0) < 1e-12, msg
    return err


def assert_identical(x, y, msg=None):
    assert x.shape == y.shape and x.nnz == y.nnz, msg
    assert np.array_equal(x.row, y.row) and np.array_equal(x.col, y.col) and np.array_equal(x.data, y.data), msg


def fetch_all(m, n):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        return [m.fetch(i) for i in range(n)]


# ------------------------------------------------------------------ stamps against mpmath

def g10_stamps(g):
    for k in range(len(g['H'])):
        H = int(g['H'][k])
        m = g['masses'][int(g['offsets'][k]):int(g['offsets'][k + 1])].reshape(2 * H + 1, 2 * H + 1)
        yield k, g['inputs'][k], str(g['kinds'][int(g['kind'][k])]), H, m


def test_stamps_against_mpmath(PM, golden):
    '''PM.get_mvn_cdf_values on the 85 stamps of G10 (17 correlations x centred / off-centre / anisotropic /
    coarse / fine; every support decision >= 6e-4 from its threshold): the reference's H, every mass within
    VAL_ATOL of the mpmath value.  The oracle's own distance from G10 is 6.7e-16 (test_bvn_ref_cpu.py).'''
    g = golden('g10_bvn_mp')
    worst = {}
    for k, c, kind, H, ref in g10_stamps(g):
        mat = PM.get_mvn_cdf_values(c[0], np.array(c[1:3]), PM.Dmat(*c[3:6]))
        msg = 'case %d rho=%g %s' % (k, c[5], kind)
        assert mat.shape == ref.shape, (msg, mat.shape, ref.shape)
        err = float(np.abs(mat - ref).max())
        cls = rho_class(c[5])
        worst[cls] = max(worst.get(cls, 0.0), err)
        assert err < VAL_ATOL, (msg, err)
    for cls in sorted(worst):
        print('stamps, |rho| < %-5g: worst |device - mpmath| = %.3g' % (cls, worst[cls]))
    assert sorted(worst) == [0.3, 0.75, 0.925, 1.0]


def test_stamp_mass_and_orientation(PM, golden):
    '''each stamp holds all but 1e-3 of the mass; for rho > 0 the two quadrants along the diagonal (upper
    right, lower left) outweigh the other two, for rho < 0 the reverse (true of G10's exact masses too)'''
    g = golden('g10_bvn_mp')
    for k, c, kind, H, ref in g10_stamps(g):
        mat = PM.get_mvn_cdf_values(c[0], np.array(c[1:3]), PM.Dmat(*c[3:6]))
        msg = 'case %d rho=%g %s' % (k, c[5], kind)
        assert mat.shape == ref.shape, msg
        assert 0.999 < mat.sum() < 1, (msg, mat.sum())
        along = mat[:H, H + 1:].sum() + mat[H + 1:, :H].sum()
        across = mat[:H, :H].sum() + mat[H + 1:, H + 1:].sum()
        if c[5] > 0:
            assert along > across, msg
        elif c[5] < 0:
            assert along < across, msg


# ------------------------------------------------------------------ prob_mass through every instance

def check_batch(PM, wd, days, rho, rho_l, mu_r):
    '''one device batch of `days` against the oracle's days: kernels, support half widths, loss, warnings'''
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        res = PM.prob_mass_batch(days, wd, HP, SIG + (rho,), SIG_L + (rho_l,), mu_r, NPER, RAD_DIST, R)
    model = PM._model_for(wd)
    nwarn = 0
    worst = 0.0
    for i, (d, got) in enumerate(zip(days, res)):
        ref, dbg, nw = oracle_day(wd, d, rho, rho_l, mu_r)
        msg = 'rho=%g rho_l=%g mu_r=%g day %d' % (rho, rho_l, mu_r, d)
        worst = max(worst, assert_same_kernel(got, ref, msg))
        mine = model.debug(i)
        assert list(mine['H']) == dbg['H'], msg
        print('%s: loss %.17g (oracle %.17g) pmfsum %.6g' % (msg, mine['loss'], dbg['loss'], mine['pmfsum']))
        assert abs(mine['loss'] - dbg['loss']) < 1e-15, (msg, mine['loss'], dbg['loss'])
        assert abs(mine['pmfsum'] - dbg['pmfsum']) < 1e-13, msg
        assert int(model.last['warned'][i]) == nw, msg
        nwarn += nw
    assert sum(issubclass(x.category, RuntimeWarning) for x in w) == nwarn
    return worst


@pytest.mark.parametrize('rho,rho_l', PAIRS)
def test_prob_mass_every_class(PM, wind48, rho, rho_l):
    '''Three days in one batch against the oracle: identical shape and COO pattern, values to VAL_ATOL,
    sum 1, the oracle's H per period, loss to 1e-15, the oracle's warnings per day (days[0] is clean,
    days[1] has clipped windows and one period that leaves the domain).  In-flow classes: <true, 0> at
    0.95, -0.97, 0.999; the 10-node rule in <false, 0> at 0.8, -0.9249, 0.75; <false, 3> at 0.253, 0.2999.
    Out-of-flow rule (k_day_prep's support, k_day_local's stamp): second branch at 0.93, -0.96, 0.925,
    -0.999; 10 nodes at -0.8; 6 at -0.3, 0.7499.'''
    wd, days = wind48
    worst = check_batch(PM, wd, days[:3], rho, rho_l, MU_R)
    print('prob_mass rho=%g (|rho| < %g) rho_l=%g: worst |device - oracle| = %.3g' % (rho, rho_class(rho), rho_l, worst))
    assert oracle_day(wd, days[0], rho, rho_l)[2] == 0 and oracle_day(wd, days[1], rho, rho_l)[2] == 1
    assert set(oracle_day(wd, days[0], rho, rho_l)[1]['H']) == {9}     # every window straddles tile borders


def test_prob_mass_clipping_in_the_high_instance(PM, wind48):
    '''rho = 0.99 with four times the advection: a third of the mass leaves (days[0]: loss 0.13; days[1]:
    0.6 % stays), windows clipped at every edge -- the same checks; and one single call with a start time'''
    wd, days = wind48
    check_batch(PM, wd, days[:3], 0.99, 0.0, 0.4)
    assert oracle_day(wd, days[0], 0.99, 0.0, 0.4)[1]['loss'] > 0.1
    assert oracle_day(wd, days[1], 0.99, 0.0, 0.4)[1]['pmfsum'] < 0.01
    ref, dbg, nw = oracle_day(wd, days[1], 0.99, 0.0, 0.4, 0.4)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        got = PM.prob_mass(days[1], wd, HP, SIG + (0.99,), SIG_L + (0.0,), 0.4, NPER, RAD_DIST, R, 0.4)
    assert sum(issubclass(x.category, RuntimeWarning) for x in w) == nw
    assert_same_kernel(got, ref, 'start_time 0.4')
    mine = PM._model_for(wd).debug(0)
    assert [h for h in mine['H'] if h >= 0] == dbg['H'] and len(dbg['H']) == 48 - 19
    assert abs(mine['loss'] - dbg['loss']) < 1e-15


def test_handle_that_crosses_classes(PM, wind48, monkeypatch):
    '''What a chain does: one handle, the correlation wandering through the classes and back.  Every batch
    equals a fresh handle's bit for bit -- the pair-list capacities guessed from the batch before (another
    instance's) and whatever else a handle keeps must not leak; also with PS_PM_SYNC=1 (always exact sizes).'''
    wd, days = wind48
    seq = (0.2, 0.95, 0.5, -0.93, 0.8, 0.2)

    def build(m, rho):
        m.build(days[:3], HP, SIG + (rho,), SIG_L + (-rho,), MU_R, NPER, RAD_DIST, R)
        return fetch_all(m, 3)

    for sync in (None, '1'):
        if sync is None:
            monkeypatch.delenv('PS_PM_SYNC', raising=False)
        else:
            monkeypatch.setenv('PS_PM_SYNC', sync)
        chain = PM.WindModel(wd)
        for step, rho in enumerate(seq):
            got = build(chain, rho)
            fresh = PM.WindModel(wd)
            ref = build(fresh, rho)
            fresh.close()
            for x, y in zip(got, ref):
                assert_identical(x, y, 'PS_PM_SYNC=%s step %d rho=%g' % (sync, step, rho))
        chain.close()


@pytest.mark.parametrize('rho', (0.95, -0.8))
def test_segment_grouping_at_high_correlation(PM, wind48, rho):
    '''test_prob_mass_day_does_not_depend_on_its_batch_beyond_round_off at the classes it never ran:
    PS_PM_SEG = 1 against 8 -- same pattern, |difference| < 1e-15; with PS_PM_SEG = 1 a day alone and the
    same day third in a batch are bit-identical'''
    wd, days = wind48
    out = {}
    for seg in (8, 1):
        m = PM.WindModel(wd)
        m.set_option('PS_PM_SEG', seg)
        m.build(days[:3], HP, SIG + (rho,), SIG_L + (0.0,), MU_R, NPER, RAD_DIST, R)
        out[seg] = fetch_all(m, 3)
        if seg == 1:
            m.build([days[2]], HP, SIG + (rho,), SIG_L + (0.0,), MU_R, NPER, RAD_DIST, R)
            assert_identical(fetch_all(m, 1)[0], out[1][2], 'alone against third in a batch')
        m.close()
    for x, y in zip(out[8], out[1]):
        assert x.shape == y.shape and x.nnz == y.nnz
        assert np.array_equal(x.row, y.row) and np.array_equal(x.col, y.col)
        assert np.abs(x.data - y.data).max() < 1e-15


@pytest.mark.parametrize('rho', (0.95, -0.95))
def test_stamp_and_pair_kernel_agree(PM, rho):
    '''TEST_RUN mode (one wind vector, one period that carries 0.9 of the mass): the oracle agrees to
    VAL_ATOL, and the kernel is what its parts say -- hprob x get_mvn_cdf_values at the same residual mean
    where the flyers land (k_pair_masses<true, 0> against k_mvn_cdf_values), (1 - total) x the out-of-flow
    stamp at the origin, small values removed and the remainder spread (CalcSol.py:112-136) -- within 1e-15'''
    hp = (0.9, 5.0, 6, -4., 2., 19., 2.)
    mu_r = 0.01
    want = np.array([20.3 * CELL, -11.6 * CELL])       # flight stamp (H = 9) clear of the origin's (H = 4)
    w = want / (86400.0 * mu_r)
    wd = {1: np.array([w[0], w[1], np.hypot(w[0], w[1])])}
    Dp, Dl = SIG + (rho,), SIG_L + (-rho,)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        ref = OM.prob_mass(1, wd, hp, Dp, Dl, mu_r, 1, RAD_DIST, R)
        model = PM.WindModel(wd)
        model.build([1], hp, Dp, Dl, mu_r, 1, RAD_DIST, R)
        got = model.fetch(0)
    dbg = model.debug(0)
    assert_same_kernel(got, ref, 'TEST_RUN rho=%g' % rho)
    # the parts, as ParasitoidModel.py:439-499 places them
    mu_v = wd[1][0:2] * (3600 * 24 * (1 / 1)) * mu_r
    cdf_mu = mu_v - np.round(mu_v / CELL) * CELL
    stamp = model.mvn_cdf_values(CELL, cdf_mu, PM.Dmat(*Dp))
    local = model.mvn_cdf_values(CELL, np.zeros(2), PM.Dmat(*Dl))
    model.close()
    H, Hl = stamp.shape[0] // 2, local.shape[0] // 2
    assert list(dbg['H']) == [H] and H == 9 and Hl >= 3
    hprob = float(dbg['hprob'][0])
    assert 0.89 < hprob <= 0.9 and dbg['loss'] == 0.0
    rc, cc = R + int(np.round(-mu_v[1] / CELL)), R + int(np.round(mu_v[0] / CELL))
    assert max(abs(rc - R), abs(cc - R)) > H + Hl           # the two stamps do not overlap
    N = 2 * R + 1
    E = np.zeros((N, N))
    E[rc - H:rc + H + 1, cc - H:cc + H + 1] = hprob * stamp
    total = dbg['pmfsum'] + dbg['loss']
    assert abs(E.sum() - dbg['pmfsum']) < 1e-14
    E[R - Hl:R + Hl + 1, R - Hl:R + Hl + 1] += (1 - total) * local
    keep = (E != 0) & ~(E < 1e-8)
    E = np.where(keep, E + (1 - E[keep].sum()) / keep.sum(), 0.0)
    off = R - got.shape[0] // 2
    G = sparse.coo_matrix((got.data, (got.row + off, got.col + off)), shape=(N, N)).toarray()
    assert np.array_equal(G != 0, keep)
    flyers = (slice(rc - H, rc + H + 1), slice(cc - H, cc + H + 1))
    print('TEST_RUN rho=%g: flyer part |kernel - hprob x stamp| = %.3g, whole kernel %.3g' % (
        rho, np.abs(G[flyers] - E[flyers]).max(), np.abs(G - E).max()))
    assert keep[flyers].sum() > 100
    assert np.abs(G[flyers] - E[flyers]).max() < 1e-15
    assert np.abs(G - E).max() < 1e-15

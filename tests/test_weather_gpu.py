"""GPU tests of the weather ensembles: many sequences of days over one batch of day kernels
(ps_chain_set_kernels_from_model_indexed, PopModel.build_pool / run_sequence), the variance split on the device
(ps_nested_*, predictive.WeatherShare) bit for bit against its numpy replay (weather_ref.NestedReplay), and
posterior_predictive with wind=.  Kalbar wind, R = 64 (N = 129: N*N is odd, the tail cell exists; the launches cover
every pair with a thread of its own, so no size takes another path), 6 days, the members and helpers of
test_sites_gpu.py."""
import copy
import ctypes as C
import json
import os
import types
import warnings

import numpy as np
import pytest

from helpers import HP, DLP, NPER
from test_sites_gpu import MEMBERS, _chain, _csr, _metres, _pop_model
from weather_ref import NestedReplay

pytestmark = pytest.mark.gpu

R, N = 64, 129
DAYS = list(range(6))
EXPO = [0, 2, 5]
PLAN = [(0, 0, 1.0, 0), (-5, 3, 0.5, 0), (7, -4, 0.25, 0)]
RAW = ('imean', 'iM2', 'omean', 'oM2', 'wS')


def _quiet(fn, *args, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        return fn(*args, **kw)


def _sequences(days):
    """the recorded order, a reordering with a repeat, and one that starts on another day"""
    d = list(days)
    return [d, [d[0], d[3], d[3], d[1], d[5], d[2]], [d[4], d[5], d[0], d[0], d[2], d[1]]]


def _pool(pm, member, seqs):
    dp, mu = member
    used = sorted({x for s in seqs for x in s})
    _quiet(pm.build_pool, HP, dp, DLP, mu, NPER, used, [s[0] for s in seqs])


def _records(pm):
    """the dense records of the last run: the state, then every chain day"""
    from parasitoids_amd import _lib as L
    s = pm.solver
    return [s.dense(L.REC_STATE, 0)] + [s.dense(L.REC_CHAIN, i) for i in range(pm._nd - 1)]


def _fields(pm):
    return [pm.population(d).toarray() for d in range(pm._nd)]


# ---------------------------------------------------------------- indexed adoption
def test_indexed_adoption_is_set_kernels_with_those_kernels():
    from parasitoids_amd import _lib as L
    lib = L.load()
    pm = _pop_model(R)
    dp, mu = MEMBERS[1]
    _quiet(pm.evaluate, HP, dp, DLP, mu, NPER, want_stats=False)       # set_kernels_from_model(1, nd - 1)
    s, m = pm.solver, pm.model
    want = _records(pm)

    def run(adopt):
        s.set_state_from_model(m, 0)
        adopt()
        s.run_chain(0, 5, negval=1e-8, scale=float(pm.r_number), renorm=False)
        return _records(pm)
    got = run(lambda: s.set_kernels_from_model_indexed(m, [1, 2, 3, 4, 5]))
    for d in range(6):
        assert np.array_equal(got[d], want[d]), (d, np.abs(got[d] - want[d]).max())
    idx = [3, 3, 1, 5, 2]
    got = run(lambda: s.set_kernels_from_model_indexed(m, idx))
    again = run(lambda: s.set_kernels_from_model_indexed(m, idx))        # the staging block is used a second time
    want = run(lambda: s.set_kernels([m.fetch(i) for i in idx]))
    assert np.abs(want[5] - _records(pm)[5]).max() == 0 and want[5].sum() > 0
    for d in range(6):
        assert np.array_equal(got[d], want[d]), (d, np.abs(got[d] - want[d]).max())
        assert np.array_equal(again[d], want[d])
    assert not np.array_equal(got[1], run(lambda: s.set_kernels_from_model_indexed(m, [1, 2, 3, 4, 5]))[1])
    # the refusals of the C ABI
    fn = lib.ps_chain_set_kernels_from_model_indexed
    ok = L.i32([1, 2])
    assert fn(None, m._h, L.p_i32(ok), 2) == L.PS_ERR_BAD_ARG
    assert fn(s._h, None, L.p_i32(ok), 2) == L.PS_ERR_BAD_ARG
    assert fn(s._h, m._h, None, 2) == L.PS_ERR_BAD_ARG
    assert fn(s._h, m._h, L.p_i32(ok), -1) == L.PS_ERR_BAD_ARG
    for bad in ([1, 6], [-1, 2]):
        assert fn(s._h, m._h, L.p_i32(L.i32(bad)), 2) == L.PS_ERR_STATE and b'not in the last batch' in lib.ps_last_error()
    assert fn(s._h, m._h, L.p_i32(ok), 0) == L.PS_OK                 # no kernels: as set_kernels_from_model(_, 0)
    # a day that failed its checks: its own status (lam = 3 makes prob_mass raise, test_prob_mass_bad_parameters)
    from parasitoids_amd import mcmc
    status = _quiet(m.build, pm.days, (3.0,) + tuple(HP[1:]), dp, DLP, mu, NPER, pm.rad_dist, pm.rad_res)[3]
    bad = [int(i) for i in np.flatnonzero(status)]
    assert bad and int(status[bad[0]]) in mcmc._PARAMETER_ERRORS
    assert fn(s._h, m._h, L.p_i32(L.i32(bad[:1])), 1) == int(status[bad[0]])
    assert b'failed its checks' in lib.ps_last_error()
    # and the handles stay usable
    _quiet(pm.evaluate, HP, dp, DLP, mu, NPER, want_stats=False)
    assert np.array_equal(_records(pm)[5], run(lambda: s.set_kernels_from_model_indexed(m, [1, 2, 3, 4, 5]))[5])
    pm.close()


# ---------------------------------------------------------------- run_sequence against evaluate
@pytest.mark.parametrize('mode, r_start', [('auto', None), ('fast', None), ('auto', 0.4)])
def test_run_sequence_of_the_recorded_days_is_evaluate(mode, r_start):
    """Kernel entries differ by < 1e-15 between batches (test_prob_mass_day_does_not_depend_on_its_batch_beyond_
    round_off), so a day adds at most 1e-15 x mass; six days and the transforms stay two orders below 1e-12 x the
    record's total."""
    pm = _pop_model(R, mode=mode, r_start=r_start)
    worst = 0.0
    for member in MEMBERS[:2]:
        dp, mu = member
        stats = _quiet(pm.evaluate, HP, dp, DLP, mu, NPER)
        want = _records(pm)
        seqs = _sequences(pm.days)
        _pool(pm, member, seqs)
        assert len(pm.model.last['days']) == 6 + (2 if r_start is not None else 0)
        got_stats = pm.run_sequence(seqs[0], want_stats=True)
        got = _records(pm)
        assert pm._nd == 6 and len(got_stats) == 6
        np.testing.assert_allclose([t for _n, t in got_stats], [t for _n, t in stats], rtol=1e-12)
        for d in range(6):
            ratio = np.abs(got[d] - want[d]).max() / want[d].sum()
            worst = max(worst, ratio)
            assert ratio <= 1e-12, (mode, d, ratio)
        other = _quiet(pm.run_sequence, seqs[1])
        assert other is None and not np.array_equal(_records(pm)[3], want[3])
        with pytest.raises(ValueError, match='leaves the days'):
            pm.run_sequence([pm.days[0], 9999])
    print('run_sequence against evaluate, mode %s, r_start %r: largest |difference| / total %.3g' % (mode, r_start, worst))
    _quiet(pm.evaluate, HP, dp, DLP, mu, NPER, want_stats=False)
    with pytest.raises(ValueError, match='has built another since'):
        pm.run_sequence(seqs[0])
    pm.close()


# ---------------------------------------------------------------- the variance split
GROUPS = [(MEMBERS[0], 3, 1), (MEMBERS[1], 3, 3), (MEMBERS[2], 3, 2), (MEMBERS[3], 2, 2)]    # member, draws, weight


def _same(W, keys, ref, names=RAW):
    for e, key in enumerate(keys):
        for name in names:
            got, want = W.plane(key, name), getattr(ref, name)[e]
            assert np.array_equal(got, want), (key, name, np.abs(got - want).max())
            assert not np.signbit(got).any()


def _same_final(W, keys, ref):
    out = ref.finalize()
    for e, key in enumerate(keys):
        assert np.array_equal(W.variance(key, 'weather'), out['vw'][e])
        assert np.array_equal(W.variance(key, 'parameter'), out['vp'][e])
        assert np.array_equal(W.variance(key, 'total'), out['vp'][e] + out['vw'][e])
        assert np.array_equal(W.share(key), out['share'][e])
        assert np.array_equal(W.mean(key), ref.omean[e])
    return out


@pytest.fixture(scope='module')
def fed():
    """the four groups evaluated once over one batch of kernels each; the day records', a plan's and a projection's
    WeatherShare fed alongside and compared with the replay after every add and close; two halves for the merge"""
    from parasitoids_amd.predictive import Projection, ReleaseSites, WeatherShare, exposure_weights
    pm = _pop_model(R)
    f = types.SimpleNamespace(pm=pm, seqs=_sequences(pm.days))
    f.A = ReleaseSites(pm, _metres(PLAN, R), DAYS)
    f.PJ = Projection(pm, exposure_weights(DAYS, EXPO), DAYS)
    f.W, f.Wlo, f.Whi, f.Wempty = [WeatherShare(pm) for _ in range(4)]
    f.WA, f.WJ = WeatherShare.for_projection(f.A), WeatherShare.for_projection(f.PJ)
    f.W.profile(True)
    f.ref, f.lo, f.hi = [NestedReplay((6, N, N)) for _ in range(3)]
    f.refA, f.refJ = NestedReplay((6, N, N)), NestedReplay((len(EXPO), N, N))
    f.draws = []
    for g, (member, k, w) in enumerate(GROUPS):
        _pool(pm, member, f.seqs[:k])
        half, rhalf = (f.Wlo, f.lo) if g < 2 else (f.Whi, f.hi)
        for seq in f.seqs[:k]:
            _quiet(pm.run_sequence, seq)
            for acc in (f.W, half):
                acc.add()
            v = np.array(_fields(pm))
            f.A.apply()
            f.PJ.apply()
            f.WA.add()
            f.WJ.add()
            f.ref.add(v)
            rhalf.add(v)
            f.refA.add(np.array([f.A.field(e) for e in range(6)]))
            f.refJ.add(np.array([f.PJ.field(e) for e in range(len(EXPO))]))
            f.draws.append(v)
            _same(f.W, DAYS, f.ref)
            assert (f.W.open_draws, f.W.members, f.W.groups) == (f.ref.k, f.ref.members, f.ref.G)
        for acc in (f.W, half, f.WA, f.WJ):
            acc.close_group(w)
        for r in (f.ref, rhalf, f.refA, f.refJ):
            r.close(w)
        _same(f.W, DAYS, f.ref)
        _same(f.WA, DAYS, f.refA)
        _same(f.WJ, range(len(EXPO)), f.refJ)
    f.all = [f.W, f.Wlo, f.Whi, f.Wempty, f.WA, f.WJ]
    yield f
    for h in f.all + [f.A, f.PJ, pm]:
        h.close()


def test_every_plane_is_the_replay_bit_for_bit(fed):
    W, ref = fed.W, fed.ref
    assert (W.groups, W.members, W.total_weight, W.open_draws) == (4, 11, 8.0, 0)
    assert W._info()[4] == ref.wk == 1.0 / 3 + 3.0 / 3 + 2.0 / 3 + 2.0 / 2
    assert W.nbytes == 6 * W.pitch * 64 and W.days == DAYS
    assert not W.plane(0, 'imean').any() and not W.plane(5, 'iM2').any()          # closed: the open group is +0.0
    out = _same_final(W, DAYS, ref)
    for e in (1, 5):
        # the split says something here: weather and parameters both move cells, and some cells only one of them
        assert out['vw'][e].max() > 0 and out['vp'][e].max() > 0
        assert ((out['share'][e] > 0) & (out['share'][e] < 1)).any()
        assert out['share'][e].max() <= 1.0 and out['share'][e].min() >= 0.0
    # the tail cell, its neighbour and the pairs that straddle a row end are those of the replay
    rows, cols = np.array([N - 1, N - 1, 2, 3, R]), np.array([N - 1, N - 2, N - 1, 0, R])
    assert np.array_equal(W.plane(5, 'oM2')[rows, cols], ref.oM2[5][rows, cols])
    _same_final(fed.WA, DAYS, fed.refA)
    _same_final(fed.WJ, range(len(EXPO)), fed.refJ)
    assert fed.WA.days == DAYS and fed.WJ.days == list(range(len(EXPO)))
    add_ms, adds, close_ms, closes = W.profile()
    assert (adds, closes) == (11, 4) and add_ms > 0 and close_ms > 0


def test_merge_of_two_halves(fed):
    from parasitoids_amd.predictive import WeatherShare
    lo, hi, empty = fed.Wlo, fed.Whi, fed.Wempty
    _same(lo, DAYS, fed.lo)
    _same(hi, DAYS, fed.hi)
    with WeatherShare(fed.pm) as nothing:
        hi.merge(nothing)                   # a source without groups changes nothing
    _same(hi, DAYS, fed.hi)
    assert (hi.groups, hi.members, hi.total_weight) == (2, 5, 4.0)
    empty.merge(lo)                         # into a handle without groups: a device copy
    assert (empty.groups, empty.members, empty.total_weight) == (2, 6, 4.0)
    _same(empty, DAYS, fed.lo)
    empty.merge(hi)
    both = copy.deepcopy(fed.lo)
    both.merge(fed.hi)
    assert (empty.groups, empty.members, empty.total_weight) == (4, 11, 8.0) == (both.G, both.members, both.W)
    assert empty._info()[4] == both.wk
    _same(empty, DAYS, both)
    out = _same_final(empty, DAYS, both)
    whole = fed.ref.finalize()
    # and the merged weather variance, a sum of non-negative terms, is the whole one up to the order of the sum
    np.testing.assert_allclose(out['vw'], whole['vw'], rtol=1e-12)
    with pytest.raises(ValueError, match='different days'):
        with WeatherShare(fed.pm, [0, 1]) as other:
            lo.merge(other)


def test_exact_identities_on_the_device(fed):
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import ReleaseSites, WeatherShare
    pm = fed.pm
    # three plans applied to one evaluation hold three different fields at once: the draws of a group that can be
    # added again bit for bit (an evaluation run again is the same only up to round-off)
    plans = [PLAN, [(dr, dc, 2.0 * a, lag) for dr, dc, a, lag in PLAN], [(0, 0, 1.0, 0), (3, -2, 0.5, 0)]]
    with WeatherShare(pm) as same_draws, ReleaseSites(pm, _metres(plans[0], R), DAYS) as A0, \
            ReleaseSites(pm, _metres(plans[1], R), DAYS) as A1, ReleaseSites(pm, _metres(plans[2], R), DAYS) as A2, \
            WeatherShare.for_projection(A0) as same_groups:
        # identical draws in every group: no weather
        for member, k, w in GROUPS[:3]:
            _pool(pm, member, fed.seqs[:1])
            _quiet(pm.run_sequence, fed.seqs[0])
            for _ in range(k):
                same_draws.add()
            same_draws.close_group(w)
        # identical groups: no parameter variance
        for A in (A0, A1, A2):
            A.apply()
        for w in (1, 3, 2):
            for A in (A0, A1, A2):
                assert same_groups._lib.ps_nested_add_sites(same_groups._h, A._h) == L.PS_OK
            same_groups.close_group(w)
        assert (same_groups.groups, same_groups.members) == (3, 9)
        for d in DAYS:
            assert not same_draws.variance(d, 'weather').any() and not same_draws.share(d).any()
            assert np.array_equal(same_draws.variance(d, 'parameter'), same_draws.plane(d, 'oM2') / 6.0)
            assert not same_groups.variance(d, 'parameter').any() and not same_groups.plane(d, 'oM2').any()
            tot = same_groups.variance(d, 'total')
            assert np.array_equal(same_groups.share(d), (tot > 0).astype(np.float64))
        assert same_draws.variance(5, 'parameter').max() > 0 and same_groups.variance(5, 'weather').max() > 0


def test_refusals_at_the_c_abi_and_the_handle_stays_usable(fed):
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import ReleaseSites, WeatherShare
    lib = L.load()
    dev = L.default_device()
    h = L._VP()
    create = lambda N=129, nslot=3, device=dev: lib.ps_nested_create(device, N, nslot, C.byref(h))
    assert create(N=0) == L.PS_ERR_BAD_ARG and not h
    assert create(nslot=0) == L.PS_ERR_BAD_ARG and not h
    assert lib.ps_nested_create(dev, 129, 3, None) == L.PS_ERR_BAD_ARG
    assert create(device=99) == L.PS_ERR_NO_DEVICE and not h
    assert create(N=60001, nslot=64) == L.PS_ERR_OOM and not h and b'GB free' in lib.ps_last_error()     # 15 TB
    assert create() == L.PS_OK and h
    lib.ps_nested_destroy(h)
    pm, big = fed.pm, _pop_model(128)
    out = np.empty((N, N))
    _pool(pm, MEMBERS[0], fed.seqs)
    _quiet(pm.run_sequence, fed.seqs[0])
    dp, mu = MEMBERS[0]
    _quiet(big.evaluate, HP, dp, DLP, mu, NPER, want_stats=False)
    with WeatherShare(pm, [0, 2, 5]) as X, WeatherShare(pm, [0, 2, 5]) as Y, WeatherShare(big, [0, 2, 5]) as Xbig, \
            WeatherShare(pm, [0, 2]) as X2, ReleaseSites(pm, _metres(PLAN, R), [0, 2]) as A2, \
            ReleaseSites(pm, _metres(PLAN, R), [0, 2, 5]) as A3:
        stat, post = L.f64([1.0] * 3), L.f64([1.0] * 3)
        args = (3, L.p_i32(X._kind), L.p_i32(X._idx), L.p_f64(stat), L.p_f64(post), L.p_i32(X._delta), 1e-8)
        assert lib.ps_nested_add(None, pm.solver._h, *args) == L.PS_ERR_BAD_ARG
        assert lib.ps_nested_add(X._h, None, *args) == L.PS_ERR_BAD_ARG
        assert lib.ps_nested_add(X._h, pm.solver._h, 3, None, *args[2:]) == L.PS_ERR_BAD_ARG
        assert lib.ps_nested_add(X._h, pm.solver._h, 2, *args[1:]) == L.PS_ERR_BAD_ARG and b'2 slots given' in lib.ps_last_error()
        assert lib.ps_nested_add(X._h, big.solver._h, *args) == L.PS_ERR_BAD_ARG and b'domain 257' in lib.ps_last_error()
        assert lib.ps_nested_add_sites(X._h, A3._h) == L.PS_ERR_STATE                      # never applied
        A2.apply()
        A3.apply()
        assert lib.ps_nested_add_sites(X._h, A2._h) == L.PS_ERR_BAD_ARG and b'has 2 outputs' in lib.ps_last_error()
        assert lib.ps_nested_add_sites(X._h, None) == L.PS_ERR_BAD_ARG
        assert lib.ps_nested_add_project(None, A3._h) == L.PS_ERR_BAD_ARG
        for fn in (lib.ps_nested_finalize, lib.ps_nested_reset):
            assert fn(None) == L.PS_ERR_BAD_ARG
        assert lib.ps_nested_close(None, 1) == L.PS_ERR_BAD_ARG
        assert lib.ps_nested_info(None, None, None, None, None, None) == L.PS_ERR_BAD_ARG
        assert lib.ps_nested_prof(None, 0, None, None, None, None) == L.PS_ERR_BAD_ARG
        for a, b in ((X, None), (None, X), (X, X), (X, Xbig), (X, X2)):
            assert lib.ps_nested_merge(a and a._h, b and b._h) == L.PS_ERR_BAD_ARG
        assert (X.members, X.groups, X.open_draws) == (0, 0, 0)           # nothing of the above was added
        # the states
        assert lib.ps_nested_close(X._h, 1) == L.PS_ERR_STATE and b'2 needed' in lib.ps_last_error()      # no draw
        assert lib.ps_nested_finalize(X._h) == L.PS_ERR_STATE and b'2 needed' in lib.ps_last_error()     # no group
        X.add()
        assert lib.ps_nested_close(X._h, 1) == L.PS_ERR_STATE                                             # one draw
        assert lib.ps_nested_finalize(X._h) == L.PS_ERR_STATE and b'open group' in lib.ps_last_error()
        assert lib.ps_nested_merge(X._h, Y._h) == L.PS_ERR_STATE and lib.ps_nested_merge(Y._h, X._h) == L.PS_ERR_STATE
        _quiet(pm.run_sequence, fed.seqs[1])
        X.add()
        assert lib.ps_nested_close(X._h, 0) == L.PS_ERR_BAD_ARG and b'weight must be >= 1' in lib.ps_last_error()
        X.close_group(2)
        assert lib.ps_nested_finalize(X._h) == L.PS_ERR_STATE                                             # one group
        assert lib.ps_nested_fetch(X._h, 0, 5, L.p_f64(out)) == L.PS_ERR_STATE and b'finalize' in lib.ps_last_error()
        for seq in fed.seqs[1:]:
            _quiet(pm.run_sequence, seq)
            X.add()
        X.close_group(1)
        for slot, what in ((-1, 0), (3, 0), (0, -1), (0, 8)):
            assert lib.ps_nested_fetch(X._h, slot, what, L.p_f64(out)) == L.PS_ERR_BAD_ARG
        assert lib.ps_nested_fetch(X._h, 0, 0, None) == L.PS_ERR_BAD_ARG
        assert lib.ps_nested_fetch(None, 0, 0, L.p_f64(out)) == L.PS_ERR_BAD_ARG
        assert lib.ps_nested_finalize(X._h) == L.PS_OK
        assert lib.ps_nested_fetch(X._h, 2, 7, L.p_f64(out)) == L.PS_OK and out.max() > 0
        share = X.share(5)
        assert np.array_equal(share, out)
        X.add()                                  # a later add: the results are stale
        assert lib.ps_nested_fetch(X._h, 2, 7, L.p_f64(out)) == L.PS_ERR_STATE
        assert lib.ps_nested_fetch(X._h, 2, 3, L.p_f64(out)) == L.PS_OK                                   # a raw plane
        X.add()
        X.close_group(1)
        assert (X.groups, X.members, X.total_weight) == (3, 6, 4.0)
        assert X.share(5).shape == (N, N)        # finalized again on demand
        with pytest.raises(ValueError):
            X.close_group(0)
        with pytest.raises(ValueError):
            X.variance(0, 'wind')
        with pytest.raises(ValueError):
            X.share(1)                           # day 1 is not among the handle's days
        X.reset()
        assert (X.groups, X.members, X.total_weight, X.open_draws) == (0, 0, 0.0, 0) and not X.plane(5, 'oM2').any()
    big.close()


# ---------------------------------------------------------------- the driver
THR = (1.0,)


def _load(path):
    with np.load(path) as f:
        return {k: f[k] for k in f.files}


def test_posterior_predictive_with_wind(tmp_path):
    from parasitoids_amd import mcmc
    from parasitoids_amd import predictive as PR
    trace, names = _chain([2, 1, 3])
    chains = [(trace, names)]                               # three runs of lengths 2, 1 and 3
    pa, pb, pc = [_pop_model(R) for _ in range(3)]
    seqs = _sequences(pa.days)
    plan = dict(sites=[s[:3] for s in _metres(PLAN, R)], days=DAYS)
    kw = dict(thresholds=THR, exposure=EXPO, sites=plan)
    res = _quiet(PR.posterior_predictive, pa, chains, wind=dict(sequences=seqs), **kw)
    assert res.failed == 0 and res.evaluations == 3 and len(res.runs) == 3
    assert res.wind['sequences'].tolist() == seqs and res.wind['used'] == sorted(pa.days)
    assert len(res.wind['build_s']) == 3 and res.wind['pool_kernels'] and res.wind['share']
    S, W = res.summary, res.weather
    assert S.members == 9 and S.total_weight == 18 and (W.members, W.groups, W.total_weight) == (9, 3, 6.0)
    # by hand, in the driver's order
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    with PR.SpreadSummary(pb, None, THR) as S2, PR.WeatherShare(pb) as W2, \
            PR.ReleaseSites(pb, plan['sites'], DAYS) as A, PR.WeatherShare.for_projection(A) as WA:
        for first, length in ((0, 2), (2, 1), (3, 3)):
            args = mcmc.model_args(trace[first, cols])
            _quiet(pb.build_pool, *args, sorted(pb.days), [s[0] for s in seqs])
            for seq in seqs:
                _quiet(pb.run_sequence, seq)
                S2.add(length)
                W2.add()
                A.apply()
                WA.add()
            W2.close_group(length)
            WA.close_group(length)
        for d in DAYS:
            assert np.array_equal(S.mean(d), S2.mean(d)) and np.array_equal(S.variance(d), S2.variance(d))
            assert np.array_equal(S.exceedance(d, 0), S2.exceedance(d, 0))
            for name in ('omean', 'oM2', 'wS', 'vw', 'vp', 'share'):
                assert np.array_equal(W.plane(d, name), W2.plane(d, name)), (d, name)
                assert np.array_equal(res.sites.weather.plane(d, name), WA.plane(d, name)), (d, name)
        assert (S2.members, S2.total_weight) == (9, 18)
    assert res.exposure.weather.groups == 3 and res.sites.summary.members == 9
    assert res.weather.share(5).max() > 0 and res.weather.variance(5, 'parameter').max() > 0
    # the files and the json block
    npz, js = res.save(str(tmp_path / 'pp'))
    f = _load(str(tmp_path / 'pp_weather.npz'))
    labels = [pa.days[d] for d in DAYS]
    for d, label in zip(DAYS, labels):
        for suffix, part in (('vw', 'weather'), ('vp', 'parameter')):
            m = W.variance(d, part)
            assert np.array_equal(_csr(f, '%s_%s' % (label, suffix), N), np.where(m >= 1e-8, m, 0.0))
        m = W.share(d)
        assert np.array_equal(_csr(f, '%s_share' % label, N), np.where(m >= 1e-8, m, 0.0))
        assert 'sites_%s_share_data' % d in f
    assert 'exposure_%s_vw_data' % EXPO[-1] in f
    block = json.load(open(js))['predictive']['wind']
    assert block['sequences'] == seqs and block['groups'] == 3 and block['members'] == 9 and block['block'] == 3
    assert block['pool'] == sorted(pa.wind_data.keys()) and block['sites']['groups'] == 3
    for d, label in zip(DAYS, labels):
        mean, share = S.mean(d), W.share(d)
        assert block['weather_share'][str(label)] == float((share * mean).sum() / mean.sum())
    assert 0 < block['weather_share'][str(labels[5])] < 1
    # the A/B leg: every sequence as a model of its own
    slow = _quiet(PR.posterior_predictive, pc, chains, wind=dict(sequences=seqs, pool_kernels=False), **kw)
    assert pc.days == pa.days and slow.summary.members == 9 and slow.weather.groups == 3
    worst = 0.0
    for d in DAYS:
        for a, b in ((S.mean(d), slow.summary.mean(d)), (res.sites.summary.mean(d), slow.sites.summary.mean(d))):
            ratio = np.abs(a - b).max() / a.sum()
            worst = max(worst, ratio)
            assert ratio <= 1e-12, (d, ratio)
    print('pool_kernels=False against the pool: largest |difference of the means| / total %.3g' % worst)
    # share=False: one sequence is enough, and nothing of the split is built
    one = _quiet(PR.posterior_predictive, pc, chains, wind=dict(sequences=seqs[1:2], share=False), thresholds=THR)
    assert one.weather is None and one.summary.members == 3 and one.wind['sequences'].tolist() == seqs[1:2]
    one.save(str(tmp_path / 'one'))
    assert not os.path.exists(str(tmp_path / 'one_weather.npz'))
    assert json.load(open(str(tmp_path / 'one.json')))['predictive']['wind']['sequences'] == seqs[1:2]
    for r in (res, slow, one):
        for fs in (r.exposure, r.sites):
            if fs is not None:
                fs.close()
        for acc in (r.summary, r.weather):
            if acc is not None:
                acc.close()
    for pm in (pa, pb, pc):
        pm.close()


def test_without_wind_nothing_changes(tmp_path):
    from parasitoids_amd import predictive as PR
    trace, names = _chain([2, 1, 3])
    saved = []
    for tag in ('a', 'b'):
        pm = _pop_model(R)               # a model of its own: an evaluation is reproducible from the same history
        res = _quiet(PR.posterior_predictive, pm, [(trace, names)], thresholds=THR, exposure=EXPO)
        assert res.weather is None and res.wind is None and res.exposure.weather is None
        assert res.summary.members == 3
        res.save(str(tmp_path / tag))
        assert not [n for n in os.listdir(str(tmp_path)) if 'weather' in n]
        assert 'wind' not in json.load(open(str(tmp_path / (tag + '.json'))))['predictive']
        saved.append((_load(str(tmp_path / (tag + '.npz'))), _load(str(tmp_path / (tag + '_exposure.npz')))))
        res.exposure.close()
        res.summary.close()
        pm.close()
    for a, b in zip(*saved):
        assert sorted(a) == sorted(b)
        for k in a:
            assert np.array_equal(a[k], b[k]), k

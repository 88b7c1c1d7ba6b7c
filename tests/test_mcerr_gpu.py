"""GPU tests of the Monte Carlo error of the posterior maps (ps_mcerr_*, predictive.MonteCarloError): the device's
gmean, counts and bookkeeping bit for bit against the numpy replay (mcerr_ref) of the members' fetched fields, gM2
and wM2 within the tolerances of the SpreadSummary tests; the library's split of a weight against the caller's own
and against unit adds; merge; exact identities under a scaling by 2 and for identical members; the split R-hat;
projections and release plans as sources; posterior_predictive with mc_error=; the refusals of the C ABI; and the
grid-stride path at R = 768.  Kalbar wind, R = 64 (N = 129: odd, so the tail cell and the pairs that straddle a
row end exist), 6 days, the members of test_sites_gpu.py."""
import ctypes as C
import json
import os
import types
import warnings

import numpy as np
import pytest

import mcerr_ref
from parasitoids_amd.predictive import MonteCarloError, split_rhat
from test_sites_gpu import MEMBERS, _chain, _csr, _evaluate, _metres, _pop_model

pytestmark = pytest.mark.gpu

R, N = 64, 129
THR = [1.0, 10.0]
DAYS = list(range(6))
WEIGHTS = [1, 3, 1, 2, 1, 4, 2, 1, 3, 2, 1, 3]     # 24 rows, b = 3: 8 batches; runs straddle, the 4 crosses two
BW = 3
PLAN = [(0, 0, 1.0, 0), (-5, 3, 0.5, 0), (7, -4, 0.25, 0)]
PLAN2 = [(dr, dc, 2.0 * a, lag) for dr, dc, a, lag in PLAN]
EXPO = [0, 2, 5]


def _fields(pm):
    return [pm.population(d).toarray() for d in DAYS]


def _replay(fields, weights, thr, b, members=None, finish=True):
    """per slot the mcerr_ref state over the members' fields [member][slot]"""
    idx = range(len(weights)) if members is None else members
    states = []
    for e in range(len(fields[0])):
        st = mcerr_ref.new_state(fields[0][e].shape, thr, b)
        for i in idx:
            mcerr_ref.add(st, fields[i][e], weights[i])
        states.append(mcerr_ref.finish(st) if finish else st)
    return states


def _check_exact(M, states, keys):
    """gmean and every count of M against the replay bit for bit, gM2 and wM2 within rtol 1e-12, atol 1e-15 scale^2"""
    for key, st in zip(keys, states):
        assert (M.batches, M.batch_weight, M.used_weight) == (st['B'], st['b'], st['b'] * st['B'])
        g = M.plane(key, 0)
        assert np.array_equal(g, st['gmean']), (key, np.abs(g - st['gmean']).max())
        assert np.array_equal(M.mean(key), g)
        scale = np.abs(st['gmean']).max()
        for what, name in ((1, 'gM2'), (2, 'wM2')):
            got = M.plane(key, what)
            print('%s, %r: max abs error %.3g, scale^2 %.3g' % (name, key, np.abs(got - st[name]).max(), scale ** 2))
            np.testing.assert_allclose(got, st[name], rtol=1e-12, atol=1e-12 * 1e-3 * scale ** 2)
        for k in range(len(M.thresholds)):
            s1, s2 = M.counts(key, k)
            assert s1.dtype == np.uint32 and s2.dtype == np.uint64
            assert np.array_equal(s1.astype(np.uint64), st['s1'][k]) and np.array_equal(s2, st['s2'][k]), (key, k)


@pytest.fixture(scope='module')
def fed():
    """the twelve members evaluated once, every accumulator the tests read fed alongside, the fields fetched and
    the replays computed once"""
    from parasitoids_amd.predictive import Projection, ReleaseSites, exposure_weights
    pm = _pop_model(R)
    f = types.SimpleNamespace(pm=pm)
    f.A = ReleaseSites(pm, _metres(PLAN, R), DAYS)
    f.A2 = ReleaseSites(pm, _metres(PLAN2, R), DAYS)
    f.PJ = Projection(pm, exposure_weights(DAYS, EXPO), DAYS)
    new = lambda b=BW, thr=THR: MonteCarloError(pm, b, DAYS, thr)
    f.M, f.Mown, f.Munit, f.Mlo, f.Mhi, f.M0 = new(), new(), new(), new(), new(), new(thr=())
    f.Msame = new(1)
    f.Oa, f.Ob, f.Ia, f.Ib = new(1), new(1), new(1), new(1)
    f.P = [MonteCarloError.for_projection(f.A, BW, THR) for _ in range(2)]        # rows [0, 12) and [12, 24)
    f.P2 = [MonteCarloError.for_projection(f.A2, BW, THR) for _ in range(2)]
    f.MJ = MonteCarloError.for_projection(f.PJ, BW, THR)
    f.fields, f.fa, f.fj = [], [], []
    for i, w in enumerate(WEIGHTS):
        s = i % len(MEMBERS)
        _evaluate(pm, MEMBERS[s])
        for acc in (f.M, f.M0, f.Mlo if i < 6 else f.Mhi):
            acc.add(w)
        for p in mcerr_ref.pieces(f.Mown.open_weight, BW, w):
            f.Mown.add(p)
        for _ in range(w):
            f.Munit.add(1)
        if i == 0:
            for _ in range(3):
                f.Msame.add(2)
        if s < 4 and i < 10:                     # sets 0, 1, 2, 3, (4), 0, 1, 2, 3
            (f.Oa if s < 2 else f.Ob).add(1)     # the halves use different parameter sets
            (f.Ia if i < 5 else f.Ib).add(1)     # the same members, every set in either half
        for plan, seqs in ((f.A, f.P), (f.A2, f.P2)):
            plan.apply()
            seqs[0 if i < 6 else 1].add(w)
        f.PJ.apply()
        f.MJ.add(w)
        f.fields.append(_fields(pm))
        f.fa.append([f.A.field(e) for e in range(6)])
        f.fj.append([f.PJ.field(e) for e in range(len(EXPO))])
    f.open_before = (f.M.batches, f.M.open_weight, f.M.used_weight, f.M.discarded_weight, f.M.members)
    f.all = [f.M, f.Mown, f.Munit, f.Mlo, f.Mhi, f.M0, f.Msame, f.Oa, f.Ob, f.Ia, f.Ib, f.MJ] + f.P + f.P2
    for acc in f.all:
        acc.finish()
    f.ref = _replay(f.fields, WEIGHTS, THR, BW)
    yield f
    for h in f.all + [f.A, f.A2, f.PJ, pm]:
        h.close()


def test_against_the_replay_bit_for_bit(fed):
    M, ref = fed.M, fed.ref
    assert M.N == N and M.days == DAYS and M.thresholds == THR
    assert M.nbytes == 6 * ((N * N + 63) // 64 * 64) * (40 + 16 * 2)
    # 24 rows in batches of 3: nothing open at the end, nothing discarded
    assert fed.open_before == (8, 0, 24, 0, 12)
    assert (M.batches, M.batch_weight, M.used_weight, M.open_weight, M.discarded_weight, M.members) == (8, 3, 24, 0, 0, 12)
    # the inputs can fail: batch counts that differ between batches, values in the tail cell's row or column,
    # batch means that differ on every day after the release day
    assert any((8 * st['s2'][k].astype(object) != st['s1'][k].astype(object) ** 2).any() for st in ref for k in range(2))
    edge = max(max(np.abs(fl[d][N - 1]).max(), np.abs(fl[d][:, N - 1]).max()) for fl in fed.fields for d in DAYS)
    print('largest value in the tail cell\'s row or column: %.3g' % edge)
    assert edge > 0
    assert all(ref[d]['gM2'].max() > 0 for d in DAYS[1:])
    _check_exact(M, ref, DAYS)
    # without thresholds: the moments alone, the same bits
    for d in DAYS:
        for what in range(3):
            assert np.array_equal(fed.M0.plane(d, what), M.plane(d, what))
    with pytest.raises(ValueError, match='threshold'):
        fed.M0.counts(0, 0)
    # the derived maps from the fetched planes
    for d in (0, 3, 5):
        st = ref[d]
        np.testing.assert_allclose(M.mcse(d), mcerr_ref.mcse(st), rtol=1e-12, atol=1e-15 * np.abs(st['gmean']).max())
        np.testing.assert_allclose(M.variance(d), mcerr_ref.variance(st), rtol=1e-12,
                                   atol=1e-15 * np.abs(st['gmean']).max() ** 2)
        live = st['gM2'] > 1e-6 * st['gM2'].max()
        np.testing.assert_allclose(M.ess(d)[live], mcerr_ref.ess(st)[live], rtol=1e-9)
        assert not M.ess(d)[st['gM2'] == 0].any()
        for k in range(2):
            assert np.array_equal(M.prob(d, k), st['s1'][k] / 24.0)
            assert np.array_equal(M.prob_mcse(d, k), mcerr_ref.prob_mcse(st, k))
            pe = M.prob_ess(d, k)
            assert np.isfinite(pe).all() and (pe >= 0).all() and (pe[mcerr_ref.prob_mcse(st, k) > 0] > 0).all()
    # an unfinished sequence: the open batch is bookkeeping only, and reset brings every plane back to zero
    with MonteCarloError(fed.pm, 4, [5], THR) as X:
        _evaluate(fed.pm, MEMBERS[1])
        cur = _fields(fed.pm)
        for w in (3, 6):
            X.add(w)
        assert (X.batches, X.open_weight, X.used_weight, X.members) == (2, 1, 8, 2)
        st = _replay([cur] * 2, [3, 6], THR, 4, finish=False)[5]
        assert st['open'] == 1 and st['bmean'].any()
        _check_exact(X, [st], [5])
        X.finish()
        assert (X.batches, X.open_weight, X.discarded_weight) == (2, 0, 1)
        _check_exact(X, [mcerr_ref.finish(st)], [5])
        X.reset()
        assert (X.batches, X.open_weight, X.discarded_weight, X.members) == (0, 0, 0, 0)
        for w in (4, 4):
            X.add(w)
        assert not X.plane(5, 1).any() and not X.plane(5, 2).any()
        assert np.array_equal(X.plane(5, 0), cur[5])


def test_one_add_equals_the_callers_own_split_and_unit_adds(fed):
    M = fed.M
    assert fed.Mown.members == sum(len(mcerr_ref.pieces(o, BW, w)) for o, w in zip(np.cumsum([0] + WEIGHTS) % BW, WEIGHTS))
    assert fed.Mown.members > 12 and fed.Munit.members == 24
    for other in (fed.Mown, fed.Munit):
        assert (other.batches, other.used_weight, other.discarded_weight) == (8, 24, 0)
    for d in DAYS:
        for what in range(3):
            assert np.array_equal(fed.Mown.plane(d, what), M.plane(d, what)), (d, what)
        ma, mb = M.plane(d, 0), fed.Munit.plane(d, 0)
        np.testing.assert_allclose(ma, mb, rtol=1e-13, atol=1e-16 * np.abs(ma).max())
        for what in (1, 2):
            np.testing.assert_allclose(M.plane(d, what), fed.Munit.plane(d, what), rtol=1e-13,
                                       atol=1e-13 * 1e-3 * np.abs(ma).max() ** 2)
        for k in range(2):
            for other in (fed.Mown, fed.Munit):
                assert all(np.array_equal(a, b) for a, b in zip(M.counts(d, k), other.counts(d, k)))


def test_merge(fed):
    from parasitoids_amd import _lib as L
    lo = _replay(fed.fields, WEIGHTS, THR, BW, range(6))
    hi = _replay(fed.fields, WEIGHTS, THR, BW, range(6, 12))
    _check_exact(fed.Mlo, lo, DAYS)
    _check_exact(fed.Mhi, hi, DAYS)
    with MonteCarloError(fed.pm, BW, DAYS, THR) as D, MonteCarloError(fed.pm, BW, DAYS, THR) as E, \
            MonteCarloError(fed.pm, BW, DAYS, THR) as U, MonteCarloError(fed.pm, BW + 1, DAYS, THR) as Ob, \
            MonteCarloError(fed.pm, BW, DAYS, THR[:1]) as Ot, MonteCarloError(fed.pm, BW, DAYS[:5], THR) as Od:
        D.merge(fed.Mlo)                                       # into an empty handle: a copy
        assert (D.batches, D.used_weight, D.members) == (4, 12, 6)
        for d in DAYS:
            for what in range(3):
                assert np.array_equal(D.plane(d, what), fed.Mlo.plane(d, what))
            for k in range(2):
                assert all(np.array_equal(a, b) for a, b in zip(D.counts(d, k), fed.Mlo.counts(d, k)))
        D.merge(E)                                             # an empty source changes nothing
        assert D.batches == 4
        D.merge(fed.Mhi)
        assert (D.batches, D.used_weight, D.discarded_weight, D.members) == (8, 24, 0, 12)
        for d in DAYS:
            st = mcerr_ref.merge(lo[d], hi[d])
            scale = np.abs(st['gmean']).max()
            np.testing.assert_allclose(D.plane(d, 0), st['gmean'], rtol=1e-12, atol=1e-15 * scale)
            for what, name in ((1, 'gM2'), (2, 'wM2')):
                np.testing.assert_allclose(D.plane(d, what), st[name], rtol=1e-12, atol=1e-15 * scale ** 2)
            for k in range(2):
                s1, s2 = D.counts(d, k)
                assert np.array_equal(s1.astype(np.uint64), st['s1'][k]) and np.array_equal(s2, st['s2'][k])
                # pooled batches: the integers of one handle over all rows
                assert all(np.array_equal(a, b) for a, b in zip((s1, s2), fed.M.counts(d, k)))
            np.testing.assert_allclose(D.plane(d, 0), fed.M.plane(d, 0), rtol=1e-12, atol=1e-15 * scale)
        # an unfinished handle on either side, and handles that do not match
        _evaluate(fed.pm, MEMBERS[0])
        U.add(BW + 1)
        lib = D._lib
        assert lib.ps_mcerr_merge(D._h, U._h) == L.PS_ERR_STATE and b'open batch' in lib.ps_last_error()
        assert lib.ps_mcerr_merge(U._h, D._h) == L.PS_ERR_STATE
        U.finish()
        assert lib.ps_mcerr_merge(D._h, U._h) == L.PS_OK and D.batches == 9 and D.discarded_weight == 1
        assert lib.ps_mcerr_merge(D._h, Ob._h) == L.PS_ERR_BAD_ARG and b'batch weight' in lib.ps_last_error()
        assert lib.ps_mcerr_merge(D._h, Ot._h) == L.PS_ERR_BAD_ARG
        assert lib.ps_mcerr_merge(D._h, Od._h) == L.PS_ERR_BAD_ARG
        assert lib.ps_mcerr_merge(D._h, D._h) == L.PS_ERR_BAD_ARG
        with pytest.raises(ValueError, match='different days'):
            D.merge(Od)


def test_exact_identities_on_the_device(fed):
    """amounts x 2: every field doubles exactly, so mean x 2, gM2 and wM2 x 4, and ESS and R-hat do not move a bit"""
    for e in range(6):
        for a, a2 in zip(fed.P, fed.P2):
            assert a.batches == a2.batches == 4
            assert np.array_equal(a2.mean(e), 2.0 * a.mean(e)) and a.mean(e).max() > 0
            assert np.array_equal(a2.plane(e, 1), 4.0 * a.plane(e, 1))
            assert np.array_equal(a2.plane(e, 2), 4.0 * a.plane(e, 2))
            assert np.array_equal(a2.ess(e), a.ess(e))
            assert np.array_equal(a2.mcse(e), 2.0 * a.mcse(e))
        r, r2 = split_rhat(fed.P, e), split_rhat(fed.P2, e)
        assert np.array_equal(r, r2)
        assert e == 0 or (r.max() > 0 and fed.P[0].ess(e).max() > 0 and fed.P[0].plane(e, 2).max() > 0)
    # identical members: nothing varies anywhere
    S = fed.Msame
    assert (S.batches, S.members) == (6, 3)
    for d in DAYS:
        assert np.array_equal(S.mean(d), fed.fields[0][d])
        assert not S.plane(d, 1).any() and not S.plane(d, 2).any() and not S.mcse(d).any() and not S.ess(d).any()
        assert not split_rhat([S, S], d).any()
        for k in range(2):
            s1, s2 = S.counts(d, k)
            assert np.array_equal(np.uint64(6) * s2, s1.astype(np.uint64) ** 2) and not S.prob_mcse(d, k).any()
            assert not S.prob_ess(d, k).any()


def test_split_rhat(fed):
    seqs = [fed.Mlo, fed.Mhi, fed.M]                # 4, 4 and 8 batches
    assert [s.batches for s in seqs] == [4, 4, 8]
    for d in DAYS:
        got = split_rhat(seqs, d)
        want = mcerr_ref.rhat([(s.plane(d, 0), s.plane(d, 1), s.plane(d, 2), s.used_weight) for s in seqs], BW)
        assert got.shape == (N, N) and (d == 0 or got.max() > 0)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
        assert not got[want == 0].any()
    # two halves from different parameter sets against the same members spread over both halves
    assert [s.batches for s in (fed.Oa, fed.Ob, fed.Ia, fed.Ib)] == [4, 4, 4, 4]
    for d in DAYS[1:]:
        apart, mixed = split_rhat([fed.Oa, fed.Ob], d), split_rhat([fed.Ia, fed.Ib], d)
        print('day %d: R-hat max %.4f with the halves apart, %.4f interleaved' % (d, apart.max(), mixed.max()))
        assert apart.max() > mixed.max() and apart.max() > 1.0
    with pytest.raises(ValueError, match='sequences'):
        split_rhat([fed.M], 0)
    with pytest.raises(ValueError, match='sequences'):
        split_rhat([fed.M] * 17, 0)
    assert split_rhat([fed.M] * 16, 5).shape == (N, N)


def test_for_projection(fed):
    # a release plan: the two halves of the rows, and a Projection over all of them
    _check_exact(fed.P[0], _replay(fed.fa, WEIGHTS, THR, BW, range(6)), range(6))
    _check_exact(fed.P[1], _replay(fed.fa, WEIGHTS, THR, BW, range(6, 12)), range(6))
    assert fed.MJ.days == [0, 1, 2] and fed.MJ.members == 12 and fed.MJ.batches == 8
    ref = _replay(fed.fj, WEIGHTS, THR, BW)
    assert all(st['gM2'].max() > 0 for st in ref[1:]) and ref[2]['s1'][1].max() > 0
    _check_exact(fed.MJ, ref, range(3))
    with pytest.raises(ValueError, match='not in the sequence'):
        fed.MJ.mean(3)


def test_posterior_predictive_with_mc_error(tmp_path):
    from parasitoids_amd import mcmc
    from parasitoids_amd import predictive as PR
    trace, names = _chain([3, 1, 2, 1, 2, 2])
    # 5 and 6 rows, b = 1: the run of three straddles chain 0's half (row 2), a run of two chain 1's (row 3)
    chains = [(trace[:5], names), (trace[5:], names)]
    kw = dict(thresholds=THR, exposure=[2, 5])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        pa, pb, pc, pd = (_pop_model(R, mode='exact') for _ in range(4))
        res = PR.posterior_predictive(pa, chains, mc_error=dict(batches=4), **kw)
        par = PR.posterior_predictive([pb, pc], chains, mc_error=dict(batches=4), **kw)
        plain = PR.posterior_predictive(pd, chains, **kw)
    X = res.mc_error
    assert plain.mc_error is None and plain.mc_plan is None and plain.exposure.mc_error is None
    assert res.mc_plan == {'batches': 4, 'batch_weight': 1, 'sequences': 4} and res.failed == 0
    assert (X.batches, X.batch_weight, X.used_weight, X.discarded_weight, X.members) == (11, 1, 11, 0, 9)
    assert res.exposure.mc_error.batches == 11 and sorted(X.rhat) == DAYS and sorted(res.exposure.mc_error.rhat) == [0, 1]
    # every other result does not know about it
    for d in DAYS:
        for k in range(3):
            assert np.array_equal(res.summary.fetch_slot(d, k), plain.summary.fetch_slot(d, k))
    for e in range(2):
        assert np.array_equal(res.exposure.summary.mean(e), plain.exposure.summary.mean(e))
        assert np.array_equal(res.exposure.summary.variance(e), plain.exposure.summary.variance(e))
    # by hand: two sequences per chain, cut at the chain's half; R-hat over the four, merged in chain order
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    pm = _pop_model(R, mode='exact')
    b, halves = PR.mc_batch_plan([5, 6], 4)
    assert b == 1 and halves == [(2, 5), (3, 6)]
    assert [r[1:] for r in res.runs] == [(0, 3), (3, 1), (4, 1), (0, 1), (1, 1), (2, 2), (4, 2)]
    seqs = [[MonteCarloError(pm, b, DAYS, THR) for _ in range(2)] for _ in range(2)]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        for ci, first, weight in res.runs:
            pm.evaluate(*mcmc.model_args(chains[ci][0][first, cols]), want_stats=False)
            for seq, w in zip(seqs[ci], PR.mc_split(first, weight, halves[ci][0])):
                if w:
                    seq.add(w)
    flat = [s for pair in seqs for s in pair]
    assert [s.batches for s in flat] == [2, 3, 3, 3] and [s.members for s in flat] == [1, 3, 3, 2]
    for s in flat:
        s.finish()
    rh = {d: split_rhat(flat, d) for d in DAYS}
    for s in flat[1:]:
        flat[0].merge(s)
    for got in (X, par.mc_error):
        for d in DAYS:
            for what in range(3):
                assert np.array_equal(got.plane(d, what), flat[0].plane(d, what)), (d, what)
            for k in range(2):
                assert all(np.array_equal(a, c) for a, c in zip(got.counts(d, k), flat[0].counts(d, k)))
            assert np.array_equal(got.rhat[d], rh[d])
    for e in range(2):                     # the parallel run's projection against the sequential one's
        for what in range(3):
            assert np.array_equal(par.exposure.mc_error.plane(e, what), res.exposure.mc_error.plane(e, what))
        assert np.array_equal(par.exposure.mc_error.rhat[e], res.exposure.mc_error.rhat[e])
    assert rh[5].max() > 0 and X.mcse(5).max() > 0
    # the mean over the used rows is the summary's: nothing was discarded
    np.testing.assert_allclose(X.mean(5), res.summary.mean(5), rtol=1e-12, atol=1e-15 * res.summary.mean(5).max())
    # the result files
    npz, js = res.save(str(tmp_path / 'a' / 'pp'))
    plain.save(str(tmp_path / 'p' / 'pp'))
    assert not os.path.exists(str(tmp_path / 'p' / 'pp_mcerr.npz'))
    for name in ('pp.npz', 'pp_exposure.npz'):
        with np.load(str(tmp_path / 'a' / name)) as fx, np.load(str(tmp_path / 'p' / name)) as fp:
            assert set(fx.files) == set(fp.files) and all(np.array_equal(fx[key], fp[key]) for key in fp.files)
    labels = [res.summary.pm.days[d] for d in DAYS]
    with np.load(str(tmp_path / 'a' / 'pp_mcerr.npz')) as fz:
        want = {'days'}
        E = res.exposure.mc_error
        for src, keys, labs in ((X, DAYS, [str(x) for x in labels]), (E, [0, 1], ['exposure_2', 'exposure_5'])):
            for key, lab in zip(keys, labs):
                for suffix, m in (('_mcse', src.mcse(key)), ('_ess', src.ess(key)), ('_rhat', src.rhat[key]),
                                  ('_pmcse0', src.prob_mcse(key, 0)), ('_pmcse1', src.prob_mcse(key, 1))):
                    assert np.array_equal(_csr(fz, lab + suffix, N), np.where(m >= 1e-8, m, 0.0)), (lab, suffix)
                    want |= {'%s%s_%s' % (lab, suffix, t) for t in ('data', 'ind', 'indptr')}
        assert set(fz.files) == want
        assert [str(x) for x in fz['days']] == [str(x) for x in labels] + ['exposure_2', 'exposure_5']
    mc = json.load(open(js))['predictive']['mc_error']
    assert (mc['batches'], mc['batch_weight'], mc['sequences']) == (4, 1, 4)
    assert (mc['used_weight'], mc['discarded_weight'], mc['batches_pooled'], mc['members']) == (11, 0, 11, 9)
    assert mc['thresholds'] == THR and len(mc['outputs']) == 6 and len(mc['exposure']['outputs']) == 2
    live = X.counts(5, 0)[0] > 0
    out5 = mc['outputs'][5]
    assert out5['cells'] == int(live.sum()) > 0 and out5['ess_min'] == float(X.ess(5)[live].min())
    assert out5['ess_median'] == float(np.median(X.ess(5)[live])) and out5['rhat_max'] == float(X.rhat[5][live].max())
    assert 'mc_error' not in json.load(open(str(tmp_path / 'p' / 'pp.json')))['predictive']
    for r in (res, par, plain):
        for acc in (r.summary, r.exposure, r.mc_error):
            if acc is not None:
                acc.close()
    for h in flat + [pm, pa, pb, pc, pd]:
        h.close()


def test_refusals_at_the_c_abi_and_the_handle_stays_usable(fed):
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import ReleaseSites
    lib = L.load()
    dev = L.default_device()
    h = L._VP()

    def create(thr, N=129, nslot=3, device=dev, b=3):
        t = L.f64(thr if len(thr) else [0.0])
        return lib.ps_mcerr_create(device, N, nslot, len(thr), L.p_f64(t), b, C.byref(h))
    assert create([1, 2, 3, 4, 5]) == L.PS_ERR_BAD_ARG and not h
    for bad in ([np.nan], [np.inf], [1.0, 1.0], [2.0, 1.0]):
        assert create(bad) == L.PS_ERR_BAD_ARG and not h
        assert b'threshold' in lib.ps_last_error()
    assert create([1.0], b=0) == L.PS_ERR_BAD_ARG and not h and b'batch_weight' in lib.ps_last_error()
    assert create([1.0], nslot=0) == L.PS_ERR_BAD_ARG and not h
    assert create([1.0], N=0) == L.PS_ERR_BAD_ARG and not h
    assert create([1.0], device=99) == L.PS_ERR_NO_DEVICE and not h
    assert create([1.0, 2.0, 3.0, 4.0], N=60001, nslot=32) == L.PS_ERR_OOM and not h      # 12 TB
    assert b'GB free' in lib.ps_last_error()
    assert create([], b=2 ** 32 - 1) == L.PS_OK and h
    lib.ps_mcerr_destroy(h)
    pm, big = fed.pm, _pop_model(128)
    out = np.empty((N, N))
    s1 = np.empty((N, N), dtype=np.uint32)
    s2 = np.empty((N, N), dtype=np.uint64)
    p1, p2 = s1.ctypes.data_as(C.POINTER(C.c_uint32)), s2.ctypes.data_as(C.POINTER(C.c_uint64))
    _evaluate(pm, MEMBERS[0])
    _evaluate(big, MEMBERS[0])
    cur = [pm.population(d).toarray() for d in (0, 2, 5)]
    with MonteCarloError(pm, 2, [0, 2, 5], THR) as X, MonteCarloError(pm, 2, [0, 2, 5], THR) as Y, \
            MonteCarloError(big, 2, [0, 2, 5], THR) as Xbig, ReleaseSites(pm, _metres(PLAN, R), [0, 2]) as A2, \
            ReleaseSites(pm, _metres(PLAN, R), [0, 2, 5]) as A3:
        X.profile(True)
        stat, post = L.f64([1.0] * 3), L.f64([1.0] * 3)
        args = (3, L.p_i32(X._kind), L.p_i32(X._idx), L.p_f64(stat), L.p_f64(post), L.p_i32(X._delta), 1e-8)
        assert lib.ps_mcerr_add(None, pm.solver._h, *args, 1) == L.PS_ERR_BAD_ARG
        assert lib.ps_mcerr_add(X._h, None, *args, 1) == L.PS_ERR_BAD_ARG
        assert lib.ps_mcerr_add(X._h, pm.solver._h, *args, 0) == L.PS_ERR_BAD_ARG and b'weight must be >= 1' in lib.ps_last_error()
        assert lib.ps_mcerr_add(X._h, pm.solver._h, 2, *args[1:], 1) == L.PS_ERR_BAD_ARG and b'2 slots given' in lib.ps_last_error()
        assert lib.ps_mcerr_add(X._h, big.solver._h, *args, 1) == L.PS_ERR_BAD_ARG and b'domain 257' in lib.ps_last_error()
        assert lib.ps_mcerr_add_sites(X._h, A3._h, 1) == L.PS_ERR_STATE                     # never applied
        A2.apply()
        A3.apply()
        assert lib.ps_mcerr_add_sites(X._h, A2._h, 1) == L.PS_ERR_BAD_ARG and b'has 2 outputs' in lib.ps_last_error()
        assert lib.ps_mcerr_add_sites(X._h, None, 1) == L.PS_ERR_BAD_ARG
        assert lib.ps_mcerr_add_sites(X._h, A3._h, 0) == L.PS_ERR_BAD_ARG
        for fn in (lib.ps_mcerr_finish, lib.ps_mcerr_reset):
            assert fn(None) == L.PS_ERR_BAD_ARG
        assert lib.ps_mcerr_info(None, None, None, None, None, None, None) == L.PS_ERR_BAD_ARG
        assert lib.ps_mcerr_merge(X._h, None) == L.PS_ERR_BAD_ARG and lib.ps_mcerr_merge(None, X._h) == L.PS_ERR_BAD_ARG
        assert X.members == 0 and X.profile()[1] == 0 and X.profile()[3] == 0                # nothing was enqueued
        # fewer than two batches: nothing to fetch yet
        X.add(3)
        assert (X.batches, X.open_weight) == (1, 1)
        assert lib.ps_mcerr_fetch(X._h, 0, 0, L.p_f64(out)) == L.PS_ERR_STATE and b'2 needed' in lib.ps_last_error()
        assert lib.ps_mcerr_fetch_counts(X._h, 0, 0, p1, p2) == L.PS_ERR_STATE
        X.add(1)
        Y.add(4)
        assert lib.ps_mcerr_add(X._h, pm.solver._h, *args, 0xfffffffc) == L.PS_ERR_BAD_ARG    # total weight past 2^32 - 1
        assert b'overflow' in lib.ps_last_error()
        for slot, what in ((-1, 0), (3, 0), (0, -1), (0, 3)):
            assert lib.ps_mcerr_fetch(X._h, slot, what, L.p_f64(out)) == L.PS_ERR_BAD_ARG
        for slot, k in ((3, 0), (-1, 0), (0, -1), (0, 2)):
            assert lib.ps_mcerr_fetch_counts(X._h, slot, k, p1, p2) == L.PS_ERR_BAD_ARG
        assert lib.ps_mcerr_fetch_counts(X._h, 0, 0, None, None) == L.PS_ERR_BAD_ARG
        assert lib.ps_mcerr_fetch(None, 0, 0, L.p_f64(out)) == L.PS_ERR_BAD_ARG
        # R-hat: 2..16 finished sequences with two batches each
        hs = lambda seqs: (L._VP * len(seqs))(*[s._h.value if s is not None else None for s in seqs])
        assert lib.ps_mcerr_rhat(hs([X]), 1, 0, L.p_f64(out)) == L.PS_ERR_BAD_ARG
        assert lib.ps_mcerr_rhat(hs([X] * 17), 17, 0, L.p_f64(out)) == L.PS_ERR_BAD_ARG and b'17 sequences' in lib.ps_last_error()
        assert lib.ps_mcerr_rhat(hs([X, None]), 2, 0, L.p_f64(out)) == L.PS_ERR_BAD_ARG
        assert lib.ps_mcerr_rhat(None, 2, 0, L.p_f64(out)) == L.PS_ERR_BAD_ARG
        assert lib.ps_mcerr_rhat(hs([X, Y]), 2, 3, L.p_f64(out)) == L.PS_ERR_BAD_ARG
        assert lib.ps_mcerr_rhat(hs([X, Xbig]), 2, 0, L.p_f64(out)) == L.PS_ERR_BAD_ARG
        Xbig.add(4)
        X.add(1)                                                                           # an open batch again
        assert lib.ps_mcerr_rhat(hs([X, Y]), 2, 0, L.p_f64(out)) == L.PS_ERR_STATE and b'open batch' in lib.ps_last_error()
        assert lib.ps_mcerr_rhat(hs([Y, X]), 2, 0, L.p_f64(out)) == L.PS_ERR_STATE
        X.finish()
        with MonteCarloError(pm, 2, [0, 2, 5], THR) as Z:
            Z.add(2)
            assert lib.ps_mcerr_rhat(hs([X, Z]), 2, 0, L.p_f64(out)) == L.PS_ERR_STATE and b'2 needed' in lib.ps_last_error()
        assert lib.ps_mcerr_rhat(hs([X, Y]), 2, 2, L.p_f64(out)) == L.PS_OK and not out.any()   # one member: constant
        # the handle still works: one member, weights 3 + 1 (+ 1 discarded), two batches of 2
        assert (X.batches, X.used_weight, X.discarded_weight, X.members) == (2, 4, 1, 3)
        assert X.profile()[1] == 4 and X.profile()[3] == 2                                  # pieces 2 + 1, 1, 1; two closes
        ref = _replay([cur] * 3, [3, 1, 1], THR, 2)
        _check_exact(X, ref, [0, 2, 5])
    big.close()


def test_the_grid_stride_path():
    """at R = 64 every launch is a single pass; the grid stride shows once the pairs of cells exceed the launch cap
    of 4096 x 256, from R = 724 on: R = 768, 2 days, two members, b = 1, through a release plan with a site beyond
    the grid's first pass and one on the south-east corner, so that the tail cell counts too"""
    from parasitoids_amd.predictive import ReleaseSites
    big = 768
    n = 2 * big + 1
    assert (n * n) // 2 > 4096 * 256 and (n * n) % 2 == 1
    pm = _pop_model(big, ndays=2)
    plan = [(0, 0, 1.0, 0), (700, -25, 0.5, 0), (big, big, 0.5, 0)]
    thr = [1.0, 100.0]
    fields = []
    with ReleaseSites(pm, _metres(plan, big), [0, 1]) as A, MonteCarloError.for_projection(A, 1, thr) as M:
        for mem in MEMBERS[:2]:
            _evaluate(pm, mem)
            A.apply()
            M.add(1)
            fields.append([A.field(e) for e in range(2)])
        ref = _replay(fields, [1, 1], thr, 1)
        first_pass = 2 * 4096 * 256
        # cells beyond the first pass of the grid carry values, counts and a spread between the batches
        assert (fields[0][1].ravel()[first_pass:] >= thr[0]).sum() > 0 and ref[1]['gM2'].ravel()[first_pass:].max() > 0
        assert fields[0][0][n - 1, n - 1] >= thr[1] and ref[0]['s1'][1][n - 1, n - 1] == 2
        assert (M.batches, M.used_weight) == (2, 2)
        for e in range(2):
            st = ref[e]
            assert np.array_equal(M.plane(e, 0), st['gmean'])
            for k in range(2):
                s1, s2 = M.counts(e, k)
                assert np.array_equal(s1.astype(np.uint64), st['s1'][k]) and np.array_equal(s2, st['s2'][k])
    pm.close()

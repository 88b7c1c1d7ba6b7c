"""GPU tests of the posterior dependence maps (ps_depend_*, predictive.DependenceMaps): the device mean and every
bin-sum plane bit for bit against the numpy replay (depend_ref.add of `PopModel.population(d)`), mean and M2 bit
for bit against a SpreadSummary fed alongside, the finalize and the merge against their replays, projections and
release plans as sources, the ring of cells around the plume that depends on the diffusion scale without being
correlated with it, posterior_predictive with dependence= and its saved files, and the refusals of the C ABI.
Kalbar wind, R = 128 (N = 257: N * N is odd and the pitch differs from it), 6 days, the members and weights of
test_sensitivity_gpu.py; the ring and the driver at R = 64 (N = 129, as odd).  An add launches once per 32 slots; no source has more (a projection and a plan hold at
most 32 outputs, the wind file 18 days), so every add here is one launch."""
import contextlib
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest
from scipy import sparse

import depend_ref
from helpers import HP, DP, DLP, MU_R, NPER

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.abspath(__file__))
MEMBERS = [(DP, MU_R), ((160.0, 150.0, 0.2), 1.1), ((185.0, 140.0, 0.3), 1.25), ((171.82, 160.0, 0.1), 1.0),
           ((150.0, 135.0, 0.28), 1.15)]
WEIGHTS = [1, 3, 1, 2, 1]
DAYS = list(range(6))
THREE = ['sig_x', 'sig_y', 'mu_r']
N = 257
PITCH = (N * N + 63) // 64 * 64


def _wind():
    from parasitoids_amd import ParasitoidModel as PM
    return PM.get_wind_data(os.path.join(ROOT, 'golden', 'data', 'kalbar'), 30, '00:00')


def _pop_model(R=128, first=0, ndays=6, **kw):
    from parasitoids_amd.pop_model import PopModel
    wd, days = _wind()
    return PopModel(wd, days[first:ndays], domain_info=(10000.0, R), r_number=130000, **kw)


def _evaluate(pm, member, **kw):
    dp, mu = member
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        pm.evaluate(HP, dp, DLP, mu, NPER, want_stats=False, **kw)


def _fields(pm, days=DAYS):
    return np.array([pm.population(d).toarray() for d in days])


def _names():
    from parasitoids_amd import mcmc
    return [m[0] for m in mcmc.MODEL_BLOCK]


def _member_trace(mems, repeats):
    from parasitoids_amd import mcmc
    t0 = np.array([m[2] for m in mcmc.MODEL_BLOCK])
    names = _names()
    rows = []
    for (dp, mu), n in zip(mems, repeats):
        t = t0.copy()
        t[names.index('sig_x')], t[names.index('sig_y')], t[names.index('corr_p')] = dp[0], dp[1], (dp[2] + 1) / 2
        t[names.index('mu_r')] = mu
        rows += [t] * n
    return np.array(rows), names


def _thetas(mems=MEMBERS):
    return _member_trace(mems, [1] * len(mems))[0]


def _cols(params):
    names = _names()
    return [names.index(p) for p in (names if params is None else params)]


def _spread_edges(T, params, nbin):
    """explicit edges, nbin - 1 per parameter, evenly spread strictly between its smallest and largest value, so that
    a member lands in bin 0 and one in the last bin; a parameter that never changes sits in bin 0 (even index) or
    in the last bin (odd index)"""
    out = []
    for i, c in enumerate(_cols(params)):
        lo, hi = T[:, c].min(), T[:, c].max()
        if lo == hi:
            step = max(abs(lo), 1.0)
            out.append(lo + step * np.arange(1, nbin) if i % 2 == 0 else lo - step * np.arange(nbin - 1, 0, -1))
        else:
            out.append(np.linspace(lo, hi, nbin + 1)[1:-1])
    return out


def _pooled_edges(T, weights, params, bins):
    from parasitoids_amd.predictive import dependence_edges
    return [dependence_edges(T[:, c], np.asarray(weights), bins) for c in _cols(params)]


def _planes(H, d):
    """every S[p][b] plane of day d that can hold anything, {(p, b): plane}"""
    return {(p, b): H.fetch_slot(H._slot[d], 256 + 16 * p + b) for p in range(len(H.params)) for b in range(H.nbin)}


def _eta(H, d):
    return np.array([H.ratio(d, n) for n in H.params])


@pytest.mark.parametrize('nbin', [2, 16])
@pytest.mark.parametrize('prob_model', [False, True])
def test_mean_and_bin_sums_equal_the_replay_bit_for_bit(prob_model, nbin):
    from parasitoids_amd.predictive import DependenceMaps, SpreadSummary
    pm = _pop_model(prob_model=prob_model)
    T = _thetas()
    sets = [['mu_r'], THREE, None]                         # 1, 3 and 15 parameters: below, across and two load batches
    with contextlib.ExitStack() as stack:
        S = stack.enter_context(SpreadSummary(pm, DAYS))
        Hs = [stack.enter_context(DependenceMaps(pm, p, _spread_edges(T, p, nbin), DAYS)) for p in sets]
        assert [len(H.params) for H in Hs] == [1, 3, 15] and all(H.nbin == nbin for H in Hs)
        for H in Hs:
            assert H.nbytes == ((2 + len(H.params) * nbin + len(H.params)) * 8 + 1) * 6 * PITCH
        state = [depend_ref.new_state((6, N, N), len(H.params), nbin, dense=False) for H in Hs]
        for mem, t, w in zip(MEMBERS, T, WEIGHTS):
            _evaluate(pm, mem)
            S.add(w)
            for H in Hs:
                H.add(t, w)
            f = _fields(pm)
            for H, st in zip(Hs, state):
                depend_ref.add(st, f, H.bins_of(t), w)
        if prob_model:      # the device delta is in: every kept entry carries the renormalisation
            assert any(pm.stats[d].delta != 0.0 for d in range(5))
        for H, st in zip(Hs, state):
            assert H.total_weight == float(sum(WEIGHTS)) and H.members == 5
            assert np.array_equal(H.bin_weights, st['Wb'])
            varies = [i for i in range(len(H.params)) if np.count_nonzero(st['Wb'][i]) > 1]
            assert varies and all(st['Wb'][i, 0] > 0 and st['Wb'][i, nbin - 1] > 0 for i in varies)
            assert st['Wb'][:, 0].any() and st['Wb'][:, nbin - 1].any()
            for d in DAYS:
                mean = H.mean(d)
                assert np.array_equal(mean, st['mean'][d]), (len(H.params), d)
                assert np.array_equal(mean, S.mean(d)) and np.array_equal(H.variance(d), S.variance(d))
                m2 = H.fetch_slot(H._slot[d], 3)
                assert np.array_equal(m2 / float(sum(WEIGHTS)), S.variance(d))
                for (p, b), plane in _planes(H, d).items():
                    assert np.array_equal(plane, st['S'][p, b][d]), (len(H.params), d, p, b)
                    assert plane.any() == bool(st['Wb'][p, b]), (p, b)
                # the planes of a parameter sum to W x mean, up to the rounding of the sums
                tot = sum(H.bin_sum(d, H.params[0], b) for b in range(nbin))
                np.testing.assert_allclose(tot, mean * sum(WEIGHTS), rtol=1e-13, atol=1e-300)
    pm.close()


def test_finalize_equals_its_replay_bit_for_bit():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import DependenceMaps
    pm = _pop_model()
    T = _thetas()
    params = ['sig_x', 'mu_r', 'lam']                      # the last never changes
    edges = _pooled_edges(T, WEIGHTS, params, 2)
    assert [e.size for e in edges] == [1, 1, 0]
    with DependenceMaps(pm, params, edges) as H:
        out = np.empty((N, N))
        for mem, t, w in zip(MEMBERS, T, WEIGHTS):
            _evaluate(pm, mem)
            H.add(t, w)
        for what in (2, 16, 18):
            rc = H._lib.ps_depend_fetch(H._h, 0, what, L.p_f64(out))
            assert rc == L.PS_ERR_STATE and b'not finalized' in H._lib.ps_last_error()
        H.finalize()
        assert H.bins_used('sig_x') == 2 and H.bins_used('lam') == 1
        assert H.floor('sig_x') == 0.25 and H.floor('lam') == 0.0
        for d in DAYS:
            var, mean = H.variance(d), H.mean(d)
            S = [[H.bin_sum(d, n, b) for b in range(2)] for n in params]
            eta, dom = depend_ref.finalize(mean, var, S, H.bin_weights)
            got, gd = _eta(H, d), H.dominant(d)
            assert gd.dtype == np.int8
            assert np.array_equal(got, eta), (d, np.abs(got - eta).max())
            assert np.array_equal(gd, dom), d
            assert got.min() >= 0.0 and got.max() <= 1.0
            assert not got[2].any()                        # a parameter that never changes
            assert np.all(gd[var == 0.0] == -1) and not got[:, var == 0.0].any()
            assert set(np.unique(gd)) <= {-1, 0, 1}
            adj = H.adjusted(d, 'sig_x')
            assert np.all(adj <= got[0] + 1e-15) and adj.min() >= 0.0
        assert _eta(H, 5)[:2].max() > 0.5 and H.dominant(5).max() >= 0
        _evaluate(pm, MEMBERS[1])
        H.add(T[1], 1)                                     # one more add: the result is stale
        for fetch in (lambda: H.ratio(0, 'sig_x'), lambda: H.dominant(0)):
            with pytest.raises(L.HipError) as err:
                fetch()
            assert err.value.code == L.PS_ERR_STATE
        H.finalize()
        H.ratio(0, 'mu_r')
        with DependenceMaps(pm, params, edges) as other:
            other.add(T[0], 1)
            H.merge(other)                                 # and so it is after a merge
            with pytest.raises(L.HipError) as err:
                H.dominant(0)
            assert err.value.code == L.PS_ERR_STATE
        # too few members per bin: refused on the host, the planes stay available
        H.reset()
        assert H.total_weight == 0 and not H.bin_weights.any()
        for mem, t in zip(MEMBERS[:3], T):
            _evaluate(pm, mem)
            H.add(t, 2)
        with pytest.raises(ValueError, match="3 members in 2 bins of 'sig_x'"):
            H.finalize()
        assert H.bin_sum(5, 'sig_x', 0).max() > 0
    pm.close()


def test_merge_equals_the_replay_of_the_merge_bit_for_bit():
    from parasitoids_amd.predictive import DependenceMaps
    pm = _pop_model()
    T = _thetas()
    edges = _pooled_edges(T, WEIGHTS, THREE, 2)
    with DependenceMaps(pm, THREE, edges) as all_, DependenceMaps(pm, THREE, edges) as a, \
            DependenceMaps(pm, THREE, edges) as b:
        ra, rb = (depend_ref.new_state((6, N, N), 3, 2) for _ in range(2))
        for i, (mem, t, w) in enumerate(zip(MEMBERS, T, WEIGHTS)):
            _evaluate(pm, mem)
            all_.add(t, w)
            (a if i < 2 else b).add(t, w)
            depend_ref.add(ra if i < 2 else rb, _fields(pm), a.bins_of(t), w)
        # the replay merges what the device holds: its adds give M2 as the device contracts it only on the device
        for H, st in ((a, ra), (b, rb)):
            for d in DAYS:
                assert np.array_equal(H.mean(d), st['mean'][d])
                st['M2'][d] = H.fetch_slot(d, 3)
        depend_ref.merge(ra, rb)
        a.merge(b)
        assert a.total_weight == all_.total_weight == ra['W'] and a.members == all_.members == 5
        assert np.array_equal(a.bin_weights, all_.bin_weights) and np.array_equal(a.bin_weights, ra['Wb'])
        for d in DAYS:
            assert np.array_equal(a.mean(d), ra['mean'][d]) and np.array_equal(a.fetch_slot(d, 3), ra['M2'][d])
            for (p, bb), plane in _planes(a, d).items():
                assert np.array_equal(plane, ra['S'][p, bb][d]), (d, p, bb)
            m = all_.mean(d)
            np.testing.assert_allclose(a.mean(d), m, rtol=1e-12, atol=1e-15 * np.abs(m).max())
            np.testing.assert_allclose(a.variance(d), all_.variance(d), rtol=1e-12, atol=1e-15 * np.abs(m).max() ** 2)
        a.finalize()
        all_.finalize()
        np.testing.assert_allclose(_eta(a, 5), _eta(all_, 5), rtol=0, atol=1e-9)
        # merging into an empty handle is a copy, bit for bit
        with DependenceMaps(pm, THREE, edges) as e:
            e.merge(all_)
            assert e.total_weight == all_.total_weight and e.members == 5
            assert np.array_equal(e.bin_weights, all_.bin_weights)
            for d in DAYS:
                assert np.array_equal(e.mean(d), all_.mean(d)) and np.array_equal(e.variance(d), all_.variance(d))
                assert all(np.array_equal(v, w) for v, w in zip(_planes(e, d).values(), _planes(all_, d).values()))
            keep = _planes(all_, 3)                        # and an empty source changes nothing
            with DependenceMaps(pm, THREE, edges) as none:
                all_.merge(none)
            assert all(np.array_equal(v, w) for v, w in zip(_planes(all_, 3).values(), keep.values()))
            assert all_.members == 5
        moved = [x.copy() for x in edges]
        moved[0] = moved[0] + 1.0
        with DependenceMaps(pm, THREE, moved) as other:
            with pytest.raises(ValueError, match='different days, parameters or edges'):
                a.merge(other)
        with DependenceMaps(pm, ['sig_x', 'mu_r'], edges[:2]) as other:
            with pytest.raises(ValueError, match='different days, parameters or edges'):
                a.merge(other)
    pm.close()


def test_projections_and_release_plans_as_sources():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import DependenceMaps, Projection, ReleaseSites, exposure_weights, lagged_models
    pm = _pop_model()
    T = _thetas()
    res = 10000.0 / 128
    late = lagged_models(pm, [0, 2])
    plan = [(0.0, 0.0, 0.6, 0), (13 * res, 6 * res, 0.4, 2)]      # two sites, the second released two days later
    W = exposure_weights([0, 1, 2], [0, 1, 2])
    edges = _pooled_edges(T, WEIGHTS, THREE, 2)
    with Projection(pm, W, [0, 1, 2]) as P, ReleaseSites(pm, plan, [0, 2, 3, 5], late) as RS, \
            DependenceMaps.for_projection(P, THREE, edges) as HP_, DependenceMaps.for_projection(RS, THREE, edges) as HS:
        lib = HP_._lib
        b0 = L.i32([0, 0, 0])
        assert lib.ps_depend_add_project(HP_._h, P._h, 3, L.p_i32(b0), 1) == L.PS_ERR_STATE     # nothing applied yet
        assert lib.ps_depend_add_sites(HS._h, RS._h, 3, L.p_i32(b0), 1) == L.PS_ERR_STATE
        sp, ss = depend_ref.new_state((3, N, N), 3, 2), depend_ref.new_state((4, N, N), 3, 2)
        for mem, t, w in zip(MEMBERS, T, WEIGHTS):
            _evaluate(pm, mem)
            _evaluate(late[2], mem, ndays=4)
            P.apply()
            RS.apply()
            HP_.add(t, w)
            HS.add(t, w)
            depend_ref.add(sp, np.array([P.field(k) for k in range(3)]), HP_.bins_of(t), w)
            depend_ref.add(ss, np.array([RS.field(k) for k in range(4)]), HS.bins_of(t), w)
        for H, st, n in ((HP_, sp, 3), (HS, ss, 4)):
            assert H.members == 5 and H.days == list(range(n)) and np.array_equal(H.bin_weights, st['Wb'])
            for k in range(n):
                assert np.array_equal(H.mean(k), st['mean'][k])
                for (p, b), plane in _planes(H, k).items():
                    assert np.array_equal(plane, st['S'][p, b][k]), (n, k, p, b)
            assert max(np.abs(v).max() for v in _planes(H, n - 1).values()) > 0
            H.finalize()
            e = _eta(H, n - 1)
            assert e.min() >= 0.0 and e.max() <= 1.0 and e.max() > 0.3
        # a read while a pass over the plan's groups is open is refused, and adds nowhere
        calls = RS._calls()
        L.check(lib.ps_sites_apply(RS._h, *calls[0]))
        keep = HS.bin_weights.copy()
        with pytest.raises(L.HipError) as err:
            HS.add(T[0], 1)
        assert err.value.code == L.PS_ERR_STATE and HS.members == 5 and np.array_equal(HS.bin_weights, keep)
        L.check(lib.ps_sites_apply(RS._h, *calls[1]))
        HS.add(T[0], 1)
        assert HS.members == 6 and HS.bin_weights[0].sum() == sum(WEIGHTS) + 1
    for m in (pm, late[2]):
        m.close()


def test_the_ring_around_the_plume_depends_on_the_diffusion_scale_without_correlation():
    """twelve members that differ in the diffusion scale alone: around the plume the density first rises and then
    falls with it, so the correlation is near 0 where the dependence is strong (40 cells on the CPU oracle)"""
    from parasitoids_amd.predictive import DependenceMaps, SensitivityMaps
    pm = _pop_model(R=64, ndays=2)
    sig = np.linspace(110.0, 250.0, 12)
    mems = [((s, 0.85 * s, 0.25), MU_R) for s in sig]
    T = _thetas(mems)
    params = ['sig_x', 'mu_r']
    edges = _pooled_edges(T, np.ones(12, dtype=int), params, 4)
    assert [e.size for e in edges] == [3, 0]
    n = 129
    with DependenceMaps(pm, params, edges, [0]) as H, SensitivityMaps(pm, params, [0]) as X:
        st = depend_ref.new_state((1, n, n), 2, 4)
        for mem, t in zip(mems, T):
            _evaluate(pm, mem)
            H.add(t, 1)
            X.add(t, 1)
            depend_ref.add(st, _fields(pm, [0]), H.bins_of(t), 1)
        H.finalize()
        assert H.bin_weights.tolist() == [[3, 3, 3, 3], [12, 0, 0, 0]]
        mean, var = H.mean(0), H.variance(0)
        assert np.array_equal(mean, st['mean'][0])
        # the replay on the fetched member fields; the variance is the device's, whose M2 is contracted
        eta, dom = depend_ref.finalize(st['mean'][0], var, [[st['S'][p, b][0] for b in range(4)] for p in range(2)],
                                       st['Wb'])
        got = _eta(H, 0)
        assert np.array_equal(got, eta) and np.array_equal(H.dominant(0), dom)
        r = X.correlation(0, 'sig_x')
        live = mean > 1.0
        ring = live & (r * r < 0.25) & (got[0] > 0.6)
        print('%d cells with mean > 1, %d of them with r2 < 0.25 and eta2 > 0.6; the smallest eta2 %.6f, floor %.6f'
              % (live.sum(), ring.sum(), got[0][var > 0].min(), H.floor('sig_x')))
        assert ring.sum() >= 20
        assert H.floor('sig_x') == 3 / 11
        assert got[0][var > 0].min() >= H.floor('sig_x') * (1 - 1e-9)
        assert not got[1].any()                            # mu_r never changes
        assert set(np.unique(H.dominant(0))) <= {-1, 0}
        ex = H.excess(0, 'sig_x', X)
        assert ex.min() >= 0.0 and ex[ring].min() > 0.2 and np.array_equal(ex > 0, H.adjusted(0, 'sig_x') > r * r)
    pm.close()


def _csr(f, key, n):
    return sparse.csr_matrix((f[key + '_data'], f[key + '_ind'], f[key + '_indptr']), shape=(n, n)).toarray()


def _npz_equal(a, b):
    with np.load(a) as fa, np.load(b) as fb:
        assert sorted(fa.files) == sorted(fb.files), (a, b)
        for k in fa.files:
            assert np.array_equal(fa[k], fb[k]), (a, k)


def _close(*results):
    for r in results:
        for fs in (r, r.exposure, r.sites):
            if fs is not None:
                for acc in (fs.summary, fs.sensitivity, fs.dependence):
                    if acc is not None:
                        acc.close()


# the driver tests run at R = 64 (N = 129: N * N is odd too, and the pitch differs from it)
DRIVER_DAYS = [0, 2, 5]
DRIVER_PARAMS = ['sig_x', 'mu_r']


def test_the_driver_equals_a_hand_fed_handle_and_saves(tmp_path):
    from parasitoids_amd import mcmc
    from parasitoids_amd.predictive import DependenceMaps, posterior_predictive
    days, params, n = DRIVER_DAYS, DRIVER_PARAMS, 129
    tr = _member_trace(MEMBERS, WEIGHTS)
    pa, pc = _pop_model(R=64), _pop_model(R=64)
    a = posterior_predictive(pa, tr, days=days, thresholds=(1.0,), sensitivity=params,
                             dependence=dict(params=params, bins=2))
    D = a.dependence
    assert D.params == params and D.members == 5 and D.total_weight == 8 and D.days == days and D.nbin == 2
    T = _thetas()
    edges = _pooled_edges(T, WEIGHTS, params, 2)           # pooled over the rows: the runs with their lengths
    assert all(np.array_equal(x, y) for x, y in zip(D.edges, edges))
    with DependenceMaps(pc, params, edges, days) as hand:
        for t, w in zip(T, WEIGHTS):                       # the driver's evaluation: the model block alone
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                pc.evaluate(*mcmc.model_args(t), want_stats=False)
            hand.add(t, w)
        hand.finalize()
        npz, js = a.save(str(tmp_path / 'out' / 'pp'), {'site': 'kalbar'})      # finalizes the maps it writes
        assert np.array_equal(D.bin_weights, hand.bin_weights)
        for d in days:
            assert np.array_equal(D.mean(d), hand.mean(d)) and np.array_equal(D.mean(d), a.summary.mean(d))
            assert np.array_equal(D.variance(d), a.summary.variance(d))
            assert np.array_equal(_eta(D, d), _eta(hand, d)) and np.array_equal(D.dominant(d), hand.dominant(d))
            assert all(np.array_equal(v, w) for v, w in zip(_planes(D, d).values(), _planes(hand, d).values()))
    with np.load(str(tmp_path / 'out' / 'pp_depend.npz')) as f:
        assert list(f['days']) == [pa.days[d] for d in days]
        for d in days:
            label = str(pa.days[d])
            assert f[label + '_dom'].dtype == np.int8 and np.array_equal(f[label + '_dom'], D.dominant(d))
            for name in params:
                e = D.ratio(d, name)
                assert np.array_equal(_csr(f, '%s_eta2_%s' % (label, name), n), np.where(e >= 1e-8, e, 0.0))
                x = D.excess(d, name, a.sensitivity)
                assert np.array_equal(_csr(f, '%s_excess_%s' % (label, name), n), np.where(x >= 1e-8, x, 0.0))
        assert _csr(f, str(pa.days[5]) + '_eta2_sig_x', n).max() > 0.3
    blk = json.load(open(js))['predictive']['dependence']
    assert blk['params'] == params and blk['bins'] == 2 and blk['bins_used'] == [2, 2] and blk['finalized'] is True
    assert blk['members'] == 5 and blk['total_weight'] == 8 and 'reason' not in blk
    assert blk['edges'] == [e.tolist() for e in edges] and blk['floor'] == [0.25, 0.25]
    assert blk['bin_weights'] == D.bin_weights.tolist() and all(sum(r) == 8 for r in blk['bin_weights'])
    _close(a)
    for p in (pa, pc):
        p.close()


def test_the_driver_gives_projections_and_plans_their_own_and_changes_nothing_else(tmp_path):
    from parasitoids_amd.predictive import posterior_predictive
    days, params = DRIVER_DAYS, DRIVER_PARAMS
    tr = _member_trace(MEMBERS, WEIGHTS)
    res = 10000.0 / 64
    kw = dict(days=days, thresholds=(1.0,), sensitivity=params, exposure=[2, 5],
              sites=dict(sites=[(0.0, 0.0, 0.6), (7 * res, 3 * res, 0.4, 2)], days=[0, 2, 5]))
    pa, pb = _pop_model(R=64), _pop_model(R=64)
    a = posterior_predictive(pa, tr, dependence=dict(params=params, bins=2), **kw)
    b = posterior_predictive(pb, tr, **kw)
    assert b.dependence is None and b.exposure.dependence is None and b.sites.dependence is None
    npz, js = a.save(str(tmp_path / 'with' / 'pp'), {'site': 'kalbar'})
    b.save(str(tmp_path / 'without' / 'pp'), {'site': 'kalbar'})
    for owner in (a.exposure, a.sites):
        own = owner.dependence
        assert own is not None and own.members == 5 and own.params == params
        assert all(np.array_equal(x, y) for x, y in zip(own.edges, a.dependence.edges))
        assert np.array_equal(own.mean(1), owner.summary.mean(1)) and own.ratio(1, 'sig_x').max() > 0.3
    assert a.sites.dependence.days == [0, 1, 2] and a.exposure.dependence.days == [0, 1]
    with np.load(str(tmp_path / 'with' / 'pp_exposure_depend.npz')) as f:
        assert list(f['days']) == [2, 5] and '5_eta2_sig_x_data' in f and '2_excess_mu_r_data' in f and '2_dom' in f
    with np.load(str(tmp_path / 'with' / 'pp_sites_depend.npz')) as f:
        assert list(f['days']) == [0, 2, 5] and '5_eta2_mu_r_data' in f and '0_dom' in f
    meta = json.load(open(js))['predictive']
    assert meta['exposure']['dependence']['finalized'] is True and meta['sites']['dependence']['params'] == params
    # every other saved map is the same with and without dependence=
    other = json.load(open(str(tmp_path / 'without' / 'pp.json')))['predictive']
    assert 'dependence' not in other and 'dependence' not in other['sites']
    for cut in (meta, meta['exposure'], meta['sites']):
        cut.pop('dependence')
    assert meta == other
    names = sorted(os.listdir(str(tmp_path / 'without')))
    assert sorted(x for x in os.listdir(str(tmp_path / 'with')) if '_depend' not in x) == names and len(names) >= 6
    for x in names:
        if x.endswith('.npz'):
            _npz_equal(str(tmp_path / 'with' / x), str(tmp_path / 'without' / x))
    _close(a, b)
    for p in (pa, pb):
        p.close()


def test_the_driver_reports_why_finalize_refused(tmp_path):
    """three members in two bins: the reason in the json, no ratio maps"""
    from parasitoids_amd.predictive import posterior_predictive
    days = DRIVER_DAYS
    pd = _pop_model(R=64)
    few = posterior_predictive(pd, _member_trace(MEMBERS[:3], [2, 1, 3]), days=days, thresholds=(1.0,),
                               dependence=dict(params=['sig_x'], bins=2))
    npz, js = few.save(str(tmp_path / 'few'))
    blk = json.load(open(js))['predictive']['dependence']
    assert blk['finalized'] is False and "3 members in 2 bins of 'sig_x'" in blk['reason'] and blk['bins_used'] == [2]
    assert blk['members'] == 3 and blk['total_weight'] == 6
    with np.load(str(tmp_path / 'few_depend.npz')) as f:
        assert not [k for k in f.files if 'eta2' in k or '_dom' in k] and list(f['days']) == [pd.days[d] for d in days]
    _close(few)
    pd.close()


def test_c_abi_refusals():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import NEGVAL, DependenceMaps, _day_scales
    pm = _pop_model()
    _evaluate(pm, MEMBERS[0])
    lib = L.load()
    T = _thetas()

    def refused(rc, code, *words):
        msg = lib.ps_last_error()
        assert rc == code, (rc, msg)
        for w in words:
            assert w in msg, msg

    h = L._VP()
    for nparam, nbin in ((3, 1), (3, 17), (0, 4), (17, 4)):
        refused(lib.ps_depend_create(0, N, 3, nparam, nbin, C.byref(h)), L.PS_ERR_BAD_ARG, b'depend_create', b'bins')
    refused(lib.ps_depend_create(0, N, 0, 3, 4, C.byref(h)), L.PS_ERR_BAD_ARG, b'depend_create')
    refused(lib.ps_depend_create(0, 801, 200000, 16, 16, C.byref(h)), L.PS_ERR_OOM, b'depend_create', b'GB free')
    assert not h
    edges = _spread_edges(T, THREE, 4)
    with DependenceMaps(pm, THREE, edges, [0, 1, 2]) as H:
        out = np.empty((N, N))
        refused(lib.ps_depend_fetch(H._h, 0, 0, L.p_f64(out)), L.PS_ERR_STATE, b'nothing accumulated')
        refused(lib.ps_depend_finalize(H._h, 3, 4, L.p_f64(L.f64(np.zeros((3, 4))))), L.PS_ERR_STATE,
                b'nothing accumulated')
        stat, post = _day_scales(pm, H.days)

        def add(nslot=3, nparam=3, bins=(0, 3, 1), w=1):
            b = L.i32(bins)
            return lib.ps_depend_add(H._h, pm.solver._h, nslot, L.p_i32(H._kind), L.p_i32(H._idx), L.p_f64(stat),
                                     L.p_f64(post), L.p_i32(H._delta), NEGVAL, nparam, L.p_i32(b), w)
        assert add() == L.PS_OK and H.members == 1
        info = H._info()
        plane = H.fetch_slot(2, 256 + 16 * 1 + 3)
        assert plane.any()

        def unchanged():
            assert H._info() == info and np.array_equal(H.fetch_slot(2, 256 + 16 * 1 + 3), plane)
            assert not H.fetch_slot(2, 256 + 16 * 1 + 0).any()
        refused(add(bins=(0, 4, 1)), L.PS_ERR_BAD_ARG, b'bin[1] = 4', b'0..3')
        unchanged()
        refused(add(bins=(-1, 3, 1)), L.PS_ERR_BAD_ARG, b'bin[0] = -1')
        unchanged()
        refused(add(w=0), L.PS_ERR_BAD_ARG, b'weight must be >= 1')
        unchanged()
        refused(add(nparam=2), L.PS_ERR_BAD_ARG, b'2 parameters given', b'has 3')
        unchanged()
        refused(add(nslot=2), L.PS_ERR_BAD_ARG, b'2 slots given', b'has 3')
        unchanged()
        refused(add(w=0xffffffff), L.PS_ERR_BAD_ARG, b'total weight 4294967296', b'2^32')
        unchanged()
        # finalize: the bin weights have to be the handle's shape, integers, and sum to the total weight
        Wb = np.zeros((3, 4))
        Wb[0, 0] = Wb[1, 3] = Wb[2, 1] = 1.0
        refused(lib.ps_depend_finalize(H._h, 2, 4, L.p_f64(L.f64(Wb))), L.PS_ERR_BAD_ARG, b'3 parameters x 4 bins')
        refused(lib.ps_depend_finalize(H._h, 3, 3, L.p_f64(L.f64(Wb))), L.PS_ERR_BAD_ARG, b'3 parameters x 4 bins')
        for bad in (0.5, -1.0, np.nan, 2.0 ** 32):
            Wx = Wb.copy()
            Wx[1, 3] = bad
            refused(lib.ps_depend_finalize(H._h, 3, 4, L.p_f64(L.f64(Wx))), L.PS_ERR_BAD_ARG, b'Wb[1][3]')
        Wx = Wb.copy()
        Wx[2, 2] = 1.0
        refused(lib.ps_depend_finalize(H._h, 3, 4, L.p_f64(L.f64(Wx))), L.PS_ERR_BAD_ARG, b'parameter 2 sum to 2')
        for what in (2, 16, 18):
            refused(lib.ps_depend_fetch(H._h, 0, what, L.p_f64(out)), L.PS_ERR_STATE, b'not finalized')
        refused(lib.ps_depend_fetch(H._h, 3, 0, L.p_f64(out)), L.PS_ERR_BAD_ARG, b'slot 3 of 3')
        for what in (4, 15, 19, -1, 255, 256 + 4, 256 + 16 * 3, 256 + 16 * 2 + 15):
            refused(lib.ps_depend_fetch(H._h, 0, what, L.p_f64(out)), L.PS_ERR_BAD_ARG, b'quantity')
        assert lib.ps_depend_finalize(H._h, 3, 4, L.p_f64(L.f64(Wb))) == L.PS_OK
        assert lib.ps_depend_fetch(H._h, 0, 2, L.p_f64(out)) == L.PS_OK and set(np.unique(out)) <= {-1.0}
        assert lib.ps_depend_fetch(H._h, 0, 16, L.p_f64(out)) == L.PS_OK and not out.any()    # one member: one bin
        unchanged()
        refused(lib.ps_depend_merge(H._h, H._h), L.PS_ERR_BAD_ARG, b'same handle')
        with DependenceMaps(pm, THREE, _spread_edges(T, THREE, 2), [0, 1, 2]) as H2:
            refused(lib.ps_depend_merge(H._h, H2._h), L.PS_ERR_BAD_ARG, b'3 parameters x 4 bins', b'3 x 2')
        with DependenceMaps(pm, THREE, edges, [0, 1]) as H2:
            refused(lib.ps_depend_merge(H._h, H2._h), L.PS_ERR_BAD_ARG, b'dst has 3 slots, src 2')
        unchanged()
        # the wrapper
        with pytest.raises(ValueError, match='theta has 3 entries'):
            H.add([1.0, 2.0, 3.0])
        with pytest.raises(ValueError, match='positive integer'):
            H.add(T[0], 0)
        assert H._members == 0 and not H.bin_weights.any()      # the C calls above went past the wrapper
        with pytest.raises(ValueError, match='is not among'):
            H.ratio(0, 'lam')
        with pytest.raises(ValueError, match='day 4 is not in'):
            H.mean(4)
        with pytest.raises(ValueError, match='strictly increasing'):
            DependenceMaps(pm, ['sig_x'], [[2.0, 1.0]])
        with pytest.raises(ValueError, match='1 lists of edges for 3'):
            DependenceMaps(pm, THREE, [[1.0]])
    refused(lib.ps_depend_reset(None), L.PS_ERR_BAD_ARG, b'null handle')
    refused(lib.ps_depend_info(None, None, None), L.PS_ERR_BAD_ARG, b'null handle')
    pm.close()

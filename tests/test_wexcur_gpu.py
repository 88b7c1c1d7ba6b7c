"""GPU tests of the reweighted excursion regions (ps_wexcur_*, predictive.ReweightedExcursion,
ExcursionMaps.reweighted): the weighted counts, the members' bounds, the three excursion functions, the probability,
the region maps and the areas bit for bit against the numpy reference (wexcur_ref) built from
`PopModel.population(d)`; the integer tie to the parent ExcursionMaps; members dropped at -inf against maps fed
the others only; 67 members with 67 different log-weights; that steep weights do move the region; the same bits on
repeat; a parent that gained a member; the refusals; a release plan as the parent; and posterior_predictive with
maps=('excursion',).  Kalbar wind, R = 128, 6 days: N = 257, N * N = 1032 * 64 + 1, so the last mask word holds one
real cell and 63 pad bits.  The members, weights and helpers of test_arrival_gpu.py; every member is evaluated once,
in the module's fixture."""
import ctypes as C
import json
import math
import os
import warnings

import numpy as np
import pytest

import excur_ref as R
import wexcur_ref as WR
import test_arrival_gpu as TA
from sites_ref import plan_fields

pytestmark = pytest.mark.gpu

MEMBERS, WEIGHTS, THR = TA.MEMBERS, TA.WEIGHTS, TA.THR
_pop_model, _evaluate, _fields = TA._pop_model, TA._evaluate, TA._fields
LEVELS = (0.51, 0.9, 1.0)
INF = math.inf
MILD = [0.0, -0.3, 0.2, -0.1, 0.4]
STEEP = [-6.0, 0.0, -INF, -9.0, -3.0]
KEPT = [0, 2, 4]
MANY = 67
OWNER = [i * len(MEMBERS) // MANY for i in range(MANY)]     # the evaluation behind each of the 67 adds
N_MANY = [1 + (i % 3) for i in range(MANY)]
LW_MANY = [float(v) for v in np.random.default_rng(67).normal(0.0, 2.0, MANY)]


@pytest.fixture(scope='module')
def world():
    """every member evaluated once: the plain maps E, maps of KEPT alone, a parent the staleness test may add to and
    one of 67 adds; `fields` [member][day, N, N]"""
    from parasitoids_amd.predictive import ExcursionMaps
    pm = _pop_model()
    days = list(range(6))
    E, sub, spare, many = (ExcursionMaps(pm, THR) for _ in range(4))
    fields = []
    for m, (mem, w) in enumerate(zip(MEMBERS, WEIGHTS)):
        _evaluate(pm, mem)
        E.add(w)
        spare.add(w)
        if m in KEPT:
            sub.add(w)
        for i in range(MANY):
            if OWNER[i] == m:
                many.add(N_MANY[i])
        fields.append(_fields(pm, days))
    assert many.members == MANY and len(set(LW_MANY)) == MANY and sorted(set(OWNER)) == list(range(len(MEMBERS)))
    yield {'pm': pm, 'E': E, 'sub': sub, 'spare': spare, 'many': many, 'fields': fields, 'days': days}
    for acc in (E, sub, spare, many):
        acc.close()
    pm.close()


def _check_against_reference(RW, fields, n, lw, thr, days=None):
    """every device output of RW against the numpy reference of the members' [nslot, N, N] fields"""
    X = np.asarray(fields)
    N = RW.N
    w = WR.member_weights(n, lw)
    assert RW.weights.dtype == np.float64 and np.array_equal(RW.weights, w)
    assert RW.total == WR.total(w) and RW.ess == float(w.sum()) ** 2 / float((w * w).sum())
    for k, t in enumerate(thr):
        for s, d in enumerate(RW.days):
            if days is not None and d not in days:
                continue
            P = WR.plane(X[:, s], n, lw, t)
            got = RW.counts(k, d)
            assert got.dtype == np.float64 and got.shape == (N, N) and np.array_equal(got, P['C']), (k, d)
            hi, lo = RW.bounds(k, d)
            assert hi.dtype == lo.dtype == np.float64
            assert np.array_equal(hi, P['hi']) and np.array_equal(lo, P['lo']), (k, d)
            maps = {'above': RW.above(k, d), 'below': RW.below(k, d), 'contour': RW.contour(k, d),
                    'prob': RW.prob(k, d)}
            for name, m in maps.items():
                assert m.dtype == np.float64 and np.array_equal(m, P[name]), (name, k, d)
            for level in LEVELS:
                reg = RW.region(k, d, level)
                assert reg.dtype == np.int8 and np.array_equal(reg, R.region(P['above'], P['below'], level)), (k, d, level)
            assert RW.areas(k, d, LEVELS) == R.areas(P['above'], P['below'], P['contour'], LEVELS, RW.cell_area)


def _all_maps(X):
    out = []
    for k in range(len(X.thresholds)):
        for d in X.days:
            out += [X.above(k, d), X.below(k, d), X.contour(k, d)]
    return out


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('lw', [MILD, STEEP], ids=['mild', 'steep'])
def test_device_maps_match_the_numpy_reference(world, lw):
    E = world['E']
    with E.reweighted(lw) as RW:
        assert RW.N == 257 and RW.pitch == 1033 * 64 and RW.days == world['days'] and RW.thresholds == THR
        assert RW.run_lengths.tolist() == WEIGHTS
        _check_against_reference(RW, world['fields'], WEIGHTS, lw, THR)
        assert RW.nbytes == 2 * 1033 * 64 * 8 + 3 * 64 * 8
    if lw is STEEP:
        assert RW.weights[2] == 0.0 and RW.ess < 1.2


@pytest.mark.parametrize('level', [0.0, -700.0])
def test_equal_log_weights_hold_the_bits_of_the_parent(world, level):
    E = world['E']
    with E.reweighted([level] * len(WEIGHTS)) as RW:
        assert RW.weights.tolist() == [float(w) for w in WEIGHTS] and RW.total == float(sum(WEIGHTS))
        assert _same(_all_maps(RW), _all_maps(E))
        for k in range(len(THR)):
            for d in E.days:
                assert np.array_equal(RW.counts(k, d), E.counts(k, d).astype(np.float64)), (k, d)
                hi, lo, _w = E.bounds(k, d)
                got = RW.bounds(k, d)
                assert np.array_equal(got[0], hi.astype(np.float64))
                assert np.array_equal(got[1], np.where(lo == R.NONE, np.inf, lo.astype(np.float64)))
                for p in LEVELS:
                    assert np.array_equal(RW.region(k, d, p), E.region(k, d, p))
                assert RW.areas(k, d, LEVELS) == E.areas(k, d, LEVELS)


def test_members_at_minus_infinity_hold_the_bits_of_maps_fed_the_others(world):
    E, sub = world['E'], world['sub']
    lw = [0.0 if m in KEPT else -INF for m in range(len(WEIGHTS))]
    with E.reweighted(lw) as RW:
        assert RW.total == float(sum(WEIGHTS[m] for m in KEPT)) == sub.total_weight
        assert _same(_all_maps(RW), _all_maps(sub))
        for k in range(len(THR)):
            for d in E.days:
                assert np.array_equal(RW.counts(k, d), sub.counts(k, d).astype(np.float64)), (k, d)
        # a dropped member keeps its bounds on the others' counts
        hi, lo = RW.bounds(1, 3)
        P = WR.plane(np.asarray(world['fields'])[:, 3], WEIGHTS, lw, THR[1])
        assert np.array_equal(hi, P['hi']) and np.array_equal(lo, P['lo']) and np.isfinite(lo[1])


def test_sixty_seven_members_cross_every_unroll_of_the_member_loops(world):
    many = world['many']
    X = [world['fields'][OWNER[i]] for i in range(MANY)]
    with many.reweighted(LW_MANY) as RW:
        assert RW.weights.size == MANY and RW.run_lengths.tolist() == N_MANY
        _check_against_reference(RW, X, N_MANY, LW_MANY, THR, days=[1, 5])
        assert RW.nbytes == 2 * 1033 * 64 * 8 + 3 * 128 * 8


def test_steep_weights_move_the_surely_reached_region(world):
    E = world['E']
    with E.reweighted(STEEP) as RW:
        moved = [int(((RW.above(1, d) >= 0.9) != (E.above(1, d) >= 0.9)).sum()) for d in E.days]
    assert max(moved) >= 1, moved


def test_the_same_call_gives_the_same_bits_and_one_plane_build_serves_its_maps(world):
    E = world['E']
    with E.reweighted(MILD) as RW:
        RW.profile(True)
        first = [RW.above(0, 1), RW.below(0, 1), RW.contour(0, 1), RW.prob(0, 1), RW.counts(0, 1)]
        _c, nc, _b, nb, _m, nm = RW.profile()
        assert (nc, nb, nm) == (1, 1, 4)                      # the three maps and prob rest on one plane build
        again = [RW.above(0, 1), RW.below(0, 1), RW.contour(0, 1), RW.prob(0, 1), RW.counts(0, 1)]
        assert _same(first, again) and RW.profile()[1] == 1
        other = RW.above(1, 4)                                # another plane in between
        assert not np.array_equal(other, first[0])
        third = [RW.above(0, 1), RW.below(0, 1), RW.contour(0, 1), RW.prob(0, 1), RW.counts(0, 1)]
        assert _same(first, third) and RW.profile()[1] == 3
        times = RW.profile()
        assert times[0] > 0.0 and times[2] > 0.0 and times[4] > 0.0


def test_a_further_add_on_the_parent_is_refused_with_a_clear_message(world):
    from parasitoids_amd import _lib as L
    spare = world['spare']
    lib = L.load()
    out = np.empty((257, 257))
    with spare.reweighted(MILD) as RW:
        before = RW.above(1, 2)
        spare.add(1)                                          # the last evaluation once more: a sixth member
        for call in (lambda: RW.above(1, 2), lambda: RW.counts(1, 2), lambda: RW.bounds(0, 0), lambda: RW.prob(1, 3)):
            with pytest.raises(ValueError, match='take a new reweighted'):
                call()
        # the library refuses on its own: the plane was formed over five members
        assert lib.ps_wexcur_map(RW._h, 0, L.p_f64(out)) == L.PS_ERR_STATE and b'5 members' in lib.ps_last_error()
        assert lib.ps_wexcur_fetch_counts(RW._h, L.p_f64(out)) == L.PS_ERR_STATE
        with pytest.raises(ValueError, match='6 members'):
            spare.reweighted(MILD)
        with spare.reweighted(MILD + [-INF]) as RW6:          # the new member without weight: the maps of before
            assert np.array_equal(RW6.above(1, 2), before)
    assert not RW._h and not RW6._h


def test_refusals_enqueue_nothing_and_the_device_stays_usable(world):
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import ExcursionMaps
    E = world['E']
    lib = L.load()
    out = np.empty((257, 257))
    for bad in ([0.0] * 4, [0.0] * 6, [0.0, math.nan, 0.0, 0.0, 0.0], [0.0, INF, 0.0, 0.0, 0.0], [-INF] * 5):
        with pytest.raises(ValueError):
            E.reweighted(bad)
    with pytest.raises(ValueError):
        E.reweighted(np.zeros((5, 1)))
    h = L._VP()
    assert lib.ps_wexcur_create(L.default_device(), 129, E._h, C.byref(h)) == L.PS_ERR_BAD_ARG and not h
    with ExcursionMaps(world['pm'], THR) as empty:
        with pytest.raises(ValueError):
            empty.reweighted([])
    with E.reweighted(MILD) as RW:
        RW.profile(True)
        assert lib.ps_wexcur_map(RW._h, 0, L.p_f64(out)) == L.PS_ERR_STATE          # no current plane yet
        assert lib.ps_wexcur_fetch_bounds(RW._h, None, None) == L.PS_ERR_STATE
        want = RW.above(1, 3)
        launches = RW.profile()[1::2]
        w = RW.weights

        def plane(k, slot, weights):
            a = np.ascontiguousarray(weights, dtype=np.float64)
            return lib.ps_wexcur_plane(RW._h, k, slot, a.size, L.p_f64(a))
        assert plane(1, 3, w[:4]) == L.PS_ERR_BAD_ARG and b'members' in lib.ps_last_error()
        assert plane(1, 3, np.append(w, 1.0)) == L.PS_ERR_BAD_ARG
        for bad in (-1.0, math.nan, INF, -INF):
            v = w.copy()
            v[3] = bad
            assert plane(1, 3, v) == L.PS_ERR_BAD_ARG and b'weight 3' in lib.ps_last_error(), bad
        assert plane(1, 3, np.zeros(5)) == L.PS_ERR_BAD_ARG and b'every weight is 0' in lib.ps_last_error()
        for k, slot in ((-1, 0), (2, 0), (0, -1), (0, 6)):
            assert plane(k, slot, w) == L.PS_ERR_BAD_ARG, (k, slot)
        assert lib.ps_wexcur_map(RW._h, 4, L.p_f64(out)) == L.PS_ERR_BAD_ARG
        assert lib.ps_wexcur_map(RW._h, -1, L.p_f64(out)) == L.PS_ERR_BAD_ARG
        n = np.empty(4, dtype=np.uint32)
        assert lib.ps_wexcur_member_weights(RW._h, 4, n.ctypes.data_as(C.POINTER(C.c_uint32))) == L.PS_ERR_BAD_ARG
        # nothing was enqueued, the current plane is the one of before and the handle works on
        assert RW.profile()[1::2] == launches
        assert lib.ps_wexcur_map(RW._h, 0, L.p_f64(out)) == L.PS_OK and np.array_equal(out, want)
        with pytest.raises(ValueError):
            RW.above(2, 0)
        with pytest.raises(ValueError):
            RW.above(0, 6)
        with pytest.raises(ValueError):
            RW.region(0, 1, 0.5)
        assert np.array_equal(RW.above(1, 3), want)
        _check_against_reference(RW, world['fields'], WEIGHTS, MILD, THR, days=[5])


def test_a_release_plan_as_the_parent():
    from parasitoids_amd.predictive import ExcursionMaps, ReleaseSites, lagged_models
    Rr = 64
    res = 10000.0 / Rr
    pm = _pop_model(R=Rr)
    out = [0, 1, 2, 3, 5]
    sites = [(0.0, 0.0, 0.6, 0), (13 * res, 6 * res, 0.5, 2)]          # the second site two days later
    late = lagged_models(pm, [2])
    lw = [-0.5, 0.0, -2.0]
    plan_f = []
    with ReleaseSites(pm, sites, out, late) as S, ExcursionMaps.for_projection(S, THR) as ES:
        cells = [(s['drow'], s['dcol'], s['amount'], s['lag']) for s in S.sites]
        for mem, w in zip(MEMBERS[:3], WEIGHTS[:3]):
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                S.evaluate(TA.HP, mem[0], TA.DLP, mem[1], TA.NPER)
            ES.add(w)
            plan_f.append(plan_fields({0: _fields(pm, list(range(6))), 2: _fields(late[2], list(range(4)))}, cells, out))
        RW = ES.reweighted(lw)
        assert RW.days == out and RW.N == 129
        _check_against_reference(RW, plan_f, WEIGHTS[:3], lw, THR)
    assert not RW._h                                          # closed with its maps
    for m in late.values():
        m.close()
    pm.close()


def _csr(f, key, N):
    from scipy import sparse
    return sparse.csr_matrix((f[key + '_data'], f[key + '_ind'], f[key + '_indptr']), shape=(N, N)).toarray()


def _npz_equal(a, b):
    fa, fb = np.load(a), np.load(b)
    return sorted(fa.files) == sorted(fb.files) and all(np.array_equal(fa[k], fb[k]) for k in fa.files)


def test_posterior_predictive_with_the_excursion_option(tmp_path):
    from parasitoids_amd import mcmc
    from parasitoids_amd import predictive as PR
    from test_reweight_gpu import _chain
    N = 257
    res_m = 10000.0 / 128
    lengths = [3, 2, 4, 3]
    trace, names = _chain(lengths)
    chain = (trace, names)
    given = [(0, 0, 1, 'count', 1e-3, 3), (3000, 0, 2, 'none', 0.5)]
    tilt = np.repeat([0.0, 1.5, -0.75, 2.5], lengths) + 0.01 * np.random.default_rng(4).normal(size=12)
    rw = {'trap': dict(probes=given), 'tilt': dict(log_weights=[tilt]), 'options': dict(min_ess=0)}
    out = [0, 2, 3, 5]
    kw = dict(thresholds=THR, excursion=dict(thresholds=THR, levels=(0.9,)),
              sites=dict(sites=[(0.0, 0.0, 0.6), (13 * res_m, 6 * res_m, 0.5, 2)], days=out))
    pm = _pop_model(mode='exact')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        plain = PR.posterior_predictive(pm, chain, reweight=dict(rw), **kw)
        res = PR.posterior_predictive(pm, chain, reweight=dict(rw, options=dict(min_ess=0, maps=('excursion',))), **kw)
    assert plain.reweight_excursion is None and plain.sites.reweight_excursion is None
    assert 'maps' not in plain.reweight_info and res.reweight_info['maps'] == ['excursion']
    RX, SX = res.reweight_excursion, res.sites.reweight_excursion
    assert list(RX) == list(SX) == ['trap', 'tilt']
    assert RX['tilt'].excursion is res.excursion and SX['tilt'].excursion is res.sites.excursion
    assert RX['tilt'].days == list(range(6)) and SX['tilt'].days == out
    # by hand: every run once more through the model, the probes from the device's own gathered values
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    prow, pcol = [128, 128], [128, 128 + int(np.around(3000 / res_m))]
    lam = {'trap': [], 'tilt': []}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        with PR.ReleaseSites.with_lagged_models(pm, kw['sites']['sites'], out) as P:
            for ci, first, length in res.runs:
                P.evaluate(*mcmc.model_args(trace[first, cols]))
                got = pm.gather_days([1, 2], prow, pcol)
                lam['trap'].append(PR.probes_loglik(PR.check_probes(given, 10000.0, 128), [got[0, 0], got[1, 1]]))
                lam['tilt'].append(PR.run_log_weight(tilt[first:first + length]))
    assert [r[2] for r in res.runs] == lengths
    for parent, rx in ((res.excursion, RX), (res.sites.excursion, SX)):
        for name in ('trap', 'tilt'):
            got = rx[name]
            assert got.log_weights.tolist() == lam[name] and got.run_lengths.tolist() == lengths
            assert np.array_equal(got.weights, WR.member_weights(lengths, lam[name]))
            with PR.ReweightedExcursion(parent, lam[name]) as hand:
                assert _same(_all_maps(got), _all_maps(hand)) and hand.total == got.total and hand.ess == got.ess
    assert not np.array_equal(RX['tilt'].above(1, 5), res.excursion.above(1, 5))
    # the files
    plain.save(str(tmp_path / 'p' / 'pp'))
    res.save(str(tmp_path / 'm' / 'pp'))
    new = ['pp_reweight_excur.npz', 'pp_sites_reweight_excur.npz']
    old = sorted(os.listdir(str(tmp_path / 'p')))
    assert sorted(os.listdir(str(tmp_path / 'm'))) == sorted(old + new) and not set(old) & set(new)
    for name in old:                                   # every file the option does not name holds what it held
        if name.endswith('.npz'):
            assert _npz_equal(str(tmp_path / 'p' / name), str(tmp_path / 'm' / name)), name
    jp = json.load(open(str(tmp_path / 'p' / 'pp.json')))
    jm = json.load(open(str(tmp_path / 'm' / 'pp.json')))
    assert 'excursion' not in jp['predictive']['reweight'] and 'reweight' not in jp['predictive']['sites']
    meta = jm['predictive']['reweight']
    assert meta.pop('maps') == ['excursion']
    block = meta.pop('excursion')
    sblock = jm['predictive']['sites'].pop('reweight')['excursion']
    assert jm == jp                                    # but for the new keys the json is what it was
    assert block['scenarios'] == ['trap', 'tilt'] and block['thresholds'] == THR and block['levels'] == [0.9]
    assert block['days'] == list(range(6)) and sblock['days'] == out
    for name in ('trap', 'tilt'):
        assert block['scenario'][name]['ess'] == RX[name].ess and block['scenario'][name]['members'] == 4
        assert block['scenario'][name]['total_weight'] == RX[name].total
        assert block['scenario'][name]['areas'][1][5] == {'day': 5, 'levels': RX[name].areas(1, 5, [0.9])}
        assert sblock['scenario'][name]['areas'][0][2] == {'day': 3, 'levels': SX[name].areas(0, 3, [0.9])}
    for path, rx, days in (('pp_reweight_excur.npz', RX, list(range(6))), ('pp_sites_reweight_excur.npz', SX, out)):
        f = np.load(str(tmp_path / 'm' / path))
        assert [str(n) for n in f['wexcur_scenarios']] == ['trap', 'tilt'] and f['wexcur_days'].tolist() == days
        assert f['wexcur_thresholds'].tolist() == THR and f['days'].tolist() == days
        assert f['wexcur_counts'].shape == (2, 2, len(days), N, N) and f['wexcur_counts'].dtype == np.float64
        assert f['wexcur_hi'].shape == f['wexcur_lo'].shape == (2, 2, len(days), 4)
        for j, name in enumerate(('trap', 'tilt')):
            X = rx[name]
            assert np.array_equal(f['wexcur_weights'][j], X.weights)
            for k in range(2):
                for s, d in enumerate(days):
                    for what in ('above', 'below', 'contour'):
                        m = getattr(X, what)(k, d)
                        assert np.array_equal(_csr(f, '%s_s%d_%s%d' % (d, j, what, k), N), np.where(m >= 1e-8, m, 0.0))
                    reg = f['%s_s%d_region%d_l90' % (d, j, k)]
                    assert reg.dtype == np.int8 and np.array_equal(reg, X.region(k, d, 0.9))
                    assert np.array_equal(f['wexcur_counts'][j, k, s], X.counts(k, d))
                    hi, lo = X.bounds(k, d)
                    assert np.array_equal(f['wexcur_hi'][j, k, s], hi) and np.array_equal(f['wexcur_lo'][j, k, s], lo)
    pm.close()

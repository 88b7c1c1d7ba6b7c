"""GPU tests of the joint excursion sets (ps_excur_*, predictive.ExcursionMaps): every mask word of every member,
the counts, the members' bounds, the three excursion functions bit for bit, the region maps and the areas against
the numpy reference (excur_ref) built from `PopModel.population(d)`; the ties to SpreadSummary filled in the same
run; that joint < marginal where the members cross; four thresholds, day subsets, one slot, 18 slots; weights, add
and merge order; a finalize gone stale; reset; growth of the member masks; solver switches; release plans and peak
maps as sources; the refusals; and posterior_predictive with excursion thresholds.  Kalbar wind, R = 128, 6 days:
N = 257, N * N = 1032 * 64 + 1, so the last mask word holds one real cell and 63 pad bits.  The members, weights and
helpers of test_arrival_gpu.py."""
import ctypes as C
import json
import warnings

import numpy as np
import pytest

import excur_ref as R
import peak_ref
import test_arrival_gpu as TA
from sites_ref import plan_fields

pytestmark = pytest.mark.gpu

MEMBERS, WEIGHTS, THR, THR4 = TA.MEMBERS, TA.WEIGHTS, TA.THR, TA.THR4
_pop_model, _evaluate, _fields = TA._pop_model, TA._evaluate, TA._fields
LEVELS = (0.51, 0.9, 1.0)


def _check_against_reference(E, fields, weights, thr):
    """every device output of E against the numpy reference of the members' [nslot, N, N] fields
    -> {(k, day): the reference plane}"""
    X = np.asarray(fields)
    N = E.N
    nword = (N * N + 63) // 64
    assert E.total_weight == sum(weights) and E.members == len(weights)
    planes = {}
    for k, t in enumerate(thr):
        for s, d in enumerate(E.days):
            P = planes[k, d] = R.plane(X[:, s], weights, t)
            for m in range(len(weights)):
                got = E.mask(m, k, d)
                assert got.dtype == np.uint64 and got.shape == (nword,)
                assert np.array_equal(got, P['words'][m]), (m, k, d)
            got = E.counts(k, d)
            assert got.dtype == np.uint32 and got.shape == (N, N)
            assert np.array_equal(got.astype(np.int64), P['C']), (k, d)
            hi, lo, w = E.bounds(k, d)
            assert hi.dtype == lo.dtype == w.dtype == np.uint32
            assert np.array_equal(hi.astype(np.int64), P['hi']) and np.array_equal(lo.astype(np.int64), P['lo']), (k, d)
            assert w.tolist() == list(weights)
            Fp, Fm, Fc = E.above(k, d), E.below(k, d), E.contour(k, d)
            for name, got in (('above', Fp), ('below', Fm), ('contour', Fc)):
                assert got.dtype == np.float64 and np.array_equal(got, P[name]), (name, k, d)
            for level in LEVELS:
                reg = E.region(k, d, level)
                assert reg.dtype == np.int8 and np.array_equal(reg, R.region(P['above'], P['below'], level)), (k, d, level)
            assert E.areas(k, d, LEVELS) == R.areas(P['above'], P['below'], P['contour'], LEVELS, E.cell_area)
    return planes


def _all_maps(E):
    """every count plane and every map of E, for bit-for-bit comparisons between handles"""
    out = []
    for k in range(len(E.thresholds)):
        for d in E.days:
            out += [E.counts(k, d), E.above(k, d), E.below(k, d), E.contour(k, d)]
    return out


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('prob_model', [False, True])
@pytest.mark.parametrize('mode', ['exact', None])
def test_device_maps_match_the_numpy_reference(prob_model, mode):
    from parasitoids_amd.predictive import ExcursionMaps, SpreadSummary
    pm = _pop_model(prob_model=prob_model, **({} if mode is None else {'mode': mode}))
    days = list(range(6))
    scale = 1.0 / 130000 if prob_model else 1.0     # prob_model holds probabilities: the same densities
    thr, thr4 = [t * scale for t in THR], [t * scale for t in THR4]
    fields = []
    with ExcursionMaps(pm, thr) as E, ExcursionMaps(pm, thr4, days) as E4, SpreadSummary(pm, days, thr) as S:
        assert E.days == days and E.N == 257 and E.cell_area == (10000.0 / 128) ** 2 and E.thresholds == thr
        assert E.pitch == 1033 * 64 and E.member_nbytes == 2 * 6 * 1033 * 8
        for mem, w in zip(MEMBERS, WEIGHTS):
            _evaluate(pm, mem)
            for acc in (E, E4, S):
                acc.add(w)
            fields.append(_fields(pm, days))
        planes = _check_against_reference(E, fields, WEIGHTS, thr)
        _check_against_reference(E4, fields, WEIGHTS, thr4)
        W = float(sum(WEIGHTS))
        for k in range(2):
            for d in days:
                exc = S.exceedance(d, k)
                assert np.array_equal(E.counts(k, d) / W, exc), (k, d)       # the tie between the two accumulators
                assert np.all(E.above(k, d) <= exc), (k, d)
        # not vacuous, from the device's own fields: at t = 10 the members cross on every day, so the joint function
        # is strictly below the marginal somewhere and its 0.5 set a strict subset of the marginal one
        for d in days:
            P = planes[1, d]
            marginal = P['C'] / W
            assert (P['above'] < marginal).sum() > 0, d
            joint, marg = P['above'] >= 0.5, marginal >= 0.5
            assert np.all(marg[joint]) and joint.sum() < marg.sum(), d
            assert np.array_equal(E.above(1, d) >= 0.5, joint)
    pm.close()


def test_day_subsets_one_slot_and_eighteen_slots():
    from parasitoids_amd.predictive import ExcursionMaps
    pm = _pop_model()
    sub = [1, 3, 4]
    fields = []
    with ExcursionMaps(pm, THR, sub) as E, ExcursionMaps(pm, THR, [3]) as E1:
        for mem, w in zip(MEMBERS, WEIGHTS):
            _evaluate(pm, mem)
            E.add(w)
            E1.add(w)
            fields.append(_fields(pm, list(range(6))))
        _check_against_reference(E, [f[sub] for f in fields], WEIGHTS, THR)
        _check_against_reference(E1, [f[[3]] for f in fields], WEIGHTS, THR)
        with pytest.raises(ValueError):
            E.above(0, 2)                                   # not a listed day
        with pytest.raises(ValueError):
            E.region(0, 1, 0.5)                             # both signs could hold at 0.5
    pm.close()
    pm = _pop_model(R=64, ndays=18)                         # more slots than the one record in flight
    fields = []
    with ExcursionMaps(pm, THR) as E:
        assert len(E.days) == 18 and E.N == 129
        for mem, w in zip(MEMBERS[:3], WEIGHTS[:3]):
            _evaluate(pm, mem)
            E.add(w)
            fields.append(_fields(pm, E.days))
        _check_against_reference(E, fields, WEIGHTS[:3], THR)
    pm.close()


def test_weights_add_order_and_merge_order():
    """the counts and the maps do not depend on any order; the bounds come back permuted with the members"""
    from parasitoids_amd.predictive import ExcursionMaps
    pm = _pop_model()
    days = [0, 2, 5]
    hs = [ExcursionMaps(pm, THR, days) for _ in range(7)]
    fwd, rev, unit, a1, b1, a2, b2 = hs
    order = list(range(len(MEMBERS)))
    for i in order:
        _evaluate(pm, MEMBERS[i])
        fwd.add(WEIGHTS[i])
        for _ in range(WEIGHTS[i]):
            unit.add(1)
        (a1 if i < 2 else b1).add(WEIGHTS[i])
        (a2 if i < 2 else b2).add(WEIGHTS[i])
    for i in reversed(order):
        _evaluate(pm, MEMBERS[i])
        rev.add(WEIGHTS[i])
    a1.merge(b1)              # first half + second half
    b2.merge(a2)              # second half + first half
    want = _all_maps(fwd)
    assert unit.members == sum(WEIGHTS) and unit.total_weight == fwd.total_weight == sum(WEIGHTS)
    for other in (rev, unit, a1, b2):
        assert _same(_all_maps(other), want)
    for k in range(2):
        for d in days:
            hi, lo, w = fwd.bounds(k, d)
            for other, perm in ((rev, order[::-1]), (a1, order), (b2, order[2:] + order[:2])):
                h2, l2, w2 = other.bounds(k, d)
                assert np.array_equal(h2, hi[perm]) and np.array_equal(l2, lo[perm]) and np.array_equal(w2, w[perm])
                for j, m in enumerate(perm):
                    assert np.array_equal(other.mask(j, k, d), fwd.mask(m, k, d))
            hu, lu, wu = unit.bounds(k, d)
            assert np.array_equal(hu, np.repeat(hi, w)) and np.array_equal(lu, np.repeat(lo, w)) and np.all(wu == 1)
    with ExcursionMaps(pm, THR, days) as e:             # merging into an empty handle
        e.merge(fwd)
        assert _same(_all_maps(e), want) and e.members == fwd.members
    with ExcursionMaps(pm, [1.0, 20.0], days) as other, pytest.raises(Exception):
        fwd.merge(other)                                # different thresholds
    for h in hs:
        h.close()
    pm.close()


def test_a_further_add_makes_the_finalize_stale_and_reset_starts_over():
    from parasitoids_amd.predictive import ExcursionMaps
    pm = _pop_model()
    days = [2, 5]
    fields = []
    with ExcursionMaps(pm, THR, days) as E:
        for mem, w in zip(MEMBERS[:3], WEIGHTS[:3]):
            _evaluate(pm, mem)
            E.add(w)
            fields.append(_fields(pm, days))
        before = E.above(1, 5)                            # finalizes
        assert np.array_equal(before, R.plane(np.asarray(fields)[:, 1], WEIGHTS[:3], THR[1])['above'])
        _evaluate(pm, MEMBERS[3])
        E.add(WEIGHTS[3])                                 # the bounds of every member change with the counts
        fields.append(_fields(pm, days))
        after = E.above(1, 5)
        assert np.array_equal(after, R.plane(np.asarray(fields)[:, 1], WEIGHTS[:4], THR[1])['above'])
        assert not np.array_equal(after, before)
        _check_against_reference(E, fields, WEIGHTS[:4], THR)
        E.reset()
        assert E.members == 0 and E.total_weight == 0
        from parasitoids_amd import _lib as L
        with pytest.raises(L.HipError) as err:
            E.above(0, 2)
        assert err.value.code == L.PS_ERR_STATE
        E.add(2)                                          # the last evaluation once more, alone
        _check_against_reference(E, fields[3:], [2], THR)
    pm.close()


def test_growth_past_the_reserved_members_keeps_every_mask():
    from parasitoids_amd.predictive import ExcursionMaps
    pm = _pop_model(ndays=3)
    fields = []
    with ExcursionMaps(pm, THR) as E:
        assert E.capacity == 0
        base = E.nbytes
        E.reserve(2)
        assert E.capacity == 2 and E.nbytes == base + 2 * E.member_nbytes
        for rnd in range(2):                              # the same five members twice: the weights double
            for i, mem in enumerate(MEMBERS):
                _evaluate(pm, mem)
                E.add(WEIGHTS[i])
                if rnd == 0:
                    fields.append(_fields(pm, E.days))
        assert E.capacity >= 10 and E.members == 10
        _check_against_reference(E, fields + fields, WEIGHTS + WEIGHTS, THR)
    pm.close()


def test_members_on_different_cached_solvers_in_exact_mode():
    """the kernel extent moves with the diffusion parameters; in exact mode each extent has its own solver and
    stream, and successive adds from them are ordered by the handle's event"""
    from parasitoids_amd.predictive import ExcursionMaps
    pm = _pop_model(mode='exact')
    mems = [((120.0, 100.0, 0.2), 1.0), ((260.0, 230.0, 0.25), 1.2), ((120.0, 100.0, 0.2), 1.05),
            ((200.0, 170.0, 0.1), 1.1)]
    w = [2, 1, 1, 3]
    solvers = set()
    with ExcursionMaps(pm, THR, [1, 4]) as E:
        for mem, wi in zip(mems, w):
            _evaluate(pm, mem)
            solvers.add(id(pm.solver))
            E.add(wi)
        fields = []
        for mem in mems:       # read back only now: every add was enqueued behind the next evaluation
            _evaluate(pm, mem)
            fields.append(_fields(pm, E.days))
        assert len(solvers) >= 2
        _check_against_reference(E, fields, w, THR)
    pm.close()


def test_release_plans_and_peak_maps_as_sources():
    from parasitoids_amd.predictive import ExcursionMaps, PeakMaps, ReleaseSites, lagged_models
    Rr = 64
    res = 10000.0 / Rr
    pm = _pop_model(R=Rr)
    out = [0, 1, 2, 3, 5]
    sites = [(0.0, 0.0, 0.6, 0), (13 * res, 6 * res, 0.5, 2)]          # the second site two days later
    late = lagged_models(pm, [2])
    plan_f, peak_f = [], []
    with ReleaseSites(pm, sites, out, late) as S, PeakMaps(pm, THR) as PK, \
            ExcursionMaps.for_projection(S, THR) as ES, ExcursionMaps.for_projection(PK, THR) as EP:
        assert ES.days == out and EP.days == [0]
        cells = [(s['drow'], s['dcol'], s['amount'], s['lag']) for s in S.sites]
        for mem, w in zip(MEMBERS[:3], WEIGHTS[:3]):
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                S.evaluate(TA.HP, mem[0], TA.DLP, mem[1], TA.NPER)       # the base model, the lagged one and the apply
            PK.add(w)
            ES.add(w)
            EP.add(w)                                                    # the peak field PK has just written
            f0 = _fields(pm, list(range(6)))
            f2 = _fields(late[2], list(range(4)))
            plan_f.append(plan_fields({0: f0, 2: f2}, cells, out))
            peak_f.append(peak_ref.peak_field(f0)[None])
        planes = _check_against_reference(ES, plan_f, WEIGHTS[:3], THR)
        assert planes[0, 5]['C'].max() == sum(WEIGHTS[:3])
        _check_against_reference(EP, peak_f, WEIGHTS[:3], THR)
    for m in late.values():
        m.close()
    pm.close()


def test_refusals_enqueue_nothing_and_the_device_stays_usable():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import NEGVAL, ExcursionMaps, PeakMaps, _day_scales, _day_slots
    lib = L.load()
    dev = L.default_device()
    h = L._VP()
    thr5 = L.f64([1.0, 2.0, 3.0, 4.0, 5.0])
    assert lib.ps_excur_create(dev, 257, 33, 2, L.p_f64(thr5), C.byref(h)) == L.PS_ERR_BAD_ARG and not h
    assert lib.ps_excur_create(dev, 257, 6, 5, L.p_f64(thr5), C.byref(h)) == L.PS_ERR_BAD_ARG and not h
    assert lib.ps_excur_create(dev, 257, 6, 0, L.p_f64(thr5), C.byref(h)) == L.PS_ERR_BAD_ARG and not h
    assert lib.ps_excur_create(dev, 257, 6, 2, L.p_f64(L.f64([2.0, 1.0])), C.byref(h)) == L.PS_ERR_BAD_ARG and not h
    assert lib.ps_excur_create(dev, 257, 6, 2, L.p_f64(L.f64([0.0, 1.0])), C.byref(h)) == L.PS_ERR_BAD_ARG and not h
    rc = lib.ps_excur_create(dev, 40001, 32, 4, L.p_f64(thr5), C.byref(h))      # ~0.8 TB of counts
    assert rc == L.PS_ERR_OOM and not h and b'GB free' in lib.ps_last_error()
    pm, small = _pop_model(), _pop_model(R=64)
    _evaluate(pm, MEMBERS[0])
    _evaluate(small, MEMBERS[0])
    days = [1, 4]
    kind, idx, delta = _day_slots(days)
    stat, post = _day_scales(pm, days)

    def add(E, solver, n, w, k=None):
        return lib.ps_excur_add(E._h, solver._h, n, L.p_i32(kind if k is None else k), L.p_i32(idx), L.p_f64(stat),
                                L.p_f64(post), L.p_i32(delta), NEGVAL, w)
    with ExcursionMaps(pm, THR, days) as E, ExcursionMaps(pm, [1.0, 20.0], days) as other, PeakMaps(pm, THR) as PK:
        for call in (lambda: E.above(0, 1), lambda: E.bounds(0, 1)):
            with pytest.raises(L.HipError) as err:
                call()                                   # before the first add
            assert err.value.code == L.PS_ERR_STATE
        assert lib.ps_excur_finalize(E._h) == L.PS_ERR_STATE
        assert add(E, pm.solver, 3, 1) == L.PS_ERR_BAD_ARG                       # wrong slot count
        assert add(E, pm.solver, 2, 0) == L.PS_ERR_BAD_ARG                       # weight 0
        assert add(E, small.solver, 2, 1) == L.PS_ERR_BAD_ARG                    # wrong N
        assert add(E, pm.solver, 2, 1, L.i32([L.REC_CHAIN, 99])) != L.PS_OK      # a bad slot: nothing enqueued
        assert lib.ps_excur_add_peak(E._h, PK._h, 1) == L.PS_ERR_STATE           # no peak field yet
        PK.add(1)
        assert lib.ps_excur_add_peak(E._h, PK._h, 1) == L.PS_ERR_BAD_ARG         # one output, two slots
        with pytest.raises(ValueError):
            E.add(0)
        assert E.members == 0 and E.total_weight == 0 and E.capacity == 0
        E.add(0xfffffffd)
        assert add(E, pm.solver, 2, 2) == L.PS_ERR_BAD_ARG and b'overflow' in lib.ps_last_error()   # W = 2^32 - 1
        E.add(1)                                                                 # W = 2^32 - 2 is the last one in
        assert E.members == 2 and E.total_weight == 0xfffffffe
        X = _fields(pm, days)
        assert np.array_equal(E.counts(1, 4).astype(np.int64), 0xfffffffe * (X[1] >= 10.0))
        hi, lo, w = E.bounds(1, 4)
        assert hi.tolist() == [0, 0] and lo.tolist() == [0xfffffffe] * 2         # nested: two copies of one member
        assert np.array_equal(E.above(1, 4), (X[1] >= 10.0).astype(np.float64))
        other.add(1)
        E.reset()
        with pytest.raises(L.HipError) as err:
            E.merge(other)                           # different thresholds
        assert err.value.code == L.PS_ERR_BAD_ARG
        E.add(2)
        _check_against_reference(E, [X], [2], THR)
    pm.close()
    small.close()


def _csr(f, key, N):
    from scipy import sparse
    return sparse.csr_matrix((f[key + '_data'], f[key + '_ind'], f[key + '_indptr']), shape=(N, N)).toarray()


def test_posterior_predictive_with_excursion_maps_and_a_release_plan(tmp_path):
    from parasitoids_amd import mcmc
    from parasitoids_amd import predictive as PR
    from test_peak_gpu import _chain
    Rr, N = 64, 129
    res_m = 10000.0 / Rr
    out = [0, 1, 2, 3, 5]
    trace, names = _chain([2, 1, 3, 1, 2])
    chains = [(trace[:5], names), (trace[5:], names)]       # the run of three is cut in two: 2 + 1 + 2 | 1 + 1 + 2
    arg = dict(sites=[(0.0, 0.0, 0.6), (13 * res_m, 6 * res_m, 0.5, 2)], days=out)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        one, pa, pb = (_pop_model(R=Rr, mode='exact') for _ in range(3))
        res = PR.posterior_predictive(one, chains, thresholds=[1, 10], excursion=[1, 10], sites=arg)
        two = PR.posterior_predictive([pa, pb], chains, thresholds=[1, 10],
                                      excursion=dict(thresholds=[1, 10], levels=(0.75,)))
        plain = PR.posterior_predictive(one, chains, thresholds=[1, 10])
    assert plain.excursion is None and plain.excursion_levels is None
    assert res.failed == 0 and res.evaluations == 6 and len(res.runs) == 6
    E = res.excursion
    assert res.excursion_levels == [0.9, 0.95] and two.excursion_levels == [0.75] and two.sites is None
    assert E.days == list(range(6)) and E.thresholds == [1.0, 10.0]
    assert E.total_weight == res.summary.total_weight == 9 and E.members == res.summary.members == 6
    # by hand: every run once more through the model, and through the numpy reference
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    fields, plan_f, weights = [], [], []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        with PR.ReleaseSites.with_lagged_models(pa, arg['sites'], out) as P:
            for ci, first, weight in res.runs:
                P.evaluate(*mcmc.model_args(chains[ci][0][first, cols]))
                fields.append(_fields(pa, E.days))
                plan_f.append(np.array([P.field(e) for e in range(len(out))]))
                weights.append(weight)
    assert weights == [2, 1, 2, 1, 1, 2]
    _check_against_reference(E, fields, weights, [1.0, 10.0])
    assert _same(_all_maps(two.excursion), _all_maps(E))                       # two models, merged in chain order
    assert all(np.array_equal(a, b) for d in E.days for a, b in zip(two.excursion.bounds(1, d), E.bounds(1, d)))
    for k in range(2):
        for d in E.days:
            assert np.array_equal(E.counts(k, d) / 9.0, res.summary.exceedance(d, k))
    ES = res.sites.excursion
    assert ES.days == out and ES.members == 6 and ES.total_weight == 9
    _check_against_reference(ES, plan_f, weights, [1.0, 10.0])
    npz, js = res.save(str(tmp_path / 'a' / 'pp'))
    npz_p, js_p = plain.save(str(tmp_path / 'p' / 'pp'))
    assert not (tmp_path / 'p' / 'pp_excur.npz').exists()
    with np.load(npz) as fa, np.load(npz_p) as fp:          # the main file does not know about the excursion maps
        assert set(fa.files) == set(fp.files) and all(np.array_equal(fa[key], fp[key]) for key in fp.files)
    for path, H in ((tmp_path / 'a' / 'pp_excur.npz', E), (tmp_path / 'a' / 'pp_sites_excur.npz', ES)):
        want = {'days', 'excur_counts', 'excur_hi', 'excur_lo', 'excur_weights', 'excur_thresholds', 'excur_days'}
        with np.load(str(path)) as fz:
            for d in H.days:
                for k in range(2):
                    for name, fn in (('above', H.above), ('below', H.below), ('contour', H.contour)):
                        key = '%d_%s%d' % (d, name, k)
                        m = fn(k, d)
                        assert np.array_equal(_csr(fz, key, N), np.where(m >= 1e-8, m, 0.0)), key
                        want |= {'%s_%s' % (key, t) for t in ('data', 'ind', 'indptr')}
                    for p, tag in ((0.9, 'l90'), (0.95, 'l95')):
                        key = '%d_region%d_%s' % (d, k, tag)
                        assert fz[key].dtype == np.int8 and np.array_equal(fz[key], H.region(k, d, p)), key
                        want.add(key)
            assert set(fz.files) == want
            assert fz['excur_days'].tolist() == H.days and fz['excur_thresholds'].tolist() == [1.0, 10.0]
            assert fz['excur_counts'].shape == (2, len(H.days), N, N) and fz['excur_counts'].dtype == np.uint16
            assert np.array_equal(fz['excur_counts'][1, 2], H.counts(1, H.days[2]))
            hi, lo, w = H.bounds(0, H.days[-1])
            assert np.array_equal(fz['excur_hi'][0, -1], hi) and np.array_equal(fz['excur_lo'][0, -1], lo)
            assert np.array_equal(fz['excur_weights'], w) and w.tolist() == weights
    meta = json.load(open(js))['predictive']
    blk = meta['excursion']
    assert blk['thresholds'] == [1.0, 10.0] and blk['days'] == list(range(6)) and blk['levels'] == [0.9, 0.95]
    assert blk['members'] == 6 and blk['total_weight'] == 9 and blk['cell_area'] == E.cell_area
    assert blk['areas'] == [[{'day': d, 'levels': E.areas(k, d, [0.9, 0.95])} for d in E.days] for k in range(2)]
    assert meta['sites']['excursion']['days'] == out
    assert 'excursion' not in json.load(open(js_p))['predictive']
    for r in (res, two, plain):
        for acc in (r.summary, r.excursion, r.sites):
            if acc is not None:
                acc.close()
    for p in (one, pa, pb):
        p.close()


def test_profile_times_the_three_kinds_of_launch():
    from parasitoids_amd.predictive import ExcursionMaps
    pm = _pop_model(R=64, ndays=3)
    _evaluate(pm, MEMBERS[0])
    with ExcursionMaps(pm, THR) as E:
        E.profile(True)
        for _ in range(300):                              # more than the pairs a handle keeps pending
            E.add(1)
        E.above(0, 2)
        E.below(0, 2)
        add_ms, adds, fin_ms, fins, map_ms, maps = E.profile()
        assert adds == 300 and fins == 1 and maps == 2 and add_ms > 0 and fin_ms > 0 and map_ms > 0
        assert E.profile(False)[1] == 300
        E.add(1)
        assert E.profile()[1] == 300 and E.total_weight == 301 and E.capacity >= 301
    pm.close()

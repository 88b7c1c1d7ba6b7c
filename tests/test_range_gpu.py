"""GPU tests of the core-range maps (ps_range_*, predictive.RangeMaps): count planes, levels, cell counts, integer
masses and exponents bit for bit against the numpy restatement (range_ref) of `PopModel.population(d)`, the
invariants of the level from the device's own fields, one slot and eighteen, weights, add and merge order, reset,
growth of the member rows, solver switches, release plans and projections as sources, the refusals, and
posterior_predictive with core_range=.  Kalbar wind, R = 128, 6 days, the members, weights and helpers of
test_arrival_gpu.py.  N = 257, N * N = 1032 * 64 + 1: the last wave holds one real cell and 63 pad cells."""
import ctypes as C
import json
import warnings

import numpy as np
import pytest

import range_ref as R
import test_arrival_gpu as TA

pytestmark = pytest.mark.gpu

MEMBERS, WEIGHTS = TA.MEMBERS, TA.WEIGHTS
_pop_model, _evaluate, _fields = TA._pop_model, TA._evaluate, TA._fields
FR = [0.5, 0.95]
FR4 = [0.1, 0.5, 0.9, 0.99]
AREA_LEVELS = (0.05, 0.3, 0.5, 0.95, 1.0)


def _check_against_reference(G, fields, weights, check_maps=True):
    """every device output of G against the numpy reference of the members' [nslot, N, N] fields -> the reference"""
    from parasitoids_amd.predictive import range_area
    ref = R.accumulate(fields, weights, G.fractions)
    W = float(sum(weights))
    assert G.total_weight == W and G.members == len(fields) and G.weights.tolist() == list(weights)
    for s, d in enumerate(G.days):
        Q, E = G.mass(d)
        assert Q.dtype == np.uint64 and E.dtype == np.int32
        assert [int(x) for x in Q] == [int(x) for x in ref['Q'][:, s]], d
        assert np.array_equal(E, ref['E'][:, s]), d
        for j in range(len(G.fractions)):
            got = G.counts(j, d)
            assert got.dtype == np.uint32 and got.shape == ref['counts'].shape[2:]
            assert np.array_equal(got.astype(np.int64), ref['counts'][j, s]), (j, d)
            lam, n = G.levels(j, d), G.cells(j, d)
            assert lam.dtype == np.float64 and np.array_equal(lam, ref['lam'][:, j, s]), (j, d)
            assert np.array_equal(n, ref['n'][:, j, s]), (j, d)
            if check_maps:
                P = G.prob(j, d)
                assert np.array_equal(P, ref['counts'][j, s].astype(np.float64) / W), (j, d)
                for level in (0.2, 0.5, 1.0):
                    rg = G.range(j, d, level)
                    assert rg.dtype == bool and np.array_equal(rg, P >= level)
                assert G.area(j, d, AREA_LEVELS) == range_area(ref['n'][:, j, s], weights, G.cell_area, AREA_LEVELS, d)
    return ref


@pytest.mark.parametrize('prob_model', [False, True])
@pytest.mark.parametrize('mode', ['exact', None])
def test_device_maps_match_the_numpy_reference(prob_model, mode):
    from parasitoids_amd.predictive import RangeMaps
    pm = _pop_model(prob_model=prob_model, **({} if mode is None else {'mode': mode}))
    days, sub = list(range(6)), [0, 2, 5]
    fields = []
    with RangeMaps(pm, FR) as G, RangeMaps(pm, FR4, sub) as G4:
        assert G.days == days and G4.days == sub and G.N == 257 and G.cell_area == (10000.0 / 128) ** 2
        assert G.fractions == FR and G.capacity >= 1 and G.nbytes >= 2 * 6 * (257 * 257 + 63) // 64 * 64 * 4
        for mem, w in zip(MEMBERS, WEIGHTS):
            _evaluate(pm, mem)
            G.add(w)
            G4.add(w)
            fields.append(_fields(pm, days))
        ref = _check_against_reference(G, fields, WEIGHTS)
        _check_against_reference(G4, [f[sub] for f in fields], WEIGHTS)
        # not vacuous, from the device's own fields, levels and masses
        W = sum(WEIGHTS)
        ties = 0
        for s, d in enumerate(days):
            Q, E = G.mass(d)
            lam = [G.levels(j, d) for j in range(2)]
            n = [G.cells(j, d) for j in range(2)]
            C0, C1 = G.counts(0, d).astype(np.int64), G.counts(1, d).astype(np.int64)
            assert ((C1 > 0) & (C1 < W)).any(), d                    # the members' sets differ
            assert (C0 <= C1).all() and (C0 < C1).any()
            for m, F in enumerate(fields):
                v = F[s]
                assert np.all(np.isfinite(lam[0][m])) and lam[0][m] > lam[1][m] > 0      # a strict subset
                assert 0 < n[0][m] < n[1][m] < (v > 0).sum()
                q = np.where(v > 0, np.floor(np.ldexp(v, 36 - int(E[m]))), 0.0).astype(np.uint64)
                assert int(q.sum(dtype=np.uint64)) == int(Q[m]) and 2 ** 36 <= int(q.max()) < 2 ** 37
                for j, p in enumerate(FR):
                    need = R.needed_mass(p, int(Q[m]))
                    inside = int(q[v >= lam[j][m]].sum(dtype=np.uint64))
                    without = int(q[v > lam[j][m]].sum(dtype=np.uint64))
                    assert inside >= need > without, (d, m, j)
                    assert n[j][m] == int((v >= lam[j][m]).sum())
                    ties += int((v == lam[j][m]).sum()) - 1
        print('core-range: cells tied at a level beyond the level itself: %d; prob_model=%r mode=%r' % (ties, prob_model, mode))
        assert ref['counts'].max() == W
    pm.close()


def test_one_slot_and_eighteen_slots():
    from parasitoids_amd.predictive import RangeMaps
    pm = _pop_model(ndays=18)
    days = list(range(18))
    fields = []
    with RangeMaps(pm, FR) as G, RangeMaps(pm, [0.75], [7]) as G1:
        for mem, w in zip(MEMBERS[:2], WEIGHTS[:2]):
            _evaluate(pm, mem)
            G.add(w)
            G1.add(w)
            fields.append(_fields(pm, days))
        _check_against_reference(G, fields, WEIGHTS[:2], check_maps=False)
        _check_against_reference(G1, [f[[7]] for f in fields], WEIGHTS[:2])
    pm.close()


def _same_planes(a, b):
    return all(np.array_equal(a.counts(j, d), b.counts(j, d)) and np.array_equal(a.prob(j, d), b.prob(j, d))
               for j in range(len(a.fractions)) for d in a.days)


def _rows(G):
    """per member (weight, lambda, n, Q, E over all fractions and days) as comparable tuples"""
    w = G.weights.tolist()
    lam = np.array([[G.levels(j, d) for d in G.days] for j in range(len(G.fractions))])
    n = np.array([[G.cells(j, d) for d in G.days] for j in range(len(G.fractions))])
    mass = [G.mass(d) for d in G.days]
    return [(w[m], lam[:, :, m].tobytes(), n[:, :, m].tobytes(), tuple(int(x[0][m]) for x in mass),
             tuple(int(x[1][m]) for x in mass)) for m in range(len(w))]


def test_weights_add_order_and_merge_order_do_not_change_a_bit():
    from parasitoids_amd.predictive import RangeMaps
    pm = _pop_model(mode='exact')
    days = [0, 2, 5]
    hs = [RangeMaps(pm, FR, days) for _ in range(7)]
    fwd, rev, unit, a1, b1, a2, b2 = hs
    order = list(range(len(MEMBERS)))
    f_fwd, f_rev = [], []
    for i in order:
        _evaluate(pm, MEMBERS[i])
        f_fwd.append(_fields(pm, days))
        fwd.add(WEIGHTS[i])
        (a1 if i < 2 else b1).add(WEIGHTS[i])
        (a2 if i < 2 else b2).add(WEIGHTS[i])
        for _ in range(WEIGHTS[i]):
            unit.add(1)
    for i in reversed(order):
        _evaluate(pm, MEMBERS[i])
        f_rev.append(_fields(pm, days))
        rev.add(WEIGHTS[i])
    a1.merge(b1)              # A + B
    b2.merge(a2)              # B + A
    assert unit.members == sum(WEIGHTS) and unit.total_weight == fwd.total_weight == sum(WEIGHTS)
    for other in (unit, a1, b2):
        assert _same_planes(other, fwd)
    rf = _rows(fwd)
    assert _rows(a1) == rf and _rows(b2) == rf[2:] + rf[:2]                                  # tables permuted
    # the reversed order evaluates every member anew; in exact mode an evaluation repeats to the last bit
    assert all(np.array_equal(a, b) for a, b in zip(f_fwd, f_rev[::-1]))
    assert _same_planes(rev, fwd) and _rows(rev) == rf[::-1]
    _check_against_reference(rev, f_rev, WEIGHTS[::-1])
    _check_against_reference(fwd, f_fwd, WEIGHTS)
    assert _rows(unit) == [(1,) + r[1:] for r, w in zip(rf, WEIGHTS) for _ in range(w)]
    assert [fwd.area(1, d) for d in days] == [b2.area(1, d) for d in days] == [unit.area(1, d) for d in days]
    with RangeMaps(pm, FR, days) as e:             # merging into an empty handle
        e.merge(fwd)
        assert _same_planes(e, fwd) and _rows(e) == rf
    from parasitoids_amd import _lib as L
    with RangeMaps(pm, [0.5, 0.9], days) as other:
        other.add(1)
        with pytest.raises(L.HipError) as err:
            fwd.merge(other)                       # different fractions
        assert err.value.code == L.PS_ERR_BAD_ARG
    with RangeMaps(pm, FR, [0, 2, 4]) as other, pytest.raises(ValueError):
        fwd.merge(other)                           # different days
    for h in hs:
        h.close()
    pm.close()


def test_reset_starts_over_and_the_rows_grow_past_the_reserve():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import RangeMaps
    pm = _pop_model(ndays=3)
    fields = []
    with RangeMaps(pm, FR) as G:
        cap0, base = G.capacity, G.nbytes
        G.reserve(cap0 + 1)
        per_member = 2 * 3 * 12 + 3 * 12           # lambda and n per (fraction, slot), Q and E per slot
        assert G.capacity == 2 * cap0 and G.nbytes == base + cap0 * per_member
        weights = [1 + r % 3 for r in range(2 * cap0 + 6)]
        for r, w in enumerate(weights):            # past the reserve: the rows double and keep what they held
            if r < len(MEMBERS):
                _evaluate(pm, MEMBERS[r])
                fields.append(_fields(pm, G.days))
            G.add(w)
        assert G.capacity == 4 * cap0 and G.members == len(weights)
        every = fields + [fields[-1]] * (len(weights) - len(fields))
        _check_against_reference(G, every, weights, check_maps=False)
        G.reset()
        assert G.members == 0 and G.total_weight == 0 and G.capacity == 4 * cap0
        for call in (lambda: G.prob(0, 1), lambda: G.counts(0, 1), lambda: G.levels(0, 1), lambda: G.mass(1)):
            with pytest.raises(L.HipError) as err:
                call()
            assert err.value.code == L.PS_ERR_STATE
        G.add(2)                                   # the last evaluation once more, alone
        _check_against_reference(G, fields[-1:], [2])
    pm.close()


def test_members_on_different_cached_solvers_in_exact_mode():
    """the kernel extent moves with the diffusion parameters; in exact mode each extent has its own solver and
    stream, and successive adds from them -- which share the handle's pass scratch -- are ordered by its event"""
    from parasitoids_amd.predictive import RangeMaps
    pm = _pop_model(mode='exact')
    mems = [((120.0, 100.0, 0.2), 1.0), ((260.0, 230.0, 0.25), 1.2), ((120.0, 100.0, 0.2), 1.05),
            ((200.0, 170.0, 0.1), 1.1)]
    w = [2, 1, 1, 3]
    solvers = set()
    with RangeMaps(pm, FR, [1, 4]) as G:
        for mem, wi in zip(mems, w):
            _evaluate(pm, mem)
            solvers.add(id(pm.solver))
            G.add(wi)
        fields = []
        for mem in mems:       # read back only now: every add was enqueued behind the next evaluation
            _evaluate(pm, mem)
            fields.append(_fields(pm, G.days))
        assert len(solvers) >= 2
        _check_against_reference(G, fields, w)
    pm.close()


def test_release_plans_and_projections_as_sources():
    from parasitoids_amd.predictive import Projection, RangeMaps, ReleaseSites, exposure_weights, lagged_models
    from project_ref import project
    from sites_ref import plan_fields
    Rr = 64
    res = 10000.0 / Rr
    pm = _pop_model(R=Rr)
    out = [0, 1, 2, 3, 5]
    sites = [(0.0, 0.0, 0.6, 0), (13 * res, 6 * res, 0.5, 2)]          # the second site two days later
    late = lagged_models(pm, [2])
    Wp = np.concatenate([exposure_weights(list(range(6)), [0, 2]), np.zeros((1, 6)),
                         exposure_weights(list(range(6)), [5])])
    plan_f, proj_f = [], []
    with ReleaseSites(pm, sites, out, late) as S, Projection(pm, Wp, list(range(6))) as X, \
            RangeMaps.for_projection(S, FR) as GS, RangeMaps.for_projection(X, FR4) as GX:
        assert GS.days == out and X.live == [0, 1, 3] and GX.days == [0, 1, 3]
        cells = [(s['drow'], s['dcol'], s['amount'], s['lag']) for s in S.sites]
        for mem, w in zip(MEMBERS[:3], WEIGHTS[:3]):
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                S.evaluate(TA.HP, mem[0], TA.DLP, mem[1], TA.NPER)       # the base model, the lagged one and the apply
            X.apply()
            GS.add(w)
            GX.add(w)
            f0 = _fields(pm, list(range(6)))
            f2 = _fields(late[2], list(range(4)))
            plan_f.append(plan_fields({0: f0, 2: f2}, cells, out))
            proj_f.append(project(f0, Wp)[[0, 1, 3]])
        ref = _check_against_reference(GS, plan_f, WEIGHTS[:3])
        assert ref['n'][:, 1, -1].min() > ref['n'][:, 0, -1].min() > 0
        _check_against_reference(GX, proj_f, WEIGHTS[:3])
    for m in late.values():
        m.close()
    pm.close()


def test_refusals_enqueue_nothing_and_the_device_stays_usable():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import NEGVAL, RangeMaps, _day_scales, _day_slots
    lib = L.load()
    dev = L.default_device()
    h = L._VP()

    def create(N, nslot, fr):
        return lib.ps_range_create(dev, N, nslot, len(fr), L.p_f64(L.f64(fr)), C.byref(h))
    for fr in ([0.0, 0.5], [0.5, 1.0], [0.5, float('nan')], [0.95, 0.5], [0.5, 0.5], [0.1, 0.2, 0.3, 0.4, 0.5],
               [-0.5], [float('inf')]):
        assert create(257, 6, fr) == L.PS_ERR_BAD_ARG and not h, fr
    assert lib.ps_range_create(dev, 257, 6, 0, L.p_f64(L.f64([0.5])), C.byref(h)) == L.PS_ERR_BAD_ARG and not h
    assert create(257, 33, FR) == L.PS_ERR_BAD_ARG and not h
    assert create(257, 0, FR) == L.PS_ERR_BAD_ARG and not h
    assert create(5793, 6, FR) == L.PS_ERR_BAD_ARG and not h                 # N * N >= 2^25: the mass could overflow
    for bad in ([0.0, 0.5], [0.5, 1.0], [float('nan')], [0.95, 0.5], [0.1, 0.2, 0.3, 0.4, 0.5]):
        with pytest.raises(ValueError):
            RangeMaps(None, bad)                                             # refused before the model is touched
    pm, small = _pop_model(), _pop_model(R=64)
    _evaluate(pm, MEMBERS[0])
    _evaluate(small, MEMBERS[0])
    days = [1, 4]
    kind, idx, delta = _day_slots(days)
    stat, post = _day_scales(pm, days)

    def add(G, solver, n, w, k=None):
        return lib.ps_range_add(G._h, solver._h, n, L.p_i32(kind if k is None else k), L.p_i32(idx), L.p_f64(stat),
                                L.p_f64(post), L.p_i32(delta), NEGVAL, w)
    with RangeMaps(pm, FR, days) as G:
        for call in (lambda: G.prob(0, 1), lambda: G.counts(1, 4), lambda: G.levels(0, 1), lambda: G.cells(0, 1),
                     lambda: G.mass(4), lambda: G.area(0, 1)):
            with pytest.raises(L.HipError) as err:
                call()                                   # before the first add
            assert err.value.code == L.PS_ERR_STATE
        assert add(G, pm.solver, 3, 1) == L.PS_ERR_BAD_ARG                       # wrong slot count
        assert add(G, pm.solver, 2, 0) == L.PS_ERR_BAD_ARG                       # weight 0
        assert add(G, small.solver, 2, 1) == L.PS_ERR_BAD_ARG                    # wrong N
        assert add(G, pm.solver, 2, 1, L.i32([L.REC_CHAIN, 99])) != L.PS_OK      # a bad slot: nothing enqueued
        with pytest.raises(ValueError):
            G.add(0)
        with pytest.raises(ValueError):
            G.prob(2, 1)
        with pytest.raises(ValueError):
            G.prob(0, 3)
        assert G.members == 0 and G.total_weight == 0
        G.add(0xfffffffe)
        assert add(G, pm.solver, 2, 2) == L.PS_ERR_BAD_ARG and b'overflow' in lib.ps_last_error()   # W past 2^32 - 1
        G.add(1)                                                                 # W = 2^32 - 1 is the last one in
        assert G.members == 2 and G.total_weight == 0xffffffff
        X = _fields(pm, days)
        lam = R.member_levels(X[1], FR)[0]
        assert np.array_equal(G.counts(1, 4).astype(np.int64), 0xffffffff * (X[1] >= lam[1]))
        assert np.array_equal(G.prob(1, 4), (X[1] >= lam[1]).astype(np.float64))
        G.reset()
        G.add(2)
        _check_against_reference(G, [X], [2])
    pm.close()
    small.close()


def _csr(f, key, N):
    from scipy import sparse
    return sparse.csr_matrix((f[key + '_data'], f[key + '_ind'], f[key + '_indptr']), shape=(N, N)).toarray()


def test_posterior_predictive_with_core_range_and_a_release_plan(tmp_path):
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
        res = PR.posterior_predictive(one, chains, thresholds=[1, 10], core_range=[0.5, 0.95], sites=arg)
        two = PR.posterior_predictive([pa, pb], chains, thresholds=[1, 10],
                                      core_range=dict(fractions=[0.5, 0.95], levels=(0.75,)))
        plain = PR.posterior_predictive(one, chains, thresholds=[1, 10])
    assert plain.core_range is None and plain.core_range_levels is None
    assert res.failed == 0 and res.evaluations == 6 and len(res.runs) == 6
    G = res.core_range
    assert res.core_range_levels == [0.5, 0.9] and two.core_range_levels == [0.75] and two.sites is None
    assert G.days == list(range(6)) and G.fractions == [0.5, 0.95]
    assert G.total_weight == res.summary.total_weight == 9 and G.members == res.summary.members == 6
    # by hand: every run once more through the model into a hand-fed handle, and through the numpy reference
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    fields, plan_f, weights = [], [], []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        with PR.ReleaseSites.with_lagged_models(pa, arg['sites'], out) as P, PR.RangeMaps(pa, [0.5, 0.95]) as hand:
            for ci, first, weight in res.runs:
                P.evaluate(*mcmc.model_args(chains[ci][0][first, cols]))
                hand.add(weight)
                fields.append(_fields(pa, G.days))
                plan_f.append(np.array([P.field(e) for e in range(len(out))]))
                weights.append(weight)
            assert _same_planes(hand, G) and _rows(hand) == _rows(G)
    assert weights == [2, 1, 2, 1, 1, 2]
    _check_against_reference(G, fields, weights)
    assert _same_planes(two.core_range, G) and _rows(two.core_range) == _rows(G)     # two models, merged in chain order
    GS = res.sites.core_range
    assert GS.days == out and GS.members == 6 and GS.total_weight == 9
    _check_against_reference(GS, plan_f, weights)
    npz, js = res.save(str(tmp_path / 'a' / 'pp'))
    npz_p, js_p = plain.save(str(tmp_path / 'p' / 'pp'))
    assert not (tmp_path / 'p' / 'pp_range.npz').exists()
    with np.load(npz) as fa, np.load(npz_p) as fp:          # the main file does not know about the core-range maps
        assert set(fa.files) == set(fp.files) and all(np.array_equal(fa[key], fp[key]) for key in fp.files)
    for path, H in ((tmp_path / 'a' / 'pp_range.npz', G), (tmp_path / 'a' / 'pp_sites_range.npz', GS)):
        want = {'days', 'range_counts', 'range_lambda', 'range_cells', 'range_Q', 'range_E', 'range_weights',
                'range_fractions', 'range_days'}
        with np.load(str(path)) as fz:
            for d in H.days:
                for j in range(2):
                    key = '%d_prange%d' % (d, j)
                    assert np.array_equal(_csr(fz, key, N), H.prob(j, d)), key
                    want |= {'%s_%s' % (key, t) for t in ('data', 'ind', 'indptr')}
            assert set(fz.files) == want
            assert fz['range_days'].tolist() == H.days and fz['range_fractions'].tolist() == [0.5, 0.95]
            assert fz['range_counts'].shape == (2, len(H.days), N, N) and fz['range_counts'].dtype == np.uint16
            assert np.array_equal(fz['range_counts'][1, 2], H.counts(1, H.days[2]))
            assert fz['range_lambda'].dtype == np.float64 and fz['range_Q'].dtype == np.uint64
            assert np.array_equal(fz['range_lambda'][0, -1], H.levels(0, H.days[-1]))
            assert np.array_equal(fz['range_cells'][1, 1], H.cells(1, H.days[1]))
            Q, E = H.mass(H.days[3])
            assert np.array_equal(fz['range_Q'][3], Q) and np.array_equal(fz['range_E'][3], E)
            assert fz['range_weights'].tolist() == weights
    meta = json.load(open(js))['predictive']
    blk = meta['core_range']
    assert blk['fractions'] == [0.5, 0.95] and blk['days'] == list(range(6)) and blk['levels'] == [0.5, 0.9]
    assert blk['members'] == 6 and blk['total_weight'] == 9 and blk['cell_area'] == G.cell_area
    for j in range(2):
        for s, d in enumerate(G.days):
            rec = dict(G.area(j, d, (0.05, 0.5, 0.95)))
            P = G.prob(j, d)
            rec['consensus'] = [{'level': p, 'area': float((P >= p).sum()) * G.cell_area} for p in (0.5, 0.9)]
            assert blk['areas'][j][s] == rec
    assert meta['sites']['core_range']['days'] == out
    assert 'core_range' not in json.load(open(js_p))['predictive']
    for r in (res, two, plain):
        for m in (r.summary, r.core_range, r.sites):
            if m is not None:
                m.close()
    for p in (one, pa, pb):
        p.close()

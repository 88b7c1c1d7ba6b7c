"""GPU tests of the patch maps (ps_patch_*, predictive.PatchMaps): the crafted shapes at N = 129 (N * N = 260 * 64 + 1:
the last wave holds one real cell) injected through HipSolve.set_state, then the model's fields -- every row and both
count planes bit for bit against the numpy restatement (patch_ref), the tie to ExcursionMaps.counts, weights, add
and merge order, reset, growth of the member rows, solver switches, release plans and projections as sources, the
refusals, and posterior_predictive with patches=.  Kalbar wind, R = 128, 6 days, the members, weights and helpers of
test_arrival_gpu.py."""
import ctypes as C
import json
import warnings

import numpy as np
import pytest

import patch_ref as P
import test_arrival_gpu as TA

pytestmark = pytest.mark.gpu

MEMBERS, WEIGHTS, THR, THR4 = TA.MEMBERS, TA.WEIGHTS, TA.THR, TA.THR4
_pop_model, _evaluate, _fields = TA._pop_model, TA._evaluate, TA._fields
LEVELS = (0.05, 0.3, 0.5, 0.95, 1.0)
U32P = C.POINTER(C.c_uint32)


def _check_against_reference(G, fields, weights, check_maps=True):
    """every device output of G against the numpy reference of the members' [nslot, N, N] fields -> the reference"""
    from parasitoids_amd.predictive import patch_number, range_area
    ref = P.accumulate(fields, weights, G.thresholds, G.connectivity)
    W = float(sum(weights))
    assert G.total_weight == W and G.members == len(fields) and G.weights.tolist() == list(weights)
    for k in range(len(G.thresholds)):
        for s, d in enumerate(G.days):
            for which, key in (('main', 'main'), ('satellite', 'sat')):
                got = G.counts(k, d, which)
                assert got.dtype == np.uint32 and got.shape == ref[key].shape[2:]
                assert np.array_equal(got.astype(np.int64), ref[key][k, s]), (k, d, which)
                if check_maps:
                    assert np.array_equal(G.prob(k, d, which), ref[key][k, s].astype(np.float64) / W), (k, d, which)
            lab = np.where(ref['main_label'][:, k, s] == P.NONE, -1, ref['main_label'][:, k, s])
            for got, want in ((G.patches(k, d), ref['npatch'][:, k, s]), (G.cells(k, d), ref['cells'][:, k, s]),
                              (G.main_cells(k, d), ref['main_cells'][:, k, s]), (G.main_label(k, d), lab),
                              (G.largest_satellite(k, d), ref['sat_cells_max'][:, k, s])):
                assert got.dtype == np.int64 and np.array_equal(got, want), (k, d)
            if check_maps:
                assert G.number(k, d, LEVELS) == patch_number(ref['npatch'][:, k, s], weights, LEVELS, d)
                n, m = ref['cells'][:, k, s], ref['main_cells'][:, k, s]
                for which, cells in (('main', m), ('satellite', n - m), ('all', n)):
                    assert G.area(k, d, which, LEVELS) == range_area(cells, weights, G.cell_area, LEVELS, d)
    return ref


@pytest.mark.parametrize('connectivity', [4, 8])
def test_crafted_shapes_at_a_wave_and_one_cell(connectivity):
    """every crafted shape as one member of a one-slot handle, weights 1..3, three nested sets per add"""
    from parasitoids_amd import _lib as L
    from parasitoids_amd import hip_lib
    from parasitoids_amd.predictive import NEGVAL
    from scipy import sparse
    N = 129
    shapes = P.shapes(N)
    lib, dev, h = L.load(), L.default_device(), L._VP()
    s = hip_lib.HipSolve(sparse.coo_matrix(shapes[1][1]), [5, 5], mode='exact')
    L.check(lib.ps_patch_create(dev, N, 1, 3, L.p_f64(L.f64(P.SHAPE_THR)), connectivity, C.byref(h)))
    one, zero = L.f64([1.0]), L.i32([0])
    fields, weights = [], []
    try:
        for i, (name, f) in enumerate(shapes):
            s.set_state(sparse.coo_matrix(f))
            w = 1 + i % 3
            L.check(lib.ps_patch_add(h, s._h, 1, L.p_i32(L.i32([L.REC_STATE])), L.p_i32(zero), L.p_f64(one),
                                     L.p_f64(one), L.p_i32(zero), NEGVAL, w))
            back = s.dense(L.REC_STATE, 0)            # the reference gets the device's own field
            assert np.array_equal(back, f), name
            fields.append(back[None])
            weights.append(w)
        ref = P.accumulate(fields, weights, P.SHAPE_THR, connectivity)
        m = len(fields)
        for k in range(3):
            for which, key in ((0, 'main'), (1, 'sat')):
                got = np.empty((N, N), dtype=np.uint32)
                L.check(lib.ps_patch_fetch_counts(h, k, 0, which, got.ctypes.data_as(U32P)))
                assert np.array_equal(got.astype(np.int64), ref[key][k, 0]), (k, key)
            rows = [np.empty(m, dtype=np.uint32) for _ in range(6)]
            L.check(lib.ps_patch_fetch_members(h, k, 0, *[a.ctypes.data_as(U32P) for a in rows]))
            for a, name in zip(rows, P.FIELDS):
                bad = np.flatnonzero(a.astype(np.int64) != ref[name][:, k, 0])
                assert bad.size == 0, (k, name, [shapes[i][0] for i in bad])
            assert rows[5].tolist() == weights
        # not vacuous: what the shapes are there for, from the device's rows at the lowest threshold
        rows = [np.empty(m, dtype=np.uint32) for _ in range(6)]
        L.check(lib.ps_patch_fetch_members(h, 0, 0, *[a.ctypes.data_as(U32P) for a in rows]))
        npatch = dict(zip([n for n, _f in shapes], rows[0].tolist()))
        assert npatch['empty'] == 0 and npatch['full'] == 1 and npatch['spiral'] == 1 and npatch['comb'] == 1
        assert npatch['checkerboard'] == ((N * N + 1) // 2 if connectivity == 4 else 1)
        assert npatch['diagonal'] == npatch['antidiagonal'] == (2 if connectivity == 4 else 1)
        assert npatch['edge_next_row'] == npatch['edge_two_rows'] == 2 and npatch['ring_island'] == 2
    finally:
        lib.ps_patch_destroy(h)
        s.close()


@pytest.mark.parametrize('prob_model', [False, True])
@pytest.mark.parametrize('mode', ['exact', None])
def test_device_maps_match_the_numpy_reference(prob_model, mode):
    from parasitoids_amd.predictive import ExcursionMaps, PatchMaps
    pm = _pop_model(prob_model=prob_model, **({} if mode is None else {'mode': mode}))
    days, sub = list(range(6)), [0, 2, 5]
    scale = 1.0 / 130000 if prob_model else 1.0     # prob_model holds probabilities: the same densities
    thr, thr4 = [t * scale for t in THR], [t * scale for t in THR4]
    fields = []
    with PatchMaps(pm, thr) as G, PatchMaps(pm, thr, connectivity=8) as G8, PatchMaps(pm, thr4, sub) as G4, \
            PatchMaps(pm, thr4, sub, connectivity=8) as G48, ExcursionMaps(pm, thr) as X:
        assert G.days == days and G4.days == sub and G.N == 257 and G.cell_area == (10000.0 / 128) ** 2
        assert G.thresholds == thr and G.connectivity == 4 and G8.connectivity == 8 and G.capacity >= 1
        assert G.nbytes >= 4 * 2 * 6 * ((257 * 257 + 63) // 64 * 64) * 4
        for mem, w in zip(MEMBERS, WEIGHTS):
            _evaluate(pm, mem)
            for acc in (G, G8, G4, G48, X):
                acc.add(w)
            fields.append(_fields(pm, days))
        _check_against_reference(G, fields, WEIGHTS)
        _check_against_reference(G8, fields, WEIGHTS, check_maps=False)
        _check_against_reference(G4, [f[sub] for f in fields], WEIGHTS, check_maps=False)
        _check_against_reference(G48, [f[sub] for f in fields], WEIGHTS, check_maps=False)
        for k in range(2):                           # main + satellite is the weighted exceedance count
            for d in days:
                for H in (G, G8):
                    total = H.counts(k, d, 'main') + H.counts(k, d, 'satellite')
                    assert np.array_equal(total, X.counts(k, d)), (k, d)
        # not vacuous, from the device's own rows: at t = 10 the plume detaches for some members and not for others
        for d in (0, 2):
            assert len(set(G.patches(1, d).tolist())) > 1, d
        n, m = G.cells(1, 0), G.main_cells(1, 0)
        assert G.counts(1, 0, 'satellite').any() and ((0 < m) & (m < n)).any()
        assert G.largest_satellite(1, 0).max() >= 30 and G.number(1, 0)['p_fragmented'] > 0
        for d in days:                               # at t = 1 one front throughout
            assert G.patches(0, d).tolist() == [1] * len(MEMBERS), d
            assert not G.counts(0, d, 'satellite').any() and G.largest_satellite(0, d).tolist() == [0] * len(MEMBERS)
            assert np.array_equal(G.main_cells(0, d), G.cells(0, d))
        print('patches at t = 10, day 0..5, per member: %r; prob_model=%r mode=%r'
              % ([G.patches(1, d).tolist() for d in days], prob_model, mode))
    pm.close()


def _same_planes(a, b):
    return all(np.array_equal(a.counts(k, d, w), b.counts(k, d, w)) and np.array_equal(a.prob(k, d, w), b.prob(k, d, w))
               for k in range(len(a.thresholds)) for d in a.days for w in ('main', 'satellite'))


def _rows(G):
    """per member (weight, the five row words over all thresholds and days) as comparable tuples"""
    w = G.weights.tolist()
    r = np.array([[G._members(k, d)[:5] for d in G.days] for k in range(len(G.thresholds))])   # [K, days, 5, members]
    return [(w[m], r[:, :, :, m].tobytes()) for m in range(len(w))]


def test_weights_add_order_and_merge_order_do_not_change_a_bit():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import PatchMaps
    pm = _pop_model(mode='exact')
    days = [0, 2, 5]
    hs = [PatchMaps(pm, THR, days) for _ in range(7)]
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
            unit.add(1)                            # a weight of 3 equals three unit adds
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
    assert _rows(a1) == rf and _rows(b2) == rf[2:] + rf[:2]                                  # rows permuted
    assert sorted(_rows(b2)) == sorted(rf)
    # the reversed order evaluates every member anew; in exact mode an evaluation repeats to the last bit
    assert all(np.array_equal(a, b) for a, b in zip(f_fwd, f_rev[::-1]))
    assert _same_planes(rev, fwd) and _rows(rev) == rf[::-1]
    _check_against_reference(rev, f_rev, WEIGHTS[::-1])
    _check_against_reference(fwd, f_fwd, WEIGHTS)
    assert _rows(unit) == [(1,) + r[1:] for r, w in zip(rf, WEIGHTS) for _ in range(w)]
    assert [fwd.number(1, d) for d in days] == [b2.number(1, d) for d in days] == [unit.number(1, d) for d in days]
    with PatchMaps(pm, THR, days) as e:             # merging into an empty handle
        e.merge(fwd)
        assert _same_planes(e, fwd) and _rows(e) == rf
    for other in (PatchMaps(pm, [1.0, 20.0], days), PatchMaps(pm, THR, days, connectivity=8)):
        with other:
            other.add(1)
            with pytest.raises(L.HipError) as err:
                fwd.merge(other)                       # different thresholds, another connectivity
            assert err.value.code == L.PS_ERR_BAD_ARG
    with PatchMaps(pm, THR, [0, 2, 4]) as other, pytest.raises(ValueError):
        fwd.merge(other)                           # different days
    assert _rows(fwd) == rf and fwd.members == len(MEMBERS)
    for h in hs:
        h.close()
    pm.close()


def test_reset_starts_over_and_the_rows_grow_past_the_reserve():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import PatchMaps
    pm = _pop_model(ndays=3)
    fields = []
    with PatchMaps(pm, THR) as G:
        cap0, base = G.capacity, G.nbytes
        G.reserve(cap0 + 1)
        assert G.capacity == 2 * cap0 and G.nbytes == base + cap0 * 2 * 3 * 20       # 20 B per member, k and slot
        weights = [1 + r % 3 for r in range(cap0 + 6)]                             # 70 members
        assert len(weights) == 70
        G.reset()
        G2 = PatchMaps(pm, THR)                      # this one starts at the rows of create and has to grow
        for r, w in enumerate(weights):
            if r < len(MEMBERS):
                _evaluate(pm, MEMBERS[r])
                fields.append(_fields(pm, G.days))
            G.add(w)
            G2.add(w)
        assert G2.capacity == 2 * cap0 and G2.members == len(weights) == G.members
        every = fields + [fields[-1]] * (len(weights) - len(fields))
        _check_against_reference(G2, every, weights, check_maps=False)
        assert _same_planes(G, G2) and _rows(G) == _rows(G2)
        G2.close()
        G.reset()
        assert G.members == 0 and G.total_weight == 0 and G.capacity == 2 * cap0
        for call in (lambda: G.prob(0, 1, 'main'), lambda: G.counts(0, 1, 'satellite'), lambda: G.patches(0, 1)):
            with pytest.raises(L.HipError) as err:
                call()
            assert err.value.code == L.PS_ERR_STATE
        G.add(2)                                   # the last evaluation once more, alone
        _check_against_reference(G, fields[-1:], [2])
    pm.close()


def test_members_on_different_cached_solvers_in_exact_mode():
    """the kernel extent moves with the diffusion parameters; in exact mode each extent has its own solver and
    stream, and successive adds from them -- which share the handle's scratch -- are ordered by its event"""
    from parasitoids_amd.predictive import PatchMaps
    pm = _pop_model(mode='exact')
    mems = [((120.0, 100.0, 0.2), 1.0), ((260.0, 230.0, 0.25), 1.2), ((120.0, 100.0, 0.2), 1.05),
            ((200.0, 170.0, 0.1), 1.1)]
    w = [2, 1, 1, 3]
    solvers = set()
    with PatchMaps(pm, THR, [1, 4]) as G:
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
    from parasitoids_amd.predictive import PatchMaps, Projection, ReleaseSites, exposure_weights, lagged_models
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
            PatchMaps.for_projection(S, THR) as GS, PatchMaps.for_projection(X, THR4, connectivity=8) as GX:
        assert GS.days == out and X.live == [0, 1, 3] and GX.days == [0, 1, 3] and GX.connectivity == 8
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
        assert ref['npatch'][:, 0, 2:].min() >= 1 and ref['cells'].max() > 0
        _check_against_reference(GX, proj_f, WEIGHTS[:3])
    for m in late.values():
        m.close()
    pm.close()


def test_refusals_enqueue_nothing_and_the_device_stays_usable():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import NEGVAL, PatchMaps, _day_scales, _day_slots
    lib = L.load()
    dev = L.default_device()
    h = L._VP()

    def create(N, nslot, thr, conn=4):
        return lib.ps_patch_create(dev, N, nslot, len(thr), L.p_f64(L.f64(thr)), conn, C.byref(h))
    for thr in ([0.0, 1.0], [-1.0], [1.0, float('nan')], [float('inf')], [10.0, 1.0], [1.0, 1.0], [1.0, 2.0, 3.0, 4.0, 5.0]):
        assert create(257, 6, thr) == L.PS_ERR_BAD_ARG and not h, thr
    assert lib.ps_patch_create(dev, 257, 6, 0, L.p_f64(L.f64([1.0])), 4, C.byref(h)) == L.PS_ERR_BAD_ARG and not h
    for conn in (5, 0, 6, 16):
        assert create(257, 6, THR, conn) == L.PS_ERR_BAD_ARG and not h, conn
    assert create(257, 33, THR) == L.PS_ERR_BAD_ARG and not h
    assert create(257, 0, THR) == L.PS_ERR_BAD_ARG and not h
    assert create(5793, 6, THR) == L.PS_ERR_BAD_ARG and not h                # N * N >= 2^25
    pm, small = _pop_model(), _pop_model(R=64)
    _evaluate(pm, MEMBERS[0])
    _evaluate(small, MEMBERS[0])
    days = [1, 4]
    kind, idx, delta = _day_slots(days)
    stat, post = _day_scales(pm, days)

    def add(G, solver, n, w, k=None):
        return lib.ps_patch_add(G._h, solver._h, n, L.p_i32(kind if k is None else k), L.p_i32(idx), L.p_f64(stat),
                                L.p_f64(post), L.p_i32(delta), NEGVAL, w)
    with PatchMaps(pm, THR, days) as G:
        for call in (lambda: G.prob(0, 1, 'main'), lambda: G.counts(1, 4, 'satellite'), lambda: G.patches(0, 1),
                     lambda: G.main_label(0, 1), lambda: G.number(0, 1), lambda: G.area(0, 1)):
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
            G.prob(2, 1, 'main')
        with pytest.raises(ValueError):
            G.prob(0, 3, 'main')
        with pytest.raises(ValueError):
            G.prob(0, 1, 'all')
        out = np.empty((257, 257), dtype=np.uint32)
        assert lib.ps_patch_fetch_counts(G._h, 0, 0, 2, out.ctypes.data_as(U32P)) == L.PS_ERR_BAD_ARG
        assert G.members == 0 and G.total_weight == 0
        G.add(0xfffffffe)
        assert add(G, pm.solver, 2, 2) == L.PS_ERR_BAD_ARG and b'overflow' in lib.ps_last_error()   # W past 2^32 - 1
        G.add(1)                                                                 # W = 2^32 - 1 is the last one in
        assert G.members == 2 and G.total_weight == 0xffffffff
        X = _fields(pm, days)
        total = G.counts(1, 4, 'main').astype(np.int64) + G.counts(1, 4, 'satellite')
        assert np.array_equal(total, 0xffffffff * (X[1] >= THR[1]))
        G.reset()
        G.add(2)
        _check_against_reference(G, [X], [2])
    pm.close()
    small.close()


def _csr(f, key, N):
    from scipy import sparse
    return sparse.csr_matrix((f[key + '_data'], f[key + '_ind'], f[key + '_indptr']), shape=(N, N)).toarray()


def test_posterior_predictive_with_patches_and_a_release_plan(tmp_path):
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
        res = PR.posterior_predictive(one, chains, thresholds=[1, 10], patches=[1, 10], sites=arg)
        two = PR.posterior_predictive([pa, pb], chains, thresholds=[1, 10],
                                      patches=dict(thresholds=[1, 10], connectivity=8, levels=(0.5,)))
        plain = PR.posterior_predictive(one, chains, thresholds=[1, 10])
    assert plain.patches is None and plain.patch_levels is None
    assert res.failed == 0 and res.evaluations == 6 and len(res.runs) == 6
    G = res.patches
    assert res.patch_levels == [0.05, 0.5, 0.95] and two.patch_levels == [0.5] and two.sites is None
    assert G.days == list(range(6)) and G.thresholds == [1.0, 10.0] and G.connectivity == 4
    assert two.patches.connectivity == 8
    assert G.total_weight == res.summary.total_weight == 9 and G.members == res.summary.members == 6
    # by hand: every run once more through the model, and through the numpy reference
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    fields, plan_f, weights = [], [], []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        with PR.ReleaseSites.with_lagged_models(pa, arg['sites'], out) as S:
            for ci, first, weight in res.runs:
                S.evaluate(*mcmc.model_args(chains[ci][0][first, cols]))
                fields.append(_fields(pa, G.days))
                plan_f.append(np.array([S.field(e) for e in range(len(out))]))
                weights.append(weight)
    assert weights == [2, 1, 2, 1, 1, 2]
    _check_against_reference(G, fields, weights)
    _check_against_reference(two.patches, fields, weights, check_maps=False)   # two models, merged in chain order
    GS = res.sites.patches
    assert GS.days == out and GS.members == 6 and GS.total_weight == 9
    _check_against_reference(GS, plan_f, weights)
    npz, js = res.save(str(tmp_path / 'a' / 'pp'))
    npz_p, js_p = plain.save(str(tmp_path / 'p' / 'pp'))
    assert not (tmp_path / 'p' / 'pp_patch.npz').exists()
    with np.load(npz) as fa, np.load(npz_p) as fp:          # the main file does not know about the patch maps
        assert set(fa.files) == set(fp.files) and all(np.array_equal(fa[key], fp[key]) for key in fp.files)
    for path, H in ((tmp_path / 'a' / 'pp_patch.npz', G), (tmp_path / 'a' / 'pp_sites_patch.npz', GS)):
        want = {'days', 'patch_weights', 'patch_thresholds', 'patch_connectivity', 'patch_days'}
        want |= {'patch_' + name for name in P.FIELDS}
        with np.load(str(path)) as fz:
            for d in H.days:
                for k in range(2):
                    for tag, which in (('pmain', 'main'), ('psat', 'satellite')):
                        key = '%d_%s%d' % (d, tag, k)
                        assert np.array_equal(_csr(fz, key, N), H.prob(k, d, which)), key
                        want |= {'%s_%s' % (key, t) for t in ('data', 'ind', 'indptr')}
            assert set(fz.files) == want
            assert fz['patch_days'].tolist() == H.days and fz['patch_thresholds'].tolist() == [1.0, 10.0]
            assert int(fz['patch_connectivity']) == 4 and fz['patch_weights'].tolist() == weights
            assert fz['patch_npatch'].shape == (2, len(H.days), 6)
            assert np.array_equal(fz['patch_npatch'][1, 2], H.patches(1, H.days[2]))
            assert np.array_equal(fz['patch_main_label'][0, -1], H.main_label(0, H.days[-1]))
            assert np.array_equal(fz['patch_sat_cells_max'][1, 0], H.largest_satellite(1, H.days[0]))
    meta = json.load(open(js))['predictive']
    blk = meta['patches']
    assert blk['thresholds'] == [1.0, 10.0] and blk['days'] == list(range(6)) and blk['connectivity'] == 4
    assert blk['members'] == 6 and blk['total_weight'] == 9 and blk['cell_area'] == G.cell_area
    for k in range(2):
        for s, d in enumerate(G.days):
            rec = G.number(k, d)
            got = blk['number'][k][s]
            assert got['p_fragmented'] == rec['p_fragmented'] and got['mean_patches'] == rec['mean']
            assert got['satellite_share'] == PR.patch_satellite_share(G.cells(k, d), G.main_cells(k, d), weights)
    assert meta['sites']['patches']['days'] == out
    assert 'patches' not in json.load(open(js_p))['predictive']
    for r in (res, two, plain):
        for m in (r.summary, r.patches, r.sites):
            if m is not None:
                m.close()
    for p in (one, pa, pb):
        p.close()


def test_every_option_on_gives_the_same_patch_maps_as_patches_alone():
    from parasitoids_amd import predictive as PR
    from test_peak_gpu import _chain
    from test_predictive_driver_gpu import R, RES_M, _close, _options
    from test_sites_gpu import _pop_model as _model
    trace, names = _chain([2, 1, 3, 1, 2])
    chains = [(trace[:5], names), (trace[5:], names)]
    options = _options(chains)
    arg = dict(thresholds=[1.0, 10.0], connectivity=8)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        pm = _model(R=R, mode='exact')
        alone = PR.posterior_predictive(pm, chains, thresholds=[1.0, 10.0], patches=arg, sites=options['sites'])
        every = PR.posterior_predictive(pm, chains, thresholds=[1.0, 10.0], cell_area=RES_M ** 2, patches=arg,
                                        **options)
    for a, b in ((alone.patches, every.patches), (alone.sites.patches, every.sites.patches)):
        assert a.members == b.members == 6 and a.days == b.days
        assert _same_planes(a, b) and _rows(a) == _rows(b)
    assert every.emergence.patches is None and every.exposure.patches is None
    for r in (alone, every):
        _close(r)
        for m in (r.patches, r.sites.patches):
            m.close()
    pm.close()

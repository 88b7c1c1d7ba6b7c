"""GPU tests of the neighbourhood fields (ps_nbhd_*, predictive.NeighbourhoodFields) and of the accumulators fed
from them: the device fields against the numpy restatement (nbhd_ref) bit for bit -- a maximum is exact -- on a field
of isolated spikes and on model fields, the empty-tile skip against its absence, gather, determinism, the
projection and release-plan sources, SpreadSummary / SpreadHistogram / MonteCarloError / ReweightedSummary
.for_projection against the numpy loops fed the fetched bits, the untouched day-based path, the refusals, and
posterior_predictive(neighbourhood=) against a hand loop with its files.  Kalbar wind, 6 days, the members and
weights of test_projection_gpu.py."""
import ctypes as C
import json
import os
import types
import warnings

import numpy as np
import pytest

import hist_ref
import nbhd_ref
import reweight_ref as RR
from test_arrival_gpu import MEMBERS, WEIGHTS, THR, _pop_model, _evaluate, _fields

pytestmark = pytest.mark.gpu

SPIKE_R2 = [0, 1, 2, 5, 25, 169, 1024]
SPIKE_IN = [0, 0, 1, 0, 1, 0, 1]         # two and more outputs share input 0, the others read input 1


def _pitch(N):
    return (N * N + 63) // 64 * 64


def _nbytes(N, nout, nin):
    return nout * _pitch(N) * 8 + nin * ((N + 31) // 32) * ((N + 63) // 64) * 4


def _spikes(N):
    """about 40 cells of distinct values: the corners (the last one the tail cell of the odd N * N), the mid-edges,
    two spikes closer than most radii, one more in the last row and one in the last column, the rest scattered"""
    rng = np.random.default_rng(12)
    h = N // 2
    cells = [(0, 0), (0, N - 1), (N - 1, 0), (N - 1, N - 1), (0, h), (h, 0), (N - 1, h), (h, N - 1), (40, 40),
             (42, 43), (N - 1, 17), (90, N - 1)]
    while len(cells) < 40:
        c = (int(rng.integers(N)), int(rng.integers(N)))
        if c not in cells:
            cells.append(c)
    v = np.zeros((N, N))
    vals = rng.permutation(40) + 1.0
    for (r, c), x in zip(cells, vals):
        v[r, c] = x * 1.25
    return v


def test_spike_field_against_the_restatement():
    from scipy import sparse
    from parasitoids_amd import _lib as L
    from parasitoids_amd.hip_lib import HipSolve
    lib = L.load()
    N = 129
    v = _spikes(N)
    assert (v > 0).sum() == 40 and np.unique(v[v > 0]).size == 40
    solver = HipSolve(sparse.coo_matrix(v), [65, 65], mode='exact')
    state = solver.dense(L.REC_STATE, 0)
    assert np.array_equal(state, v)                       # the record the handle reads holds the spikes themselves
    h = L._VP()
    nout = len(SPIKE_R2)
    L.check(lib.ps_nbhd_create(0, N, 2, nout, L.p_i32(L.i32(SPIKE_IN)), L.p_i32(L.i32(SPIKE_R2)), C.byref(h)))
    try:
        one, zero = L.f64([1.0, 1.0]), L.i32([0, 0])
        kind = L.i32([L.REC_STATE, L.REC_STATE])

        def apply():
            L.check(lib.ps_nbhd_apply(h, solver._h, 2, L.p_i32(kind), L.p_i32(zero), L.p_f64(one), L.p_f64(one),
                                      L.p_i32(zero), 0.0))

        def fetch(e):
            out = np.empty((N, N))
            L.check(lib.ps_nbhd_fetch(h, e, L.p_f64(out)))
            return out
        apply()
        got = [fetch(e) for e in range(nout)]
        for e, r2 in enumerate(SPIKE_R2):
            want = nbhd_ref.neighbourhood_max(v, r2)
            bad = np.argwhere(got[e] != want)
            assert np.array_equal(got[e], want), (r2, len(bad), bad[:4].tolist())
        assert np.array_equal(got[0], v)                  # r2 = 0: the input itself
        # every disc of r2 = 1024 spans several tiles, and those of the corner spikes leave the domain
        assert got[-1][0, 0] >= v[0, 0] and got[-1][N - 1, N - 1] >= v[N - 1, N - 1]
        # the skip switched off: the same bits
        L.check(lib.ps_nbhd_set_skip(h, 0))
        apply()
        for e in range(nout):
            assert np.array_equal(fetch(e), got[e]), e
    finally:
        lib.ps_nbhd_destroy(h)
        solver.close()


def _windows(R):
    """eight windows over five of the six days, the days out of order and shared, the radii from 0 to 32 cells"""
    cell = 10000.0 / R
    return [(5, 3 * cell), (1, 0.0), (3, 1.5 * cell), (5, 12 * cell), (2, 32 * cell), (0, 5 * cell), (1, 7.3 * cell),
            (3, 20 * cell)]


@pytest.mark.parametrize('R', [64, 128])
def test_model_fields_against_the_restatement(R):
    from scipy import ndimage
    from parasitoids_amd.predictive import NeighbourhoodFields
    pm = _pop_model(R)
    N = 2 * R + 1
    _evaluate(pm, MEMBERS[0])
    fields = _fields(pm, range(6))
    windows = _windows(R)
    with NeighbourhoodFields(pm, windows) as NF:
        assert NF.in_days == [0, 1, 2, 3, 5] and NF.nout == 8 and NF.fields_kind == 'nbhd'
        assert NF.windows == windows and NF.radii_m == [t[1] for t in windows]
        assert NF.r2 == [9, 0, 2, 144, 1024, 25, 53, 400] and NF.half == [3, 0, 1, 12, 32, 5, 7, 20]
        assert NF.cells == [len(nbhd_ref.disc_offsets(r2)) for r2 in NF.r2] and NF.live == list(range(8))
        assert NF.nbytes == _nbytes(N, 8, 5)
        NF.apply()
        assert NF.applies == 1
        first = [NF.field(e) for e in range(8)]
        for e, (day, _radius) in enumerate(windows):
            v = fields[day]
            Z = first[e]
            assert np.array_equal(Z, nbhd_ref.neighbourhood_max(v, NF.r2[e])), e
            assert (Z >= v).all()
            reach = ndimage.binary_dilation(v != 0, structure=nbhd_ref.disc_footprint(NF.r2[e]))
            assert np.array_equal(Z != 0, reach), e            # zero exactly where the dilated support is empty
        assert np.array_equal(first[1], fields[1])
        assert any((z == 0).any() for z in first)
        # gather: the tail cell of the odd N * N, a corner and the release cell
        rows, cols = [N - 1, 0, R], [N - 1, 0, R]
        got = NF.gather(rows, cols)
        assert got.shape == (8, 3)
        for e in range(8):
            assert np.array_equal(got[e], first[e][rows, cols])
        assert got[:, 2].min() > 0
        # a second apply, and one with the skip switched off: the same bits
        NF.apply()
        assert all(np.array_equal(NF.field(e), first[e]) for e in range(8))
        NF.set_skip(False)
        NF.apply()
        assert all(np.array_equal(NF.field(e), first[e]) for e in range(8))
        NF.set_skip(True)
        assert NF.applies == 3
        # another member overwrites the first, zeros included
        _evaluate(pm, MEMBERS[2])
        NF.apply()
        other = _fields(pm, range(6))
        for e in (3, 4):
            assert np.array_equal(NF.field(e), nbhd_ref.neighbourhood_max(other[windows[e][0]], NF.r2[e])), e
    pm.close()


def test_the_other_sources():
    from parasitoids_amd.predictive import NeighbourhoodFields, Projection, ReleaseSites
    pm = _pop_model(64, mode='exact')
    res_m = 10000.0 / 64
    _evaluate(pm, MEMBERS[0])
    windows = _windows(64)
    days = [0, 1, 2, 3, 5]
    by_index = [(days.index(d), r) for d, r in windows]
    plan_days = [0, 1, 3, 5]
    plan_windows = [t for t in windows if t[0] in plan_days]
    with NeighbourhoodFields(pm, windows) as NF, Projection(pm, np.eye(5), days) as P, \
            NeighbourhoodFields.for_projection(P, by_index) as NP, \
            ReleaseSites(pm, [(0.0, 0.0, 0.6), (7 * res_m, -3 * res_m, 0.5)], plan_days) as RS, \
            NeighbourhoodFields.for_projection(RS, plan_windows) as NS:
        NF.apply()
        first = [NF.field(e) for e in range(8)]
        # identity weights: the projection's outputs are the day fields, and so are their neighbourhood fields
        P.apply()
        NP.apply()
        assert NP.in_days is None and NP.r2 == NF.r2
        assert all(np.array_equal(NP.field(e), first[e]) for e in range(8))
        # a release plan of two sites: the restatement applied to the plan's fetched fields
        RS.apply()
        NS.apply()
        plan = {d: RS.field(e) for e, d in enumerate(plan_days)}
        for e, (day, _radius) in enumerate(plan_windows):
            assert np.array_equal(NS.field(e), nbhd_ref.neighbourhood_max(plan[day], NS.r2[e])), e
        assert NS.nbytes == _nbytes(129, len(plan_windows), 4)
        # output labels that do not exist, or carry no weight, are refused on the host
        with pytest.raises(ValueError, match='output'):
            NeighbourhoodFields.for_projection(RS, [(2, 100.0)])
        with pytest.raises(ValueError, match='output'):
            NeighbourhoodFields.for_projection(P, [(5, 100.0)])
        W = np.eye(5)
        W[2] = 0.0
        with Projection(pm, W, days) as P0:
            with pytest.raises(ValueError, match='carries weight'):
                NeighbourhoodFields.for_projection(P0, [(2, 100.0)])
    pm.close()


@pytest.fixture(scope='module')
def fed():
    """the five members in two passes on one exact-mode model (the same member gives the same bits each time):
    first every accumulator fed without a host synchronisation in between, with the fields fetched after the
    adds, then a day summary alone"""
    from parasitoids_amd.predictive import (MonteCarloError, NeighbourhoodFields, ReweightedSummary, SpreadHistogram,
                                            SpreadSummary)
    f = types.SimpleNamespace()
    pm = f.pm = _pop_model(64, mode='exact')
    f.windows = _windows(64)[:5]
    f.NF = NeighbourhoodFields(pm, f.windows)
    f.S = SpreadSummary.for_projection(f.NF, THR)
    f.H = SpreadHistogram.for_projection(f.NF)
    f.RW = ReweightedSummary.for_projection(f.NF, ['flat'], THR)
    f.M = MonteCarloError.for_projection(f.NF, 3, THR)
    f.D_with, f.D_alone = SpreadSummary(pm, None, THR), SpreadSummary(pm, None, THR)
    f.Z = []
    for m, w in zip(MEMBERS, WEIGHTS):
        _evaluate(pm, m)
        f.D_with.add(w)
        f.NF.apply()
        f.S.add(w)
        f.H.add(w)
        f.RW.add([0.0], w)
        f.M.add(w)
        f.Z.append(np.array([f.NF.field(e) for e in range(len(f.windows))]))
    f.M.finish()
    for m, w in zip(MEMBERS, WEIGHTS):
        _evaluate(pm, m)
        f.D_alone.add(w)
    yield f
    for h in (f.S, f.H, f.RW, f.M, f.D_with, f.D_alone, f.NF):
        h.close()
    pm.close()


def test_summary_of_neighbourhood_fields_against_the_numpy_loop(fed):
    S, n = fed.S, len(fed.windows)
    assert (S.total_weight, S.members, S.thresholds) == (8.0, 5, THR)
    st = RR.new_state(fed.Z[0].shape, THR, 1)
    for i in range(5):
        RR.add(st, fed.Z[i], [0.0], WEIGHTS[i])
    sc = st[0]
    for e in range(n):
        assert np.array_equal(S.mean(e), sc['mean'][e]), e                      # bit for bit
        for k in range(2):
            assert np.array_equal(S.exceedance(e, k), RR.exceedance(sc, k)[e]), (e, k)   # the counts, exactly
        scale = np.abs(sc['mean'][e]).max()
        np.testing.assert_allclose(S.variance(e), RR.variance(sc)[e], rtol=1e-12, atol=1e-15 * scale ** 2)
        assert S.mean(e).max() > 0
    assert any(S.variance(e).max() > 0 for e in range(n))
    assert any((S.exceedance(e, 1) == 1.0).any() for e in range(n))


def test_histogram_of_neighbourhood_fields_against_the_numpy_counts(fed):
    H = fed.H
    assert (H.total_weight, H.members) == (8.0, 5)
    for e in range(len(fed.windows)):
        want = hist_ref.weighted_counts([z[e] for z in fed.Z], WEIGHTS, H.edges)
        got = H.counts(e)
        assert np.array_equal(got.astype(np.int64), want), e
        _b, value, _lo, _hi = hist_ref.quantile_from_counts(want, H.edges, 0.5)
        np.testing.assert_allclose(H.quantile(e, 0.5), value, rtol=1e-12, atol=0.0)


def test_reweighted_summary_with_zero_log_weights_holds_the_summary_bits(fed):
    S, RW = fed.S, fed.RW
    assert RW.members('flat') == 5 and RW.skipped('flat') == 0
    for e in range(len(fed.windows)):
        assert np.array_equal(RW.mean('flat', e), S.mean(e))
        assert np.array_equal(RW.variance('flat', e), S.variance(e))
        for k in range(2):
            assert np.array_equal(RW.exceedance('flat', e, k), S.exceedance(e, k))


def test_monte_carlo_error_of_neighbourhood_fields_against_the_replay(fed):
    from test_mcerr_gpu import _check_exact, _replay
    n = len(fed.windows)
    ref = _replay(fed.Z, WEIGHTS, THR, 3)
    assert (fed.M.batches, fed.M.used_weight, fed.M.discarded_weight) == (2, 6, 2)
    _check_exact(fed.M, ref, list(range(n)))


def test_the_day_summary_beside_a_neighbourhood_handle_does_not_move(fed):
    A, B = fed.D_with, fed.D_alone
    assert A.total_weight == B.total_weight == 8.0
    for d in A.days:
        assert np.array_equal(A.mean(d), B.mean(d)) and np.array_equal(A.variance(d), B.variance(d))
        for k in range(2):
            assert np.array_equal(A.exceedance(d, k), B.exceedance(d, k))


def test_refusals():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import NeighbourhoodFields, Projection, SpreadSummary
    lib = L.load()
    N = 129

    def create(nin, nout, inputs, r2, n=N):
        h = L._VP()
        rc = lib.ps_nbhd_create(0, n, nin, nout, L.p_i32(L.i32(inputs)), L.p_i32(L.i32(r2)), C.byref(h))
        if rc == L.PS_OK:
            lib.ps_nbhd_destroy(h)
        return rc
    assert create(2, 2, [0, 1], [0, 1088]) == L.PS_OK          # H = 32 to its last r2
    assert create(1, 32, [0] * 32, [4] * 32) == L.PS_OK
    for args in [(0, 1, [0], [1]), (33, 1, [0], [1]), (1, 0, [0], [1]), (1, 33, [0] * 33, [1] * 33),
                 (2, 1, [2], [1]), (2, 1, [-1], [1]), (1, 1, [0], [1089]), (1, 1, [0], [-1]),
                 (2, 2, [0, 1], [1, 33 * 33])]:
        assert create(*args) == L.PS_ERR_BAD_ARG, args
    assert create(1, 1, [0], [1], n=0) == L.PS_ERR_BAD_ARG
    with pytest.raises(ValueError, match='radius'):
        NeighbourhoodFields(types.SimpleNamespace(), [(1, -1.0)])     # refused before the model is looked at
    with pytest.raises(ValueError, match='33 windows'):
        NeighbourhoodFields(types.SimpleNamespace(), [(1, 1.0)] * 33)
    pm = _pop_model(64)
    cell = 10000.0 / 64
    with pytest.raises(ValueError, match='half-width'):
        NeighbourhoodFields(pm, [(1, 33 * cell)])                      # H = 33
    with NeighbourhoodFields(pm, [(1, cell), (2, 32 * cell)]) as NF, SpreadSummary.for_projection(NF, THR) as S, \
            Projection(pm, np.eye(3), [0, 1, 2]) as P3, SpreadSummary.for_projection(P3, THR) as S3, \
            NeighbourhoodFields(pm, [(9, cell)]) as N9:
        # before the model's first evaluation, and a day the evaluation does not have
        with pytest.raises(ValueError, match='evaluation'):
            NF.apply()
        _evaluate(pm, MEMBERS[0])
        with pytest.raises(ValueError, match='evaluation'):
            N9.apply()
        # before the first apply
        for call in (lambda: NF.field(0), lambda: NF.gather([0], [0]), lambda: S.add(1)):
            with pytest.raises(L.HipError) as ei:
                call()
            assert ei.value.code == L.PS_ERR_STATE
        # a solver of another domain: nothing is enqueued
        other = L._VP()
        L.check(lib.ps_nbhd_create(0, 131, 2, 2, L.p_i32(L.i32([0, 1])), L.p_i32(L.i32([1, 4])), C.byref(other)))
        kind, idx, delta = L.i32([L.REC_CHAIN] * 2), L.i32([0, 1]), L.i32([1, 1])
        one = L.f64([1.0, 1.0])
        assert lib.ps_nbhd_apply(other, pm.solver._h, 2, L.p_i32(kind), L.p_i32(idx), L.p_f64(one), L.p_f64(one),
                                 L.p_i32(delta), 1e-8) == L.PS_ERR_BAD_ARG
        out = np.empty((131, 131))
        assert lib.ps_nbhd_fetch(other, 0, L.p_f64(out)) == L.PS_ERR_STATE
        lib.ps_nbhd_destroy(other)
        assert lib.ps_nbhd_apply(NF._h, pm.solver._h, 3, L.p_i32(kind), L.p_i32(idx), L.p_f64(one), L.p_f64(one),
                                 L.p_i32(delta), 1e-8) == L.PS_ERR_BAD_ARG      # three inputs given, the handle has two
        NF.apply()
        # slot counts that do not fit: nothing is enqueued, the accumulator stays empty
        assert lib.ps_summary_add_nbhd(S3._h, NF._h, 1) == L.PS_ERR_BAD_ARG
        assert S3.members == 0
        assert lib.ps_summary_add_nbhd(S._h, NF._h, 0) == L.PS_ERR_BAD_ARG       # weight >= 1
        assert lib.ps_summary_add_nbhd(S._h, None, 1) == L.PS_ERR_BAD_ARG
        assert lib.ps_nbhd_apply_project(NF._h, P3._h) == L.PS_ERR_STATE          # P3 not applied yet
        P3.apply()
        assert lib.ps_nbhd_apply_project(NF._h, P3._h) == L.PS_ERR_BAD_ARG        # 3 outputs, 2 inputs
        assert NF.applies == 1
        with pytest.raises(ValueError):
            NF.field(2)
        with pytest.raises(L.HipError):
            NF.gather([129], [0])
        S.add(2)
        assert S.members == 1 and S.total_weight == 2.0
    pm.close()


def _csr(f, key, N):
    from scipy import sparse
    return sparse.csr_matrix((f[key + '_data'], f[key + '_ind'], f[key + '_indptr']), shape=(N, N)).toarray()


def test_posterior_predictive_with_neighbourhood_against_a_hand_loop(tmp_path):
    from parasitoids_amd import mcmc
    from parasitoids_amd import predictive as PR
    from test_reweight_gpu import _chain
    R, N = 64, 129
    res_m = 10000.0 / R
    ta, names = _chain([3, 2])
    tb, _ = _chain([1, 2, 2])
    traces = [ta, tb[1:]]                                    # the second chain: two runs of other members
    chains = [(t, names) for t in traces]
    windows = [(1, 0), (3, 200.0), (5, 400.0)]
    plan = dict(sites=[(0.0, 0.0, 0.6), (7 * res_m, -3 * res_m, 0.5)], days=[0, 1, 5])     # day 3 is no output day
    rw = {'flat': dict(log_weights=[np.zeros(len(t)) for t in traces]), 'options': dict(min_ess=1)}
    pm = _pop_model(R, mode='exact')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        res = PR.posterior_predictive(pm, chains, thresholds=THR, neighbourhood=windows, sites=plan, reweight=rw,
                                      mc_error=dict(batches=4), quantiles=[0.5], cell_area=res_m ** 2)
    nb = res.neighbourhood
    assert res.failed == 0 and res.evaluations == 4
    assert nb.windows == [(1, 0.0), (3, 200.0), (5, 400.0)] and nb.thresholds == THR and nb.r2 == [0, 1, 6]
    assert nb.cells == [1, 5, 21] and nb.given == [[1, 0.0], [3, 200.0], [5, 400.0]]
    assert (nb.summary.total_weight, nb.summary.members) == (9.0, 4)
    assert res.sites.neighbourhood.windows == [(1, 0.0), (5, 400.0)]          # the windows on the plan's output days
    assert res.catch is None
    # the hand loop: every run once more, per chain a summary of its own, merged in chain order
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    hand, hand_pl = [], []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        with PR.NeighbourhoodFields(pm, windows) as NF, PR.ReleaseSites(pm, plan['sites'], plan['days']) as RS, \
                PR.NeighbourhoodFields.for_projection(RS, [windows[0], windows[2]]) as NS:
            for ci in range(2):
                hand.append(PR.SpreadSummary.for_projection(NF, THR))
                hand_pl.append(PR.SpreadSummary.for_projection(NS, THR))
                for c, first, weight in res.runs:
                    if c != ci:
                        continue
                    pm.evaluate(*mcmc.model_args(traces[ci][first, cols]), want_stats=False)
                    NF.apply()
                    hand[ci].add(weight)
                    RS.apply()
                    NS.apply()
                    hand_pl[ci].add(weight)
            for hs in (hand, hand_pl):
                hs[0].merge(hs[1])
                hs[1].close()
    for got, want, n in ((nb, hand[0], 3), (res.sites.neighbourhood, hand_pl[0], 2)):
        assert got.summary.total_weight == want.total_weight == 9.0
        for e in range(n):
            assert np.array_equal(got.maximum(e), want.mean(e)), e
            var = want.variance(e)
            assert np.array_equal(got.sd(e), np.sqrt(np.maximum(var, 0.0))), e
            for k in range(2):
                assert np.array_equal(got.prob(e, k), want.exceedance(e, k)), (e, k)
    for k in range(2):
        # radius 0 is the cell itself: the day summary's exceedance map; a radius never lowers the probability
        assert np.array_equal(nb.prob(0, k), res.summary.exceedance(1, k))
        assert (nb.prob(1, k) >= res.summary.exceedance(3, k)).all()
        assert (nb.prob(2, k) >= res.summary.exceedance(5, k)).all()
        assert (nb.prob(2, k) > res.summary.exceedance(5, k)).any()
    assert np.array_equal(nb.maximum(0), res.summary.mean(1))
    q = nb.quantile(2, 0.5)
    assert q.shape == (N, N) and q.max() > 0
    # log-weights 0: the reweighted maps hold the summary's bits; the Monte Carlo error has its own handle
    for got in (nb, res.sites.neighbourhood):
        assert np.array_equal(got.reweight.mean('flat', 0), got.maximum(0))
        assert (got.mc_error.batches, got.mc_error.used_weight) == (res.mc_error.batches, res.mc_error.used_weight)
        assert got.mc_error.batches >= 4 and got.mc_error.thresholds == THR
        assert np.isfinite(got.mc_error.mcse(0)).all()
    # the files
    npz, js = res.save(str(tmp_path / 'a' / 'pp'))
    names_out = sorted(os.listdir(str(tmp_path / 'a')))
    for want in ('pp_nbhd.npz', 'pp_sites_nbhd.npz', 'pp_nbhd_reweight.npz'):
        assert want in names_out
    f = np.load(str(tmp_path / 'a' / 'pp_nbhd.npz'))
    assert list(f['days']) == [1, 3, 5] and list(f['radii_m']) == [0.0, 200.0, 400.0]
    assert list(f['r2']) == [0, 1, 6] and list(f['cells']) == [1, 5, 21] and list(f['thresholds']) == THR
    for e in range(3):
        for key, m in (('n%d' % e, nb.maximum(e)), ('n%d_sd' % e, nb.sd(e)), ('n%d_pexc1' % e, nb.prob(e, 1)),
                       ('n%d_q50' % e, nb.quantile(e, 0.5))):
            assert np.array_equal(_csr(f, key, N), np.where(m >= 1e-8, m, 0.0)), key
    fs = np.load(str(tmp_path / 'a' / 'pp_sites_nbhd.npz'))
    assert list(fs['days']) == [1, 5] and 'n1_pexc0_data' in fs.files
    meta = json.load(open(js))['predictive']
    block = meta['neighbourhood']
    assert block['given'] == [[1, 0.0], [3, 200.0], [5, 400.0]] and block['windows'] == block['given']
    assert block['members'] == 4 and block['total_weight'] == 9.0 and block['thresholds'] == THR
    for e, out in enumerate(block['outputs']):
        assert out['window'] == list(nb.windows[e]) and out['r2'] == nb.r2[e]
        assert out['area'] == [float((nb.prob(e, k) >= 0.5).sum() * res_m ** 2) for k in range(2)]
    assert len(meta['sites']['neighbourhood']['outputs']) == 2
    assert 'neighbourhood' in meta['mc_error'] and 'sites_neighbourhood' in meta['mc_error']
    for h in (hand[0], hand_pl[0], res.summary, res.histogram, res.reweight, res.mc_error, res.sites, nb):
        h.close()
    pm.close()


def test_without_neighbourhood_nothing_changes(tmp_path):
    from parasitoids_amd import predictive as PR
    from test_reweight_gpu import _chain
    pm = _pop_model(64)
    trace, names = _chain([2, 1])
    plan = dict(sites=[(0.0, 0.0, 1.0)], days=[1, 3])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        res = PR.posterior_predictive(pm, (trace, names), thresholds=THR, sites=plan)
    assert res.neighbourhood is None and res.sites.neighbourhood is None
    res.save(str(tmp_path / 'p' / 'pp'))
    assert sorted(os.listdir(str(tmp_path / 'p'))) == ['pp.json', 'pp.npz', 'pp_sites.npz']
    assert not any('nbhd' in name for name in os.listdir(str(tmp_path / 'p')))
    meta = json.load(open(str(tmp_path / 'p' / 'pp.json')))['predictive']
    assert 'neighbourhood' not in meta and 'neighbourhood' not in meta['sites']
    res.summary.close()
    res.sites.close()
    pm.close()

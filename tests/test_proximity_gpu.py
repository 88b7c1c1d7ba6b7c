"""GPU tests of the proximity fields (ps_prox_*, predictive.ProximityFields) and of the accumulators fed from them:
the squared distances and the metres against the numpy restatement (prox_ref) bit for bit -- both are exact -- on the
crafted sets and on model fields, both sides, the narrowed column strip against the default, the cross-check against
NeighbourhoodFields, ProximityPosterior against numpy loops over the reference fields, the projection and
release-plan sources, the refusals of the C ABI, and posterior_predictive(proximity=) against the class fed by hand.
Kalbar wind, 6 days, the members of test_projection_gpu.py at R = 32."""
import ctypes as C
import json
import os
import types
import warnings

import numpy as np
import pytest

import hist_ref
import prox_ref
import reweight_ref as RR
from test_arrival_gpu import MEMBERS, _pop_model, _evaluate, _fields

pytestmark = pytest.mark.gpu

R = 32
N = 2 * R + 1
CELL = 10000.0 / R
T = 2.0                       # the threshold of the crafted fields (prox_ref.as_field)


def _u32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


class _Raw():
    """one ps_prox handle over the state record of a solver, through the C ABI: output 0 'to', output 1 'in'"""

    def __init__(self, n, cell_m):
        from scipy import sparse
        from parasitoids_amd import _lib as L
        from parasitoids_amd.hip_lib import HipSolve
        self.L, self.lib, self.n = L, L.load(), n
        self.solver = HipSolve(sparse.coo_matrix(np.ones((n, n))), [33, 33], mode='exact')
        self.h = L._VP()
        L.check(self.lib.ps_prox_create(0, n, 1, 2, L.p_i32(L.i32([0, 0])), L.p_f64(L.f64([T, T])),
                                        L.p_i32(L.i32([0, 1])), cell_m, C.byref(self.h)))

    def apply(self, v=None):
        L = self.L
        if v is not None:
            self.solver.set_state(v)
        one, zero, kind = L.f64([1.0]), L.i32([0]), L.i32([L.REC_STATE])
        L.check(self.lib.ps_prox_apply(self.h, self.solver._h, 1, L.p_i32(kind), L.p_i32(zero), L.p_f64(one),
                                       L.p_f64(one), L.p_i32(zero), 0.0))

    def planes(self):
        """[(d2, metres)] of both outputs"""
        out = []
        for e in range(2):
            d2, m = np.empty((self.n, self.n), dtype=np.uint32), np.empty((self.n, self.n))
            self.L.check(self.lib.ps_prox_fetch_d2(self.h, e, _u32(d2)))
            self.L.check(self.lib.ps_prox_fetch(self.h, e, self.L.p_f64(m)))
            out.append((d2, m))
        return out

    def strip(self, width=None):
        if width is not None:
            self.L.check(self.lib.ps_prox_set_strip(self.h, width))
        w = C.c_int()
        self.L.check(self.lib.ps_prox_info(self.h, None, None, None, None, C.byref(w)))
        return w.value

    def close(self):
        self.lib.ps_prox_destroy(self.h)
        self.solver.close()


@pytest.mark.parametrize('n', [65, 129])
def test_crafted_sets_against_the_restatement_bit_for_bit(n):
    cell = 10000.0 / (n // 2)
    raw = _Raw(n, cell)
    try:
        F = prox_ref.far2(n)
        assert raw.strip() == 64                         # two strips at 65, three at 129: none is the whole domain
        for name, s in prox_ref.crafted(n):
            v = prox_ref.as_field(s, T)                  # exactly t on the set, one ulp below t off it
            raw.apply(v)
            if name == 'ring':
                assert np.array_equal(raw.solver.dense(raw.L.REC_STATE, 0), v)      # the record holds the field itself
            got = raw.planes()
            for e, side in enumerate(('to', 'in')):
                want_d2, want_m = prox_ref.field(v, T, side, cell)
                bad = np.argwhere(got[e][0] != want_d2)
                assert np.array_equal(got[e][0], want_d2), (name, side, len(bad), bad[:4].tolist())
                assert np.array_equal(got[e][1], want_m), (name, side)
            to, inside = got[0][0], got[1][0]
            assert np.array_equal(to == 0, s) and np.array_equal(inside == 0, ~s), name
            if name == 'empty':
                assert (to == F).all() and (inside == 0).all() and (got[0][1] == np.sqrt(np.float64(F)) * cell).all()
            if name == 'whole':
                assert (to == 0).all() and (inside == F).all()
            if name == 'corner0':
                assert to[n - 1, n - 1] == 2 * (n - 1) ** 2 == F - 1
            if name == 'ring':                           # the hole is found, the domain's edge is not unreached ground
                assert inside[n // 2, n // 2] == 0 and 0 < inside.max() < (n // 3) ** 2
                keep = got
        # determinism: a second apply, and the strip narrowed to 16, 2 and 1 columns, give the ring's bits again
        ring = prox_ref.as_field(dict(prox_ref.crafted(n))['ring'], T)
        for width in (0, 16, 2, 1, 0):
            assert raw.strip(width) == (width or 64)
            raw.apply(ring)
            again = raw.planes()
            for e in range(2):
                assert np.array_equal(again[e][0], keep[e][0]) and np.array_equal(again[e][1], keep[e][1]), (width, e)
        for width in (3, 128, -1):
            assert raw.lib.ps_prox_set_strip(raw.h, width) == raw.L.PS_ERR_BAD_ARG
    finally:
        raw.close()


def _thresholds(fields, day):
    """two thresholds the day's field separates: a low one with a wide set and a high one with a small one"""
    top = fields[day].max()
    return [float(np.float32(top * 1e-3)), float(np.float32(top * 0.2))]


def test_model_fields_against_the_restatement():
    from parasitoids_amd.predictive import ProximityFields, prox_far
    pm = _pop_model(R, mode='exact')
    _evaluate(pm, MEMBERS[0])
    fields = _fields(pm, range(6))
    (a1, b1), (a3, b3) = _thresholds(fields, 1), _thresholds(fields, 3)
    windows = [(3, a3), (1, a1), (1, b1, 'in'), (3, b3, 'to')]
    with ProximityFields(pm, windows) as PF:
        assert PF.in_days == [1, 3] and PF.nout == 4 and PF.fields_kind == 'prox' and PF.live == [0, 1, 2, 3]
        assert PF.windows == [(3, a3, 'to'), (1, a1, 'to'), (1, b1, 'in'), (3, b3, 'to')]
        assert PF.sides == ['to', 'to', 'in', 'to'] and PF.thresholds == [a3, a1, b1, b3]
        assert (PF.far2, PF.far_m) == prox_far(N, CELL) and PF.far2 == 2 * 64 * 64 + 1 and PF.cell_m == CELL
        pitch = (N * N + 63) // 64 * 64
        assert PF.nbytes == 4 * pitch * 14 + 4 * pitch // 8 and PF.strip == 64
        PF.profile(True)
        PF.apply()
        assert PF.applies == 1
        first = []
        for e, (day, t, side) in enumerate(PF.windows):
            want_d2, want_m = prox_ref.field(fields[day], t, side, CELL)
            got_d2, got_m = PF.d2(e), PF.field(e)
            assert got_d2.dtype == np.uint32 and np.array_equal(got_d2, want_d2), e
            assert np.array_equal(got_m, want_m), e
            assert 0 < (got_d2 == 0).sum() < N * N and got_d2.max() < PF.far2, e      # neither empty nor whole
            first.append((got_d2, got_m))
        rows, cols = [N - 1, 0, R], [N - 1, 0, R]
        got = PF.gather(rows, cols)
        assert got.shape == (4, 3)
        for e in range(4):
            assert np.array_equal(got[e], first[e][1][rows, cols])
        assert got[1, 2] == 0.0 and got[2, 2] > 0.0          # the release cell: in the set, and at some depth in it
        PF.apply()
        PF.set_strip(8)
        PF.apply()
        assert PF.strip == 8 and PF.applies == 3
        for e in range(4):
            assert np.array_equal(PF.d2(e), first[e][0]) and np.array_equal(PF.field(e), first[e][1])
        row_ms, n_row, col_ms, n_col = PF.profile()
        assert n_row == n_col == 3 and row_ms > 0 and col_ms > 0
        # another member overwrites the first
        _evaluate(pm, MEMBERS[2])
        PF.apply()
        other = _fields(pm, range(6))
        assert np.array_equal(PF.d2(0), prox_ref.field(other[3], a3, 'to', CELL)[0])
    pm.close()


def test_cross_check_against_the_neighbourhood_fields():
    """on a grid of 25 m cells: the largest value within r of a cell is >= t exactly where the nearest cell of
    {v >= t} lies within r"""
    from parasitoids_amd.predictive import NeighbourhoodFields, ProximityFields
    pm = _pop_model(R, mode='exact')
    _evaluate(pm, MEMBERS[1])
    fields = _fields(pm, range(6))
    day = 3
    t = _thresholds(fields, day)[1]
    # the same evaluation seen on 25 m cells: the handles take the grid from the model's rad_dist / rad_res
    grid = types.SimpleNamespace(rad_dist=25.0 * R, rad_res=R, device=pm.device, solver=pm.solver, _nd=pm._nd,
                                 r_number=pm.r_number)
    radii = [0.0, 1.0, np.sqrt(2.0) * 25.0, 200.0, 800.0]
    with NeighbourhoodFields(grid, [(day, r) for r in radii]) as NF, ProximityFields(grid, [(day, t)]) as PF:
        assert NF.r2 == [0, 0, 2, 64, 1024] and PF.cell_m == 25.0
        NF.apply()
        PF.apply()
        d2 = PF.d2(0)
        assert np.array_equal(d2, prox_ref.d2(fields[day] >= t))
        for e, r2 in enumerate(NF.r2):
            assert np.array_equal(NF.field(e) >= t, d2 <= r2), (e, r2)
        assert np.array_equal(PF.field(0), np.sqrt(d2.astype(np.float64)) * 25.0)
    pm.close()


ACC_W = [1, 3, 2]
ACC_M = [MEMBERS[0], MEMBERS[1], MEMBERS[3]]
RADII = [400.0, 1600.0, 6000.0]
LEVELS = [0.05, 0.5, 0.95]


@pytest.fixture(scope='module')
def fed():
    """three members with weights 1, 3, 2 on one exact-mode model (the same member gives the same bits each time):
    their fields first, from which a threshold is taken that the second window's set of one member misses
    altogether; then one posterior fed in sequence, and two that share the members and are merged"""
    from parasitoids_amd.predictive import ProximityFields, ProximityPosterior
    f = types.SimpleNamespace()
    pm = f.pm = _pop_model(R, mode='exact')
    f.v = []
    for m in ACC_M:
        _evaluate(pm, m)
        f.v.append(_fields(pm, range(6)))
    tops = sorted(v[5].max() for v in f.v)
    f.windows = [(2, _thresholds(f.v[0], 2)[0], 'to'), (5, float(np.float32(0.5 * (tops[0] + tops[1]))), 'to'),
                 (2, _thresholds(f.v[0], 2)[1], 'in')]
    f.empty = [i for i, v in enumerate(f.v) if not (v[5] >= f.windows[1][1]).any()]
    f.Z = [np.array([prox_ref.field(v[d], t, side, CELL)[1] for d, t, side in f.windows]) for v in f.v]
    f.PF = ProximityFields(pm, f.windows)
    f.P = ProximityPosterior(f.PF, RADII, LEVELS)
    f.A, f.B = ProximityPosterior(f.PF, RADII, LEVELS), ProximityPosterior(f.PF, RADII, LEVELS)
    f.got = []
    for i, (m, w) in enumerate(zip(ACC_M, ACC_W)):
        _evaluate(pm, m)
        f.P.add(w)
        (f.A if i < 2 else f.B).add(w)
        f.got.append(np.array([f.PF.field(e) for e in range(3)]))
    f.A.merge(f.B)
    yield f
    for post in (f.A, f.B):
        post.fields = None                # the handle is f.P's to close
        post.close()
    f.P.close()
    pm.close()


def test_the_posterior_against_numpy_loops_over_the_reference_fields(fed):
    P = fed.P
    assert len(fed.empty) == 1                                    # one member's set is empty in the second window
    for z, got in zip(fed.Z, fed.got):
        assert np.array_equal(z, got)
    assert (fed.Z[fed.empty[0]][1] == P.far_m).all()
    assert P.thresholds == RADII + [P.far_m] and P.summary.thresholds == P.thresholds
    assert (P.summary.total_weight, P.summary.members) == (6.0, 3)
    st = RR.new_state(fed.Z[0].shape, P.thresholds, 1)            # the replay the neighbourhood test uses
    for z, w in zip(fed.Z, ACC_W):
        RR.add(st, z, [0.0], w)
    sc = st[0]
    W = float(sum(ACC_W))
    for e in range(3):
        assert np.array_equal(P.mean(e), sc['mean'][e]), e                        # bit for bit
        scale = np.abs(sc['mean'][e]).max()
        np.testing.assert_allclose(P.summary.variance(e), RR.variance(sc)[e], rtol=1e-12, atol=1e-15 * scale ** 2)
        np.testing.assert_allclose(P.sd(e), np.sqrt(np.maximum(RR.variance(sc)[e], 0.0)), rtol=1e-6, atol=1e-7 * scale)
        for k, r in enumerate(RADII):                                             # the counts, exactly
            count = sum(w * (z[e] >= r) for z, w in zip(fed.Z, ACC_W))
            assert np.array_equal(P.beyond(e, k) * W, count), (e, k)
            assert np.array_equal(P.nearer(e, k), 1.0 - P.beyond(e, k))
        share = sum(w for i, w in enumerate(ACC_W) if (fed.Z[i][e] == P.far_m).all()) / W
        assert P.empty_share(e) == share
    assert P.empty_share(1) == ACC_W[fed.empty[0]] / W and P.empty_share(0) == 0.0
    assert np.unique(P.beyond(0, 0)).size > 1                     # the map is not the same everywhere


def test_the_histogram_the_quantiles_and_the_radius(fed):
    from parasitoids_amd.predictive import default_ladder
    P = fed.P
    edges = P.histogram.edges
    assert np.array_equal(edges, default_ladder(CELL, P.far_m)) and P.ladder == list(edges)
    for e in range(3):
        want = hist_ref.weighted_counts([z[e] for z in fed.Z], ACC_W, edges)
        assert np.array_equal(P.histogram.counts(e).astype(np.int64), want), e
        for p in LEVELS:
            _b, value, _lo, _hi = hist_ref.quantile_from_counts(want, edges, p)
            np.testing.assert_allclose(P.quantile(e, p), value, rtol=1e-12, atol=0.0)
        for level in (0.3, 0.5, 1.0):
            loop = np.full((N, N), np.nan)
            for k in range(len(edges) - 1, -1, -1):              # the loop over the ladder
                near = 1.0 - hist_ref.exceedance_from_counts(want, k)
                loop = np.where(near >= level, edges[k], loop)
            assert np.array_equal(P.radius(e, level), loop, equal_nan=True), (e, level)
    # where a member has no such ground, only the last rung, the one beyond far_m, reaches every member
    assert edges[-1] > P.far_m >= edges[-2]
    assert (P.radius(1, 1.0) == edges[-1]).all() and not np.isnan(P.radius(1, 0.5)).any()
    assert (P.radius(1, 0.5) < edges[-1]).any()


def test_merge_of_two_posteriors_equals_one_fed_in_sequence(fed):
    P, A = fed.P, fed.A
    assert (A.summary.total_weight, A.summary.members) == (6.0, 3)
    for e in range(3):
        for k in range(3):
            assert np.array_equal(A.beyond(e, k), P.beyond(e, k))
        assert A.empty_share(e) == P.empty_share(e)
        assert np.array_equal(A.histogram.counts(e), P.histogram.counts(e))
        scale = np.abs(P.mean(e)).max()
        np.testing.assert_allclose(A.mean(e), P.mean(e), rtol=1e-13, atol=1e-15 * scale)
        np.testing.assert_allclose(A.summary.variance(e), P.summary.variance(e), rtol=1e-10, atol=1e-13 * scale ** 2)
        for p in LEVELS:
            assert np.array_equal(A.quantile(e, p), P.quantile(e, p))
    from parasitoids_amd.predictive import ProximityPosterior
    other = ProximityPosterior(fed.PF, RADII[:2])
    try:
        with pytest.raises(ValueError, match='different'):
            P.merge(other)
    finally:
        other.fields = None
        other.close()


def test_the_other_sources():
    from parasitoids_amd.predictive import Projection, ProximityFields, ReleaseSites
    pm = _pop_model(R, mode='exact')
    _evaluate(pm, MEMBERS[0])
    fields = _fields(pm, range(6))
    days = [0, 1, 3, 5]
    windows = [(3, _thresholds(fields, 3)[0]), (1, _thresholds(fields, 1)[1], 'in'), (5, _thresholds(fields, 5)[0])]
    by_index = [(days.index(t[0]),) + tuple(t[1:]) for t in windows]
    plan_days = [1, 3, 5]
    with ProximityFields(pm, windows) as PF, Projection(pm, np.eye(4), days) as P, \
            ProximityFields.for_projection(P, by_index) as PP, \
            ReleaseSites(pm, [(0.0, 0.0, 0.6), (7 * CELL, -3 * CELL, 0.5)], plan_days) as RS, \
            ProximityFields.for_projection(RS, windows) as PS:
        PF.apply()
        # identity weights: the projection's outputs are the day fields, and so are their distances
        P.apply()
        PP.apply()
        assert PP.in_days is None
        for e in range(3):
            assert np.array_equal(PP.d2(e), PF.d2(e)) and np.array_equal(PP.field(e), PF.field(e))
        # a release plan of two sites: the restatement applied to the plan's fetched fields
        RS.apply()
        PS.apply()
        plan = {d: RS.field(e) for e, d in enumerate(plan_days)}
        for e, (day, t, side) in enumerate(PS.windows):
            want_d2, want_m = prox_ref.field(plan[day], t, side, CELL)
            assert np.array_equal(PS.d2(e), want_d2) and np.array_equal(PS.field(e), want_m), e
        with pytest.raises(ValueError, match='output'):
            ProximityFields.for_projection(RS, [(2, 1.0)])
        with pytest.raises(ValueError, match='output'):
            ProximityFields.for_projection(P, [(4, 1.0)])
        W = np.eye(4)
        W[2] = 0.0
        with Projection(pm, W, days) as P0:
            with pytest.raises(ValueError, match='carries weight'):
                ProximityFields.for_projection(P0, [(2, 1.0)])
    pm.close()


def test_refusals_of_the_c_abi():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import Projection, ProximityFields, SpreadSummary
    lib = L.load()

    def create(nin, nout, inputs, thr, side, n=N, cell=CELL):
        h = L._VP()
        rc = lib.ps_prox_create(0, n, nin, nout, L.p_i32(L.i32(inputs)), L.p_f64(L.f64(thr)), L.p_i32(L.i32(side)),
                                cell, C.byref(h))
        if rc == L.PS_OK:
            lib.ps_prox_destroy(h)
        return rc
    assert create(2, 2, [0, 1], [1.0, 2.0], [0, 1]) == L.PS_OK
    assert create(1, 32, [0] * 32, [1.0] * 32, [0] * 32) == L.PS_OK
    for args in [(0, 1, [0], [1.0], [0]), (33, 1, [0], [1.0], [0]), (1, 0, [0], [1.0], [0]),
                 (1, 33, [0] * 33, [1.0] * 33, [0] * 33), (2, 1, [2], [1.0], [0]), (2, 1, [-1], [1.0], [0]),
                 (1, 1, [0], [1.0], [2]), (1, 1, [0], [1.0], [-1]), (1, 1, [0], [float('nan')], [0])]:
        assert create(*args) == L.PS_ERR_BAD_ARG, args
    assert create(1, 1, [0], [1.0], [0], n=0) == L.PS_ERR_BAD_ARG
    assert create(1, 1, [0], [1.0], [0], n=32768) == L.PS_ERR_BAD_ARG          # a squared distance past 32 bits
    assert create(1, 1, [0], [1.0], [0], cell=0.0) == L.PS_ERR_BAD_ARG
    # null handles
    out = np.empty((N, N))
    assert lib.ps_prox_fetch(None, 0, L.p_f64(out)) == L.PS_ERR_BAD_ARG
    assert lib.ps_prox_fetch_d2(None, 0, None) == L.PS_ERR_BAD_ARG
    assert lib.ps_prox_set_strip(None, 0) == L.PS_ERR_BAD_ARG
    assert lib.ps_prox_info(None, None, None, None, None, None) == L.PS_ERR_BAD_ARG
    assert lib.ps_prox_prof(None, -1, None, None, None, None) == L.PS_ERR_BAD_ARG
    assert lib.ps_prox_gather(None, 0, None, None, None) == L.PS_ERR_BAD_ARG
    assert lib.ps_prox_apply_project(None, None) == L.PS_ERR_BAD_ARG
    assert lib.ps_prox_apply_sites(None, None) == L.PS_ERR_BAD_ARG
    lib.ps_prox_destroy(None)
    pm = _pop_model(R)
    with ProximityFields(pm, [(1, 1.0), (2, 1.0, 'in')]) as PF, \
            SpreadSummary.for_projection(PF, [100.0, PF.far_m]) as S, \
            Projection(pm, np.eye(3), [0, 1, 2]) as P3, SpreadSummary.for_projection(P3, [1.0]) as S3, \
            ProximityFields(pm, [(9, 1.0)]) as P9:
        with pytest.raises(ValueError, match='evaluation'):
            PF.apply()
        _evaluate(pm, MEMBERS[0])
        with pytest.raises(ValueError, match='evaluation'):
            P9.apply()
        for call in (lambda: PF.field(0), lambda: PF.d2(0), lambda: PF.gather([0], [0]), lambda: S.add(1)):
            with pytest.raises(L.HipError) as ei:
                call()
            assert ei.value.code == L.PS_ERR_STATE
        kind, idx, delta = L.i32([L.REC_CHAIN] * 2), L.i32([0, 1]), L.i32([1, 1])
        one = L.f64([1.0, 1.0])
        assert lib.ps_prox_apply(None, pm.solver._h, 2, L.p_i32(kind), L.p_i32(idx), L.p_f64(one), L.p_f64(one),
                                 L.p_i32(delta), 1e-8) == L.PS_ERR_BAD_ARG
        assert lib.ps_prox_apply(PF._h, None, 2, L.p_i32(kind), L.p_i32(idx), L.p_f64(one), L.p_f64(one),
                                 L.p_i32(delta), 1e-8) == L.PS_ERR_BAD_ARG
        assert lib.ps_prox_apply(PF._h, pm.solver._h, 3, L.p_i32(kind), L.p_i32(idx), L.p_f64(one), L.p_f64(one),
                                 L.p_i32(delta), 1e-8) == L.PS_ERR_BAD_ARG      # three inputs given, the handle has two
        other = L._VP()                                                          # a handle of another domain
        L.check(lib.ps_prox_create(0, N + 2, 2, 2, L.p_i32(L.i32([0, 1])), L.p_f64(one), L.p_i32(L.i32([0, 0])), CELL,
                                   C.byref(other)))
        assert lib.ps_prox_apply(other, pm.solver._h, 2, L.p_i32(kind), L.p_i32(idx), L.p_f64(one), L.p_f64(one),
                                 L.p_i32(delta), 1e-8) == L.PS_ERR_BAD_ARG
        lib.ps_prox_destroy(other)
        assert PF.applies == 0
        PF.apply()
        assert lib.ps_summary_add_prox(S3._h, PF._h, 1) == L.PS_ERR_BAD_ARG       # three slots, two outputs
        assert S3.members == 0
        assert lib.ps_summary_add_prox(S._h, PF._h, 0) == L.PS_ERR_BAD_ARG        # weight >= 1
        assert lib.ps_summary_add_prox(S._h, None, 1) == L.PS_ERR_BAD_ARG
        assert lib.ps_summary_add_prox(None, PF._h, 1) == L.PS_ERR_BAD_ARG
        assert lib.ps_hist_add_prox(None, PF._h, 1) == L.PS_ERR_BAD_ARG
        assert lib.ps_mcerr_add_prox(None, PF._h, 1) == L.PS_ERR_BAD_ARG
        assert lib.ps_wsum_add_prox(None, PF._h, 1, None, None) == L.PS_ERR_BAD_ARG
        assert lib.ps_prox_apply_project(PF._h, P3._h) == L.PS_ERR_STATE          # P3 not applied yet
        P3.apply()
        assert lib.ps_prox_apply_project(PF._h, P3._h) == L.PS_ERR_BAD_ARG        # 3 outputs, 2 inputs
        assert PF.applies == 1
        with pytest.raises(ValueError):
            PF.field(2)
        with pytest.raises(L.HipError):
            PF.gather([N], [0])
        S.add(2)
        assert S.members == 1 and S.total_weight == 2.0
    pm.close()


def _csr(f, key):
    from scipy import sparse
    return sparse.csr_matrix((f[key + '_data'], f[key + '_ind'], f[key + '_indptr']), shape=(N, N)).toarray()


def test_posterior_predictive_with_proximity_against_the_class_fed_by_hand(tmp_path):
    from parasitoids_amd import mcmc
    from parasitoids_amd import predictive as PR
    from test_reweight_gpu import _chain
    THR = [1.0, 10.0]
    ta, names = _chain([3, 2])
    tb, _ = _chain([1, 2, 2])
    traces = [ta, tb[1:]]                                    # the second chain: two runs of other members
    chains = [(t, names) for t in traces]
    plan = dict(sites=[(0.0, 0.0, 0.6), (7 * CELL, -3 * CELL, 0.5)], days=[0, 1, 5])     # day 3 is no output day
    pm = _pop_model(R, mode='exact')
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        pm.evaluate(*mcmc.model_args(ta[0, cols]), want_stats=False)
    fields = _fields(pm, range(6))
    windows = [(3, _thresholds(fields, 3)[1]), (5, _thresholds(fields, 5)[0], 'in')]
    arg = dict(windows=windows, radii_m=[400.0, 1600.0], levels=[0.5])
    common = dict(thresholds=THR, sites=plan, quantiles=[0.5], mc_error=dict(batches=4), cell_area=CELL ** 2)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        res = PR.posterior_predictive(pm, chains, proximity=arg, **common)
        bare = PR.posterior_predictive(pm, chains, **common)
    px = res.proximity
    assert res.failed == 0 and res.evaluations == 4 and bare.proximity is None and bare.sites.proximity is None
    assert px.windows == [windows[0] + ('to',), windows[1]] and px.radii_m == [400.0, 1600.0]
    assert px.given['windows'] == [list(w) for w in px.windows] and px.levels == [0.5]
    assert (px.summary.total_weight, px.summary.members) == (9.0, 4)
    assert res.sites.proximity.windows == [windows[1]]               # the window on the plan's output days
    # the other maps are what they are without proximity=
    for got, want in ((res.summary, bare.summary), (res.sites.summary, bare.sites.summary)):
        for d in want.days:
            assert np.array_equal(got.mean(d), want.mean(d)) and np.array_equal(got.variance(d), want.variance(d))
            for k in range(2):
                assert np.array_equal(got.exceedance(d, k), want.exceedance(d, k))
    for d in bare.histogram.days:
        assert np.array_equal(res.histogram.counts(d), bare.histogram.counts(d))
    assert np.array_equal(res.mc_error.mcse(1), bare.mc_error.mcse(1), equal_nan=True)
    # the class fed by hand: every run once more, per chain a posterior of its own, merged in chain order
    hand = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        PF = PR.ProximityFields(pm, windows)
        for ci in range(2):
            hand.append(PR.ProximityPosterior(PF, arg['radii_m'], arg['levels']))
            for c, first, weight in res.runs:
                if c == ci:
                    pm.evaluate(*mcmc.model_args(traces[ci][first, cols]), want_stats=False)
                    hand[ci].add(weight)
        hand[0].merge(hand[1])
    want = hand[0]
    for e in range(2):
        assert np.array_equal(px.mean(e), want.mean(e)) and np.array_equal(px.sd(e), want.sd(e)), e
        for k in range(2):
            assert np.array_equal(px.beyond(e, k), want.beyond(e, k)), (e, k)
        assert px.empty_share(e) == want.empty_share(e) == 0.0
        assert np.array_equal(px.quantile(e, 0.5), want.quantile(e, 0.5))
        assert np.array_equal(px.radius(e, 0.5), want.radius(e, 0.5), equal_nan=True)
    assert px.mc_error.batches >= 4 and px.mc_error.thresholds == px.thresholds
    assert np.isfinite(px.mc_error.mcse(0)).all()
    # the files
    npz, js = res.save(str(tmp_path / 'a' / 'pp'))
    bare.save(str(tmp_path / 'b' / 'pp'))
    names_a, names_b = sorted(os.listdir(str(tmp_path / 'a'))), sorted(os.listdir(str(tmp_path / 'b')))
    assert sorted(set(names_a) - set(names_b)) == ['pp_prox.npz', 'pp_sites_prox.npz']
    for name in names_b:
        if name.endswith('.npz') and name != 'pp_mcerr.npz':      # the Monte Carlo error file gains the new blocks
            fa, fb = np.load(str(tmp_path / 'a' / name)), np.load(str(tmp_path / 'b' / name))
            assert fa.files == fb.files and all(np.array_equal(fa[k], fb[k]) for k in fb.files), name
    f = np.load(str(tmp_path / 'a' / 'pp_prox.npz'))
    assert list(f['days']) == [3, 5] and list(f['sides']) == ['to', 'in'] and list(f['radii_m']) == [400.0, 1600.0]
    assert list(f['thresholds']) == [w[1] for w in windows] and float(f['far_m']) == px.far_m
    assert np.array_equal(f['ladder'], px.histogram.edges) and list(f['empty_share']) == [0.0, 0.0]
    for e in range(2):
        for key, m in (('x%d' % e, px.mean(e)), ('x%d_sd' % e, px.sd(e)), ('x%d_pnear1' % e, px.nearer(e, 1)),
                       ('x%d_q50' % e, px.quantile(e, 0.5))):
            assert np.array_equal(_csr(f, key), np.where(m >= 1e-8, m, 0.0)), key
    meta = json.load(open(js))['predictive']
    block = meta['proximity']
    assert block['given'] == px.given and block['members'] == 4 and block['total_weight'] == 9.0
    for e, out in enumerate(block['outputs']):
        assert out['window'] == list(px.windows[e]) and out['empty_share'] == 0.0
        assert out['area'] == [float((px.nearer(e, k) >= 0.5).sum() * CELL ** 2) for k in range(2)]
    assert len(meta['sites']['proximity']['outputs']) == 1
    assert 'proximity' in meta['mc_error'] and 'sites_proximity' in meta['mc_error']
    meta_b = json.load(open(str(tmp_path / 'b' / 'pp.json')))['predictive']
    assert 'proximity' not in meta_b and 'proximity' not in meta_b['sites']
    hand[1].fields = None
    for h in (hand[0], hand[1], res.summary, res.histogram, res.mc_error, res.sites, px, bare.summary, bare.histogram,
              bare.mc_error, bare.sites):
        h.close()
    pm.close()

"""GPU tests of the pathway maps (ps_pathway_*, predictive.PathwayMaps): the crafted sequences at N = 129 (N * N =
260 * 64 + 1: the last wave holds one real cell), each slot injected through HipSolve.set_state and kept as a chain
record, then the model's fields -- every count plane and every row bit for bit against the numpy restatement
(pathway_ref) run on the device's own fields, the ties to ArrivalMaps, weights, add and merge order, reset, growth of
the member rows, solver switches, a release plan as the source, the refusals, and posterior_predictive with
pathways=.  Kalbar wind, R = 128, 6 days, the members, weights and helpers of test_arrival_gpu.py."""
import ctypes as C
import json
import warnings

import numpy as np
import pytest

import pathway_ref as W
import patch_ref as P
import test_arrival_gpu as TA

pytestmark = pytest.mark.gpu

MEMBERS, WEIGHTS = TA.MEMBERS, TA.WEIGHTS
THR3 = [1.0, 10.0, 100.0]
_pop_model, _evaluate, _fields = TA._pop_model, TA._evaluate, TA._fields
LEVELS = (0.05, 0.3, 0.5, 0.95, 1.0)
U32P = C.POINTER(C.c_uint32)


def _check_against_reference(G, fields, weights, check_maps=True):
    """every device output of G against the numpy reference of the members' [nslot, N, N] fields -> the reference"""
    from parasitoids_amd.predictive import pathway_founded, range_area
    ref = W.accumulate(fields, weights, G.thresholds, G.connectivity, G.anchors)
    Wt = float(sum(weights))
    assert G.total_weight == Wt and G.members == len(fields) and G.weights.tolist() == list(weights)
    for k in range(len(G.thresholds)):
        total = np.zeros((G.N, G.N), dtype=np.int64)
        for which in W.CLASSES:
            got = G.counts(k, which)
            assert got.dtype == np.uint32 and got.shape == ref[which].shape[1:]
            assert np.array_equal(got.astype(np.int64), ref[which][k]), (k, which)
            total += ref[which][k]
            if check_maps:
                assert np.array_equal(G.prob(k, which), ref[which][k].astype(np.float64) / Wt), (k, which)
        if check_maps:
            for j, which in enumerate(W.CLASSES):
                share = G.share(k, which)
                assert np.array_equal(np.isnan(share), total == 0), (k, which)
                hit = total > 0
                assert np.array_equal(share[hit], ref[which][k][hit] / total[hit].astype(np.float64))
                cells = ref['rows'][:, k, :, j].sum(axis=1)
                assert G.area(k, which, LEVELS) == range_area(cells, weights, G.cell_area, LEVELS)
            assert G.founded(k, LEVELS) == pathway_founded(ref['rows'][:, k, :, 3].sum(axis=1), weights, LEVELS)
        for s, d in enumerate(G.days):
            for j, which in enumerate(W.CLASSES):
                got = G.new_cells(k, d, which)
                assert got.dtype == np.int64 and np.array_equal(got, ref['rows'][:, k, s, j]), (k, d, which)
            assert np.array_equal(G.foci(k, d), ref['rows'][:, k, s, 3]), (k, d)
    return ref


@pytest.mark.parametrize('connectivity', [4, 8])
def test_crafted_sequences_at_a_wave_and_one_cell(connectivity):
    """every crafted sequence as one member, weights 1..3, three nested histories per add; one handle per set of
    anchors; the reference runs on the fields the device holds"""
    from parasitoids_amd import _lib as L
    from parasitoids_amd import hip_lib
    from scipy import sparse
    N = 129
    seqs = W.sequences(N)
    lib, dev = L.load(), L.default_device()
    delta = sparse.coo_matrix(([1.0], ([1], [1])), shape=(3, 3))        # a day kernel that moves nothing
    s = hip_lib.HipSolve(sparse.coo_matrix(seqs[1][1][0]), [5, 5], mode='exact')
    s.set_kernels([delta] * W.NSLOT)
    kind, idx = L.i32([L.REC_CHAIN] * W.NSLOT), L.i32(list(range(W.NSLOT)))
    one, zero = L.f64([1.0] * W.NSLOT), L.i32([0] * W.NSLOT)
    groups = {}
    for i, (name, f, anchors) in enumerate(seqs):
        groups.setdefault(tuple(anchors), []).append((name, f, 1 + i % 3))
    assert len(groups) == 2
    seen = {}
    try:
        for anchors, members in groups.items():
            h = L._VP()
            L.check(lib.ps_pathway_create(dev, N, W.NSLOT, 3, L.p_f64(L.f64(P.SHAPE_THR)), connectivity, len(anchors),
                                          L.p_i32(L.i32([a[0] for a in anchors])),
                                          L.p_i32(L.i32([a[1] for a in anchors])), C.byref(h)))
            try:
                fields, weights = [], []
                for name, f, w in members:
                    for t in range(W.NSLOT):                   # one slot per state: chain record t holds slot t
                        s.set_state(sparse.coo_matrix(f[t]))
                        s.run_chain(t, 1, renorm=False)
                    L.check(lib.ps_pathway_add(h, s._h, W.NSLOT, L.p_i32(kind), L.p_i32(idx), L.p_f64(one), L.p_f64(one),
                                               L.p_i32(zero), W.NEGVAL, w))
                    back = W.record_value(np.array([s.dense(L.REC_CHAIN, t) for t in range(W.NSLOT)]))
                    for thr in P.SHAPE_THR:                    # the device holds the crafted history
                        assert np.array_equal(back >= thr, f >= thr), (name, thr)
                    fields.append(back)
                    weights.append(w)
                ref = W.accumulate(fields, weights, P.SHAPE_THR, connectivity, list(anchors))
                m = len(fields)
                for k in range(3):
                    for j, which in enumerate(W.CLASSES):
                        got = np.empty((N, N), dtype=np.uint32)
                        L.check(lib.ps_pathway_fetch_counts(h, k, j, got.ctypes.data_as(U32P)))
                        assert np.array_equal(got.astype(np.int64), ref[which][k]), (k, which)
                    for t in range(W.NSLOT):
                        rows = [np.empty(m, dtype=np.uint32) for _ in range(5)]
                        L.check(lib.ps_pathway_fetch_members(h, k, t, *[a.ctypes.data_as(U32P) for a in rows]))
                        for f, word in enumerate(W.ROW):
                            bad = np.flatnonzero(rows[f].astype(np.int64) != ref['rows'][:, k, t, f])
                            assert bad.size == 0, (k, t, word, [members[i][0] for i in bad])
                        assert rows[4].tolist() == weights
                        if k == 0:
                            for i, (name, _f, _w) in enumerate(members):
                                seen.setdefault(name, []).append([int(rows[f][i]) for f in range(4)])
            finally:
                lib.ps_pathway_destroy(h)
        # not vacuous: what the sequences are there for, from the device's rows at the lowest threshold
        c4 = connectivity == 4
        assert seen['empty'] == [[0, 0, 0, 0]] * 4 and seen['grow'][3] == [40, 0, 0, 0]
        assert seen['jump_grow_merge'] == [[9, 6, 0, 1], [0, 0, 6, 0], [2, 0, 0, 0], [5, 0, 0, 0]]
        assert seen['two_foci_diagonal'][1] == ([0, 8, 0, 2] if c4 else [4, 4, 0, 1])
        assert seen['dropout_reenter'] == [[9, 6, 0, 1], [0, 0, 0, 0], [0, 0, 5, 0], [0, 4, 0, 1]]
        assert seen['anchor_late'][:2] == [[0, 6, 0, 1], [9, 0, 0, 0]] and seen['origin_wins'][1] == [7, 0, 0, 0]
        assert seen['two_anchors'][:2] == [[18, 0, 0, 0], [0, 9, 0, 1]]
        assert seen['ring_island'] == [[32, 0, 0, 0], [0, 1, 0, 1], [0, 0, 2, 0], [2, 0, 0, 0]]
        assert seen['edge_next_row'][1] == [0, 2, 0, 2] and seen['last'][2] == [0, 1, 0, 1]
    finally:
        s.close()


@pytest.mark.parametrize('prob_model', [False, True])
def test_device_maps_match_the_numpy_reference(prob_model):
    from parasitoids_amd.predictive import ArrivalMaps, PathwayMaps
    pm = _pop_model(prob_model=prob_model, mode='exact')
    days, sub = list(range(6)), [0, 2, 5]
    scale = 1.0 / 130000 if prob_model else 1.0     # prob_model holds probabilities: the same densities
    thr = [t * scale for t in THR3]
    fields = []
    with PathwayMaps(pm, thr) as G, PathwayMaps(pm, thr, connectivity=8) as G8, PathwayMaps(pm, thr, sub) as Gs, \
            PathwayMaps(pm, thr, sub, connectivity=8) as Gs8, ArrivalMaps(pm, thr) as A, ArrivalMaps(pm, thr, sub) as As:
        assert G.days == days and Gs.days == sub and G.N == 257 and G.cell_area == (10000.0 / 128) ** 2
        assert G.thresholds == thr and G.connectivity == 4 and G8.connectivity == 8 and G.capacity >= 1
        assert G.anchors == [(128, 128)]
        pitch = (257 * 257 + 63) // 64 * 64
        assert G.nbytes == (12 * 3 + 8 * 3 * 6 + 3) * pitch + 16 * 3 * 6 * G.capacity      # the documented formula
        for mem, w in zip(MEMBERS, WEIGHTS):
            _evaluate(pm, mem)
            for acc in (G, G8, Gs, Gs8, A, As):
                acc.add(w)
            fields.append(_fields(pm, days))
        _check_against_reference(G, fields, WEIGHTS)
        _check_against_reference(G8, fields, WEIGHTS, check_maps=False)
        _check_against_reference(Gs, [f[sub] for f in fields], WEIGHTS, check_maps=False)
        _check_against_reference(Gs8, [f[sub] for f in fields], WEIGHTS, check_maps=False)
        # the three classes partition what arrived within the window, and per member the cells reached by each day
        for H, B in ((G, A), (G8, A), (Gs, As), (Gs8, As)):
            for k in range(3):
                total = sum(H.counts(k, which).astype(np.int64) for which in W.CLASSES)
                assert np.array_equal(total, sum(B.counts(k, d).astype(np.int64) for d in H.days)), k
                reached, w = B.reached(k)
                new = sum(np.array([H.new_cells(k, d, which) for d in H.days]).T for which in W.CLASSES)
                assert np.array_equal(new, np.diff(reached, axis=1, prepend=0)) and w.tolist() == WEIGHTS
        # not vacuous, from the device's own rows
        for d in days:                               # at t = 1 the front takes every cell
            assert not G.new_cells(0, d, 'jump').any() and not G.new_cells(0, d, 'secondary').any()
            assert G.foci(0, d).tolist() == [0] * len(MEMBERS)
        assert not G.counts(0, 'jump').any() and not G.counts(0, 'secondary').any() and G.counts(0, 'front').any()
        first = G.foci(1, 0)                         # at t = 10 some members found a focus on day 0, one does not
        assert (first > 0).any() and (first == 0).any()
        for which in W.CLASSES:                      # at t = 100 all three classes occur
            assert G.counts(2, which).any(), which
        print('foci at t = 10, day 0..5, per member: %r; prob_model=%r'
              % ([G.foci(1, d).tolist() for d in days], prob_model))
    pm.close()


def _same_planes(a, b):
    return all(np.array_equal(a.counts(k, w), b.counts(k, w)) for k in range(len(a.thresholds)) for w in W.CLASSES)


def _rows(G):
    """per member (weight, the four row words over all thresholds and days) as comparable tuples"""
    w = G.weights.tolist()
    r = np.array([[G._members(k, d)[:4] for d in G.days] for k in range(len(G.thresholds))])   # [K, days, 4, members]
    return [(w[m], r[:, :, :, m].tobytes()) for m in range(len(w))]


def test_weights_add_order_and_merge_order_do_not_change_a_bit():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import PathwayMaps
    pm = _pop_model(mode='exact')
    days = [0, 2, 5]
    hs = [PathwayMaps(pm, THR3, days) for _ in range(7)]
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
    # the reversed order evaluates every member anew; in exact mode an evaluation repeats to the last bit
    assert all(np.array_equal(a, b) for a, b in zip(f_fwd, f_rev[::-1]))
    assert _same_planes(rev, fwd) and _rows(rev) == rf[::-1]
    _check_against_reference(rev, f_rev, WEIGHTS[::-1])
    _check_against_reference(fwd, f_fwd, WEIGHTS)
    assert _rows(unit) == [(1,) + r[1:] for r, w in zip(rf, WEIGHTS) for _ in range(w)]
    assert fwd.founded(1) == b2.founded(1) == unit.founded(1)
    with PathwayMaps(pm, THR3, days) as e:          # merging into an empty handle
        e.merge(fwd)
        assert _same_planes(e, fwd) and _rows(e) == rf
    for other in (PathwayMaps(pm, [1.0, 20.0, 100.0], days), PathwayMaps(pm, THR3, days, connectivity=8),
                  PathwayMaps(pm, THR3, days, anchors=[(128, 128), (3, 3)])):
        with other:
            other.add(1)
            with pytest.raises(L.HipError) as err:
                fwd.merge(other)                       # different thresholds, another connectivity, other anchors
            assert err.value.code == L.PS_ERR_BAD_ARG
    with PathwayMaps(pm, THR3, [0, 2, 4]) as other, pytest.raises(ValueError):
        fwd.merge(other)                           # different days
    assert _rows(fwd) == rf and fwd.members == len(MEMBERS)
    for h in hs:
        h.close()
    pm.close()


def test_reset_starts_over_and_the_rows_grow_past_the_reserve():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import PathwayMaps
    pm = _pop_model(ndays=3)
    thr = [1.0, 10.0]
    fields = []
    with PathwayMaps(pm, thr) as G:
        cap0, base = G.capacity, G.nbytes
        G.reserve(cap0 + 1)
        assert G.capacity == 2 * cap0 and G.nbytes == base + cap0 * 2 * 3 * 16       # 16 B per member, k and slot
        weights = [1 + r % 3 for r in range(cap0 + 6)]                             # 70 members
        assert len(weights) == 70
        G.reset()
        G2 = PathwayMaps(pm, thr)                    # this one starts at the rows of create and has to grow
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
        for call in (lambda: G.counts(0, 'front'), lambda: G.foci(0, 1), lambda: G.new_cells(1, 2, 'jump')):
            with pytest.raises(L.HipError) as err:
                call()
            assert err.value.code == L.PS_ERR_STATE
        G.add(2)                                   # the last evaluation once more, alone
        _check_against_reference(G, fields[-1:], [2])
    pm.close()


def test_members_on_different_cached_solvers_in_exact_mode():
    """the kernel extent moves with the diffusion parameters; in exact mode each extent has its own solver and
    stream, and successive adds from them -- which share the handle's scratch -- are ordered by its event"""
    from parasitoids_amd.predictive import PathwayMaps
    pm = _pop_model(mode='exact')
    mems = [((120.0, 100.0, 0.2), 1.0), ((260.0, 230.0, 0.25), 1.2), ((120.0, 100.0, 0.2), 1.05),
            ((200.0, 170.0, 0.1), 1.1)]
    w = [2, 1, 1, 3]
    solvers = set()
    with PathwayMaps(pm, THR3, [1, 2, 4]) as G:
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


def test_a_release_plan_as_the_source():
    from parasitoids_amd.predictive import PathwayMaps, Projection, ReleaseSites, exposure_weights, lagged_models
    Rr = 64
    res = 10000.0 / Rr
    pm = _pop_model(R=Rr)
    out = [0, 1, 2, 3, 5]
    sites = [(0.0, 0.0, 0.6, 0), (13 * res, 6 * res, 0.5, 2)]          # the second site two days later
    late = lagged_models(pm, [2])
    plan_f = []
    with ReleaseSites(pm, sites, out, late) as S, PathwayMaps.for_projection(S, THR3) as GS, \
            PathwayMaps.for_projection(S, THR3[:2], connectivity=8) as G8:
        assert GS.days == out and GS.anchors == [(64, 64), (64 - 6, 64 + 13)] and G8.connectivity == 8
        for mem, w in zip(MEMBERS[:3], WEIGHTS[:3]):
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                S.evaluate(TA.HP, mem[0], TA.DLP, mem[1], TA.NPER)       # the base model, the lagged one and the apply
            GS.add(w)
            G8.add(w)
            plan_f.append(np.array([S.field(e) for e in range(len(out))]))
        ref = _check_against_reference(GS, plan_f, WEIGHTS[:3])
        _check_against_reference(G8, plan_f, WEIGHTS[:3], check_maps=False)
        assert ref['rows'][:, 0, 2, 0].min() > 0     # not vacuous: every member's front takes new ground on day 2
        with Projection(pm, exposure_weights(list(range(6)), [0, 2]), list(range(6))) as X, pytest.raises(ValueError):
            PathwayMaps.for_projection(X, THR3)      # its outputs are not a sequence of days
    for m in late.values():
        m.close()
    pm.close()


def test_refusals_enqueue_nothing_and_the_device_stays_usable():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import NEGVAL, PathwayMaps, _day_scales, _day_slots
    lib = L.load()
    dev = L.default_device()
    h = L._VP()

    def create(N, nslot, thr, conn=4, anchors=((128, 128),), device=dev):
        return lib.ps_pathway_create(device, N, nslot, len(thr), L.p_f64(L.f64(thr)), conn, len(anchors),
                                     L.p_i32(L.i32([a[0] for a in anchors])), L.p_i32(L.i32([a[1] for a in anchors])),
                                     C.byref(h))
    thr = [1.0, 10.0]
    for bad in ([0.0, 1.0], [-1.0], [1.0, float('nan')], [float('inf')], [10.0, 1.0], [1.0, 1.0],
                [1.0, 2.0, 3.0, 4.0, 5.0]):                                     # more than 4 thresholds among them
        assert create(257, 6, bad) == L.PS_ERR_BAD_ARG and not h, bad
    for conn in (5, 0, 6, 16):
        assert create(257, 6, thr, conn) == L.PS_ERR_BAD_ARG and not h, conn
    assert create(257, 33, thr) == L.PS_ERR_BAD_ARG and not h                   # more than 32 slots
    assert create(257, 0, thr) == L.PS_ERR_BAD_ARG and not h
    assert create(257, 6, thr, anchors=[(1, 1)] * 33) == L.PS_ERR_BAD_ARG and not h      # more than 32 anchors
    assert create(257, 6, thr, anchors=[]) == L.PS_ERR_BAD_ARG and not h
    for off in ((257, 0), (0, 257), (-1, 5), (5, -1)):                          # an anchor off the grid
        assert create(257, 6, thr, anchors=[(128, 128), off]) == L.PS_ERR_BAD_ARG and not h, off
        assert b'off the' in lib.ps_last_error()
    assert create(5793, 6, thr) == L.PS_ERR_BAD_ARG and not h                   # N * N >= 2^25
    pm, small = _pop_model(), _pop_model(R=64)
    for bad_days in ([2, 1], [1, 1], list(range(33))):                          # unsorted days, too many
        with pytest.raises(ValueError):
            PathwayMaps(pm, thr, bad_days)
    with pytest.raises(ValueError):
        PathwayMaps(pm, thr, anchors=[(257, 0)])
    with PathwayMaps(pm, thr, [1, 4]) as G0, pytest.raises(ValueError):
        G0.add(1)                                                               # an add before an evaluation
    _evaluate(pm, MEMBERS[0])
    _evaluate(small, MEMBERS[0])
    days = [1, 4]
    kind, idx, delta = _day_slots(days)
    stat, post = _day_scales(pm, days)

    def add(handle, solver, n, w, k=None):
        return lib.ps_pathway_add(handle, solver._h, n, L.p_i32(kind if k is None else k), L.p_i32(idx), L.p_f64(stat),
                                  L.p_f64(post), L.p_i32(delta), NEGVAL, w)
    # a wrong device: a handle on another device takes no member of this solver; without one, no handle there at all
    if lib.ps_device_count() > 1:
        other = (dev + 1) % lib.ps_device_count()
        assert create(257, 2, thr, device=other) == L.PS_OK and h
        assert add(h, pm.solver, 2, 1) == L.PS_ERR_BAD_ARG and b'device' in lib.ps_last_error()
        lib.ps_pathway_destroy(h)
        h = L._VP()
    else:
        assert create(257, 2, thr, device=dev + 1) != L.PS_OK and not h
    with PathwayMaps(pm, thr, days) as G:
        for call in (lambda: G.counts(0, 'front'), lambda: G.prob(1, 'jump'), lambda: G.foci(0, 1),
                     lambda: G.founded(0), lambda: G.area(0, 'front')):
            with pytest.raises(L.HipError) as err:
                call()                                   # before the first add
            assert err.value.code == L.PS_ERR_STATE
        assert add(G._h, pm.solver, 3, 1) == L.PS_ERR_BAD_ARG                    # wrong slot count
        assert add(G._h, pm.solver, 2, 0) == L.PS_ERR_BAD_ARG                    # weight 0
        assert add(G._h, small.solver, 2, 1) == L.PS_ERR_BAD_ARG                 # a domain mismatch
        assert b'domain' in lib.ps_last_error()
        assert add(G._h, pm.solver, 2, 1, L.i32([L.REC_CHAIN, 99])) != L.PS_OK   # a bad slot: nothing enqueued
        with pytest.raises(ValueError):
            G.add(0)
        with pytest.raises(ValueError):
            G.counts(2, 'front')
        with pytest.raises(ValueError):
            G.foci(0, 3)
        with pytest.raises(ValueError):
            G.counts(0, 'main')
        out = np.empty((257, 257), dtype=np.uint32)
        assert lib.ps_pathway_fetch_counts(G._h, 0, 3, out.ctypes.data_as(U32P)) == L.PS_ERR_BAD_ARG
        assert G.members == 0 and G.total_weight == 0
        G.add(0xfffffffe)
        assert add(G._h, pm.solver, 2, 2) == L.PS_ERR_BAD_ARG and b'overflow' in lib.ps_last_error()   # W past 2^32 - 1
        G.add(1)                                                                 # W = 2^32 - 1 is the last one in
        assert G.members == 2 and G.total_weight == 0xffffffff
        X = _fields(pm, days)
        total = sum(G.counts(1, which).astype(np.int64) for which in W.CLASSES)
        assert np.array_equal(total, 0xffffffff * (X >= thr[1]).any(axis=0))
        G.reset()
        G.add(2)
        _check_against_reference(G, [X], [2])
    pm.close()
    small.close()


def _csr(f, key, N):
    from scipy import sparse
    return sparse.csr_matrix((f[key + '_data'], f[key + '_ind'], f[key + '_indptr']), shape=(N, N)).toarray()


def test_posterior_predictive_with_pathways_and_a_release_plan(tmp_path):
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
        res = PR.posterior_predictive(one, chains, thresholds=[1, 10], pathways=[1, 10], sites=arg)
        two = PR.posterior_predictive([pa, pb], chains, thresholds=[1, 10],
                                      pathways=dict(thresholds=[1, 10], connectivity=8, days=[0, 2, 3], levels=(0.5,)))
        plain = PR.posterior_predictive(one, chains, thresholds=[1, 10])
    assert plain.pathways is None and plain.pathway_levels is None
    assert res.failed == 0 and res.evaluations == 6 and len(res.runs) == 6
    G = res.pathways
    assert res.pathway_levels == [0.05, 0.5, 0.95] and two.pathway_levels == [0.5] and two.sites is None
    assert G.days == list(range(6)) and G.thresholds == [1.0, 10.0] and G.connectivity == 4 and G.anchors == [(64, 64)]
    assert two.pathways.connectivity == 8 and two.pathways.days == [0, 2, 3]
    assert G.total_weight == res.summary.total_weight == 9 and G.members == res.summary.members == 6
    # by hand: every run once more through the model, and through the numpy reference
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    fields, plan_f, weights = [], [], []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        with PR.ReleaseSites.with_lagged_models(pa, arg['sites'], out) as S, PR.PathwayMaps(pa, [1, 10]) as H:
            for ci, first, weight in res.runs:
                S.evaluate(*mcmc.model_args(chains[ci][0][first, cols]))
                H.add(weight)                                # the class driven by hand
                fields.append(_fields(pa, G.days))
                plan_f.append(np.array([S.field(e) for e in range(len(out))]))
                weights.append(weight)
            assert _same_planes(G, H) and _rows(G) == _rows(H)
    assert weights == [2, 1, 2, 1, 1, 2]
    _check_against_reference(G, fields, weights)
    _check_against_reference(two.pathways, [f[[0, 2, 3]] for f in fields], weights, check_maps=False)   # two models
    GS = res.sites.pathways
    assert GS.days == out and GS.members == 6 and GS.total_weight == 9 and GS.anchors == [(64, 64), (58, 77)]
    _check_against_reference(GS, plan_f, weights)
    npz, js = res.save(str(tmp_path / 'a' / 'pp'))
    npz_p, js_p = plain.save(str(tmp_path / 'p' / 'pp'))
    assert not (tmp_path / 'p' / 'pp_pathway.npz').exists()
    with np.load(npz) as fa, np.load(npz_p) as fp:          # the main file does not know about the pathway maps
        assert set(fa.files) == set(fp.files) and all(np.array_equal(fa[key], fp[key]) for key in fp.files)
    for path, H in ((tmp_path / 'a' / 'pp_pathway.npz', G), (tmp_path / 'a' / 'pp_sites_pathway.npz', GS)):
        want = {'days', 'pathway_weights', 'pathway_thresholds', 'pathway_connectivity', 'pathway_days',
                'pathway_anchors'} | {'pathway_' + name for name in W.ROW}
        with np.load(str(path)) as fz:
            for k in range(2):
                for which in W.CLASSES:
                    key = 'window_p%s%d' % (which, k)
                    assert np.array_equal(_csr(fz, key, N), H.prob(k, which)), key
                    want |= {'%s_%s' % (key, t) for t in ('data', 'ind', 'indptr')}
            assert set(fz.files) == want
            assert fz['pathway_days'].tolist() == H.days and fz['pathway_thresholds'].tolist() == [1.0, 10.0]
            assert int(fz['pathway_connectivity']) == 4 and fz['pathway_weights'].tolist() == weights
            assert fz['pathway_anchors'].tolist() == [list(a) for a in H.anchors]
            assert fz['pathway_foci'].shape == (2, len(H.days), 6)
            assert np.array_equal(fz['pathway_foci'][1, 2], H.foci(1, H.days[2]))
            assert np.array_equal(fz['pathway_front'][0, -1], H.new_cells(0, H.days[-1], 'front'))
    meta = json.load(open(js))['predictive']
    blk = meta['pathways']
    assert blk['thresholds'] == [1.0, 10.0] and blk['days'] == list(range(6)) and blk['connectivity'] == 4
    assert blk['members'] == 6 and blk['total_weight'] == 9 and blk['cell_area'] == G.cell_area
    assert blk['anchors'] == [[64, 64]]
    for k in range(2):
        assert blk['pathways'][k]['founded'] == G.founded(k)
        for which in W.CLASSES:
            assert blk['pathways'][k]['area_' + which] == G.area(k, which)
    assert meta['sites']['pathways']['days'] == out and meta['sites']['pathways']['anchors'] == [[64, 64], [58, 77]]
    assert 'pathways' not in json.load(open(js_p))['predictive']
    for r in (res, two, plain):
        for m in (r.summary, r.pathways, r.sites):
            if m is not None:
                m.close()
    for p in (one, pa, pb):
        p.close()

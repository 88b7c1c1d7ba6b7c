"""GPU tests of the trap information fields (ps_gain_*, predictive.InformationFields) and of the maps finished from
the accumulators fed from them: the device planes against mpmath and the numpy restatement (gain_ref), zeros and
ranges, gather, determinism, the projection and release-plan sources, SpreadSummary / ReweightedSummary
.for_projection against the numpy loops fed the fetched bits, the finished gain / entropy / conditional maps and
their properties, the refusals, and posterior_predictive(information=) against a hand loop with its files.  Kalbar
wind, 6 days, the members and weights of test_arrival_gpu.py; R = 64 and 128, whose N * N is odd."""
import ctypes as C
import json
import os
import types
import warnings

import numpy as np
import pytest

import gain_ref
import reweight_ref as RR
from test_arrival_gpu import MEMBERS, WEIGHTS, THR, _pop_model, _evaluate, _fields

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -52


# Device against restatement.  The two differ in exp, expm1 and log alone, each library within 1 ulp of the exact
# function, so the two values of a call differ by at most 2 ulp.  Two evaluations of one rounded operation on
# inputs that differ by a relative delta give results that differ by at most delta + 1 ulp (half an ulp of
# rounding on either side).
#   d0 = -expm1(-mu):                 2 ulp
#   p_y, the running product from e:  2 ulp of e and 2 y rounded operations: (2 + 2 y) ulp
#   tail = catch_value:               e enters once at the end; the upper branch and n = 1 carry its 2 ulp and one
#                                     rounding, 3 ulp; the lower branch 1 - e q has the factor e q / Y <= 0.55 / 0.45
#                                     on those 3 ulp and one more rounding: 5 ulp
def class_rtol(ymax):
    return max(5, 2 + 2 * ymax) * ULP


# h = e mu - sum_c x_c, x_c = c log c over the classes c = p_1 .. p_ymax, tail.  With delta_c the relative
# difference of c from above, log c differs by delta_c absolutely and by 2 ulp of itself, the product adds a
# rounding: |dx_c| <= |x_c| (delta_c + 3 ulp) + c delta_c.  Summed with sum |x_c| <= h <= log(ymax + 2), sum c <= 1
# and delta_c <= (2 + 2 ymax) ulp (5 ulp for ymax < 2): log(ymax + 2) (delta + 3 ulp) + delta; the ymax + 2
# roundings of h itself add log(ymax + 2) ulp each.
def h_atol(ymax):
    delta = max(5, 2 + 2 * ymax)
    return (np.log(ymax + 2) * (delta + 3 + ymax + 2) + delta) * ULP


# The finish, device against gain_ref.finish fed the same mean planes: log alone differs, by 2 ulp of itself, and
# the product P l adds a rounding, 3 ulp of each |x|; sum |x| = HY <= log(ymax + 2); the ymax + 2 roundings of HY
# add HY ulp each, the subtraction G = HY - HYM one more.
def finish_atol(ymax):
    return np.log(ymax + 2) * (3 + ymax + 2 + 1) * ULP


def _mid(fields, day, ymax):
    """the rate at which the day's median density gives mu = ymax + 1, so that both branches of the tail run"""
    v = fields[day]
    return float(np.clip((ymax + 1) / np.median(v[v > 0]), 1e-6, 50.0))


def _traps(fields, which):
    """two sets of traps, 29 and 30 of a handle's 32 planes, ymax in {0, 1, 7, 15} between them: rates from 1e-6
    to 50, the middle ones put where the day's median density gives mu = ymax + 1; the inputs out of order and
    shared"""
    if which == 'a':
        return [(3, 50.0, 1), (1, _mid(fields, 1, 15), 15), (3, 1e-6, 0), (0, _mid(fields, 0, 1), 1)]
    return [(5, _mid(fields, 5, 7), 7), (2, 50.0, 7), (5, 1e-6, 1), (2, _mid(fields, 2, 0), 0), (1, 1.0, 0)]


def _rel(got, ref):
    """|got - ref| / ref where ref >= 1e-290, else the absolute difference"""
    d = np.abs(got - ref)
    big = ref >= 1e-290
    out = d.copy()
    out[big] = d[big] / ref[big]
    return out


def _pick(mu, n, k=160):
    """indices of up to k + 44 non-zero entries of mu for mpmath: evenly through the sorted values, the ends, and
    the 20 on either side of mu = n"""
    nz = np.flatnonzero(mu > 0)
    order = nz[np.argsort(mu[nz])]
    at = int(np.searchsorted(mu[order], float(n)))
    take = set(order[np.linspace(0, order.size - 1, min(k, order.size)).astype(int)])
    take |= set(order[max(at - 20, 0):at + 20]) | {order[0], order[-1]}
    return np.array(sorted(take))


def _planes(IF, e):
    return np.array([IF.plane(e, name) for name in IF.plane_names(e)])


def _check_planes(IF, v_of_trap, seen, sample=True):
    """every plane of IF against v (its input's value field): zeros, ranges, the restatement everywhere and mpmath
    on a sample; seen: counters of the cases the data hit -> the worst errors"""
    worst = dict(dev_class=0.0, ref_class=0.0, dev_h=0.0, ref_h=0.0, full_class=0.0, full_h=0.0)
    for e, (key, rate, ymax) in enumerate(IF.traps):
        v = v_of_trap[e]
        Y = _planes(IF, e)
        assert Y.dtype == np.float64 and Y.shape == (ymax + 3,) + v.shape
        assert not Y[:, v == 0.0].any() and not np.signbit(Y).any(), e           # exactly +0.0 where v == 0
        assert (Y[0][v != 0.0] > 0.0).all(), e
        assert ((Y[:-1] >= 0.0) & (Y[:-1] <= 1.0)).all(), e
        assert ((Y[-1] >= 0.0) & (Y[-1] <= np.log(ymax + 2))).all(), e
        mu = (np.float64(rate) * v).ravel()
        ref = gain_ref.apply(mu, ymax)
        Yf = Y.reshape(ymax + 3, -1)
        full_class = max(_rel(Yf[p], ref[p]).max() for p in range(ymax + 2))
        full_h = np.abs(Yf[-1] - ref[-1]).max()
        assert full_class <= class_rtol(ymax), (e, full_class)
        assert full_h <= h_atol(ymax), (e, full_h)
        worst['full_class'] = max(worst['full_class'], full_class)
        worst['full_h'] = max(worst['full_h'], full_h)
        if sample:
            idx = _pick(mu, ymax + 1)
            ex = gain_ref.exact(mu[idx], ymax)
            rel_r, h_r = gain_ref.errors(ref[:, idx], mu[idx], ymax, ex=ex)
            rel_d, h_d = gain_ref.errors(Yf[:, idx], mu[idx], ymax, ex=ex)
            for key_, val in (('ref_class', rel_r.max()), ('dev_class', rel_d.max()), ('ref_h', h_r.max()),
                              ('dev_h', h_d.max())):
                worst[key_] = max(worst[key_], float(val))
        seen['empty'] += int((mu == 0).sum())
        seen['below'] += int(((mu > 0) & (mu < ymax + 1)).sum())
        seen['above'] += int((mu >= ymax + 1).sum())
        seen['sure'] += int((Yf[ymax + 1] == 1.0).sum())
    print('largest error against mpmath: class planes device %.3g, restatement %.3g; h device %.3g, restatement '
          '%.3g; device against restatement: class planes %.3g, h %.3g'
          % (worst['dev_class'], worst['ref_class'], worst['dev_h'], worst['ref_h'], worst['full_class'],
             worst['full_h']))
    return worst


@pytest.mark.parametrize('which', ['a', 'b'])
@pytest.mark.parametrize('R', [64, 128])
def test_planes_against_mpmath_and_the_restatement(R, which):
    from parasitoids_amd.predictive import InformationFields
    pm = _pop_model(R)
    N = 2 * R + 1
    _evaluate(pm, MEMBERS[0])
    fields = _fields(pm, range(6))
    traps = _traps(fields, which)
    assert min(t[1] for t in traps) == 1e-6 and max(t[1] for t in traps) == 50.0
    nplane = sum(t[2] + 3 for t in traps)
    with InformationFields(pm, traps) as IF:
        assert IF.in_days == ([0, 1, 3] if which == 'a' else [1, 2, 5]) and IF.fields_kind == 'gain'
        assert IF.nout == nplane and IF.ntrap == len(traps)
        assert IF.nbytes == (nplane + 3 * len(traps)) * ((N * N + 63) // 64 * 64) * 8
        IF.apply()
        assert IF.applies == 1
        seen = dict(empty=0, below=0, above=0, sure=0)
        worst = _check_planes(IF, [fields[t[0]] for t in traps], seen)
        print('cells: %r' % (seen,))
        assert all(c > 0 for c in seen.values()), seen
        assert worst['dev_class'] <= 4 * worst['ref_class']
        assert worst['dev_h'] <= 4 * worst['ref_h']
        # gather: the tail cell of the odd N * N, its neighbour, the release cell and a corner
        rows, cols = [N - 1, N - 1, R, 0, R + 1], [N - 1, N - 2, R, 0, R - 2]
        got = IF.gather(rows, cols)
        assert got.shape == (nplane, 5)
        k = 0
        for e in range(len(traps)):
            for name in IF.plane_names(e):
                assert IF.plane_index(e, name) == k
                assert np.array_equal(got[k], IF.plane(e, name)[rows, cols]), (e, name)
                k += 1
        assert got[[IF.plane_index(e, 'd0') for e in range(len(traps))], 2].min() > 0   # the release cell holds wasps
    pm.close()


def test_determinism_overwrite_and_the_other_sources():
    from parasitoids_amd.predictive import InformationFields, Projection, ReleaseSites
    pm = _pop_model(64, mode='exact')
    res_m = 10000.0 / 64
    _evaluate(pm, MEMBERS[0])
    fields = _fields(pm, range(6))
    traps = _traps(fields, 'a')
    days = [0, 1, 3]
    by_index = [(days.index(d), r, y) for d, r, y in traps]
    plan_days = [0, 1, 3, 5]
    with InformationFields(pm, traps) as IF, Projection(pm, np.eye(3), days) as P, \
            InformationFields.for_projection(P, by_index) as IP, \
            ReleaseSites(pm, [(0.0, 0.0, 0.6), (7 * res_m, -3 * res_m, 0.5)], plan_days) as RS, \
            InformationFields.for_projection(RS, traps) as IS:
        n = len(traps)
        IF.apply()
        first = [_planes(IF, e) for e in range(n)]
        IF.apply()
        assert all(np.array_equal(_planes(IF, e), first[e]) for e in range(n))
        # identity weights: the projection's outputs are the day fields, and so are the planes, bit for bit
        P.apply()
        IP.apply()
        assert all(np.array_equal(_planes(IP, e), first[e]) for e in range(n))
        # a release plan: the restatement applied to the plan's fetched fields
        RS.apply()
        IS.apply()
        plan = {d: RS.field(e) for e, d in enumerate(plan_days)}
        seen = dict(empty=0, below=0, above=0, sure=0)
        _check_planes(IS, [plan[t[0]] for t in traps], seen, sample=False)
        assert seen['below'] > 0 and seen['empty'] > 0
        # a second member overwrites the first, zeros included
        _evaluate(pm, MEMBERS[2])
        IF.apply()
        other = _fields(pm, range(6))
        second = [_planes(IF, e) for e in range(n)]
        assert any(not np.array_equal(a, b) for a, b in zip(first, second))
        assert any(((a == 0) != (b == 0)).any() for a, b in zip(first, second))   # another zero pattern, checked below
        _check_planes(IF, [other[t[0]] for t in traps], dict(empty=0, below=0, above=0, sure=0), sample=False)
        assert IF.applies == 3 and IP.applies == 1
        with pytest.raises(ValueError, match='output'):
            InformationFields.for_projection(RS, [(2, 1.0)])
        with pytest.raises(ValueError, match='output'):
            InformationFields.for_projection(P, [(3, 1.0)])
    pm.close()


LAMS = [0.0, -1.5, 0.7, -0.2, 2.0]            # the log-weights of the scenario 'tilt'


@pytest.fixture(scope='module')
def fed():
    """the five members in two passes on one exact-mode model (the same member gives the same bits each time):
    first every accumulator fed without a host synchronisation in between, then the members once more with their
    planes fetched"""
    from parasitoids_amd.predictive import InformationFields, ReweightedSummary, SpreadSummary
    f = types.SimpleNamespace()
    pm = f.pm = _pop_model(64, mode='exact')
    _evaluate(pm, MEMBERS[0])
    f.traps = _traps(_fields(pm, range(6)), 'b')
    f.IF = InformationFields(pm, f.traps)
    f.S = SpreadSummary.for_projection(f.IF)
    f.Sa, f.Sb = SpreadSummary.for_projection(f.IF), SpreadSummary.for_projection(f.IF)
    f.S1 = SpreadSummary.for_projection(f.IF)
    f.RW = ReweightedSummary.for_projection(f.IF, ['flat', 'tilt'])
    for i, (m, w) in enumerate(zip(MEMBERS, WEIGHTS)):     # nothing here waits for the device
        _evaluate(pm, m)
        f.IF.apply()
        f.S.add(w)
        f.RW.add([0.0, LAMS[i]], w)
        (f.Sa if i < 2 else f.Sb).add(w)
        if i == 3:
            f.S1.add(w)
    f.Y = [None] * 5
    for i in (3, 0, 4, 1, 2):
        _evaluate(pm, MEMBERS[i])
        f.IF.apply()
        f.Y[i] = np.array([f.IF.plane(e, name) for e in range(len(f.traps)) for name in f.IF.plane_names(e)])
    f.state = RR.new_state(f.Y[0].shape, [], 2)
    for i in range(5):
        RR.add(f.state, f.Y[i], [0.0, LAMS[i]], WEIGHTS[i])
    yield f
    for h in (f.S, f.Sa, f.Sb, f.S1, f.RW, f.IF):
        h.close()
    pm.close()


def test_summary_of_the_planes_against_the_numpy_loop(fed):
    S, n = fed.S, fed.IF.nout
    assert (S.total_weight, S.members, S.thresholds) == (8.0, 5, [])
    sc = fed.state[0]
    for k in range(n):
        assert np.array_equal(S.mean(k), sc['mean'][k]), k                      # bit for bit
        scale = np.abs(sc['mean'][k]).max()
        np.testing.assert_allclose(S.variance(k), RR.variance(sc)[k], rtol=1e-12, atol=1e-15 * scale ** 2)
    assert any(S.variance(k).max() > 0 for k in range(n))


def test_two_way_merge_against_the_hand_merge(fed):
    n = fed.IF.nout
    a, b = RR.new_state(fed.Y[0].shape, [], 1), RR.new_state(fed.Y[0].shape, [], 1)
    for i in range(5):
        RR.add(a if i < 2 else b, fed.Y[i], [0.0], WEIGHTS[i])
    before = [(fed.Sa.mean(k), fed.Sb.mean(k)) for k in range(n)]
    for k in range(n):                                   # the halves hold the hand loops' bits
        assert np.array_equal(before[k][0], a[0]['mean'][k]) and np.array_equal(before[k][1], b[0]['mean'][k])
    RR.merge(a, b)
    fed.Sa.merge(fed.Sb)
    assert (fed.Sa.total_weight, fed.Sa.members) == (8.0, 5)
    for k in range(n):
        # the device forms ma + d * (Wb / W) as one fused multiply-add, numpy rounds the product first: the two
        # differ by half an ulp of the product, |d| <= max(ma, mb), and one ulp of the final rounding; where the
        # product is subnormal (class probabilities next to exp(-mu) = 0) its rounding is one subnormal spacing
        bound = 2 * ULP * np.maximum(before[k][0], before[k][1]) + 5e-324
        assert (np.abs(fed.Sa.mean(k) - a[0]['mean'][k]) <= bound).all(), k
        m = fed.S.mean(k)
        np.testing.assert_allclose(fed.Sa.mean(k), m, rtol=1e-12, atol=1e-15 * np.abs(m).max())


def test_reweighted_summary_of_the_planes_against_the_numpy_loop(fed):
    S, RW = fed.S, fed.RW
    assert RW.members('flat') == 5 and RW.members('tilt') == 5 and RW.skipped('tilt') == 0
    for k in range(fed.IF.nout):
        assert np.array_equal(RW.mean('flat', k), S.mean(k))                     # log-weights 0: the summary's bits
        assert np.array_equal(RW.mean('tilt', k), fed.state[1]['mean'][k]), k    # bit for bit
    assert any(not np.array_equal(RW.mean('tilt', k), S.mean(k)) for k in range(fed.IF.nout))


def _empty_everywhere(fed, e):
    d0 = fed.IF.plane_index(e, 'd0')
    return np.all([fed.Y[i][d0] == 0.0 for i in range(5)], axis=0)


def test_finished_maps_against_the_restatement(fed):
    IF, S = fed.IF, fed.S
    cap = gain_ref.cap(WEIGHTS)
    IF.finish(S)
    worst, tops = 0.0, []
    for e, (day, rate, ymax) in enumerate(fed.traps):
        base = IF.plane_index(e, 'd0')
        means = np.array([S.mean(base + k) for k in range(ymax + 3)])
        G, HY, HYM = gain_ref.finish(means)
        g, hy, hym = IF.result(e, 'gain'), IF.result(e, 'entropy'), IF.result(e, 'conditional')
        assert np.array_equal(hym, HYM) and np.array_equal(hym, S.mean(IF.plane_index(e, 'h')))
        err = max(np.abs(g - G).max(), np.abs(hy - HY).max())
        worst = max(worst, err)
        assert err <= finish_atol(ymax), (e, err)
        out = _empty_everywhere(fed, e)
        assert out.any() and not g[out].any() and not np.signbit(g).any()          # exactly +0.0 outside every plume
        assert not hy[out].any() and not hym[out].any()
        assert (g >= 0.0).all() and (g <= cap).all(), (e, g.max(), cap)
        assert (hy <= np.log(ymax + 2) + finish_atol(ymax)).all()
        assert g.max() > 0, e                                                      # the members do disagree
        tops.append(float(g.max()))
    assert max(tops) > 0.01, tops                  # and a trap of sensible effort sees it (one has rate 1e-6)
    print('finish: device against restatement %.3g; cap %.4g; largest gains %r' % (worst, cap, tops))


def test_a_single_member_carries_no_information(fed):
    IF = fed.IF
    IF.finish(fed.S1)
    for e in range(len(fed.traps)):
        g = IF.result(e, 'gain')
        print('trap %d: single-member gain at most %.3g' % (e, g.max()))
        assert g.max() <= 1e-12
        assert np.abs(IF.result(e, 'entropy') - IF.result(e, 'conditional')).max() <= 1e-12


def test_reweighted_finish_with_zero_log_weights_holds_the_plain_bits(fed):
    IF = fed.IF
    IF.finish(fed.S)
    plain = [[IF.result(e, what) for what in ('gain', 'entropy', 'conditional')] for e in range(len(fed.traps))]
    IF.finish(fed.RW, 'flat')
    for e in range(len(fed.traps)):
        for k, what in enumerate(('gain', 'entropy', 'conditional')):
            assert np.array_equal(IF.result(e, what), plain[e][k]), (e, what)
    IF.finish(fed.RW, 'tilt')
    tilt = IF.result(0, 'gain')
    assert not np.array_equal(tilt, plain[0][0]) and (tilt >= 0).all()
    means = np.array([fed.RW.mean('tilt', k) for k in range(fed.traps[0][2] + 3)])
    assert np.abs(tilt - gain_ref.finish(means)[0]).max() <= finish_atol(fed.traps[0][2])


def test_two_members_against_the_closed_form_from_catch_fields():
    from parasitoids_amd.predictive import CatchFields, InformationFields, SpreadSummary
    pm = _pop_model(64, mode='exact')
    day, rate = 3, 0.02
    with InformationFields(pm, [(day, rate, 0)]) as IF, SpreadSummary.for_projection(IF) as S, \
            CatchFields(pm, [(day, rate, 1)]) as CF:
        p = []
        for m in (MEMBERS[1], MEMBERS[2]):
            _evaluate(pm, m)
            IF.apply()
            S.add(2)
            CF.apply()
            p.append(CF.field(0))
            assert np.array_equal(IF.plane(0, 'd0'), p[-1]) and np.array_equal(IF.plane(0, 'tail'), p[-1])
        IF.finish(S)
        g = IF.result(0, 'gain')

    def Hb(q):
        with np.errstate(divide='ignore', invalid='ignore'):
            return -(np.where(q > 0, q * np.log(q), 0.0) + np.where(q < 1, (1 - q) * np.log1p(-q), 0.0))
    a, b = p
    want = Hb((a + b) / 2) - (Hb(a) + Hb(b)) / 2
    print('two members: largest gain %.3g, against the closed form %.3g' % (g.max(), np.abs(g - want).max()))
    assert np.abs(g - want).max() <= 1e-12
    assert 0.01 < g.max() <= np.log(2)
    pm.close()


def test_refusals():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import (InformationFields, Projection, SpreadSummary, check_information)
    lib = L.load()
    N = 129

    def create(nin, ntrap, inputs, rates, ymax, n=N):
        h = L._VP()
        rc = lib.ps_gain_create(0, n, nin, ntrap, L.p_i32(L.i32(inputs)), L.p_f64(L.f64(rates)),
                                L.p_i32(L.i32(ymax)), C.byref(h))
        if rc == L.PS_OK:
            lib.ps_gain_destroy(h)
        return rc
    assert create(2, 2, [0, 1], [1.0, 2.0], [0, 15]) == L.PS_OK
    assert create(1, 2, [0, 0], [1.0, 2.0], [15, 11]) == L.PS_OK                   # 18 + 14 = 32 planes
    for args in [(1, 2, [0, 0], [1.0, 2.0], [15, 12]),                            # 33 planes
                 (1, 11, [0] * 11, [1.0] * 11, [0] * 11),                          # 33 planes
                 (0, 1, [0], [1.0], [0]), (33, 1, [0], [1.0], [0]), (1, 0, [0], [1.0], [0]),
                 (2, 1, [2], [1.0], [0]), (2, 1, [-1], [1.0], [0]),
                 (1, 1, [0], [0.0], [0]), (1, 1, [0], [-1.0], [0]), (1, 1, [0], [float('inf')], [0]),
                 (1, 1, [0], [float('nan')], [0]), (1, 1, [0], [1.0], [-1]), (1, 1, [0], [1.0], [16])]:
        assert create(*args) == L.PS_ERR_BAD_ARG, args
    assert create(1, 1, [0], [1.0], [0], n=0) == L.PS_ERR_BAD_ARG
    for bad in ([(1, 1.0, 16)], [(1, 0.0)], [(1, float('inf'))], [(1, 1.0, 15), (1, 1.0, 12)]):
        with pytest.raises(ValueError):
            InformationFields(types.SimpleNamespace(), bad)              # refused before the model is looked at
    with pytest.raises(ValueError, match='6 days'):
        check_information(dict(traps=[(6, 1.0)]), 6)
    pm = _pop_model(64)
    with InformationFields(pm, [(1, 1.0), (2, 0.5, 3)]) as IF, SpreadSummary.for_projection(IF) as S, \
            Projection(pm, np.eye(3), [0, 1, 2]) as P3, SpreadSummary.for_projection(P3) as S3, \
            InformationFields(pm, [(7, 1.0)]) as late:
        assert IF.nout == 9
        with pytest.raises(ValueError, match='evaluation'):
            IF.apply()
        _evaluate(pm, MEMBERS[0])
        with pytest.raises(ValueError, match='day 7'):                  # a day the evaluation does not have
            late.apply()
        # before the first apply
        for call in (lambda: IF.plane(0, 'd0'), lambda: IF.gather([0], [0]), lambda: S.add(1)):
            with pytest.raises(L.HipError) as ei:
                call()
            assert ei.value.code == L.PS_ERR_STATE
        IF.apply()
        # before the first finish, and a finish from an empty accumulator
        for call in (lambda: IF.result(0, 'gain'), lambda: IF.finish(S)):
            with pytest.raises(L.HipError) as ei:
                call()
            assert ei.value.code == L.PS_ERR_STATE
        # slot counts that do not fit: nothing is enqueued, the accumulator stays empty
        assert lib.ps_summary_add_gain(S3._h, IF._h, 1) == L.PS_ERR_BAD_ARG
        assert S3.members == 0
        assert lib.ps_summary_add_gain(S._h, IF._h, 0) == L.PS_ERR_BAD_ARG       # weight >= 1
        assert lib.ps_summary_add_gain(S._h, None, 1) == L.PS_ERR_BAD_ARG
        P3.apply()
        S3.add(1)
        assert lib.ps_gain_finish_summary(IF._h, S3._h) == L.PS_ERR_BAD_ARG       # 3 slots, 9 planes
        assert lib.ps_gain_apply_project(IF._h, P3._h) == L.PS_ERR_BAD_ARG        # 3 outputs, 2 inputs
        assert IF.applies == 1
        with pytest.raises(ValueError):
            IF.plane(0, 'p1')                                           # trap 0 has ymax 0
        with pytest.raises(ValueError):
            IF.plane(2, 'd0')
        with pytest.raises(L.HipError):
            IF.gather([129], [0])
        S.add(2)
        IF.finish(S)
        assert S.members == 1 and IF.result(1, 'gain').max() <= 1e-12
    pm.close()


def _csr(f, key, N):
    from scipy import sparse
    return sparse.csr_matrix((f[key + '_data'], f[key + '_ind'], f[key + '_indptr']), shape=(N, N)).toarray()


def _chain(run_lengths):
    """a short synthetic chain: runs of identical model parameters whose plumes drift apart, so that there are cells
    which one member reaches and another does not"""
    from parasitoids_amd import mcmc
    names = [m[0] for m in mcmc.MODEL_BLOCK]
    base = np.array([m[2] for m in mcmc.MODEL_BLOCK], dtype=np.float64)
    rows = []
    for n, length in enumerate(run_lengths):
        t = base.copy()
        t[names.index('sig_x')] -= 30.0 * n
        t[names.index('mu_r')] += 0.5 * n
        rows += [t] * length
    return np.array(rows), names


def test_posterior_predictive_with_information_against_a_hand_loop(tmp_path):
    from parasitoids_amd import mcmc
    from parasitoids_amd import predictive as PR
    R, N = 64, 129
    res_m = 10000.0 / R
    # run weights 6, 1 and 1, 1: cap = 1.00 nats, and a cell that the first member alone leaves empty shows
    # H_b(1/3) = 0.64 > cap / 2 with a trap that is sure to find what is there
    ta, names = _chain([6, 1])
    tb, _ = _chain([1, 1, 1])
    traces = [ta, tb[1:]]                                    # the second chain: two runs of other members
    chains = [(t, names) for t in traces]
    traps = [(1, 0.01), (3, 1.0, 3), (5, 5.0, 7)]
    plan = dict(sites=[(0.0, 0.0, 0.6), (7 * res_m, -3 * res_m, 0.5)], days=[0, 1, 3, 5])
    arg = dict(traps=traps)
    rw = {'flat': dict(log_weights=[np.zeros(len(t)) for t in traces]), 'options': dict(min_ess=1)}
    pm = _pop_model(R, mode='exact')
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        res = PR.posterior_predictive(pm, chains, thresholds=THR, information=arg, sites=plan, reweight=rw,
                                      cell_area=res_m ** 2)
    ip = res.information
    assert res.failed == 0 and res.evaluations == 4
    assert ip.traps == [(1, 0.01, 0), (3, 1.0, 3), (5, 5.0, 7)] and ip.given == {'traps': [list(t) for t in traps]}
    assert (ip.summary.total_weight, ip.summary.members, ip.summary.thresholds) == (9.0, 4, [])
    weights = [w for _c, _first, w in res.runs]
    assert ip.weights == weights and ip.cap == gain_ref.cap(weights)
    # the warning names exactly the traps whose largest gain exceeds cap / 2
    over = [e for e in range(3) if ip.gain(e).max() > 0.5 * ip.cap]
    print('cap %.4g, largest gains %r' % (ip.cap, [float(ip.gain(e).max()) for e in range(3)]))
    told = [w for w in rec if issubclass(w.category, UserWarning) and str(w.message).startswith('information:')]
    assert over and len(told) == len(over) and all('bounded by the ensemble' in str(w.message) for w in told)
    # the hand loop: every run once more, per chain a summary of its own, merged in chain order
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    hand, hand_pl = [], []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        with PR.InformationFields(pm, traps) as IF, PR.ReleaseSites(pm, plan['sites'], plan['days']) as RS, \
                PR.InformationFields.for_projection(RS, traps) as IS:
            for ci in range(2):
                hand.append(PR.SpreadSummary.for_projection(IF))
                hand_pl.append(PR.SpreadSummary.for_projection(IS))
                for c, first, weight in res.runs:
                    if c != ci:
                        continue
                    pm.evaluate(*mcmc.model_args(traces[ci][first, cols]), want_stats=False)
                    IF.apply()
                    hand[ci].add(weight)
                    RS.apply()
                    IS.apply()
                    hand_pl[ci].add(weight)
            for hs in (hand, hand_pl):
                hs[0].merge(hs[1])
                hs[1].close()
            for got, want, F in ((ip, hand[0], IF), (res.sites.information, hand_pl[0], IS)):
                assert got.summary.total_weight == want.total_weight == 9.0
                for k in range(F.nout):
                    assert np.array_equal(got.summary.mean(k), want.mean(k)), k
                F.finish(want)
                for e, t in enumerate(got.traps):
                    assert np.array_equal(got.gain(e), F.result(e, 'gain')), e
                    assert np.array_equal(got.entropy(e), F.result(e, 'entropy')), e
                    assert np.array_equal(got.conditional(e), F.result(e, 'conditional')), e
                    assert np.array_equal(got.gain(e, scenario='flat'), got.gain(e)), e    # log-weights 0
                    base = F.plane_index(e, 'd0')
                    assert np.array_equal(got.pmf(e, 0), 1.0 - want.mean(base))
                    assert np.array_equal(got.pmf(e, t[2] + 1), want.mean(F.plane_index(e, 'tail')))
                    total = sum(got.pmf(e, y) for y in range(t[2] + 2))
                    assert np.abs(total - 1.0).max() <= 1e-13                             # a distribution
                    assert (got.gain(e) <= got.cap).all() and got.gain(e).max() > 0
                with pytest.raises(ValueError):
                    got.pmf(0, 2)
    # the files
    npz, js = res.save(str(tmp_path / 'a' / 'pp'))
    names_out = sorted(os.listdir(str(tmp_path / 'a')))
    assert 'pp_information.npz' in names_out and 'pp_sites_information.npz' in names_out
    f = np.load(str(tmp_path / 'a' / 'pp_information.npz'))
    assert list(f['days']) == [1, 3, 5] and list(f['rates']) == [0.01, 1.0, 5.0] and list(f['ymax']) == [0, 3, 7]
    want_keys = {'days', 'rates', 'ymax'}
    for e, t in enumerate(ip.traps):
        for name in ['gain', 'entropy', 'd0'] + ['p%d' % y for y in range(1, t[2] + 2)]:
            want_keys |= {'i%d_%s_%s' % (e, name, part) for part in ('data', 'ind', 'indptr')}
        for key, m in (('i%d_gain' % e, ip.gain(e)), ('i%d_entropy' % e, ip.entropy(e)),
                       ('i%d_d0' % e, 1.0 - ip.pmf(e, 0)), ('i%d_p1' % e, ip.pmf(e, 1))):
            assert np.array_equal(_csr(f, key, N), np.where(m >= 1e-8, m, 0.0)), key
    assert set(f.files) == want_keys
    meta = json.load(open(js))['predictive']
    block = meta['information']
    assert block['given'] == {'traps': [list(t) for t in traps]} and block['units'] == 'nats'
    assert block['members'] == 4 and block['total_weight'] == 9.0 and block['cap'] == ip.cap
    for e, out in enumerate(block['outputs']):
        g = ip.gain(e)
        assert out['trap'] == list(ip.traps[e]) and out['max_gain'] == float(g.max())
        assert out['half_area'] == float((g >= 0.5 * g.max()).sum() * res_m ** 2)
    assert len(meta['sites']['information']['outputs']) == 3
    for h in (hand[0], hand_pl[0], res.summary, res.reweight, res.sites, ip):
        h.close()
    # a trap day the plan does not output is refused before any evaluation
    with pytest.raises(ValueError, match='output day'):
        PR.posterior_predictive(pm, chains, information=dict(traps=[(2, 1.0)]), sites=plan)
    pm.close()


def test_without_information_nothing_changes(tmp_path):
    from parasitoids_amd import predictive as PR
    pm = _pop_model(64)
    trace, names = _chain([2, 1])
    plan = dict(sites=[(0.0, 0.0, 1.0)], days=[1, 3])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        warnings.filterwarnings('error', message='.*bounded by the ensemble.*')    # and no warning of the new kind
        res = PR.posterior_predictive(pm, (trace, names), thresholds=THR, sites=plan)
    assert res.information is None and res.sites.information is None
    res.save(str(tmp_path / 'p' / 'pp'))
    assert sorted(os.listdir(str(tmp_path / 'p'))) == ['pp.json', 'pp.npz', 'pp_sites.npz']
    meta = json.load(open(str(tmp_path / 'p' / 'pp.json')))['predictive']
    assert 'information' not in meta and 'information' not in meta['sites']
    res.summary.close()
    res.sites.close()
    pm.close()

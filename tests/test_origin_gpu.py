"""GPU tests of the origin maps (ps_origin_*, predictive.OriginMaps): the raw C ABI over crafted state records at
N = 65 and 129 -- the set {l = -inf} exactly and every finite value within the bounds of DESIGN 7y against the
restatement (origin_ref) and its 40-digit version, no cell left out -- the streaming pair, the member rows, merge,
reset, determinism, the amounts ladder bit for bit, the prior, the lagged models of the Kalbar wind, and the refusals.
A raw handle reads every day from one state record through the slot's stat_scale: day d of lag g holds
fl(state * scale(g, d)), which is what ps_record_value returns with post_scale 1, no delta and negval 0."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest

import origin_ref as OR
from test_arrival_gpu import MEMBERS, HP, DLP, NPER, _pop_model, _evaluate, _fields

pytestmark = pytest.mark.gpu

KIND = {'count': 0, 'none': 1, 'found': 2}


def _scale(lag, d):
    return 1.0 / (1.0 + 0.25 * d + 0.5 * lag)


def _ref_fields(v, lags, days):
    """{lag: {model day: field}} as the raw handle's slots present the state v"""
    return {lag: {d - lag: v * _scale(lag, d - lag) for d in days if d >= lag} for lag in lags}


class _Raw():
    """one ps_origin handle over the state record of a solver, through the C ABI.  findings: origin_ref.probe
    dicts; hypotheses: [(amount, lag)]"""

    def __init__(self, n, findings, hypotheses, prior=None, solver=None):
        from scipy import sparse
        from parasitoids_amd import _lib as L
        from parasitoids_amd.hip_lib import HipSolve
        self.L, self.lib, self.n = L, L.load(), n
        self.own = solver is None
        self.solver = HipSolve(sparse.coo_matrix(np.ones((n, n))), [33, 33], mode='exact') if solver is None else solver
        self.findings, self.hyp = findings, hypotheses
        self.days = sorted({f['day'] for f in findings})
        self.lags = sorted({g for _a, g in hypotheses})
        self.prior = None if prior is None else np.ascontiguousarray(prior, dtype=np.float64)
        self.h = L._VP()
        f = findings
        L.check(self.lib.ps_origin_create(
            0, n, len(f), L.p_i32(L.i32([p['row'] for p in f])), L.p_i32(L.i32([p['col'] for p in f])),
            L.p_i32(L.i32([self.days.index(p['day']) for p in f])), L.p_i32(L.i32([KIND[p['kind']] for p in f])),
            L.p_f64(L.f64([p['rate'] for p in f])), L.p_f64(L.f64([p['n'] or 0 for p in f])), len(self.days),
            len(hypotheses), L.p_f64(L.f64([a for a, _g in hypotheses])),
            L.p_i32(L.i32([self.lags.index(g) for _a, g in hypotheses])), len(self.lags),
            None if self.prior is None else L.p_f64(self.prior), C.byref(self.h)))

    def group_args(self, g):
        L, lag = self.L, self.lags[g]
        kind = L.i32([L.REC_STATE if d >= lag else L.REC_NONE for d in self.days])
        stat = L.f64([_scale(lag, d - lag) if d >= lag else 0.0 for d in self.days])
        zero, one = L.i32([0] * len(self.days)), L.f64([1.0] * len(self.days))
        return (g, len(self.days), L.p_i32(kind), L.p_i32(zero), L.p_f64(stat), L.p_f64(one), L.p_i32(zero), 0.0), \
            (kind, stat, zero, one)

    def add_group(self, g, weight):
        args, _keep = self.group_args(g)
        return self.lib.ps_origin_add(self.h, self.solver._h, *args, weight)

    def add(self, v, weight=1):
        self.solver.set_state(v)
        for g in range(len(self.lags)):
            self.L.check(self.add_group(g, weight))

    def plane(self, what, h):
        out = np.empty((self.n, self.n))
        self.L.check(self.lib.ps_origin_fetch(self.h, what, h, self.L.p_f64(out)))
        return out

    def planes(self, what):
        return np.stack([self.plane(what, h) for h in range(len(self.hyp))])

    def info(self):
        W, m, cap, nb = C.c_double(), C.c_int64(), C.c_int64(), C.c_int64()
        self.L.check(self.lib.ps_origin_info(self.h, C.byref(W), C.byref(m), C.byref(cap), C.byref(nb)))
        return W.value, m.value, cap.value, nb.value

    def rows(self):
        m = self.info()[1]
        rows, w = np.empty((m, len(self.hyp), 2)), np.empty(m, dtype=np.uint32)
        self.L.check(self.lib.ps_origin_members(self.h, m, self.L.p_f64(rows), w.ctypes.data_as(C.POINTER(C.c_uint32))))
        return rows, w

    def ref_fields(self, v):
        return _ref_fields(v, self.lags, self.days)

    def close(self):
        self.lib.ps_origin_destroy(self.h)
        if self.own:
            self.solver.close()


RATIOS = {'l': 0.0, 'E': 0.0, 'rows': 0.0}


def _same_pattern(got, want, what):
    bad = np.argwhere((got == -np.inf) != (want == -np.inf))
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist())
    assert not np.isnan(got).any() and not (got == np.inf).any(), what


def _against_mp(got, l_mp, parts, nfind, what):
    """device l against the 40-digit l: the pattern exactly, every finite value within the stated bound"""
    fin = OR.finite_mask(l_mp)
    bad = np.argwhere((got != -np.inf) != fin)
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist())
    assert not np.isnan(got).any() and not (got == np.inf).any(), what
    if fin.any():
        bound = OR.loglik_bound(nfind, parts)[fin]
        err = OR.diff(got[fin], l_mp[fin])
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        assert (err <= bound).all(), (what, ratio)
        RATIOS['l'] = max(RATIOS['l'], ratio)


def _check_l(raw, v, what, log_prior=None, exact=True):
    """the last member's l of every hypothesis: the pattern exactly, and every finite value within the bound against
    the 40-digit reference; exact=False, where that reference is too slow for a test (N = 129, O = 64): against the
    float64 restatement within twice the bound, since each side lies within one bound of the exact value"""
    fields = raw.ref_fields(v)
    got = raw.planes(2)
    if exact:
        l_mp, parts = OR.loglik_mp(raw.findings, raw.hyp, fields, log_prior)
        _against_mp(got, l_mp, parts, len(raw.findings), what)
        return got, None
    want = OR.loglik(raw.findings, raw.hyp, fields, log_prior)
    bound = OR.loglik_bound(len(raw.findings), OR.loglik_parts(raw.findings, raw.hyp, fields))
    _same_pattern(got, want, what)
    fin = want != -np.inf
    err = np.abs(got[fin] - want[fin])
    assert (err <= 2.0 * bound[fin]).all(), (what, float((err / np.maximum(bound[fin], 1e-300)).max()))
    return got, want


def _corner_findings(n):
    """7 findings of mixed kinds, the four corners among them: the shifted reads leave the domain on every side"""
    R = n // 2
    return [OR.probe(0, 0, 1, 'none', 0.5), OR.probe(0, n - 1, 2, 'count', 0.25, 0), OR.probe(n - 1, 0, 1, 'none', 1.0),
            OR.probe(n - 1, n - 1, 0, 'found', 0.125), OR.probe(R, R, 2, 'count', 0.5, 3),
            OR.probe(R - 5, R + 7, 1, 'count', 2.0, 1), OR.probe(R + 3, 2, 0, 'none', 0.75)]


def _many_findings(n):
    """64 findings on 32 days: a few counts, the rest 'none'"""
    out = []
    for k in range(64):
        row, col, day = (7 * k + 3) % n, (11 * k + 5) % n, k % 32
        out.append(OR.probe(row, col, day, 'count', 0.5, k % 3) if k % 16 == 5 else OR.probe(row, col, day, 'none', 0.01))
    return out


def _positive(n):
    r, c = np.mgrid[0:n, 0:n].astype(np.float64)
    return 0.5 + 3.0 * np.exp(-((r - n / 2) ** 2 + (c - n / 3) ** 2) / (0.1 * n * n)) + 0.01 * ((3 * r + 5 * c) % 7)


@pytest.mark.parametrize('n', [65, 129])
def test_crafted_fields_against_the_restatement(n):
    R = n // 2
    pos, empty, spike = _positive(n), np.zeros((n, n)), np.zeros((n, n))
    sr, sc = R - 11, R + 6
    spike[sr, sc] = 40.0
    cases = [('one', [OR.probe(R + 4, R - 9, 0, 'count', 0.5, 2)], [(1.0, 0)]),
             ('corners', _corner_findings(n), [(0.5, 0), (2.0, 0)]),
             ('many', _many_findings(n), [(1.0, 0)])]
    for name, findings, hyp in cases:
        exact = n == 65 and name != 'many'              # mpmath where a test can afford it
        raw = _Raw(n, findings, hyp)
        try:
            # everywhere positive: only a read outside the domain gives -inf
            raw.add(pos)
            got, want = _check_l(raw, pos, (name, 'positive'), exact=exact)
            assert (got != -np.inf).any()
            if name == 'corners':
                assert (got == -np.inf).any()           # a 'found' in a corner: three quarters of the shifts leave
            # one spike: each positive finding is possible from exactly one cell
            raw.add(spike)
            got, want = _check_l(raw, spike, (name, 'spike'), exact=exact)
            if name == 'one':
                f = findings[0]
                cell = (f['row'] - sr + R, f['col'] - sc + R)
                assert np.argwhere(got[0] != -np.inf).tolist() == [list(cell)]
            # nothing anywhere: a positive finding excludes every cell
            raw.add(empty)
            got, want = _check_l(raw, empty, (name, 'empty'), exact=exact)
            assert (got == -np.inf).all()
        finally:
            raw.close()
    # only 'none' findings over an empty field: E is exactly 0.0 everywhere
    raw = _Raw(n, [OR.probe(3, 4, 0, 'none', 0.5), OR.probe(n - 1, 0, 1, 'none', 2.0), OR.probe(R, R, 1, 'count', 1.0, 0)],
               [(1.0, 0), (10.0, 0)])
    try:
        raw.add(empty, 2)
        raw.add(empty, 3)
        for h in range(2):
            E = OR.evidence(raw.plane(0, h), raw.plane(1, h), 5)
            assert np.array_equal(E, np.zeros((n, n))) and not np.signbit(E).any()
        rows, w = raw.rows()
        assert np.array_equal(rows[:, :, 0], np.zeros((2, 2))) and np.array_equal(rows[:, :, 1], np.full((2, 2), n * n))
        assert w.tolist() == [2, 3]
    finally:
        raw.close()


def _member_fields(n):
    """six members: the twin experiment's plumes on day 0 widened differently, with exact zeros around them"""
    return [OR.plume(n, n // 2 + 2 - m, n // 2 - 3 + m, 2.0 + 0.3 * m, 2.6 - 0.1 * m, 3000.0) for m in range(6)]


def _twin_like_findings(n):
    R = n // 2
    return [OR.probe(R + 6, R - 4, 0, 'count', 0.5, 4), OR.probe(R + 9, R - 1, 1, 'count', 0.5, 2),
            OR.probe(R + 2, R - 8, 2, 'count', 0.25, 1), OR.probe(R + 7, R - 6, 1, 'found', 0.5),
            OR.probe(0, 0, 1, 'none', 0.5), OR.probe(n - 1, n - 1, 2, 'none', 0.5), OR.probe(R + 12, R + 12, 0, 'none', 1.0)]


WEIGHTS6 = [1, 2, 3, 4, 1, 2]
HYP3 = [(0.1, 0), (1.0, 0), (10.0, 0)]


@pytest.fixture(scope='module')
def six_members():
    """the mpmath reference of the six members at N = 65, computed once: per member (l, parts), E, the rows"""
    n = 65
    findings, vs = _twin_like_findings(n), _member_fields(n)
    days = sorted({f['day'] for f in findings})
    per = [OR.loglik_mp(findings, HYP3, _ref_fields(v, [0], days)) for v in vs]
    return types_ns(n=n, findings=findings, vs=vs, per=per, E=OR.evidence_mp([l for l, _p in per], WEIGHTS6))


def types_ns(**kw):
    import types
    return types.SimpleNamespace(**kw)


def _feed(raw, vs, weights):
    for v, w in zip(vs, weights):
        raw.add(v, w)


def test_six_members_against_mpmath(six_members):
    q = six_members
    n, O = q.n, len(q.findings)
    raw, two, a, b = (_Raw(n, q.findings, HYP3) for _ in range(4))
    try:
        _feed(raw, q.vs, WEIGHTS6)
        assert raw.info()[:2] == (float(sum(WEIGHTS6)), 6)
        # the last member's l: the pattern exactly, the values within the bound
        got = raw.planes(2)
        l_mp, parts = q.per[-1]
        fin = OR.finite_mask(l_mp)
        assert np.array_equal(got != -np.inf, fin) and fin.any() and not fin.all()
        lb = OR.loglik_bound(O, parts)
        err = OR.diff(got[fin], l_mp[fin])
        assert (err <= lb[fin]).all(), float((err / lb[fin]).max())
        RATIOS['l'] = max(RATIOS['l'], float((err / lb[fin]).max()))
        # A, S and E against mpmath
        A, S = raw.planes(0), raw.planes(1)
        E = OR.evidence(A, S, sum(WEIGHTS6))
        some = OR.finite_mask(q.E)
        assert np.array_equal(E != -np.inf, some) and np.array_equal(A != -np.inf, some)
        assert (S[some] > 0).all() and (S[~some] == 0).all() and (S <= sum(WEIGHTS6) * (1 + 1e-12)).all()
        lmax = np.max([OR.loglik_bound(O, p) for _l, p in q.per], axis=0)
        eb = OR.evidence_bound(6, lmax, E)
        err = OR.diff(E[some], q.E[some])
        assert (err <= eb[some]).all(), float((err / eb[some]).max())
        RATIOS['E'] = max(RATIOS['E'], float((err / eb[some]).max()))
        # the rows against mpmath: mx within the l bound, mx + log(sum) within the row bound
        rows, w = raw.rows()
        assert w.tolist() == WEIGHTS6 and rows.shape == (6, 3, 2)
        for m, (l, p) in enumerate(q.per):
            want = OR.rows_mp(l)
            lbm = OR.loglik_bound(O, p)
            for h, (val, cells) in enumerate(want):
                assert val is not None and cells > 0
                got_lm = rows[m, h, 0] + math.log(rows[m, h, 1])
                rb = OR.row_bound(float(lbm[h].max()), cells, float(val))
                e = float(OR.diff([got_lm], [val])[0])
                assert e <= rb, (m, h, e / rb)
                RATIOS['rows'] = max(RATIOS['rows'], e / rb)
                assert 1.0 <= rows[m, h, 1] <= cells
        print('observed error / bound: l %.3f, E %.3f, rows %.3f' % (RATIOS['l'], RATIOS['E'], RATIOS['rows']))
        # the same calls give the same bits: a second handle, and the first one after reset
        _feed(two, q.vs, WEIGHTS6)
        for what in range(3):
            assert np.array_equal(two.planes(what), raw.planes(what)), what
        assert np.array_equal(two.rows()[0], rows)
        raw.L.check(raw.lib.ps_origin_reset(raw.h))
        assert raw.info()[:2] == (0.0, 0)
        assert raw.lib.ps_origin_fetch(raw.h, 0, 0, raw.L.p_f64(np.empty((n, n)))) == raw.L.PS_ERR_STATE
        _feed(raw, q.vs, WEIGHTS6)
        assert np.array_equal(raw.planes(0), A) and np.array_equal(raw.planes(1), S) and np.array_equal(raw.rows()[0], rows)
        # two handles merged: E within the bound of the single pass, the -inf pattern and the rows exactly
        _feed(a, q.vs[:3], WEIGHTS6[:3])
        _feed(b, q.vs[3:], WEIGHTS6[3:])
        a.L.check(a.lib.ps_origin_merge(a.h, b.h))
        assert a.info()[:2] == (float(sum(WEIGHTS6)), 6)
        Em = OR.evidence(a.planes(0), a.planes(1), sum(WEIGHTS6))
        assert np.array_equal(Em != -np.inf, some)
        err = OR.diff(Em[some], q.E[some])
        assert (err <= eb[some]).all(), float((err / eb[some]).max())
        assert np.array_equal(a.planes(0), A)                        # the maximum does not depend on the order
        mr, mw = a.rows()
        assert np.array_equal(mr, rows) and mw.tolist() == WEIGHTS6
        assert np.array_equal(b.rows()[0], rows[3:])                 # the source is unchanged
    finally:
        for r in (raw, two, a, b):
            r.close()


def test_amounts_ladder_equals_premultiplied_rates_bit_for_bit():
    n = 65
    findings, vs = _twin_like_findings(n), _member_fields(n)[:2]
    ladder = _Raw(n, findings, HYP3)
    try:
        _feed(ladder, vs, [2, 1])
        for h, (amount, _lag) in enumerate(HYP3):
            scaled = [dict(f, rate=f['rate'] * amount) for f in findings]
            one = _Raw(n, scaled, [(1.0, 0)])
            try:
                _feed(one, vs, [2, 1])
                for what in range(3):
                    assert np.array_equal(one.plane(what, 0), ladder.plane(what, h)), (h, what)
                assert np.array_equal(one.rows()[0][:, 0], ladder.rows()[0][:, h])
            finally:
                one.close()
    finally:
        ladder.close()


def test_prior_masks_cells_and_weighs_the_rows():
    n = 65
    findings, vs = _twin_like_findings(n), _member_fields(n)[:3]
    days = sorted({f['day'] for f in findings})
    r, c = np.mgrid[0:n, 0:n]
    prior = -0.002 * ((r - 40.0) ** 2 + (c - 30.0) ** 2)
    prior[(r + 2 * c) % 5 == 0] = -np.inf               # scattered through every wave
    prior[:, :20] = -np.inf                             # and whole waves
    raw, flat = _Raw(n, findings, HYP3, prior), _Raw(n, findings, HYP3)
    try:
        for v in vs:
            raw.add(v)
            flat.add(v)
            got, free = raw.planes(2), flat.planes(2)
            assert (got[:, prior == -np.inf] == -np.inf).all()
            assert np.array_equal(got[:, prior != -np.inf], free[:, prior != -np.inf])    # the prior changes no l
        A = raw.planes(0)
        assert (A[:, prior == -np.inf] == -np.inf).all() and (raw.planes(1)[:, prior == -np.inf] == 0).all()
        assert (A != -np.inf).any()
        rows, _w = raw.rows()
        for m, v in enumerate(vs):
            l_mp, parts = OR.loglik_mp(findings, HYP3, _ref_fields(v, [0], days), prior)
            lb = OR.loglik_bound(len(findings), parts)
            for h, (val, cells) in enumerate(OR.rows_mp(l_mp, prior)):
                e = float(OR.diff([rows[m, h, 0] + math.log(rows[m, h, 1])], [val])[0])
                assert e <= OR.row_bound(float(lb[h].max()), cells, float(val)), (m, h)
        assert not np.array_equal(rows, flat.rows()[0])
        # a prior with NaN or +inf is refused with the cell named
        bad = prior.copy()
        bad[3, 4] = np.nan
        with pytest.raises(Exception, match='cell 199'):
            _Raw(n, findings, HYP3, bad)
    finally:
        raw.close()
        flat.close()


def test_raw_lag_groups_and_a_finding_before_the_release():
    """two groups over one record: lag 2 sees other scales, and nothing on the days before its release"""
    n = 65
    findings = _twin_like_findings(n)                    # days 0, 1, 2: two of them lie before a release on day 2
    hyp = [(1.0, 0), (1.0, 2), (4.0, 2), (0.25, 0)]
    v = _member_fields(n)[1]
    raw = _Raw(n, findings, hyp)
    try:
        raw.add(v, 3)
        got, want = _check_l(raw, v, 'lags')
        assert (got[1] == -np.inf).all()                 # a positive count on day 0 cannot come from a day-2 release
        assert (got[0] != -np.inf).any()
    finally:
        raw.close()
    soft = [OR.probe(f['row'], f['col'], f['day'], 'none', f['rate']) for f in findings[:3]] + \
        [OR.probe(n // 2 + 4, n // 2 - 2, 2, 'count', 0.5, 2)]
    raw = _Raw(n, soft, hyp)
    try:
        raw.add(v, 3)
        got, want = _check_l(raw, v, 'lags, soft')
        assert (got[1] != -np.inf).any() and not np.array_equal(got[1], got[0])
    finally:
        raw.close()


def test_lagged_models_against_the_reference():
    """the Kalbar model, lags 0 and 2, a finding earlier than the lag: the class against the restatement over the
    fields fetched from the lagged models"""
    from parasitoids_amd.predictive import OriginMaps
    R = 32
    res = 10000.0 / R
    pm = _pop_model(R, mode='exact')
    findings = [(2 * res, 3 * res, 3, 'count', 0.02, 2), (-4 * res, 1 * res, 4, 'found', 0.05),
                (10 * res, -8 * res, 1, 'none', 0.01), (0.0, 5 * res, 5, 'count', 0.001, 0),
                (R * res, -R * res, 4, 'none', 0.01)]
    arg = dict(findings=findings, amounts=[2.0], lags=[0, 2])
    with OriginMaps.with_lagged_models(pm, arg) as om:
        assert om.lags == [0, 2] and om.days == [1, 3, 4, 5] and om.pairs == [(2.0, 0), (2.0, 2)]
        assert om.slots == [[1, 3, 4, 5], [None, 1, 2, 3]]
        ls, bounds = [], []
        for member, w in zip(MEMBERS[:3], (1, 2, 1)):
            _evaluate(pm, member)
            om.evaluate_lagged(HP, member[0], DLP, member[1], NPER)
            om.add(w)
            fields = {0: dict(enumerate(_fields(pm, range(6)))), 2: dict(enumerate(_fields(om.lagged[2], range(4))))}
            l_mp, parts = OR.loglik_mp(om.findings, om.pairs, fields)
            got = np.stack([om.plane('l', h) for h in range(2)])
            _against_mp(got, l_mp, parts, len(findings), member)
            assert OR.finite_mask(l_mp).any()
            ls.append(l_mp)
            bounds.append(OR.loglik_bound(len(findings), parts))
        assert om.members == 3 and om.total_weight == 4.0
        E_mp = OR.evidence_mp(ls, (1, 2, 1))
        for h in range(2):
            E = om.log_evidence(h)
            fin = OR.finite_mask(E_mp[h])
            assert np.array_equal(E != -np.inf, fin), h
            eb = OR.evidence_bound(3, np.max(bounds, axis=0)[h], E)
            err = OR.diff(E[fin], E_mp[h][fin])
            assert (err <= eb[fin]).all(), (h, float((err / eb[fin]).max()))
            RATIOS['E'] = max(RATIOS['E'], float((err / eb[fin]).max()))
        P = om.posterior()
        assert abs(P.sum() - 1.0) < 1e-12 and om.region(0.5).sum() <= om.region(0.95).sum()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', UserWarning)
            mode, d = om.mode(), om.diagnostics()
        Ph = om.posterior(mode['hypothesis'])
        assert Ph[mode['row'], mode['col']] == Ph.max() == mode['mass'] and d['rows'] == 4
        assert mode['cell_mass'] == P[mode['row'], mode['col']]
        assert om.log_weights().shape == (4,) and om.nbytes > 0 and om.capacity >= 3


def test_refusals_of_the_c_abi():
    n = 65
    findings = _twin_like_findings(n)
    raw = _Raw(n, findings, [(1.0, 0), (1.0, 2)])
    L, lib = raw.L, raw.lib
    try:
        buf = np.empty((n, n))
        assert lib.ps_origin_fetch(raw.h, 0, 0, L.p_f64(buf)) == L.PS_ERR_STATE          # before the first member
        assert 'no member' in lib.ps_last_error().decode()
        raw.solver.set_state(_member_fields(n)[0])
        assert raw.add_group(1, 1) == L.PS_ERR_STATE                                     # group 1 before group 0
        assert 'group 1 given' in lib.ps_last_error().decode()
        args0, _keep0 = raw.group_args(0)
        assert lib.ps_origin_add(raw.h, raw.solver._h, 2, *args0[1:], 1) == L.PS_ERR_BAD_ARG       # group 2 of 2
        assert raw.add_group(0, 0) == L.PS_ERR_BAD_ARG                                            # weight 0
        assert raw.add_group(0, 2) == L.PS_OK
        assert raw.add_group(0, 2) == L.PS_ERR_STATE                                     # group 0 may not come early
        assert lib.ps_origin_fetch(raw.h, 0, 0, L.p_f64(buf)) == L.PS_ERR_STATE          # a member under way
        assert raw.add_group(1, 3) == L.PS_ERR_BAD_ARG                                   # another weight
        assert 'weight 3' in lib.ps_last_error().decode()
        assert raw.info()[1] == 0                                                        # not counted yet
        assert raw.add_group(1, 2) == L.PS_OK and raw.info()[:2] == (2.0, 1)
        assert lib.ps_origin_fetch(raw.h, 3, 0, L.p_f64(buf)) == L.PS_ERR_BAD_ARG
        assert lib.ps_origin_fetch(raw.h, 0, 2, L.p_f64(buf)) == L.PS_ERR_BAD_ARG
        assert lib.ps_origin_members(raw.h, 5, None, None) == L.PS_ERR_BAD_ARG
        args, _keep = raw.group_args(0)
        assert lib.ps_origin_add(raw.h, raw.solver._h, args[0], 2, *args[2:], 1) == L.PS_ERR_BAD_ARG   # slot count
        # another domain, another request
        other = _Raw(97, [OR.probe(3, 3, 0, 'none', 1.0)], [(1.0, 0)])
        try:
            assert lib.ps_origin_add(raw.h, other.solver._h, *args, 1) == L.PS_ERR_BAD_ARG
            assert 'domain' in lib.ps_last_error().decode()
            assert lib.ps_origin_merge(raw.h, other.h) == L.PS_ERR_BAD_ARG
        finally:
            other.close()
        diff = _Raw(n, findings, [(1.0, 0), (2.0, 2)], solver=raw.solver)
        try:
            assert lib.ps_origin_merge(raw.h, diff.h) == L.PS_ERR_BAD_ARG and 'differ' in lib.ps_last_error().decode()
            assert lib.ps_origin_merge(raw.h, raw.h) == L.PS_ERR_BAD_ARG
        finally:
            diff.close()
        # bad counts at create, each with the offender named
        h = L._VP()

        def create(nfind=1, row=3, kind=1, rate=1.0, cnt=0.0, nslot=1, nhyp=1, amount=1.0, group=0, ngroup=1, N=n, slot=0):
            k = max(nfind, 1)
            return lib.ps_origin_create(0, N, nfind, L.p_i32(L.i32([row] * k)), L.p_i32(L.i32([3] * k)),
                                        L.p_i32(L.i32([slot] * k)), L.p_i32(L.i32([kind] * k)), L.p_f64(L.f64([rate] * k)),
                                        L.p_f64(L.f64([cnt] * k)), nslot, nhyp, L.p_f64(L.f64([amount] * max(nhyp, 1))),
                                        L.p_i32(L.i32([group] * max(nhyp, 1))), ngroup, None, C.byref(h))
        for kw, word in [(dict(nfind=0), 'findings'), (dict(nfind=65), 'findings'), (dict(nslot=33), 'days'),
                         (dict(nhyp=9), 'hypotheses'), (dict(ngroup=5), 'groups'), (dict(N=64), 'odd'),
                         (dict(row=n), 'outside'), (dict(slot=1), 'day slot'), (dict(kind=3), 'kind'),
                         (dict(rate=0.0), 'rate'), (dict(kind=0, cnt=1.5), 'whole number'),
                         (dict(amount=float('inf')), 'amount'), (dict(group=1), 'group 1'),
                         (dict(ngroup=2), 'group 1 has no hypothesis')]:
            assert create(**kw) == L.PS_ERR_BAD_ARG, kw
            assert word in lib.ps_last_error().decode(), (kw, lib.ps_last_error())
            assert not h
    finally:
        raw.close()


def test_posterior_predictive_with_origin_against_the_class_fed_by_hand(tmp_path):
    import json
    import os
    from parasitoids_amd import mcmc
    from parasitoids_amd import predictive as PR
    from test_reweight_gpu import _chain
    R = 32
    res_m = 10000.0 / R
    ta, names = _chain([3, 2])
    tb, _ = _chain([1, 2, 2])
    traces = [ta, tb[1:]]                                    # the second chain: two runs of other members
    chains = [(t, names) for t in traces]
    plan = dict(sites=[(0.0, 0.0, 0.6), (7 * res_m, -3 * res_m, 0.5, 2)], days=[0, 3, 5])    # shares the lag-2 model
    arg = dict(findings=[(2 * res_m, 3 * res_m, 3, 'count', 0.02, 2), (-4 * res_m, res_m, 4, 'found', 0.05),
                         (10 * res_m, -8 * res_m, 1, 'none', 0.01)], amounts=[0.1, 1.0, 10.0], lags=[0, 2], levels=[0.5, 0.9])
    pm = _pop_model(R, mode='exact')
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    common = dict(thresholds=[1.0], sites=plan, cell_area=res_m ** 2)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = PR.posterior_predictive(pm, chains, origin=arg, **common)
        bare = PR.posterior_predictive(pm, chains, **common)
    om = res.origin
    assert res.failed == 0 and res.evaluations == 4 and bare.origin is None
    assert (om.total_weight, om.members) == (9.0, 4) and len(om.pairs) == 6 and om.lags == [0, 2]
    # the other maps are what they are without origin=
    for got, want in ((res.summary, bare.summary), (res.sites.summary, bare.sites.summary)):
        for d in want.days:
            assert np.array_equal(got.mean(d), want.mean(d)) and np.array_equal(got.variance(d), want.variance(d))
    # the class fed by hand: every run once more, per chain a handle of its own, merged in chain order
    hand = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for ci in range(2):
            hand.append(PR.OriginMaps.with_lagged_models(pm, arg))
            for c, first, weight in res.runs:
                if c == ci:
                    args = mcmc.model_args(traces[ci][first, cols])
                    pm.evaluate(*args, want_stats=False)
                    # as the driver evaluates it: the plan's day 5 needs 4 days of the lag-2 model, the findings 3, and
                    # the solver's FFT size -- so the last bits -- follows the days evaluated
                    hand[ci].lagged[2].evaluate(*args, ndays=4, want_stats=False)
                    hand[ci].add(weight)
        hand[0].merge(hand[1])
    want = hand[0]
    for h in range(6):
        for what in ('A', 'S'):
            assert np.array_equal(om.plane(what, h), want.plane(what, h)), (h, what)
    assert np.array_equal(om.member_rows()[0], want.member_rows()[0])
    assert om.member_rows()[1].tolist() == [w for _c, _f, w in res.runs]
    assert np.array_equal(om.log_weights(), want.log_weights()) and om.log_weights().shape == (9,)
    assert (om.posterior() > 0).any()
    # the files
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        os.makedirs(str(tmp_path / 'a'))
        os.makedirs(str(tmp_path / 'b'))
        npz, js = res.save(str(tmp_path / 'a' / 'pp'))
        bare.save(str(tmp_path / 'b' / 'pp'))
        names_a, names_b = sorted(os.listdir(str(tmp_path / 'a'))), sorted(os.listdir(str(tmp_path / 'b')))
        assert sorted(set(names_a) - set(names_b)) == ['pp_origin.npz']
        for name in names_b:
            if name.endswith('.npz'):
                fa, fb = np.load(str(tmp_path / 'a' / name)), np.load(str(tmp_path / 'b' / name))
                assert fa.files == fb.files and all(np.array_equal(fa[k], fb[k]) for k in fb.files), name
        f = np.load(str(tmp_path / 'a' / 'pp_origin.npz'))
        assert sorted(f.files) == sorted(['log_evidence_h%d' % h for h in range(6)] + ['posterior', 'region_l50', 'region_l90',
                                                                                      'member_rows', 'member_weights',
                                                                                      'hypotheses'])
        assert np.array_equal(f['posterior'], om.posterior()) and np.array_equal(f['region_l90'], om.region(0.9))
        assert np.array_equal(f['log_evidence_h3'], om.log_evidence(3)) and f['region_l50'].dtype == np.int8
        assert f['hypotheses'].tolist() == [list(h) for h in om.pairs] and f['member_rows'].shape == (4, 6, 2)
        block = json.load(open(js))['predictive']['origin']
        meta_b = json.load(open(str(tmp_path / 'b' / 'pp.json')))['predictive']
        assert 'origin' not in meta_b
        assert sorted(block) == sorted(['findings', 'hypotheses', 'levels', 'prior', 'members', 'total_weight', 'masses',
                                        'mode', 'areas', 'diagnostics', 'warnings'])
        assert block['members'] == 4 and block['total_weight'] == 9.0 and sorted(block['areas']) == ['l50', 'l90']
        assert abs(sum(h['mass'] for h in block['masses']['hypotheses']) - 1.0) < 1e-12
        assert block['mode']['row'] == om.mode()['row'] and block['diagnostics']['rows'] == 9
    # the command line's request is the argument itself
    text = ';'.join(','.join(str(x) for x in f) for f in arg['findings'])
    assert PR.origin_request(text, '0.1,1,10', '0,2', '0.5,0.9', '', 10000.0, R) == \
        dict(arg, findings=[tuple(f) for f in arg['findings']])
    # a second run takes the members' evidence as row log-weights: every forward map updated for the findings
    lw = [om.log_weights()[:5], om.log_weights()[5:]]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        again = PR.posterior_predictive(pm, chains, thresholds=[1.0], reweight={'unknown origin': dict(log_weights=lw)})
    assert again.reweight is not None and again.reweight_info['diagnostics']['unknown origin']['rows'] == 9
    for r in (res, bare, again):
        for acc in (r.summary, r.sites, r.origin, r.reweight):
            if acc is not None:
                acc.close()
    for h in hand:
        h.close()


def test_twin_experiment_on_the_device():
    """the inputs of the CPU twin experiment (origin_ref.twin_*): every member's chain runs on the device, the handle
    reads its day records, and the device's own (A, S) puts the known origin into the 50 % and the 95 % region; l, E,
    the posterior and the regions against the reference over the host-fetched records"""
    from parasitoids_amd import _lib as L
    from parasitoids_amd import predictive as PR
    from parasitoids_amd.hip_lib import HipSolve
    n, nd = OR.TWIN_N, OR.TWIN_DAYS
    findings, W = OR.twin_findings(), sum(OR.TWIN_WEIGHTS)
    days = list(range(1, nd + 1))
    lib, h = L.load(), L._VP()
    L.check(lib.ps_origin_create(
        0, n, len(findings), L.p_i32(L.i32([p['row'] for p in findings])), L.p_i32(L.i32([p['col'] for p in findings])),
        L.p_i32(L.i32([days.index(p['day']) for p in findings])), L.p_i32(L.i32([KIND[p['kind']] for p in findings])),
        L.p_f64(L.f64([p['rate'] for p in findings])), L.p_f64(L.f64([p['n'] or 0 for p in findings])), nd, 1,
        L.p_f64(L.f64([OR.TWIN_HYP[0][0]])), L.p_i32(L.i32([0])), 1, None, C.byref(h)))
    kind, idx = L.i32([L.REC_CHAIN] * nd), L.i32(list(range(nd)))        # model day d is chain record d - 1
    one, delta = L.f64([1.0] * nd), L.i32([1] * nd)
    ls, bounds = [], []
    try:
        for m, w in enumerate(OR.TWIN_WEIGHTS):
            state, kernels = OR.twin_stack(m)
            s = HipSolve(state, [OR.TWIN_K, OR.TWIN_K], mode='exact')
            try:
                s.set_kernels(kernels)
                s.run_chain()
                stats = s.chain_stats(0, nd)
                L.check(lib.ps_origin_add(h, s._h, 0, nd, L.p_i32(kind), L.p_i32(idx), L.p_f64(one), L.p_f64(one),
                                          L.p_i32(delta), 1e-8, w))
                fields = {0: {d: s.chain_solution(d - 1, stats[d - 1]).toarray() for d in days}}
                got = np.empty((1, n, n))
                L.check(lib.ps_origin_fetch(h, 2, 0, L.p_f64(got[0])))
            finally:
                s.close()
            l_mp, parts = OR.loglik_mp(findings, OR.TWIN_HYP, fields)
            _against_mp(got, l_mp, parts, len(findings), ('twin', m))
            ls.append(l_mp)
            bounds.append(OR.loglik_bound(len(findings), parts))
        A, S = np.empty((n, n)), np.empty((n, n))
        L.check(lib.ps_origin_fetch(h, 0, 0, L.p_f64(A)))
        L.check(lib.ps_origin_fetch(h, 1, 0, L.p_f64(S)))
    finally:
        lib.ps_origin_destroy(h)
    E = PR.origin_log_evidence(A, S, W)
    E_mp = OR.evidence_mp(ls, OR.TWIN_WEIGHTS)[0]
    fin = OR.finite_mask(E_mp)
    assert np.array_equal(E != -np.inf, fin) and fin.sum() > 100
    eb = OR.evidence_bound(8, np.max(bounds, axis=0)[0], E)
    err = OR.diff(E[fin], E_mp[fin])
    assert (err <= eb[fin]).all(), float((err / eb[fin]).max())
    RATIOS['E'] = max(RATIOS['E'], float((err / eb[fin]).max()))
    P = PR.origin_posterior(E[None])[0]
    P_mp = OR.posterior_mp(E_mp[None])[0]
    assert np.array_equal(P == 0.0, P_mp == 0.0) or (P_mp[P == 0.0] < 1e-300).all()
    assert (np.abs(P - P_mp) <= OR.posterior_bound(float(eb[fin].max()), int(fin.sum()), P_mp) + 1e-320).all()
    r50, r95 = PR.origin_region(P, 0.5), PR.origin_region(P, 0.95)
    assert r50[OR.TWIN_ORIGIN] == 1 and r95[OR.TWIN_ORIGIN] == 1           # the device recovers the known origin
    assert np.array_equal(r50, OR.region(P_mp, 0.5)) and np.array_equal(r95, OR.region(P_mp, 0.95))
    assert (int(r50.sum()), int(r95.sum())) == (3, 9)
    assert np.unravel_index(int(np.argmax(P)), P.shape) == OR.TWIN_ORIGIN
    print('observed error / bound after the twin experiment: l %.3f, E %.3f' % (RATIOS['l'], RATIOS['E']))


def test_member_rows_grow_past_their_first_capacity():
    """more members than the 64 rows a handle starts with: by adds, by a merge that crosses the capacity, and by a
    reserve between the two groups of a member under way; the rows are those of a handle that never grew"""
    n = 65
    findings = [OR.probe(30, 33, 0, 'count', 0.5, 1), OR.probe(5, 60, 2, 'none', 0.25)]
    hyp = [(1.0, 0), (3.0, 0), (1.0, 2)]
    vs = _member_fields(n)
    big, a, b, pre = (_Raw(n, findings, hyp) for _ in range(4))
    try:
        assert big.info()[2] == 64
        pre.L.check(pre.lib.ps_origin_reserve(pre.h, 100))
        assert pre.info()[2] >= 100 and pre.info()[3] > big.info()[3]
        for k in range(70):
            v, w = vs[k % 6], 1 + k % 3
            big.add(v, w)
            (a if k < 40 else b).add(v, w)
            if k == 10:                                  # the rows grow while the member's second group is still to come
                pre.solver.set_state(v)
                pre.L.check(pre.add_group(0, w))
                pre.L.check(pre.lib.ps_origin_reserve(pre.h, 300))
                pre.L.check(pre.add_group(1, w))
            else:
                pre.add(v, w)
        assert big.info()[1:3] == (70, 128) and a.info()[2] == 64 and pre.info()[2] >= 300
        a.L.check(a.lib.ps_origin_merge(a.h, b.h))
        assert a.info()[1:3] == (70, 128)
        rows, w = big.rows()
        assert w.tolist() == [1 + k % 3 for k in range(70)] and np.isfinite(rows[:, 0, :]).all()
        for other in (a, pre):
            r2, w2 = other.rows()
            assert np.array_equal(r2, rows) and np.array_equal(w2, w)
        assert np.array_equal(pre.planes(0), big.planes(0)) and np.array_equal(pre.planes(1), big.planes(1))
        assert np.array_equal(rows[6], rows[0])          # the same field again: the same row
    finally:
        for r in (big, a, b, pre):
            r.close()

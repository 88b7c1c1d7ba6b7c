"""GPU tests of the origin maps over known releases in the background (ps_origin_set_known, ps_origin_background,
ps_origin_fetch_background, ps_origin_null_rows; predictive.OriginMaps with known=): the raw C ABI over crafted state
records at N = 65 and 129 -- bg bit for bit against the numpy loop, l and l0 against the 40-digit reference within
the unchanged bounds of DESIGN 7y, the -inf pattern exactly, the identity l == l0, a zero background against a handle
without known releases bit for bit, members, merge, reset, row growth and every new refusal -- then the lagged models
of the Kalbar wind, the twin experiment with every chain run on the device, and the driver.  The raw handles read
every day from one state record through the slot's stat_scale, as tests/test_origin_gpu.py's do."""
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest

import origin_known_ref as KR
import origin_ref as OR
from test_arrival_gpu import MEMBERS, HP, DLP, NPER, _pop_model, _evaluate, _fields
from test_origin_gpu import KIND, WEIGHTS6, _Raw, _member_fields, _positive, _ref_fields, _scale

pytestmark = pytest.mark.gpu


class _RawK(_Raw):
    """a ps_origin handle with known releases over the state record of a solver.  knowns: origin_known_ref.known"""

    def __init__(self, n, findings, hypotheses, knowns=(), prior=None, solver=None):
        super().__init__(n, findings, hypotheses, prior, solver)
        self.knowns = list(knowns)
        self.klags = sorted({k['lag'] for k in self.knowns})
        if self.knowns:
            self.L.check(self.set_known(self.knowns))

    def set_known(self, knowns, nk=None, groups=None):
        L = self.L
        klags = sorted({k['lag'] for k in knowns})
        groups = [klags.index(k['lag']) for k in knowns] if groups is None else groups
        return self.lib.ps_origin_set_known(
            self.h, len(knowns), L.p_i32(L.i32([k['drow'] for k in knowns])), L.p_i32(L.i32([k['dcol'] for k in knowns])),
            L.p_f64(L.f64([k['amount'] for k in knowns])), L.p_i32(L.i32(groups)), len(klags) if nk is None else nk)

    def background_group(self, g):
        L, lag = self.L, self.klags[g]
        kind = L.i32([L.REC_STATE if d >= lag else L.REC_NONE for d in self.days])
        stat = L.f64([_scale(lag, d - lag) if d >= lag else 0.0 for d in self.days])
        zero, one = L.i32([0] * len(self.days)), L.f64([1.0] * len(self.days))
        return self.lib.ps_origin_background(self.h, self.solver._h, g, len(self.days), L.p_i32(kind), L.p_i32(zero),
                                             L.p_f64(stat), L.p_f64(one), L.p_i32(zero), 0.0)

    def add(self, v, weight=1):
        self.solver.set_state(v)
        for g in range(len(self.klags)):
            self.L.check(self.background_group(g))
        for g in range(len(self.lags)):
            self.L.check(self.add_group(g, weight))

    def background(self):
        bg, l0 = np.empty(len(self.findings)), C.c_double()
        self.L.check(self.lib.ps_origin_fetch_background(self.h, self.L.p_f64(bg), C.byref(l0)))
        return bg, l0.value

    def null_rows(self):
        out = np.empty(self.info()[1])
        self.L.check(self.lib.ps_origin_null_rows(self.h, len(out), self.L.p_f64(out)))
        return out

    def ref_fields(self, v):
        return _ref_fields(v, sorted(set(self.lags) | set(self.klags)), self.days)


def _against_mp(got, l_mp, parts, nfind, what):
    fin = OR.finite_mask(l_mp)
    bad = np.argwhere((got != -np.inf) != fin)
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist())             # the -inf pattern: exact
    assert not np.isnan(got).any() and not (got == np.inf).any(), what
    ratio = 0.0
    if fin.any():
        bound = OR.loglik_bound(nfind, parts)[fin]                       # DESIGN 7y's bound, unchanged
        err = OR.diff(got[fin], l_mp[fin])
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        assert (err <= bound).all(), (what, ratio)
    return ratio


def _check_null(l0, bg, findings, what):
    l0_mp, p0 = KR.null_row_mp(findings, bg)
    assert (l0 == -np.inf) == (l0_mp is None), what
    if l0_mp is not None:
        assert OR.diff([l0], [l0_mp])[0] <= OR.loglik_bound(len(findings), p0), what


def _edge_case(n):
    """findings and known releases: ours at the centre; one whose offset pushes the source row of every finding above
    row n - 5 off the domain while the column stays inside; a lag-2 group with findings before its release.  Finding 0
    can exclude and lies in our plume (bg > 0); finding 1 can exclude and lies far from every known plume (bg == 0)"""
    R = n // 2
    findings = [OR.probe(R + 3, R - 2, 0, 'count', 0.5, 4), OR.probe(R + 25, R + 20, 1, 'found', 0.5),
                OR.probe(n - 2, R + 1, 1, 'none', 0.75), OR.probe(0, 0, 2, 'none', 0.5),
                OR.probe(R - 1, R + 2, 3, 'count', 0.5, 0), OR.probe(R + 6, R - 4, 2, 'count', 0.25, 2),
                OR.probe(n - 1, R - 6, 3, 'count', 0.125, 0)]
    knowns = [KR.known(0, 0, 1.0, 0), KR.known(2, -3, 0.25, 2), KR.known(n - 5, 3, 0.5, 0), KR.known(-1, 1, 0.75, 2)]
    return findings, knowns, [(0.5, 0), (2.0, 0), (1.0, 2)]


@pytest.mark.parametrize('n', [65, 129])
def test_background_values_and_likelihood_against_the_restatement(n):
    findings, knowns, hyp = _edge_case(n)
    plume, pos = _member_fields(n)[1], _positive(n)
    raw = _RawK(n, findings, hyp, knowns)
    try:
        assert raw.klags == [0, 2] and raw.days == [0, 1, 2, 3]
        for name, v in (('plume', plume), ('positive', pos)):
            raw.add(v, 2)
            fields = raw.ref_fields(v)
            bg, l0 = raw.background()
            want = KR.background(findings, knowns, fields)
            assert np.array_equal(bg, want), (name, bg, want)            # bit for bit
            got = raw.planes(2)
            if n == 65:                                                  # mpmath where a test can afford it
                l_mp, parts = KR.loglik_mp(findings, hyp, fields, bg)
                _against_mp(got, l_mp, parts, len(findings), name)
            else:                                                        # each side within one bound of the exact value
                ref = KR.loglik(findings, hyp, fields, bg)
                assert np.array_equal(got == -np.inf, ref == -np.inf), name
                fin = ref != -np.inf
                bound = OR.loglik_bound(len(findings), KR.loglik_parts(findings, hyp, fields, bg))
                assert (np.abs(got[fin] - ref[fin]) <= 2.0 * bound[fin]).all(), name
            _check_null(l0, bg, findings, name)
            if name == 'plume':
                # an excluding finding inside our plume and one that no known release reaches
                assert bg[0] > 0 and bg[1] == 0.0 and bg[3] == 0.0
                assert (got == -np.inf).any() and (got != -np.inf).any() and l0 == -np.inf
            else:
                # the source of known 2 leaves the domain on the row axis alone for every finding above row n - 5
                assert (bg > 0).all() and l0 != -np.inf
                assert (got[:2] != -np.inf).all()                        # bg > 0: no finding excludes any cell
                lone = [k for k in knowns if k is not knowns[2]]
                without = KR.background(findings, lone, fields)
                assert [bool(a != b) for a, b in zip(bg, without)] == [f['row'] >= n - 5 for f in findings]
            # findings on day 0 and 1 precede the lag-2 group: it adds nothing to them
            early = KR.background(findings, [k for k in knowns if k['lag'] == 0], fields)
            assert all(bg[o] == early[o] for o, f in enumerate(findings) if f['day'] < 2)
        assert raw.null_rows().tolist()[1] == raw.background()[1] and raw.info()[:2] == (4.0, 2)
    finally:
        raw.close()


def test_identity_at_cells_without_a_shifted_read():
    n = 65
    R = n // 2
    findings = [OR.probe(R + 3, R - 2, 0, 'count', 0.5, 4), OR.probe(R + 6, R - 4, 1, 'found', 0.25),
                OR.probe(R, R - 5, 2, 'count', 0.5, 1), OR.probe(0, 0, 1, 'none', 0.5), OR.probe(R + 1, R - 3, 2, 'none', 0.125)]
    hyp = [(0.25, 0), (1.0, 0), (4.0, 0), (1.0, 1)]
    raw = _RawK(n, findings, hyp, [KR.known(0, 0, 1.0, 0), KR.known(1, 1, 0.5, 1)])
    try:
        for v in _member_fields(n)[:2]:
            raw.add(v)
            fields = raw.ref_fields(v)
            bg, l0 = raw.background()
            assert np.isfinite(l0) and (bg[:3] > 0).all()
            free = KR.untouched(findings, hyp, fields)
            got = raw.planes(2)
            assert free.all(axis=0).sum() > 1000 and not free.all()
            assert (got[free] == l0).all()                               # bit for bit
            assert (got[~free] != l0).any() and (got != -np.inf).all()
    finally:
        raw.close()


def test_zero_background_is_the_handle_without_known_releases():
    n = 65
    R = n // 2
    findings = [OR.probe(R + 6, R - 4, 0, 'count', 0.5, 4), OR.probe(R + 9, R - 1, 1, 'count', 0.5, 2),
                OR.probe(R + 7, R - 6, 1, 'found', 0.5), OR.probe(0, 0, 1, 'none', 0.5), OR.probe(R + 12, R + 12, 0, 'none', 1.0)]
    hyp = [(0.1, 0), (1.0, 0), (10.0, 1)]
    # a release 20 cells to the north-east, whose plume ends short of every finding, and one whose every source leaves the
    # domain
    knowns = [KR.known(-20, 20, 1.0, 0), KR.known(n - 1, -(n - 1), 3.0, 1)]
    with_bg, plain = _RawK(n, findings, hyp, knowns), _RawK(n, findings, hyp)
    try:
        for v, w in zip(_member_fields(n)[:3], (1, 3, 2)):
            with_bg.add(v, w)
            plain.add(v, w)
            bg, _l0 = with_bg.background()
            assert np.array_equal(bg, np.zeros(len(findings))) and not np.signbit(bg).any()
            assert np.array_equal(with_bg.planes(2), plain.planes(2))
        for what in (0, 1):
            assert np.array_equal(with_bg.planes(what), plain.planes(what)), what
        assert np.array_equal(with_bg.rows()[0], plain.rows()[0]) and (with_bg.planes(0) != -np.inf).any()
        assert (with_bg.null_rows() == -np.inf).all()                    # a positive count that no known release explains
        assert with_bg.info()[3] > plain.info()[3]                       # info's bytes include the tables and null rows
    finally:
        with_bg.close()
        plain.close()


def _six_case(n=65):
    R = n // 2
    findings = [OR.probe(R + 3, R - 2, 0, 'count', 0.5, 4), OR.probe(R + 6, R - 4, 1, 'found', 0.25),
                OR.probe(R + 9, R - 1, 2, 'count', 0.25, 1), OR.probe(0, 0, 1, 'none', 0.5), OR.probe(R + 1, R - 3, 2, 'none', 0.125)]
    return findings, [(0.5, 0), (2.0, 0), (1.0, 2)], [KR.known(0, 0, 1.0, 0), KR.known(2, 1, 0.5, 2)]


def _feed(raw, vs, weights):
    for v, w in zip(vs, weights):
        raw.add(v, w)


def test_six_members_merge_reset_and_the_same_bits():
    n = 65
    findings, hyp, knowns = _six_case(n)
    vs = _member_fields(n)
    raw, two, a, b, other = (_RawK(n, findings, hyp, k) for k in (knowns,) * 4 + (knowns[:1],))
    try:
        _feed(raw, vs, WEIGHTS6)
        assert raw.info()[:2] == (float(sum(WEIGHTS6)), 6)
        null = raw.null_rows()
        ls, bgs = [], []
        for m, v in enumerate(vs):                                       # every member's l0 against the restatement
            fields = raw.ref_fields(v)
            bg = KR.background(findings, knowns, fields)
            _check_null(null[m], bg, findings, m)
            bgs.append(bg)
            ls.append(KR.loglik(findings, hyp, fields, bg))
        assert np.isfinite(null).all() and len(set(null.tolist())) == 6
        assert np.array_equal(raw.background()[0], bg) and raw.background()[1] == null[-1]
        # E against the restatement's: the members' l within one bound each, the update's own term
        A, S = raw.planes(0), raw.planes(1)
        rows = raw.rows()[0]
        E, Er = OR.evidence(A, S, sum(WEIGHTS6)), OR.evidence(*OR.accumulate(ls, WEIGHTS6), sum(WEIGHTS6))
        assert np.array_equal(E == -np.inf, Er == -np.inf)
        lmax = np.max([OR.loglik_bound(len(findings), KR.loglik_parts(findings, hyp, raw.ref_fields(v), bgs[m]))
                       for m, v in enumerate(vs)], axis=0)
        fin = E != -np.inf                                               # either side within one bound of the exact E
        assert (np.abs(E[fin] - Er[fin]) <= 2.0 * OR.evidence_bound(6, lmax, E)[fin]).all()
        # the same calls give the same bits: a second handle, and the first after reset
        _feed(two, vs, WEIGHTS6)
        for what in range(3):
            assert np.array_equal(two.planes(what), raw.planes(what)), what
        assert np.array_equal(two.rows()[0], rows) and np.array_equal(two.null_rows(), null)
        raw.L.check(raw.lib.ps_origin_reset(raw.h))
        assert raw.info()[:2] == (0.0, 0) and raw.null_rows().shape == (0,)
        assert raw.lib.ps_origin_fetch_background(raw.h, None, None) == raw.L.PS_ERR_STATE
        _feed(raw, vs, WEIGHTS6)
        assert np.array_equal(raw.planes(0), A) and np.array_equal(raw.planes(1), S)
        assert np.array_equal(raw.rows()[0], rows) and np.array_equal(raw.null_rows(), null)
        # two handles merged: the null rows concatenated exactly, the source unchanged
        _feed(a, vs[:3], WEIGHTS6[:3])
        _feed(b, vs[3:], WEIGHTS6[3:])
        a.L.check(a.lib.ps_origin_merge(a.h, b.h))
        assert a.info()[:2] == (float(sum(WEIGHTS6)), 6)
        assert np.array_equal(a.null_rows(), null) and np.array_equal(b.null_rows(), null[3:])
        assert np.array_equal(a.rows()[0], rows) and np.array_equal(a.planes(0), A)
        assert a.background()[1] == null[2]                              # dst's own last member's
        # other known releases, and none at all: refused
        _feed(other, vs[:1], [1])
        assert a.lib.ps_origin_merge(a.h, other.h) == a.L.PS_ERR_BAD_ARG
        assert 'known releases' in a.lib.ps_last_error().decode()
        bare = _RawK(n, findings, hyp, solver=raw.solver)
        try:
            bare.add(vs[0])
            assert a.lib.ps_origin_merge(a.h, bare.h) == a.L.PS_ERR_BAD_ARG
            assert a.lib.ps_origin_merge(bare.h, a.h) == a.L.PS_ERR_BAD_ARG
        finally:
            bare.close()
        assert a.info()[1] == 6
    finally:
        for r in (raw, two, a, b, other):
            r.close()


def test_rows_and_null_rows_grow_past_their_first_capacity():
    """more members than the 64 rows a handle starts with: by adds, by a merge that crosses the capacity, and by a
    reserve between the backgrounds and the adds of a member under way"""
    n = 65
    findings, hyp, knowns = _six_case(n)
    vs = _member_fields(n)
    big, a, b, pre = (_RawK(n, findings, hyp, knowns) for _ in range(4))
    try:
        assert big.info()[2] == 64
        for k in range(70):
            v, w = vs[k % 6], 1 + k % 4
            big.add(v, w)
            (a if k < 40 else b).add(v, w)
            if k in (10, 64):                                # the rows grow between the backgrounds and the adds
                pre.solver.set_state(v)
                for g in range(2):
                    pre.L.check(pre.background_group(g))
                pre.L.check(pre.lib.ps_origin_reserve(pre.h, 300 if k == 10 else 700))
                pre.L.check(pre.add_group(0, w))
                pre.L.check(pre.lib.ps_origin_reserve(pre.h, 400 if k == 10 else 1100))     # and between two groups
                pre.L.check(pre.add_group(1, w))
            else:
                pre.add(v, w)
        assert big.info()[1:3] == (70, 128) and a.info()[2] == 64 and pre.info()[2] >= 1100
        a.L.check(a.lib.ps_origin_merge(a.h, b.h))
        assert a.info()[1:3] == (70, 128)
        rows, w = big.rows()
        null = big.null_rows()
        assert w.tolist() == [1 + k % 4 for k in range(70)] and np.isfinite(null).all()
        assert np.array_equal(null[6:12], null[:6]) and null[64] == null[4]
        for other in (a, pre):
            assert np.array_equal(other.rows()[0], rows) and np.array_equal(other.null_rows(), null)
        assert np.array_equal(pre.planes(0), big.planes(0)) and np.array_equal(pre.planes(1), big.planes(1))
    finally:
        for r in (big, a, b, pre):
            r.close()


def test_refusals_of_the_c_abi():
    n = 65
    findings, hyp, knowns = _six_case(n)
    raw = _RawK(n, findings, hyp)                            # no known releases yet
    L, lib = raw.L, raw.lib
    ST, BAD = L.PS_ERR_STATE, L.PS_ERR_BAD_ARG
    try:
        buf = np.empty(8)
        # a handle without known releases
        assert lib.ps_origin_fetch_background(raw.h, L.p_f64(buf), None) == ST
        assert lib.ps_origin_null_rows(raw.h, 0, L.p_f64(buf)) == ST and 'no known releases' in lib.ps_last_error().decode()
        raw.klags = [0, 2]
        raw.solver.set_state(_member_fields(n)[0])
        assert raw.background_group(0) == ST and 'no known releases' in lib.ps_last_error().decode()
        # set_known validates as create does, each with its offender named
        one = [KR.known(0, 0, 1.0)]
        for kw, word in [(dict(knowns=[]), '0 known releases'), (dict(knowns=one * 33), '33 known releases'),
                         (dict(knowns=one, nk=5), '5 known groups'), (dict(knowns=one, nk=0), '0 known groups'),
                         (dict(knowns=[KR.known(0, 0, 0.0)]), 'amount 0'), (dict(knowns=[KR.known(0, 0, np.inf)]), 'amount 0'),
                         (dict(knowns=one + [KR.known(n, 0, 1.0)]), 'known release 1 at offset'),
                         (dict(knowns=one + [KR.known(0, -n, 1.0)]), 'known release 1 at offset'),
                         (dict(knowns=one, groups=[1]), 'known group 1 of 1'),
                         (dict(knowns=one * 2, groups=[0, 0], nk=2), 'known group 1 has no release')]:
            assert raw.set_known(**kw) == BAD, kw
            assert word in lib.ps_last_error().decode(), (kw, lib.ps_last_error())
        assert lib.ps_origin_set_known(raw.h, 1, None, None, None, None, 1) == BAD
        L.check(raw.set_known(knowns))
        assert raw.set_known(knowns) == ST and 'already' in lib.ps_last_error().decode()          # once
        # the protocol of one member
        assert raw.add_group(0, 2) == ST and 'background 0 of 2' in lib.ps_last_error().decode()  # before its backgrounds
        assert raw.background_group(1) == ST and 'known group 1 given' in lib.ps_last_error().decode()   # out of order
        raw.klags = [0, 2, 4]
        assert raw.background_group(2) == BAD and 'known group 2 of 2' in lib.ps_last_error().decode()
        raw.klags = [0, 2]
        assert raw.background_group(0) == L.PS_OK
        assert raw.background_group(0) == ST                                                      # twice
        assert raw.add_group(0, 2) == ST and 'background 1 of 2' in lib.ps_last_error().decode()  # not complete yet
        assert lib.ps_origin_fetch(raw.h, 2, 0, L.p_f64(np.empty((n, n)))) == ST
        assert raw.background_group(1) == L.PS_OK
        assert raw.background_group(0) == ST and raw.background_group(1) == ST                    # complete: the adds are next
        assert raw.add_group(1, 2) == ST                                                          # group 1 before group 0
        assert raw.add_group(0, 2) == L.PS_OK
        assert raw.background_group(0) == ST and 'adds of a member are under way' in lib.ps_last_error().decode()
        assert lib.ps_origin_fetch_background(raw.h, L.p_f64(buf), None) == ST                    # a member under way
        assert raw.add_group(1, 2) == L.PS_OK and raw.info()[:2] == (2.0, 1)
        assert raw.add_group(0, 1) == ST                                                          # the next member's backgrounds first
        assert lib.ps_origin_null_rows(raw.h, 2, L.p_f64(buf)) == BAD
        assert lib.ps_origin_fetch_background(raw.h, None, None) == L.PS_OK
        # a merge while the backgrounds of a member are in and its adds are not
        two = _RawK(n, findings, hyp, knowns, solver=raw.solver)
        try:
            two.add(_member_fields(n)[1])
            assert raw.background_group(0) == L.PS_OK
            assert lib.ps_origin_merge(raw.h, two.h) == ST and lib.ps_origin_merge(two.h, raw.h) == ST
            assert raw.background_group(1) == L.PS_OK and raw.add_group(0, 1) == L.PS_OK and raw.add_group(1, 1) == L.PS_OK
            assert lib.ps_origin_merge(raw.h, two.h) == L.PS_OK and raw.info()[1] == 3
        finally:
            two.close()
        # a bad record, another domain and a wrong slot count enqueue nothing and leave the order where it was
        kind = L.i32([L.REC_STATE] * 3)
        zero, one_ = L.i32([0] * 3), L.f64([1.0] * 3)
        args = (L.p_i32(kind), L.p_i32(zero), L.p_f64(one_), L.p_f64(one_), L.p_i32(zero), 0.0)
        assert lib.ps_origin_background(raw.h, raw.solver._h, 0, 2, *args) == BAD and 'days given' in lib.ps_last_error().decode()
        assert lib.ps_origin_background(raw.h, None, 0, 3, *args) == BAD
        other = _Raw(97, [OR.probe(3, 3, 0, 'none', 1.0)], [(1.0, 0)])
        try:
            assert lib.ps_origin_background(raw.h, other.solver._h, 0, 3, *args) == BAD
            assert 'domain' in lib.ps_last_error().decode()
        finally:
            other.close()
        assert raw.background_group(0) == L.PS_OK                        # still at known group 0
        # known releases come before the first member
        late = _RawK(n, findings, hyp, solver=raw.solver)
        try:
            late.add(_member_fields(n)[0])
            assert late.set_known(knowns) == ST and 'before the first member' in lib.ps_last_error().decode()
        finally:
            late.close()
    finally:
        raw.close()


# ---------------------------------------------------------------- models and driver
def test_lagged_models_with_a_known_release():
    """the Kalbar model: two releases of ours known at lag 0, hypotheses at lag 2;
    the class against the restatement over the fields fetched from the lagged models"""
    from parasitoids_amd.predictive import OriginMaps
    R = 32
    res = 10000.0 / R
    pm = _pop_model(R, mode='exact')
    findings = [(2 * res, 3 * res, 3, 'count', 0.02, 2), (-4 * res, 1 * res, 4, 'found', 0.05),
                (10 * res, -8 * res, 1, 'none', 0.01), (0.0, 5 * res, 5, 'count', 0.001, 0), (R * res, -R * res, 4, 'none', 0.01)]
    arg = dict(findings=findings, amounts=[0.5, 2.0], lags=[2], known=[(0.0, 0.0, 1.0), (res, -2 * res, 0.5)])
    with pytest.raises(ValueError, match='no known releases'):
        with OriginMaps.with_lagged_models(pm, dict(arg, known=None)) as om:
            om.second_source()
    with OriginMaps.with_lagged_models(pm, arg) as om:
        assert om.lags == [2] and om.known_lags == [0] and om.model_lags == [0, 2] and sorted(om.lagged) == [2]
        assert om.known_slots == [[1, 3, 4, 5]] and om.slots == [[None, 1, 2, 3]]
        knowns = [KR.known(k['drow'], k['dcol'], k['amount'], k['lag']) for k in om.known]
        assert [(k['drow'], k['dcol']) for k in knowns] == [(0, 0), (2, 1)]
        null = []
        for member, w in zip(MEMBERS[:3], (1, 2, 1)):
            _evaluate(pm, member)
            om.evaluate_lagged(HP, member[0], DLP, member[1], NPER)
            om.add(w)
            fields = {0: dict(enumerate(_fields(pm, range(6)))), 2: dict(enumerate(_fields(om.lagged[2], range(4))))}
            bg, l0 = om.background()
            assert np.array_equal(bg, KR.background(om.findings, knowns, fields)) and (bg > 0).any()
            l_mp, parts = KR.loglik_mp(om.findings, om.pairs, fields, bg)
            got = np.stack([om.plane('l', h) for h in range(2)])
            _against_mp(got, l_mp, parts, len(findings), member)
            _check_null(l0, bg, om.findings, member)
            null.append(l0)
        assert om.members == 3 and np.array_equal(om.null_rows(), np.array(null))
        assert abs(om.log_evidence_null() - KR.log_mean_exp(null, (1, 2, 1))) < 1e-12
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', UserWarning)
            s = om.second_source(prior=0.5)
        assert s['log_bayes_factor'] == om.log_evidence_second() - om.log_evidence_null() and 0.0 <= s['probability'] <= 1.0
        assert om.log_weights(prior_second=0.5).shape == (4,) and 'known' in om.describe()


def test_twin_experiment_on_the_device():
    """the twin experiment of the CPU tests with each member's chain run on the device: our release known, a second
    source of amount 0.5 at origin_ref.TWIN_ORIGIN -- and the same traps with our release alone"""
    from parasitoids_amd import _lib as L
    from parasitoids_amd import predictive as PR
    from parasitoids_amd.hip_lib import HipSolve
    n, nd = OR.TWIN_N, OR.TWIN_DAYS
    days, hyp, W = list(range(1, nd + 1)), KR.twin_hypotheses(), sum(OR.TWIN_WEIGHTS)
    lib = L.load()
    kind, idx = L.i32([L.REC_CHAIN] * nd), L.i32(list(range(nd)))        # model day d is chain record d - 1
    one, delta = L.f64([1.0] * nd), L.i32([1] * nd)
    slots = (nd, L.p_i32(kind), L.p_i32(idx), L.p_f64(one), L.p_f64(one), L.p_i32(delta), 1e-8)
    cases = {name: KR.twin_findings(second) for name, second in (('both', True), ('ours', False))}
    handles = {}
    try:
        for name, findings in cases.items():
            h = L._VP()
            L.check(lib.ps_origin_create(
                0, n, len(findings), L.p_i32(L.i32([p['row'] for p in findings])), L.p_i32(L.i32([p['col'] for p in findings])),
                L.p_i32(L.i32([days.index(p['day']) for p in findings])), L.p_i32(L.i32([KIND[p['kind']] for p in findings])),
                L.p_f64(L.f64([p['rate'] for p in findings])), L.p_f64(L.f64([p['n'] or 0 for p in findings])), nd, len(hyp),
                L.p_f64(L.f64([a for a, _g in hyp])), L.p_i32(L.i32([0] * len(hyp))), 1, None, C.byref(h)))
            handles[name] = h
            L.check(lib.ps_origin_set_known(h, 1, L.p_i32(L.i32([0])), L.p_i32(L.i32([0])), L.p_f64(L.f64([1.0])),
                                            L.p_i32(L.i32([0])), 1))
        for m, w in enumerate(OR.TWIN_WEIGHTS):
            state, kernels = OR.twin_stack(m)
            s = HipSolve(state, [OR.TWIN_K, OR.TWIN_K], mode='exact')
            try:
                s.set_kernels(kernels)
                s.run_chain()
                stats = s.chain_stats(0, nd)
                for name, h in handles.items():
                    L.check(lib.ps_origin_background(h, s._h, 0, *slots))
                    L.check(lib.ps_origin_add(h, s._h, 0, *slots, w))
                if m == 3:                                               # one member against the restatement
                    fields = {0: {d: s.chain_solution(d - 1, stats[d - 1]).toarray() for d in days}}
                    bg = np.empty(len(cases['both']))
                    L.check(lib.ps_origin_fetch_background(handles['both'], L.p_f64(bg), None))
                    assert np.array_equal(bg, KR.background(cases['both'], KR.TWIN_KNOWN, fields))
            finally:
                s.close()
        out = {}
        for name, h in handles.items():
            A, S, null = np.empty((len(hyp), n, n)), np.empty((len(hyp), n, n)), np.empty(8)
            for k in range(len(hyp)):
                L.check(lib.ps_origin_fetch(h, 0, k, L.p_f64(A[k])))
                L.check(lib.ps_origin_fetch(h, 1, k, L.p_f64(S[k])))
            L.check(lib.ps_origin_null_rows(h, 8, L.p_f64(null)))
            E = PR.origin_log_evidence(A, S, W)
            out[name] = (PR.origin_posterior(E), PR.origin_log_evidence_second(E) - PR.origin_log_mean_exp(null, OR.TWIN_WEIGHTS))
    finally:
        for h in handles.values():
            lib.ps_origin_destroy(h)
    P, lbf = out['both']
    k, row, col = (int(v) for v in np.unravel_index(int(np.argmax(P)), P.shape))
    assert (row, col) == OR.TWIN_ORIGIN and hyp[k] == (0.5, 0)
    Pm = P.sum(axis=0)
    assert PR.origin_region(Pm, 0.5)[OR.TWIN_ORIGIN] == 1 and PR.origin_region(Pm, 0.95)[OR.TWIN_ORIGIN] == 1
    assert lbf > 50 and abs(out['ours'][1]) < 1
    print('twin on the device: log Bayes factor %.2f with a second source, %.3f without' % (lbf, out['ours'][1]))


def test_posterior_predictive_with_known_against_the_class_fed_by_hand(tmp_path):
    from parasitoids_amd import mcmc
    from parasitoids_amd import predictive as PR
    from test_reweight_gpu import _chain
    R = 32
    res_m = 10000.0 / R
    ta, names = _chain([3, 2])
    tb, _ = _chain([1, 2, 2])
    traces = [ta, tb[1:]]
    chains = [(t, names) for t in traces]
    plan = dict(sites=[(0.0, 0.0, 0.6), (7 * res_m, -3 * res_m, 0.5, 2)], days=[0, 3, 5])
    find = [(2 * res_m, 3 * res_m, 3, 'count', 0.02, 2), (-4 * res_m, res_m, 4, 'found', 0.05),
            (10 * res_m, -8 * res_m, 1, 'none', 0.01)]
    arg = dict(findings=find, amounts=[0.1, 1.0], lags=[0, 1], levels=[0.5, 0.9], known='sites')
    explicit = dict(arg, known=[tuple(s) for s in plan['sites']])
    pm = _pop_model(R, mode='exact')
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    common = dict(thresholds=[1.0], sites=plan, cell_area=res_m ** 2)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = PR.posterior_predictive(pm, chains, origin=arg, **common)
        bare = PR.posterior_predictive(pm, chains, origin=dict(findings=find, amounts=[0.1, 1.0], lags=[0, 1], levels=[0.5, 0.9]),
                                       **common)
        with pytest.raises(ValueError, match="known='sites'"):
            PR.posterior_predictive(pm, chains, origin=arg, thresholds=[1.0])
    om = res.origin
    assert om.known_lags == [0, 2] and om.lags == [0, 1] and om.model_lags == [0, 1, 2]
    assert om.plan['known_given'] == [[0.0, 0.0, 0.6, 0], [7 * res_m, -3 * res_m, 0.5, 2]]
    assert (om.total_weight, om.members) == (9.0, 4) and bare.origin.known is None
    # the class fed by hand: every run once more, per chain a handle of its own, merged in chain order
    hand = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for ci in range(2):
            hand.append(PR.OriginMaps.with_lagged_models(pm, explicit))
            for c, first, weight in res.runs:
                if c == ci:
                    args = mcmc.model_args(traces[ci][first, cols])
                    pm.evaluate(*args, want_stats=False)
                    # as the driver evaluates them: the plan's day 5 needs 4 days of the lag-2 model, the findings 3 of it
                    # and 4 of the lag-1 model
                    hand[ci].lagged[1].evaluate(*args, ndays=4, want_stats=False)
                    hand[ci].lagged[2].evaluate(*args, ndays=4, want_stats=False)
                    hand[ci].add(weight)
        hand[0].merge(hand[1])
        want = hand[0]
        for h in range(4):
            for what in ('A', 'S'):
                assert np.array_equal(om.plane(what, h), want.plane(what, h)), (h, what)
        assert np.array_equal(om.member_rows()[0], want.member_rows()[0])
        assert np.array_equal(om.null_rows(), want.null_rows()) and om.null_rows().shape == (4,)
        assert np.array_equal(om.background()[0], want.background()[0]) and (om.background()[0] > 0).any()
        assert om.second_source() == want.second_source()
        assert not np.array_equal(om.plane('A', 1), bare.origin.plane('A', 1))       # the background moves the evidence
        # the files: the new keys only where known was given
        for name, r in (('a', res), ('b', bare)):
            os.makedirs(str(tmp_path / name))
            r.save(str(tmp_path / name / 'pp'))
        fa, fb = np.load(str(tmp_path / 'a' / 'pp_origin.npz')), np.load(str(tmp_path / 'b' / 'pp_origin.npz'))
        today = sorted(['log_evidence_h%d' % h for h in range(4)] + ['posterior', 'region_l50', 'region_l90', 'member_rows',
                                                                    'member_weights', 'hypotheses'])
        assert sorted(fb.files) == today and sorted(fa.files) == sorted(today + ['known', 'null_rows', 'background_last'])
        assert np.array_equal(fa['null_rows'], om.null_rows()) and np.array_equal(fa['background_last'], om.background()[0])
        assert fa['known'].tolist() == [[0.0, 0.0, 0.6, 0.0], [7 * res_m, -3 * res_m, 0.5, 2.0]]
        ba = json.load(open(str(tmp_path / 'a' / 'pp.json')))['predictive']['origin']
        bb = json.load(open(str(tmp_path / 'b' / 'pp.json')))['predictive']['origin']
        base = ['findings', 'hypotheses', 'levels', 'prior', 'members', 'total_weight', 'masses', 'mode', 'areas',
                'diagnostics', 'warnings']
        assert sorted(bb) == sorted(base) and sorted(ba) == sorted(base + ['known', 'second_source'])
        assert ba['second_source']['log_bayes_factor'] == om.second_source()['log_bayes_factor']
    for r in (res, bare):
        for acc in (r.summary, r.sites, r.origin):
            if acc is not None:
                acc.close()
    for h in hand:
        h.close()

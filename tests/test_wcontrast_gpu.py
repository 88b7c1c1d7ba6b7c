"""GPU tests of the reweighted paired contrast (ps_wcontrast_*, predictive.ReweightedContrast).

On crafted fields, through the C ABI: the six crafted_plans.pair_members(N), injected into the solver
(crafted_fields.Injector), applied by two identity projections -- and once by two one-site release plans -- and read
back bit for bit before they are added, with the run lengths crafted_plans.WEIGHTS and, in four scenarios at once, the
log-weights of wcontrast_ref.LAM (flat, swing, dead, under).  Every cell of every plane of every slot is compared with
the numpy restatement wcontrast_ref bit for bit: the mean, the fetched variance against the restatement's M2 / W (the
same division), every probability against min(S / W, 1), and W, ref, members and skipped.  A NaN (M2 = inf under
r = 0, at the ties of 1e300 whose squares are beyond double) is compared as a NaN: the sign of a NaN that 0 * inf
produces is the processor's.  The restatement's own distance from the exact moments is wcontrast_ref.MEAN_ERR /
M2_ERR (test_wcontrast_cpu.py); nothing further is tolerated here.  Then every kernel instance NJ = 1..4 x K = 0..4,
the tie to a ps_contrast fed alongside, antisymmetry, the shift of the log-weights, merges and reset, and the
refusals.

On model fields (Kalbar wind, R = 64, 6 days, the members, weights and plans of test_contrast_gpu.py) through the
classes: the maps against the two-pass definitions, posterior_predictive with maps=('contrast',) against a hand-fed
ReweightedContrast bit for bit, the saved file, the json block, and that without the option every file is what it
was.
"""
import ctypes as C
import json
import math
import os
import warnings

import numpy as np
import pytest

import crafted_fields as CF
import crafted_plans as CP
import wcontrast_ref as WR

pytestmark = pytest.mark.gpu

U32P = C.POINTER(C.c_uint32)
NAMES = list(WR.NAMES)


def _f64(L, N, call, *args):
    out = np.empty((N, N))
    L.check(call(*args, L.p_f64(out)))
    return out.ravel()


def _same(a, b):
    """bit for bit, a NaN for a NaN; a zero's sign is left to the comparisons that care"""
    return np.array_equal(a, b, equal_nan=True)


class _Sources:
    """two sources of S outputs that copy the solver's state slot by slot: identity projections, or release plans of
    the one site (0, 0, 1.0) -- as test_crafted_plans_gpu.py feeds them"""

    def __init__(self, inj, N, S, kind='project'):
        L, lib = inj.L, inj.lib
        self.inj, self.N, self.S, self.kind, self.hs = inj, N, S, kind, []
        self._destroy = lib.ps_project_destroy if kind == 'project' else lib.ps_sites_destroy
        try:
            for _ in range(2):
                h = L._VP()
                if kind == 'project':
                    L.check(lib.ps_project_create(inj.dev, N, S, S, L.p_f64(L.f64(np.eye(S))), C.byref(h)))
                else:
                    L.check(lib.ps_sites_create(inj.dev, N, S, 1, L.p_i32(L.i32([1])), L.p_i32(L.i32([0])),
                                                L.p_i32(L.i32([0])), L.p_f64(L.f64([1.0])), C.byref(h)))
                self.hs.append(h)
        except Exception:
            self.close()
            raise

    def feed(self, member):
        """the member's two fields into the sources; every output read back bit for bit"""
        inj, L, lib = self.inj, self.inj.L, self.inj.lib
        _name, F, profile, _w, negval = member
        args = inj.slots(CP.slot_profile(profile, self.S), negval)
        for h, f in zip(self.hs, F):
            inj.inject(f)
            if self.kind == 'project':
                L.check(lib.ps_project_apply(h, inj.s._h, *args))
                fetch = lib.ps_project_fetch
            else:
                L.check(lib.ps_sites_apply(h, inj.s._h, 0, *args))
                fetch = lib.ps_sites_fetch
            want = CF.history(f, profile, negval).reshape(CP.NENTRY, -1)
            for s in range(self.S):
                got = _f64(L, self.N, fetch, h, s)
                assert np.array_equal(got, want[CP.entry_of(s)]) and not np.signbit(got).any(), (member[0], s)

    def close(self):
        for h in self.hs:
            self._destroy(h)
        self.hs = []


class _WC:
    """one ps_wcontrast handle with the host's side of it: the scenarios' references, moved as the class moves them"""

    def __init__(self, inj, N, S, names, K, kind='project', shift=0.0):
        from parasitoids_amd import predictive as PR
        L, lib = inj.L, inj.lib
        self.PR, self.L, self.lib, self.N, self.S, self.names, self.K, self.shift = PR, L, lib, N, S, list(names), K, shift
        self.ref = [-math.inf] * len(names)
        self._add = lib.ps_wcontrast_add_project if kind == 'project' else lib.ps_wcontrast_add_sites
        self.h = L._VP()
        thr = L.f64(CP.THR4[:K] if K else [0.0])
        L.check(lib.ps_wcontrast_create(inj.dev, N, len(names), S, K, L.p_f64(thr), C.byref(self.h)))

    def add(self, i, A, B):
        lam = [WR.LAM[n][i] + self.shift for n in self.names]
        r, om, ref = self.PR.reweight_scale(self.names, self.ref, lam, CP.WEIGHTS[i])
        L = self.L
        L.check(self._add(self.h, A, B, len(self.names), L.p_f64(L.f64(r)), L.p_f64(L.f64(om))))
        self.ref = [b if o > 0.0 else a for a, b, o in zip(self.ref, ref, om)]

    def merge(self, other):
        L = self.L
        ra, rb, ref = self.PR.reweight_merge_scale(self.ref, other.ref)
        L.check(self.lib.ps_wcontrast_merge(self.h, other.h, L.p_f64(L.f64(ra)), L.p_f64(L.f64(rb))))
        self.ref = ref

    def info(self):
        n = len(self.names)
        w, m, s = np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        self.L.check(self.lib.ps_wcontrast_info(self.h, self.L.p_f64(w), self.L.p_i64(m), self.L.p_i64(s)))
        return w.tolist(), m.tolist(), s.tolist()

    def log_total_weight(self, j):
        return self.ref[j] + math.log(self.info()[0][j])

    def fetch(self, j, s, what):
        return _f64(self.L, self.N, self.lib.ps_wcontrast_fetch, self.h, j, s, what)

    def planes(self, j, s):
        return [self.fetch(j, s, what) for what in range(4 + 2 * self.K)]

    def close(self):
        if self.h:
            self.lib.ps_wcontrast_destroy(self.h)
            self.h = self.L._VP()


class _Con:
    """a ps_contrast handle fed alongside"""

    def __init__(self, inj, N, S, K):
        L, lib = inj.L, inj.lib
        self.L, self.lib, self.N, self.K, self.h = L, lib, N, K, L._VP()
        L.check(lib.ps_contrast_create(inj.dev, N, S, K, L.p_f64(L.f64(CP.THR4[:K])), C.byref(self.h)))

    def add(self, i, A, B):
        self.L.check(self.lib.ps_contrast_add_project(self.h, A, B, CP.WEIGHTS[i]))

    def merge(self, other):
        self.L.check(self.lib.ps_contrast_merge(self.h, other.h))

    def fetch(self, s, what):
        return _f64(self.L, self.N, self.lib.ps_contrast_fetch, self.h, s, what)

    def counts(self, s, q):
        out = np.empty((self.N, self.N), dtype=np.uint32)
        self.L.check(self.lib.ps_contrast_fetch_counts(self.h, s, q, out.ctypes.data_as(U32P)))
        return out.ravel().astype(np.float64)

    def close(self):
        if self.h:
            self.lib.ps_contrast_destroy(self.h)
            self.h = self.L._VP()


def _against_reference(wc, N, names=None, tag=''):
    """every plane of every slot and scenario of wc, and its host-side figures, against wcontrast_ref -> the planes of
    the first scenario, [S][4 + 2K][n]"""
    ref, sched = WR.reference(N)
    names = names or wc.names
    W, members, skipped = wc.info()
    for j, n in enumerate(names):
        st = ref[0][n]
        assert (W[j], members[j], skipped[j]) == (st['W'], st['members'], st['skipped']), (tag, n)
        assert wc.ref[j] == sched[n][1] + wc.shift, (tag, n)
    first = []
    for s in range(wc.S):
        ent = ref[CP.entry_of(s)]
        for j, n in enumerate(names):
            got = wc.planes(j, s)
            for what, g in enumerate(got):
                want = WR.fetch(ent[n], what)
                bad = np.flatnonzero(~((g == want) | (np.isnan(g) & np.isnan(want))))
                assert bad.size == 0, (tag, n, s, what, bad[:5], g[bad[:5]], want[bad[:5]])
            if j == 0:
                first.append(got)
    return first


# ---- 1. bits ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N,S', ((65, 5), (129, 5), (65, 32)))
def test_every_plane_is_the_restatement_bit_for_bit(N, S):
    inj = CF.Injector(N)
    K = len(CP.THR4)
    with_sites = (N, S) == (65, 5)
    made = []
    try:
        src = _Sources(inj, N, S)
        made.append(src)
        wc = _WC(inj, N, S, NAMES, K)
        made.append(wc)
        sites = by_sites = None
        if with_sites:
            sites = _Sources(inj, N, S, 'sites')
            made.append(sites)
            by_sites = _WC(inj, N, S, NAMES, K, 'sites')
            made.append(by_sites)
        for i, m in enumerate(CP.pair_members(N)):
            src.feed(m)
            wc.add(i, *src.hs)
            if sites:
                sites.feed(m)
                by_sites.add(i, *sites.hs)
        flat = _against_reference(wc, N)
        if by_sites:
            _against_reference(by_sites, N, tag='sites')
        # not vacuous, from the device's own planes of `flat`: every sum plane holds something, the mean takes both
        # signs, the tail cell holds something, the last slot is not the first
        D = np.array(flat)
        assert (np.nansum(D[:, 2:], axis=(0, 2)) > 0).all() and (D[:, 0] > 0).any() and (D[:, 0] < 0).any()
        assert D[:, :, -1].any() and not _same(D[S - 1], D[0])
        # and the other scenarios are other maps
        assert not _same(wc.fetch(1, 0, 0), D[0, 0]) and not _same(wc.fetch(2, 0, 2), D[0, 2])
    finally:
        for x in reversed(made):
            x.close()
        inj.close()


# ---- 2 .. 6: one feeding pass at N = 65, S = 5 ------------------------------------------------------------------------

INSTANCES = [(nj, k) for nj in range(1, 5) for k in range(5)]


@pytest.fixture(scope='module')
def world():
    """the six members fed once into: `full` (four scenarios, four thresholds) and a ps_contrast alongside, `mirror`
    fed (b, a), `shifted` with 256 added to every log-weight, the halves 0..2 and 3..5 twice over (and of the
    ps_contrast), and one handle per kernel instance"""
    import types
    N, S, K = 65, 5, len(CP.THR4)
    inj = CF.Injector(N)
    w = types.SimpleNamespace(N=N, S=S, K=K, inj=inj, made=[])

    def keep(x):
        w.made.append(x)
        return x
    try:
        src = keep(_Sources(inj, N, S))
        w.full, w.mirror = keep(_WC(inj, N, S, NAMES, K)), keep(_WC(inj, N, S, NAMES, K))
        w.shifted = keep(_WC(inj, N, S, NAMES, K, shift=256.0))
        w.con = keep(_Con(inj, N, S, K))
        w.a, w.b, w.a2, w.b2 = (keep(_WC(inj, N, S, NAMES, K)) for _ in range(4))
        w.ca, w.cb, w.ca2, w.cb2 = (keep(_Con(inj, N, S, K)) for _ in range(4))
        w.inst = {(nj, k): keep(_WC(inj, N, S, NAMES[4 - nj:], k)) for nj, k in INSTANCES}
        w.empty = keep(_WC(inj, N, S, NAMES, K))
        A, B = src.hs
        for i, m in enumerate(CP.pair_members(N)):
            src.feed(m)
            first = i < CP.HALF
            for h in [w.full, w.shifted, w.con, w.a if first else w.b, w.a2 if first else w.b2,
                      w.ca if first else w.cb, w.ca2 if first else w.cb2] + list(w.inst.values()):
                h.add(i, A, B)
            w.mirror.add(i, B, A)
        yield w
    finally:
        for x in reversed(w.made):
            x.close()
        inj.close()


@pytest.mark.parametrize('nj,k', INSTANCES)
def test_every_kernel_instance(world, nj, k):
    wc = world.inst[(nj, k)]
    assert len(wc.names) == nj and wc.K == k
    _against_reference(wc, world.N, tag=(nj, k))


def test_flat_holds_the_bits_of_a_contrast_fed_alongside(world):
    full, con = world.full, world.con
    W = float(sum(CP.WEIGHTS))
    assert full.info()[0][0] == W
    for s in range(world.S):
        assert np.array_equal(full.fetch(0, s, 0), con.fetch(s, 0)), s
        assert np.array_equal(full.fetch(0, s, 1), con.fetch(s, 1)), s
        for q in range(2 + 2 * world.K):
            got = full.fetch(0, s, 2 + q)
            assert np.array_equal(got, con.counts(s, q) / W), (s, q)
            assert np.array_equal(got, con.fetch(s, 2 + q)), (s, q)


def test_antisymmetry(world):
    full, mirror = world.full, world.mirror
    assert mirror.info() == full.info() and mirror.ref == full.ref
    for s in range(world.S):
        for j, n in enumerate(NAMES):
            got, want = mirror.planes(j, s), full.planes(j, s)
            assert _same(got[0], -want[0]), (n, s)
            assert _same(got[1], want[1]), (n, s)
            for q in range(2 + 2 * world.K):
                assert _same(got[2 + (q ^ 1)], want[2 + q]), (n, s, q)
    assert (full.fetch(1, 0, 0) != 0).any()


def test_a_shift_of_the_log_weights_moves_the_total_alone(world):
    """the bounds of test_reweight_gpu.py for the same property: log W moves by the shift within 1e-12, the maps stay
    within atol = 1e-12 max|map|"""
    full, shifted = world.full, world.shifted
    j = NAMES.index('swing')
    assert shifted.ref[j] == full.ref[j] + 256.0
    assert abs(shifted.log_total_weight(j) - full.log_total_weight(j) - 256.0) <= 1e-12
    assert shifted.info()[1:] == full.info()[1:]
    for s in range(world.S):
        for what, (got, want) in enumerate(zip(shifted.planes(j, s), full.planes(j, s))):
            fin = np.isfinite(want)             # the variance at the ties of 1e300 is inf: there the same inf
            assert fin.sum() > fin.size // 2 and _same(got[~fin], want[~fin]), (s, what)
            np.testing.assert_allclose(got[fin], want[fin], rtol=0.0, atol=1e-12 * np.abs(want[fin]).max(),
                                       err_msg=str((s, what)))


def test_merges_in_both_orders_empty_sides_and_reset(world):
    N, S, K = world.N, world.S, world.K
    full = world.full
    ref, _sched = WR.reference(N)
    world.a.merge(world.b)              # first += last
    world.b2.merge(world.a2)            # last += first
    world.ca.merge(world.cb)
    world.cb2.merge(world.ca2)
    W = float(sum(CP.WEIGHTS))
    for wc, con in ((world.a, world.ca), (world.b2, world.cb2)):
        Wm, members, skipped = wc.info()
        assert Wm[0] == W and (members, skipped) == full.info()[1:]
        for j in range(4):
            assert abs(wc.log_total_weight(j) - full.log_total_weight(j)) <= 1e-12, j
        for s in range(S):
            # flat: the merge of the integer contrast, bit for bit
            assert np.array_equal(wc.fetch(0, s, 0), con.fetch(s, 0)) and np.array_equal(wc.fetch(0, s, 1), con.fetch(s, 1)), s
            for q in range(2 + 2 * K):
                assert np.array_equal(wc.fetch(0, s, 2 + q), con.counts(s, q) / W), (s, q)
            # the others: the project's rule against the handle fed in order, the scale taken per cell -- the
            # crafted cells span 600 orders of magnitude, and one scale for all of them would bound nothing
            scale = np.abs(ref[CP.entry_of(s)]['D']).max(0)
            tame = scale < 1e100                # beyond it d^2 leaves double and M2 is inf or NaN on either path
            for j in range(1, 4):
                got, want = wc.planes(j, s), full.planes(j, s)
                np.testing.assert_array_less(np.abs(got[0] - want[0]), 1e-12 * np.abs(want[0]) + 1e-15 * scale + 5e-324)
                assert np.isfinite(got[1][tame]).all() and np.isfinite(want[1][tame]).all()
                np.testing.assert_array_less(np.abs(got[1] - want[1])[tame],
                                             (1e-12 * np.abs(want[1]) + 1e-15 * scale * scale)[tame] + 5e-324)
                for q in range(2 + 2 * K):
                    np.testing.assert_allclose(got[2 + q], want[2 + q], rtol=1e-12, atol=1e-15)
    # an empty handle: merged into, a copy bit for bit; merged from, nothing moves
    L, lib, empty = world.inj.L, world.inj.lib, world.empty
    out = np.empty((N, N))
    assert lib.ps_wcontrast_fetch(empty.h, 0, 0, 0, L.p_f64(out)) == L.PS_ERR_STATE
    before = [full.planes(j, s) for j in range(4) for s in range(S)]
    full.merge(empty)
    assert all(_same(g, x) for got, want in zip([full.planes(j, s) for j in range(4) for s in range(S)], before)
               for g, x in zip(got, want))
    info = full.info()
    empty.merge(full)
    assert empty.info() == info and empty.ref == full.ref
    assert all(_same(g, x) for got, want in zip([empty.planes(j, s) for j in range(4) for s in range(S)], before)
               for g, x in zip(got, want))
    # reset: empty again, and it takes members as a fresh handle does
    L.check(lib.ps_wcontrast_reset(empty.h))
    empty.ref = [-math.inf] * 4
    assert empty.info() == ([0.0] * 4, [0] * 4, [0] * 4)
    assert lib.ps_wcontrast_fetch(empty.h, 0, 0, 0, L.p_f64(out)) == L.PS_ERR_STATE
    empty.merge(world.a)
    assert all(_same(g, x) for s in range(S) for g, x in zip(empty.planes(1, s), world.a.planes(1, s)))


# ---- 7. refusals -------------------------------------------------------------------------------------------------------

def test_refusals_at_the_c_abi_change_nothing_and_the_handle_stays_usable():
    N, S, K = 65, 5, 1
    inj, big = CF.Injector(N), CF.Injector(129)
    L, lib = inj.L, inj.lib
    h = L._VP()

    def create(nscen=2, nthr=1, thr=(1.0,), nslot=S, device=None):
        t = L.f64(list(thr) if len(thr) else [0.0])
        return lib.ps_wcontrast_create(inj.dev if device is None else device, N, nscen, nslot, nthr, L.p_f64(t), C.byref(h))
    for kw in (dict(nscen=0), dict(nscen=5), dict(nthr=5, thr=(1.0, 2.0, 3.0, 4.0, 5.0)), dict(nthr=2, thr=(2.0, 1.0)),
               dict(nthr=2, thr=(1.0, 1.0)), dict(thr=(0.0,)), dict(thr=(np.inf,)), dict(thr=(np.nan,)), dict(nslot=0),
               dict(nslot=33), dict(nthr=-1)):
        assert create(**kw) == L.PS_ERR_BAD_ARG and not h, kw
    assert create(device=99) == L.PS_ERR_NO_DEVICE and not h
    made = []
    try:
        src = _Sources(inj, N, S)
        made.append(src)
        four = _Sources(inj, N, 4)
        made.append(four)
        other = _Sources(big, 129, S)
        made.append(other)
        sites = _Sources(inj, N, S, 'sites')
        made.append(sites)
        wc = _WC(inj, N, S, ['flat', 'swing'], K)
        made.append(wc)
        A, B = src.hs
        mem = CP.pair_members(N)
        out = np.empty((N, N))
        r1, o1 = L.f64([1.0, 1.0]), L.f64([3.0, 3.0])

        def add(a, b, nscen=2, r=r1, om=o1, fn=lib.ps_wcontrast_add_project):
            return fn(wc.h, a, b, nscen, L.p_f64(r) if r is not None else None, L.p_f64(om) if om is not None else None)
        assert lib.ps_wcontrast_fetch(wc.h, 0, 0, 0, L.p_f64(out)) == L.PS_ERR_STATE      # nothing accumulated
        assert add(A, B) == L.PS_ERR_STATE                                                # nothing applied yet
        lib.ps_wcontrast_prof(wc.h, 1, None, None)
        src.feed(mem[2])
        four.feed(mem[2])
        other.feed(CP.pair_members(129)[2])
        sites.feed(mem[2])
        wc.add(2, A, B)
        before = [wc.planes(j, s) for j in range(2) for s in range(S)]
        info = wc.info()
        nan, inf = float('nan'), float('inf')
        refused = [
            (dict(a=A, b=A), b'same'), (dict(a=A, b=four.hs[1]), b'has 4 outputs'), (dict(a=four.hs[0], b=B), b'has 4 outputs'),
            (dict(a=A, b=other.hs[1]), b'domain 129'), (dict(a=other.hs[0], b=B), b'domain 129'),
            (dict(a=A, b=B, nscen=1), b'scenarios'), (dict(a=A, b=B, nscen=3), b'scenarios'),
            (dict(a=A, b=B, r=L.f64([1.0, -0.1])), b'rescale[1]'), (dict(a=A, b=B, r=L.f64([1.5, 1.0])), b'rescale[0]'),
            (dict(a=A, b=B, r=L.f64([nan, 1.0])), b'rescale[0]'), (dict(a=A, b=B, om=L.f64([3.0, -1.0])), b'omega[1]'),
            (dict(a=A, b=B, om=L.f64([inf, 1.0])), b'omega[0]'), (dict(a=A, b=B, om=L.f64([1.0, nan])), b'omega[1]'),
            (dict(a=A, b=None), b'bad arguments'), (dict(a=None, b=B), b'bad arguments'),
            (dict(a=A, b=B, r=None), b'bad arguments'), (dict(a=A, b=B, om=None), b'bad arguments'),
            (dict(a=sites.hs[0], b=sites.hs[0], fn=lib.ps_wcontrast_add_sites), b'same release plan')]
        for kw, msg in refused:
            assert add(**kw) == L.PS_ERR_BAD_ARG, kw
            assert msg in lib.ps_last_error(), (msg, lib.ps_last_error())
            assert wc.info() == info
        assert lib.ps_wcontrast_add_project(None, A, B, 2, L.p_f64(r1), L.p_f64(o1)) == L.PS_ERR_BAD_ARG
        for scen, slot, what in ((-1, 0, 0), (2, 0, 0), (0, -1, 0), (0, S, 0), (0, 0, -1), (0, 0, 4 + 2 * K)):
            assert lib.ps_wcontrast_fetch(wc.h, scen, slot, what, L.p_f64(out)) == L.PS_ERR_BAD_ARG
        assert lib.ps_wcontrast_merge(wc.h, wc.h, L.p_f64(r1), L.p_f64(r1)) == L.PS_ERR_BAD_ARG
        with_two = _WC(inj, N, S, ['flat', 'swing'], 2)
        made.append(with_two)
        assert lib.ps_wcontrast_merge(wc.h, with_two.h, L.p_f64(r1), L.p_f64(r1)) == L.PS_ERR_BAD_ARG     # other thresholds
        twin = _WC(inj, N, S, ['flat', 'swing'], K)
        made.append(twin)
        twin.add(2, A, B)
        for ra, rb in (([1.5, 1.0], [1.0, 1.0]), ([1.0, 1.0], [1.0, -0.5]), ([nan, 1.0], [1.0, 1.0])):
            assert lib.ps_wcontrast_merge(wc.h, twin.h, L.p_f64(L.f64(ra)), L.p_f64(L.f64(rb))) == L.PS_ERR_BAD_ARG
        # no bit moved, one launch was timed, and the handle takes the next member as if nothing had happened
        assert all(_same(g, x) for got, want in zip([wc.planes(j, s) for j in range(2) for s in range(S)], before)
                   for g, x in zip(got, want))
        ms, launches = C.c_double(), C.c_int64()
        L.check(lib.ps_wcontrast_prof(wc.h, -1, C.byref(ms), C.byref(launches)))
        assert launches.value == 1 and ms.value > 0.0 and wc.info() == info
        src.feed(mem[4])
        wc.add(4, A, B)
        for s in range(S):
            e = CP.entry_of(s)
            for j, n in enumerate(wc.names):
                st = WR.new(N * N, K)
                ref = -math.inf
                for i in (2, 4):
                    r, om, new = WR.scale(ref, WR.LAM[n][i], CP.WEIGHTS[i])
                    ref = new if om > 0.0 else ref
                    a, b = CP.values(mem[i], e)
                    WR.add(st, a, b, r, om, CP.THR4[:K])
                assert wc.ref[j] == ref and wc.info()[0][j] == st['W']
                for what, g in enumerate(wc.planes(j, s)):
                    assert _same(g, WR.fetch(st, what)), (n, s, what)
    finally:
        for x in reversed(made):
            x.close()
        inj.close()
        big.close()


# ---- 8. on model fields ------------------------------------------------------------------------------------------------

R, NM = 64, 129
THR = [1.0, 10.0]
OUT = [0, 1, 2, 3, 5]


def _plans():
    from test_sites_gpu import STAGGERED, _edge_plan, _metres
    plan_a = STAGGERED
    plan_b = [(dr, dc, 0.75 * a, lag) for dr, dc, a, lag in _edge_plan(R)]
    return _metres(plan_a, R), _metres(plan_b, R)


def _probes():
    res = 10000.0 / R
    trap = [(0.0, 0.0, 2, 'count', 2e-4, 14), (13 * res, 0.0, 3, 'found', 1e-3)]
    paddock = [(-6 * res, -9 * res, 4, 'none', 5e-3), (3 * res, 5 * res, 5, 'none', 1e-3)]
    return {'trap': dict(probes=trap), 'paddock': dict(probes=paddock)}


def _close(got, want, scale, what):
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15 * scale, err_msg=str(what))


def test_model_fields_against_the_two_pass_definitions():
    from parasitoids_amd import predictive as PR
    from test_sites_gpu import MEMBERS, WEIGHTS, _evaluate, _pop_model
    pa, pb = _plans()
    pm = _pop_model(R)
    late = PR.lagged_models(pm, [2])
    plan = PR.check_reweight(_probes(), pm.rad_dist, pm.rad_res, 6)
    names = plan['names']
    feed = PR._ReweightFeed(plan, 0)
    fa, fb, lams = [], [], []
    with PR.ReleaseSites(pm, pa, OUT, late) as A, PR.ReleaseSites(pm, pb, OUT) as B, \
            PR.ReweightedContrast(A, B, names, THR) as RC, PR.PlanContrast(A, B, THR) as X, \
            PR.ReweightedContrast(A, B, ['zero'], THR) as R0:
        assert RC.labels == OUT and RC.live == list(range(5)) and RC.nout == 5 and RC.thresholds == THR
        assert RC.nbytes == 2 * (4 + 2 * 2) * 8 * 5 * ((NM * NM + 63) // 64 * 64)
        assert RC.log_total_weight('trap') == -math.inf and RC.members('trap') == 0
        for mem, w in zip(MEMBERS, WEIGHTS):
            _evaluate(pm, mem)
            _evaluate(late[2], mem, ndays=4)
            A.apply()
            B.apply()
            lam = feed.log_weights(pm, 0, w)
            before, want = list(RC.ref), RC.scale(lam, w)
            RC.add(lam, w)
            assert RC.ref == [b if o > 0.0 else a for a, b, o in zip(before, want[2], want[1])]
            R0.add([0.0], w)
            X.add(w)
            fa.append([A.field(e) for e in range(5)])
            fb.append([B.field(e) for e in range(5)])
            lams.append(lam)
        fa, fb, lams = np.array(fa), np.array(fb), np.array(lams)
        assert np.isfinite(lams).all() and np.ptp(lams[:, 0]) > 1e-3 and np.ptp(lams[:, 1]) > 1e-3      # the probes tell the members apart
        for j, n in enumerate(names):
            om = WR.normalised(lams[:, j], WEIGHTS)
            assert om.max() < 0.999                                     # no scenario rests on one member
            assert RC.members(n) == len(MEMBERS) and RC.skipped(n) == 0
            want = math.log(float((np.array(WEIGHTS) * np.exp(lams[:, j] - lams[:, j].max())).sum())) + lams[:, j].max()
            assert abs(RC.log_total_weight(n) - want) <= 1e-12 * max(1.0, abs(want))
            for e in range(5):
                tp = WR.two_pass(fa[:, e], fb[:, e], om, THR)
                scale = np.abs(fa[:, e] - fb[:, e]).max()
                _close(RC.mean(n, e), tp['mean'], scale, (n, e, 'mean'))
                _close(RC.variance(n, e), tp['var'], scale * scale, (n, e, 'variance'))
                assert np.array_equal(RC.sd(n, e), np.sqrt(RC.variance(n, e)))
                _close(RC.prob_positive(n, e), tp['pos'], 1.0, (n, e, 'pos'))
                _close(RC.prob_negative(n, e), tp['neg'], 1.0, (n, e, 'neg'))
                for k in range(2):
                    _close(RC.gain(n, e, k), tp['gain'][k], 1.0, (n, e, 'gain', k))
                    _close(RC.loss(n, e, k), tp['loss'][k], 1.0, (n, e, 'loss', k))
        # the inputs can fail: both signs, gains and losses, and the scenarios disagree with the plain contrast
        assert (RC.mean('trap', 4) > 0).any() and (RC.mean('trap', 4) < 0).any()
        assert RC.gain('trap', 4, 1).max() > 0 and RC.loss('trap', 4, 1).max() > 0
        assert not np.array_equal(RC.mean('trap', 4), X.mean(4)) and not np.array_equal(RC.mean('trap', 4), RC.mean('paddock', 4))
        # log-weights of 0: the bits of the PlanContrast
        for e in range(5):
            assert np.array_equal(R0.mean('zero', e), X.mean(e)) and np.array_equal(R0.variance('zero', e), X.variance(e))
            assert np.array_equal(R0.prob_positive('zero', e), X.prob_positive(e))
            assert np.array_equal(R0.loss('zero', e, 1), X.loss(e, 1))
        with pytest.raises(ValueError, match='scenario'):
            RC.mean('nobody', 0)
        with pytest.raises(ValueError, match='output'):
            RC.mean('trap', 5)
        with pytest.raises(ValueError, match='threshold'):
            RC.gain('trap', 0, 2)
        with pytest.raises(ValueError, match='log-weights'):
            RC.add([0.0], 1)
        RC.profile(True)
        RC.add(lams[0].tolist(), 1)
        assert RC.profile()[1] == 1 and RC.members('trap') == len(MEMBERS) + 1
        RC.reset()
        assert RC.ref == [-math.inf] * 2 and RC.members('trap') == 0 and RC.total_weight('trap') == 0.0
    for m in (pm, late[2]):
        m.close()


def _npz_equal(a, b):
    fa, fb = np.load(a), np.load(b)
    return sorted(fa.files) == sorted(fb.files) and all(np.array_equal(fa[k], fb[k]) for k in fa.files)


def test_posterior_predictive_with_the_contrast_option(tmp_path):
    from parasitoids_amd import mcmc
    from parasitoids_amd import predictive as PR
    from test_sites_gpu import _chain, _csr, _pop_model
    pa, pb = _plans()
    trace, names = _chain([2, 1, 3, 1, 2])
    chains = [(trace[:5], names), (trace[5:], names)]

    def as_arg(sites):
        return [s[:3] + ((s[3],) if s[3] else ()) for s in sites]
    arg, cmp_arg = dict(sites=as_arg(pa), days=OUT), dict(sites=as_arg(pb))
    tilt = [np.array([0.0, 0.0, 1.5, -0.75, -0.75]), np.array([-0.75, 2.5, 0.25, 0.25])]
    rw = dict(_probes(), tilt=dict(log_weights=tilt))
    kw = dict(thresholds=THR, arrival=THR, arrival_levels=(0.5,), sites=arg, compare=cmp_arg)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        p1, p2, pm = (_pop_model(R, mode='exact') for _ in range(3))
        res = PR.posterior_predictive(p1, chains, reweight=dict(rw, options=dict(maps=('contrast',))), **kw)
        plain = PR.posterior_predictive(p2, chains, reweight=dict(rw), **kw)
    RC, X = res.reweight_contrast, res.contrast
    assert plain.reweight_contrast is None and plain.contrast is not None and 'maps' not in plain.reweight_info
    assert res.reweight_info['maps'] == ['contrast'] and RC.scenarios == ['trap', 'paddock', 'tilt']
    assert RC.labels == X.labels == OUT and RC.thresholds == X.thresholds == THR
    for n in RC.scenarios:
        assert (RC.members(n), RC.skipped(n)) == (res.reweight.members(n), res.reweight.skipped(n))
        assert RC.log_total_weight(n) == res.reweight.log_total_weight(n)
    assert RC.ref == res.reweight.ref and len(RC.member_log_weights) == X.members == 6
    # by hand: one handle per chain, merged in chain order
    plan = PR.check_reweight(dict(rw), pm.rad_dist, pm.rad_res, 6)
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    late = PR.lagged_models(pm, [2])
    lams = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with PR.ReleaseSites(pm, arg['sites'], OUT, late) as A, PR.ReleaseSites(pm, cmp_arg['sites'], OUT, late) as B, \
                PR.ReweightedContrast(A, B, plan['names'], THR) as M0, PR.ReweightedContrast(A, B, plan['names'], THR) as M1:
            feeds = [PR._ReweightFeed(plan, 0), PR._ReweightFeed(plan, 1)]
            for ci, first, weight in res.runs:
                args = mcmc.model_args(chains[ci][0][first, cols])
                pm.evaluate(*args, want_stats=False)
                late[2].evaluate(*args, ndays=OUT[-1] - 2 + 1, want_stats=False)
                lam = feeds[ci].log_weights(pm, first, weight)
                A.apply()
                B.apply()
                (M0, M1)[ci].add(lam, weight)
                lams.append([float(v) for v in lam])
            M0.merge(M1)
            assert RC.member_log_weights == lams and M0.ref == RC.ref
            for n in RC.scenarios:
                assert M0.total_weight(n) == RC.total_weight(n)
                for e in range(5):
                    for got, want in ((RC.mean(n, e), M0.mean(n, e)), (RC.variance(n, e), M0.variance(n, e)),
                                      (RC.prob_positive(n, e), M0.prob_positive(n, e)),
                                      (RC.prob_negative(n, e), M0.prob_negative(n, e)),
                                      (RC.gain(n, e, 1), M0.gain(n, e, 1)), (RC.loss(n, e, 0), M0.loss(n, e, 0))):
                        assert np.array_equal(got, want), (n, e)
    assert not np.array_equal(RC.mean('trap', 4), X.mean(4)) and not np.array_equal(RC.mean('tilt', 4), RC.mean('trap', 4))
    # the files: one more, and every other file and json key is what it was
    res.save(str(tmp_path / 'm' / 'pp'))
    plain.save(str(tmp_path / 'p' / 'pp'))
    old = sorted(os.listdir(str(tmp_path / 'p')))
    assert sorted(os.listdir(str(tmp_path / 'm'))) == sorted(old + ['pp_reweight_contrast.npz'])
    for name in old:
        if name.endswith('.npz'):
            assert _npz_equal(str(tmp_path / 'p' / name), str(tmp_path / 'm' / name)), name
    jp = json.load(open(str(tmp_path / 'p' / 'pp.json')))
    jm = json.load(open(str(tmp_path / 'm' / 'pp.json')))
    assert 'contrast' not in jp['predictive']['reweight'] and 'maps' not in jp['predictive']['reweight']
    meta = jm['predictive']['reweight']
    assert meta.pop('maps') == ['contrast']
    block = meta.pop('contrast')
    assert jm == jp                                        # but for the new keys the json is what it was
    assert sorted(block) == sorted(RC.scenarios)
    for j, n in enumerate(RC.scenarios):
        rec = block[n]
        assert rec['thresholds'] == THR and rec['log_total_weight'] == RC.log_total_weight(n)
        assert rec['members'] == RC.members(n) and rec['skipped'] == RC.skipped(n) and rec['levels'] == [0.5]
        for k in range(2):
            ca, cb, w = X.coverage(k)
            want = PR.reweighted_coverage_difference(ca, cb, w, [m[j] for m in lams], X.cell_area, (0.5,))
            for label, row in zip(OUT, want):
                row['label'] = label
            assert rec['coverage_difference'][k] == want
    assert block['trap']['coverage_difference'] != block['tilt']['coverage_difference']
    with np.load(str(tmp_path / 'm' / 'pp_reweight_contrast.npz')) as fz:
        assert [str(x) for x in fz['scenarios']] == RC.scenarios and [int(x) for x in fz['labels']] == OUT
        want = {'days', 'scenarios', 'labels'}
        for j, n in enumerate(RC.scenarios):
            for e, lab in enumerate(OUT):
                for suffix, m in (('', RC.mean(n, e)), ('_sd', RC.sd(n, e)), ('_ppos', RC.prob_positive(n, e)),
                                  ('_pneg', RC.prob_negative(n, e)), ('_pgain0', RC.gain(n, e, 0)),
                                  ('_ploss0', RC.loss(n, e, 0)), ('_pgain1', RC.gain(n, e, 1)), ('_ploss1', RC.loss(n, e, 1))):
                    key = 's%d_%d%s' % (j, lab, suffix)
                    assert np.array_equal(_csr(fz, key, NM), np.where(np.abs(m) >= 1e-8, m, 0.0)), key
                    want |= {'%s_%s' % (key, t) for t in ('data', 'ind', 'indptr')}
        assert set(fz.files) == want
        assert (_csr(fz, 's0_5', NM) < 0).any() and (_csr(fz, 's0_5', NM) > 0).any()      # the signed mean keeps both signs
    for r in (res, plain):
        for acc in (r.summary, r.arrival, r.sites, r.contrast, r.reweight, r.reweight_contrast):
            if acc is not None:
                acc.close()
    for p in (p1, p2, pm, late[2]):
        p.close()

"""ps_rank and ps_contrast on the crafted plans of crafted_plans.py, through the C ABI, and the two sources on the way
to them.  Plan j of a member is one crafted field injected into the solver (HipSolve.set_state, read back bit for bit)
and applied by an identity projection of nin = nout = S -- or, once, by a release plan of the one site (0, 0, 1.0) --
under the member's slot profile; every Y_e is fetched and required to be history(field, profile) bit for bit before the
member is added, so the references are fed the device's own fields.  Every cell of every plane of every slot is
compared; the same members go into two more pairs of handles that are merged in both orders; and after the comparisons
the cases the plans are there for are counted once more on the device's own outputs.

ps_rank.  k_rank_add<P> runs for every P = 2 .. 8, and for P >= 4 with one slot more than a launch's descriptors hold
(rank_chunk: 28, 24, 20, 18, 16 slots), so the second launch, whose descriptors start at c0 > 0, writes one slot; the
case of 8 plans and 32 slots is two full launches, the one without thresholds returns before the rows.  The regret
means are the bits of the header's statement and M2 those of fma(w * d, v - mean, M2), as in ps_summary: sum_update
(ps_common.h) is the same inline function in all three kernels.  The merged handles are the bits of
crafted_fields.merge_fused.  W = 16 in every handle, so the fetched variance M2 / W is M2 with another exponent
(above the subnormals) and equal variances are equal M2.

ps_contrast.  PS_CON_CHUNK is 32, the sources' cap on their outputs, so a contrast add never splits: S = 32 is one full
launch, and no split is forced.  A handle fed (b, a) has the negated mean, the sign planes and the gain and loss planes
swapped, and the same M2; a handle fed the same members through two one-site release plans and
ps_contrast_add_sites has every plane of the projection-fed one.

Against the exact rational moments of the regrets and differences the device lies within, largest over all cases
here and over the plain and the merged handles (units and their floor: crafted_plans.py; M2 recovered as 16 x the
fetched variance; where M2 is +inf -- ties at 1e300 -- nothing is measured), asserted at 4 x the restatement's own
distance (crafted_plans.MEAN_ERR = 2.0, M2_ERR = 2.6256), measured on an MI355X on 2026-10-21 on top of commit f10551b:
    ps_rank      mean  2.0000 x 2^-53 max_m |v_m|  (one ulp of a subnormal mean; 1.5000 at P = 2)
                 M2    2.5526 x 2^-53 sum_m w_m v_m^2  (P = 5 and 8; 2.1778 at the other P)
    ps_contrast  mean  0.5624,  M2  2.0993  (N = 129 and N = 65)
Every plane is asserted bit for bit, the fused M2 included, so these are the restatement's own figures for the cases run
here.
"""
import ctypes as C
import math

import numpy as np
import pytest

import crafted_fields as CF
import crafted_plans as CP

pytestmark = pytest.mark.gpu

U32P = C.POINTER(C.c_uint32)
W = float(sum(CP.WEIGHTS))
# nplan, nslot, N, nthr
RANK_CASES = ((2, 5, 129, 3),
              (3, 32, 65, 3),        # the full chunk of 32, no split
              (4, 29, 65, 2), (5, 25, 65, 2), (6, 21, 65, 2), (7, 19, 65, 2), (8, 17, 65, 4),      # chunk + 1
              (8, 32, 65, 1),        # two full chunks
              (8, 5, 129, 0))        # no thresholds: no rows, the early return
ONE_MORE = {4, 5, 6, 7, 8}


def _f64(L, N, call, *args):
    out = np.empty((N, N))
    L.check(call(*args, L.p_f64(out)))
    return out.ravel()


def _u32(L, N, call, *args):
    out = np.empty((N, N), dtype=np.uint32)
    L.check(call(*args, out.ctypes.data_as(U32P)))
    return out.ravel().astype(np.int64)


class _Sources:
    """P sources of S outputs that copy the solver's state slot by slot: identity projections, or release plans of
    the one site (0, 0, 1.0)"""

    def __init__(self, inj, N, P, S, kind='project'):
        L, lib = inj.L, inj.lib
        self.inj, self.N, self.S, self.kind, self.hs = inj, N, S, kind, []
        self._destroy = lib.ps_project_destroy if kind == 'project' else lib.ps_sites_destroy
        try:
            for _ in range(P):
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
        self.array = (L._VP * P)(*self.hs)

    def feed(self, member):
        """the member's fields into the sources; every output read back bit for bit"""
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


class _Handles:
    """`count` handles of one accumulator, destroyed together"""

    def __init__(self, L, create, destroy, count):
        self.hs, self._destroy = [], destroy
        try:
            for _ in range(count):
                h = L._VP()
                L.check(create(C.byref(h)))
                self.hs.append(h)
        except Exception:
            self.close()
            raise

    def close(self):
        for h in self.hs:
            self._destroy(h)
        self.hs = []


def _device_errors(worst, mom, key, mean, var):
    """the distance of one fetched mean / variance pair from the exact moments, at one cell of every distinct column"""
    at = mom['at']
    M2 = [v if math.isinf(v) else CF.Fraction(v) * 16 for v in var[at].tolist()]
    em, eq = CP.moment_errors(mean[at].tolist(), M2, mom['exact'])
    worst[0], worst[1] = max(worst[0], em), max(worst[1], eq)


ORDER = {'fused': list(range(6)), 'ab': list(range(6)), 'ba': [3, 4, 5, 0, 1, 2]}


# ---- ps_rank ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nplan,nslot,N,nthr', RANK_CASES)
def test_rank_every_plan_count_and_the_second_launch(nplan, nslot, N, nthr):
    P, S = nplan, nslot
    chunk = min(32, 1152 // (8 * nplan + 8))
    assert chunk == CP.rank_chunk(nplan)
    if nplan in ONE_MORE and (nplan, nslot) not in ((8, 32), (8, 5)):
        assert nslot == chunk + 1                      # the second launch holds one slot: a change of the budget fails here
    inj = CF.Injector(N)
    L, lib = inj.L, inj.lib
    thr = L.f64(CP.THR4[:nthr])
    mem, ref = CP.plan_members(N, nplan), CP.rank_reference(N, nplan)
    Q = nplan + nthr * (nplan + 2)
    with_sites = (nplan, nslot) == (8, 17)
    src = sites = H = None
    try:
        src = _Sources(inj, N, nplan, nslot)
        sites = _Sources(inj, N, nplan, nslot, 'sites') if with_sites else None
        H = _Handles(L, lambda out: lib.ps_rank_create(inj.dev, N, nplan, nslot, nthr, L.p_f64(thr) if nthr else None, out),
                     lib.ps_rank_destroy, 6 if with_sites else 5)
        full, a, b, a2, b2 = H.hs[:5]
        for i, m in enumerate(mem):
            src.feed(m)
            for h in (full, a if i < CP.HALF else b, a2 if i < CP.HALF else b2):
                L.check(lib.ps_rank_add_project(h, src.array, nplan, m[3]))
            if sites:
                sites.feed(m)
                L.check(lib.ps_rank_add_sites(H.hs[5], sites.array, nplan, m[3]))
            if i == 1:      # two identical members: every regret mean is the regret, M2 is 0, the second stored nothing
                for s in range(min(S, CP.NENTRY)):
                    for j in range(P):
                        mean, var = (_f64(L, N, lib.ps_rank_fetch, full, s, j, what) for what in (0, 1))
                        assert np.array_equal(mean, ref[s]['mom'][j]['first2'][0]) and not var.any(), (s, j)
        L.check(lib.ps_rank_merge(a, b))
        L.check(lib.ps_rank_merge(b2, a2))
        worst = [0.0, 0.0]
        D = np.zeros((S, Q, N * N), dtype=np.int64)          # the count planes of the handle that took every member
        M = np.zeros((S, P, N * N))                          # and its regret means
        for s in range(S):
            r = ref[CP.entry_of(s)]
            want_planes = CP.rank_count_planes(r, P, nthr)
            for h, key in ((full, 'fused'), (a, 'ab'), (b2, 'ba')):
                for j in range(P):
                    mom = r['mom'][j]
                    mean, var = (_f64(L, N, lib.ps_rank_fetch, h, s, j, what) for what in (0, 1))
                    bad = np.flatnonzero(mean != mom[key][0])
                    assert bad.size == 0, (s, j, key, bad[:5], mean[bad[:5]], mom[key][0][bad[:5]])
                    with np.errstate(over='ignore'):
                        want = mom[key][1] / W
                    bad = np.flatnonzero(var != want)
                    assert bad.size == 0, (s, j, key, bad[:5], var[bad[:5]], want[bad[:5]], (mom['plain'][1] / W)[bad[:5]])
                    if s < CP.NENTRY:
                        _device_errors(worst, mom, key, mean, var)
                    assert np.array_equal(_f64(L, N, lib.ps_rank_fetch, h, s, j, 2), r['best'][j] / W), (s, j, key)
                    if h is full:
                        M[s, j] = mean
                for q in range(Q):
                    got = _u32(L, N, lib.ps_rank_fetch_counts, h, s, q)
                    assert np.array_equal(got, want_planes[q]), (s, q, key)
                    if h is full:
                        D[s, q] = got
                if sites:
                    for j in range(P):
                        for what in (0, 1, 2):
                            assert np.array_equal(_f64(L, N, lib.ps_rank_fetch, H.hs[5], s, j, what),
                                                  _f64(L, N, lib.ps_rank_fetch, full, s, j, what))
        for h, key in ((full, 'fused'), (a, 'ab'), (b2, 'ba')) + (((H.hs[5], 'fused'),) if sites else ()):
            cells = np.zeros((len(mem), P, nthr, S), dtype=np.uint32)
            wts = np.zeros(len(mem), dtype=np.uint32)
            L.check(lib.ps_rank_fetch_coverage(h, 0, len(mem), cells.ctypes.data_as(U32P) if nthr else None,
                                               wts.ctypes.data_as(U32P)))
            order = ORDER[key]
            assert wts.tolist() == [CP.WEIGHTS[i] for i in order]
            for s in range(S):
                want = ref[CP.entry_of(s)]['rows'][order][:, :, :nthr]
                assert np.array_equal(cells[:, :, :, s], want), (key, s)
            if sites and h is H.hs[5]:
                for s in range(S):
                    for q in range(Q):
                        assert np.array_equal(_u32(L, N, lib.ps_rank_fetch_counts, h, s, q), D[s, q]), (s, q)
        print('rank P = %d, S = %d, N = %d: regret moments vs exact: mean %.4f, M2 %.4f units' % (P, S, N, worst[0], worst[1]))
        assert worst[0] <= 4 * CP.MEAN_ERR and worst[1] <= 4 * CP.M2_ERR
        # not vacuous, from the device's own planes: every plan is best somewhere; above zero a tie counted for nobody
        # (the members but the last hold something there, and less than their weight is anybody's); every sole, any and
        # all plane counts, and any is not all; the tail cell counts; the last slot holds something, and not what the
        # slot a chunk before it holds
        assert (D[:, :P].sum((0, 2)) > 0).all()
        lively = (M > 0).any(1)
        assert (lively & (D[:, :P].sum(1) < W - CP.WEIGHTS[-1] - 6)).sum() > 10
        for k in range(nthr):
            base = P + k * (P + 2)
            assert (D[:, base:base + P + 2].sum((0, 2)) > 0).all(), k
            assert (D[:, base + P] != D[:, base + P + 1]).any(), k
        assert D[:, :, -1].any() and M[:, :, -1].any()
        assert D[S - 1, :P].any() and M[S - 1].any() and (nthr == 0 or D[S - 1, P + P].any())
        if S > chunk:
            assert not np.array_equal(D[S - 1], D[S - 1 - chunk]) and not np.array_equal(M[S - 1], M[S - 1 - chunk])
    finally:
        for x in (H, sites, src):
            if x is not None:
                x.close()
        inj.close()


# ---- ps_contrast --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N', CP.SIZES)
@pytest.mark.parametrize('nslot', (5, 32))
def test_contrast_every_comparison_and_the_mirror(N, nslot):
    S, K = nslot, len(CF.THR)
    inj = CF.Injector(N)
    L, lib = inj.L, inj.lib
    thr = L.f64(CF.THR)
    mem, ref = CP.pair_members(N), CP.contrast_reference(N)
    Q = 2 + 2 * K
    src = sites = H = None
    try:
        src = _Sources(inj, N, 2, nslot)
        sites = _Sources(inj, N, 2, nslot, 'sites')
        H = _Handles(L, lambda out: lib.ps_contrast_create(inj.dev, N, nslot, K, L.p_f64(thr), out), lib.ps_contrast_destroy, 7)
        full, a, b, a2, b2, mirror, by_sites = H.hs
        A, B = src.hs
        for i, m in enumerate(mem):
            src.feed(m)
            for h in (full, a if i < CP.HALF else b, a2 if i < CP.HALF else b2):
                L.check(lib.ps_contrast_add_project(h, A, B, m[3]))
            L.check(lib.ps_contrast_add_project(mirror, B, A, m[3]))
            sites.feed(m)
            L.check(lib.ps_contrast_add_sites(by_sites, sites.hs[0], sites.hs[1], m[3]))
            if i == 1:      # a repeated negative d under a negative mean: nothing stored, the mean is d, M2 is 0
                for s in range(CP.NENTRY):
                    mean, var = (_f64(L, N, lib.ps_contrast_fetch, full, s, what) for what in (0, 1))
                    assert np.array_equal(mean, ref[s]['mom']['first2'][0]) and not var.any(), s
                    assert s or (mean < 0).sum() >= 20
        L.check(lib.ps_contrast_merge(a, b))
        L.check(lib.ps_contrast_merge(b2, a2))
        worst = [0.0, 0.0]
        D = np.zeros((S, Q, N * N), dtype=np.int64)
        crossed = 0
        for s in range(S):
            r = ref[CP.entry_of(s)]
            mom = r['mom']
            want_planes = CP.contrast_count_planes(r, K)
            for h, key in ((full, 'fused'), (a, 'ab'), (b2, 'ba')):
                mean, var = (_f64(L, N, lib.ps_contrast_fetch, h, s, what) for what in (0, 1))
                bad = np.flatnonzero(mean != mom[key][0])
                assert bad.size == 0, (s, key, bad[:5], mean[bad[:5]], mom[key][0][bad[:5]])
                with np.errstate(over='ignore'):
                    want = mom[key][1] / W
                bad = np.flatnonzero(var != want)
                assert bad.size == 0, (s, key, bad[:5], var[bad[:5]], want[bad[:5]], (mom['plain'][1] / W)[bad[:5]])
                if s < CP.NENTRY:
                    _device_errors(worst, mom, key, mean, var)
                for q in range(Q):
                    got = _u32(L, N, lib.ps_contrast_fetch_counts, h, s, q)
                    assert np.array_equal(got, want_planes[q]), (s, q, key)
                    assert np.array_equal(_f64(L, N, lib.ps_contrast_fetch, h, s, 2 + q), want_planes[q] / W), (s, q, key)
                    if h is full:
                        D[s, q] = got
                if h is full:       # (b, a): the mean negated, the sign planes and gain / loss swapped, M2 the same
                    assert np.array_equal(_f64(L, N, lib.ps_contrast_fetch, mirror, s, 0), -mean), s
                    assert np.array_equal(_f64(L, N, lib.ps_contrast_fetch, mirror, s, 1), var), s
                    for q in range(Q):
                        assert np.array_equal(_u32(L, N, lib.ps_contrast_fetch_counts, mirror, s, q ^ 1), D[s, q]), (s, q)
                    crossed += int(((mean != 0) & (D[s, 0] > 0) & (D[s, 1] > 0)).sum())
                    # the same members through two one-site release plans and ps_contrast_add_sites: the same planes
                    for what in (0, 1):
                        assert np.array_equal(_f64(L, N, lib.ps_contrast_fetch, by_sites, s, what), (mean, var)[what]), (s, what)
                    for q in range(Q):
                        assert np.array_equal(_u32(L, N, lib.ps_contrast_fetch_counts, by_sites, s, q), D[s, q]), (s, q)
        for h, key in ((full, 'fused'), (a, 'ab'), (b2, 'ba'), (mirror, 'mirror'), (by_sites, 'sites')):
            cells = np.zeros((len(mem), 2, K, S), dtype=np.uint32)
            wts = np.zeros(len(mem), dtype=np.uint32)
            L.check(lib.ps_contrast_fetch_coverage(h, 0, len(mem), cells.ctypes.data_as(U32P), wts.ctypes.data_as(U32P)))
            order = ORDER.get(key, ORDER['fused'])
            assert wts.tolist() == [CP.WEIGHTS[i] for i in order]
            for s in range(S):
                want = ref[CP.entry_of(s)]['rows'][order][:, :, :K]
                assert np.array_equal(cells[:, :, :, s], want[:, ::-1] if key == 'mirror' else want), (key, s)
        print('contrast S = %d, N = %d: difference moments vs exact: mean %.4f, M2 %.4f units' % (S, N, worst[0], worst[1]))
        assert worst[0] <= 4 * CP.MEAN_ERR and worst[1] <= 4 * CP.M2_ERR
        # not vacuous, from the device's own planes: every plane counts somewhere; cells where d was positive in one
        # member and negative in another; the tail cell counts; the last slot is not the first
        assert (D.sum((0, 2)) > 0).all() and crossed > 10 and D[:, :, -1].any()
        assert D[S - 1].any() and not np.array_equal(D[S - 1], D[0])
    finally:
        for x in (H, sites, src):
            if x is not None:
                x.close()
        inj.close()


# ---- the sources on the way ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N', CP.SIZES)
def test_sites_shift_the_ring_without_wrapping(N):
    """every shift to and across each edge, and one plan of three sites with amounts 1, 0.75 and 1 / 3: the border
    that leaves one edge does not come back at the other, nor in the neighbouring row"""
    inj = CF.Injector(N)
    L, lib = inj.L, inj.lib
    profile = ((1.0, 1.0), (1.0, 0.5))
    f = CP.ring(N)
    v = CF.history(f, profile)
    try:
        inj.inject(f)
        args = inj.slots(profile)
        moved = 0
        for plan in CP.ring_plans(N):
            dr, dc, am = (list(x) for x in zip(*plan))
            h = L._VP()
            L.check(lib.ps_sites_create(inj.dev, N, 2, 1, L.p_i32(L.i32([len(plan)])), L.p_i32(L.i32(dr)), L.p_i32(L.i32(dc)),
                                        L.p_f64(L.f64(am)), C.byref(h)))
            try:
                L.check(lib.ps_sites_apply(h, inj.s._h, 0, *args))
                for s in range(2):
                    got = _f64(L, N, lib.ps_sites_fetch, h, s).reshape(N, N)
                    want = CP.sites_expected(v[s], plan)
                    bad = np.argwhere(got != want)
                    assert bad.size == 0 and not np.signbit(got).any(), (plan, s, bad[:5])
                    moved += int((got != v[s]).sum())
            finally:
                lib.ps_sites_destroy(h)
        assert moved > 10 * N
    finally:
        inj.close()

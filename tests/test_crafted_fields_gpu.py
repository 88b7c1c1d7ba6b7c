"""The six value-level accumulators on the crafted fields of crafted_fields.py, through the C ABI: ps_summary, ps_hist,
ps_arrival, ps_peak, ps_excur and ps_range.  Every field is injected with HipSolve.set_state and read back bit for
bit before anything is compared; every slot reads PS_REC_STATE under its own (stat_scale, post_scale).  Every cell of
every plane is compared, at N = 65 and 129; the same members go into two more handles that are merged in both orders;
and after the comparisons the cases the fields are there for are counted once more on the device's own outputs.

ps_summary.  The device's mean is the bits of the header's statement, and its M2 those of the statement with the last
step fused: M2 = fma(w * d, v - mean, M2), the product (w d) (v - mean) and the addition to M2 in one rounding -- what
-ffp-contract=on makes of `m2 += w * d * (v - m)` in sum_update (ps_common.h).  ps_summary_fetch returns M2 / W with
W = 9 here, and x -> x / 9 maps neighbouring doubles to different doubles, so equal variances are equal M2.
The merged summaries (two members + three, in both orders) are the bits of crafted_fields.merge_fused, the update
with both of its last products fused as the gfx950 code of k_summary_merge has them.  Against the exact rational
moments they lie within, largest over both sizes and every slot, measured on an MI355X on 2026-10-21 on top of commit
6186f73 (M2 recovered as 9 x the fetched variance, which carries the rounding of that division too):
    mean  0.9254 x 2^-53 max_m |v_m|          (0.8089 at N = 65; asserted: <= 4 x 1.0492)
    M2    3.4569 x 2^-53 sum_m w_m v_m^2      (3.1969 at N = 65; asserted: <= 4 x 2.4446)

Not through the C ABI, so not compared: the histogram's range words (their effect is: ps_hist_quantile and
ps_hist_exceed read only the planes they bound).  The header admits p in (0, 1] for the quantiles and fractions in
(0, 1) for the ranges: p = 0 and the fraction 1 are checked as refusals, and the largest double below 1 stands in for
the fraction 1 (crafted_fields.py).
"""
import ctypes as C

import numpy as np
import pytest

import arrival_ref as AR
import crafted_fields as CF
import excur_ref as XR
import hist_ref as HR
import peak_ref as PK
import range_ref as RR

pytestmark = pytest.mark.gpu

U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
S, K = CF.NSLOT, len(CF.THR)
QUANTILES = (0.05, 0.5, 1.0)


def _f64(inj, N, call, *args):
    out = np.empty((N, N))
    inj.L.check(call(*args, inj.L.p_f64(out)))
    return out


def _u32(inj, N, call, *args):
    out = np.empty((N, N), dtype=np.uint32)
    inj.L.check(call(*args, out.ctypes.data_as(U32P)))
    return out.astype(np.int64)


def _i32(inj, N, call, *args):
    out = np.empty((N, N), dtype=np.int32)
    inj.L.check(call(*args, inj.L.p_i32(out)))
    return out.astype(np.int64)


class _Built:
    """the members in one handle (`full`), and in two halves merged as first + second (`ab`) and second + first (`ba`);
    order[...] the members' indices in each handle's fetches"""

    def __init__(self, inj, name, create, mem, after_add=None):
        L, lib = inj.L, inj.lib
        self.inj, self.lib, self._destroy, self.hs = inj, lib, getattr(lib, 'ps_%s_destroy' % name), []
        add, merge = getattr(lib, 'ps_%s_add' % name), getattr(lib, 'ps_%s_merge' % name)
        try:
            for _ in range(5):
                h = L._VP()
                L.check(create(C.byref(h)))
                self.hs.append(h)
            full, a, b, a2, b2 = self.hs
            half = len(mem) // 2
            for i, m in enumerate(mem):
                inj.inject(m[1])
                args = inj.slots(m[2], *m[4:])
                for h in (full, a if i < half else b, a2 if i < half else b2):
                    L.check(add(h, inj.s._h, *args, m[3]))
                if after_add is not None:
                    after_add(i, full)
            L.check(merge(a, b))
            L.check(merge(b2, a2))
            fwd = list(range(len(mem)))
            self.full, self.ab, self.ba = full, a, b2
            self.order = {id(full): fwd, id(a): fwd, id(b2): fwd[half:] + fwd[:half]}
        except Exception:
            self.close()
            raise

    def close(self):
        for h in self.hs:
            self._destroy(h)
        self.hs = []
        self.inj.close()


def _weights(mem):
    return [m[3] for m in mem]


# ---- ps_summary -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N', CF.SIZES)
def test_summary_mean_and_m2_bit_for_bit_and_merges_against_the_exact_moments(N):
    inj = CF.Injector(N)
    L, lib = inj.L, inj.lib
    mem, ref = CF.summary_members(N), CF.summary_reference(N)
    W = float(sum(CF.SUM_WEIGHTS))
    pair = {}

    def after_add(i, h):
        if i == 1:        # two identical members: the second stored nothing, mean == v and M2 == 0 bit for bit
            for s in range(S):
                pair[s] = (_f64(inj, N, lib.ps_summary_fetch, h, s, 0), _f64(inj, N, lib.ps_summary_fetch, h, s, 1))
    B = _Built(inj, 'summary', lambda out: lib.ps_summary_create(inj.dev, N, S, K, L.p_f64(L.f64(CF.THR)), out), mem,
               after_add)
    try:
        worst = [0.0, 0.0]
        differ = at_thr = 0
        for s in range(S):
            r = ref[s]
            V = r['V']
            assert np.array_equal(pair[s][0].ravel(), V[0]) and not pair[s][1].any(), s
            for h in (B.full, B.ab, B.ba):
                for k, t in enumerate(CF.THR):
                    got = _f64(inj, N, lib.ps_summary_fetch, h, s, 2 + k).ravel()
                    assert np.array_equal(got, r['counts'][k].astype(np.float64) / W), (s, k)
            mean = _f64(inj, N, lib.ps_summary_fetch, B.full, s, 0).ravel()
            var = _f64(inj, N, lib.ps_summary_fetch, B.full, s, 1).ravel()
            bad = np.flatnonzero(mean != r['fused'][0])
            assert bad.size == 0, (s, bad[:5], mean[bad[:5]], r['fused'][0][bad[:5]])
            bad = np.flatnonzero(var != r['fused'][1] / W)
            assert bad.size == 0, (s, bad[:5], var[bad[:5]], (r['fused'][1] / W)[bad[:5]], (r['plain'][1] / W)[bad[:5]])
            differ += int((r['fused'][1] / W != r['plain'][1] / W).sum())
            at_thr += int(sum((V == t).any(0).sum() for t in CF.THR))
            for h, key in ((B.ab, 'ab'), (B.ba, 'ba')):
                m = _f64(inj, N, lib.ps_summary_fetch, h, s, 0).ravel()
                v = _f64(inj, N, lib.ps_summary_fetch, h, s, 1).ravel()
                assert (v >= 0).all()
                assert np.array_equal(m, r[key][0]) and np.array_equal(v, r[key][1] / W), (s, key)     # the merge's bits
                M2 = np.array([x * 9 for x in map(CF.Fraction, v.tolist())], dtype=object)     # the division undone
                em, eq = CF.moment_errors(m, M2, r['exact'])
                worst = [max(worst[0], em), max(worst[1], eq)]
        print('merged summaries vs exact moments at N = %d: mean %.4f, M2 %.4f units' % (N, worst[0], worst[1]))
        assert worst[0] <= 4 * CF.MEAN_ERR and worst[1] <= 4 * CF.M2_ERR
        # not vacuous: the fused M2 is not the plain one, values sit on the thresholds, the cut took cells
        assert differ > 500 and at_thr >= 27
        assert (ref[1]['V'][3] == 0).sum() > (ref[0]['V'][3] == 0).sum()
    finally:
        B.close()


# ---- ps_hist ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N', CF.SIZES)
def test_hist_counts_quantiles_and_exceedance(N):
    inj = CF.Injector(N)
    L, lib = inj.L, inj.lib
    mem, H = CF.members(N), CF.histories(N)
    w = _weights(mem)
    nb = len(CF.EDGES) + 1
    B = _Built(inj, 'hist', lambda out: lib.ps_hist_create(inj.dev, N, S, len(CF.EDGES), L.p_f64(L.f64(CF.EDGES)), out), mem)
    try:
        def quantile(h, s, p):
            out = [np.empty((N, N)) for _ in range(3)]
            L.check(lib.ps_hist_quantile(h, s, p, *[L.p_f64(a) for a in out]))
            return out
        dev_counts = []
        for s in range(S):
            ref = HR.weighted_counts([h[s] for h in H], w, CF.EDGES)
            got = {id(h): np.array([_u32(inj, N, lib.ps_hist_fetch_counts, h, s, b) for b in range(nb)])
                   for h in (B.full, B.ab, B.ba)}
            for h in (B.full, B.ab, B.ba):
                assert np.array_equal(got[id(h)], ref), s
            dev_counts.append(got[id(B.full)])
            for p in QUANTILES:
                bstar, val, lo, hi = HR.quantile_from_counts(ref, CF.EDGES, p)
                gv, glo, ghi = quantile(B.full, s, p)
                assert np.array_equal(glo, lo) and np.array_equal(ghi, hi), (s, p)      # the bracket names the bin
                np.testing.assert_allclose(gv, val, rtol=1e-12, atol=0)
                assert np.array_equal(gv[(bstar == 0) | (bstar == nb - 1)], val[(bstar == 0) | (bstar == nb - 1)])
                for h in (B.ab, B.ba):
                    assert all(np.array_equal(x, y) for x, y in zip(quantile(h, s, p), (gv, glo, ghi)))
            for k in range(len(CF.EDGES)):
                want = HR.exceedance_from_counts(ref, k)
                for h in (B.full, B.ab, B.ba):
                    assert np.array_equal(_f64(inj, N, lib.ps_hist_exceed, h, s, k), want), (s, k)
        one = np.empty((N, N))
        assert lib.ps_hist_quantile(B.full, 0, 0.0, L.p_f64(one), None, None) == L.PS_ERR_BAD_ARG      # p in (0, 1]
        # not vacuous, from the device's counts: weight in bin 0 and in bin B + 1, on both sides of every edge by one
        # ulp, pairs that share a plane and pairs that do not, the tail cell in every bin
        D = np.array(dev_counts).reshape(S, nb, -1)
        assert D[:, 0].min() > 0 and (D[:, nb - 1] > 0).sum() > 50
        assert set(np.flatnonzero(D[:, :, -1].sum(0))) == set(range(nb))
        left = np.zeros((S, nb, N * N), dtype=np.int64)
        for s in range(S):
            for h, wi in zip(H, w):
                b = np.searchsorted(np.array(CF.EDGES), h[s].ravel(), side='left')
                left[s, b, np.arange(N * N)] += wi
        assert ((left != D).any(1).sum(1) > 50).all()                # side='left' would have been seen in every slot
        top = nb - 1 - np.argmax(D[:, ::-1] > 0, axis=1)           # the highest bin any member put the cell in
        pairs = top[:, :N * N - 1].reshape(S, -1, 2)
        assert (pairs[..., 0] != pairs[..., 1]).sum() > 100 and ((pairs[..., 0] == pairs[..., 1]) & (pairs[..., 0] > 0)).sum() > 100
    finally:
        B.close()


# ---- ps_arrival ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N', CF.SIZES)
def test_arrival_counts_rows_probabilities_and_quantiles(N):
    inj = CF.Injector(N)
    L, lib = inj.L, inj.lib
    mem, H = CF.members(N), CF.histories(N)
    w = _weights(mem)
    B = _Built(inj, 'arrival', lambda out: lib.ps_arrival_create(inj.dev, N, S, K, L.p_f64(L.f64(CF.THR)), out), mem)
    try:
        ref = AR.weighted_counts(H, w, CF.THR)
        rows, prob = AR.reached_rows(H, CF.THR), AR.probability(ref)
        for h in (B.full, B.ab, B.ba):
            for k in range(K):
                for s in range(S + 1):
                    assert np.array_equal(_u32(inj, N, lib.ps_arrival_fetch_counts, h, k, s), ref[k, s]), (k, s)
                for s in range(S):
                    assert np.array_equal(_f64(inj, N, lib.ps_arrival_prob, h, k, s), prob[k, s]), (k, s)
                for p in QUANTILES:
                    assert np.array_equal(_i32(inj, N, lib.ps_arrival_quantile, h, k, p), AR.quantile_slots(ref, p)[k]), (k, p)
            cells = np.empty((len(mem), K, S), dtype=np.uint32)
            wts = np.empty(len(mem), dtype=np.uint32)
            L.check(lib.ps_arrival_fetch_reached(h, 0, len(mem), cells.ctypes.data_as(U32P), wts.ctypes.data_as(U32P)))
            order = B.order[id(h)]
            bad = np.flatnonzero((cells.astype(np.int64) != rows[order]).any((1, 2)))
            assert bad.size == 0, [mem[order[i]][:3:2] for i in bad]
            assert wts.tolist() == [w[i] for i in order]
        one = np.empty((N, N), dtype=np.int32)
        assert lib.ps_arrival_quantile(B.full, 0, 0.0, L.p_i32(one)) == L.PS_ERR_BAD_ARG
        # not vacuous, from the device's planes and rows: arrivals at every slot and never; members that reach the
        # lower thresholds only; a member whose every cell passes the top threshold at slot 0 (its waves leave at once);
        # a member that re-crosses counted at its first slot, not at the one after which it stays
        D = np.array([[_u32(inj, N, lib.ps_arrival_fetch_counts, B.full, k, s) for s in range(S + 1)] for k in range(K)])
        assert (D.reshape(K, S + 1, -1).sum(2) > 0).all()
        cells = np.empty((len(mem), K, S), dtype=np.uint32)
        L.check(lib.ps_arrival_fetch_reached(B.full, 0, len(mem), cells.ctypes.data_as(U32P), None))
        assert ((cells[:, 0, -1] > 0) & (cells[:, -1, -1] == 0)).sum() >= 5
        assert (cells[:, -1, 0] == N * N).sum() >= 1 and (cells[:, :, -1] == 0).all(1).sum() >= 2
        i = [j for j, m in enumerate(mem) if m[0] == 'full' and m[2] == 'recross'][0]
        assert cells[i, -1].tolist() == [N * N] * S and cells[i, 0].tolist() == [N * N] * S
    finally:
        B.close()


# ---- ps_peak ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N', CF.SIZES)
def test_peak_field_days_and_durations(N):
    inj = CF.Injector(N)
    L, lib = inj.L, inj.lib
    mem, H = CF.members(N), CF.histories(N)
    w = _weights(mem)
    seen = {'ties': 0, 'zero': 0}

    def after_add(i, h):                      # Y is the peak field of the last member: every add rewrites it
        Y = _f64(inj, N, lib.ps_peak_fetch_field, h)
        want = PK.peak_field(H[i])
        assert np.array_equal(Y, want) and not np.signbit(Y).any(), mem[i][:3:2]
        seen['ties'] += int((((H[i] == want).sum(0) >= 2) & (want > 0)).sum())
        seen['zero'] += int(not Y.any())
    B = _Built(inj, 'peak', lambda out: lib.ps_peak_create(inj.dev, N, S, K, L.p_f64(L.f64(CF.THR)), out), mem, after_add)
    try:
        dc, uc = PK.day_counts(H, w), PK.duration_counts(H, w, CF.THR)
        last = np.zeros_like(dc)
        for h_i, wi in zip(H, w):                 # the altered rule: the last slot of a tie
            m = h_i.max(0)
            p = np.where(m > 0, S - 1 - np.argmax((h_i == m)[::-1], 0), S)
            for s in range(S + 1):
                last[s] += wi * (p == s)
        for h in (B.full, B.ab, B.ba):
            pk = np.array([_u32(inj, N, lib.ps_peak_fetch_day_counts, h, s) for s in range(S)])
            assert np.array_equal(pk, dc[:S])
            for p in QUANTILES:
                assert np.array_equal(_i32(inj, N, lib.ps_peak_day_quantile, h, p), PK.day_quantile(dc, p)), p
            for s in range(S):
                assert np.array_equal(_f64(inj, N, lib.ps_peak_day_prob, h, s), PK.day_prob(dc)[s]), s
            for k in range(K):
                du = np.array([_u32(inj, N, lib.ps_peak_fetch_duration_counts, h, k, n) for n in range(S + 1)])
                assert np.array_equal(du, uc[k]), k
                for p in QUANTILES:
                    got = _i32(inj, N, lib.ps_peak_duration_quantile, h, k, p)
                    assert np.array_equal(got, PK.duration_quantile(uc[k], p)), (k, p)
                assert np.array_equal(_f64(inj, N, lib.ps_peak_duration_mean, h, k), PK.duration_mean(uc[k])), k
                for n in range(1, S + 1):
                    assert np.array_equal(_f64(inj, N, lib.ps_peak_duration_prob, h, k, n), PK.duration_prob(uc[k])[n]), (k, n)
        # not vacuous, from the device: ties in time took the first slot (the last one would show), members of zeros,
        # peaks on every slot, every duration 0 .. S
        pk = np.array([_u32(inj, N, lib.ps_peak_fetch_day_counts, B.full, s) for s in range(S)])
        assert seen['ties'] > 1000 and seen['zero'] >= 3 and (pk != last[:S]).any(1).sum() > 100
        assert (pk.reshape(S, -1).sum(1) > 0).tolist() == [True, True, True, False, True]    # slot 3 is only ever the
        # second slot of a tie ('tie', 'prob'): no weight may land there
        du = np.array([_u32(inj, N, lib.ps_peak_fetch_duration_counts, B.full, 0, n) for n in range(S + 1)])
        assert (du.reshape(S + 1, -1).sum(1) > 0).all()
    finally:
        B.close()


# ---- ps_excur -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N', CF.SIZES)
def test_excursion_counts_masks_bounds_and_maps(N):
    inj = CF.Injector(N)
    L, lib = inj.L, inj.lib
    mem, H = CF.members(N), CF.histories(N)
    w = _weights(mem)
    M, nword = len(mem), (N * N + 63) // 64
    B = _Built(inj, 'excur', lambda out: lib.ps_excur_create(inj.dev, N, S, K, L.p_f64(L.f64(CF.THR)), out), mem)
    try:
        empty = full = 0
        for k, t in enumerate(CF.THR):
            for s in range(S):
                fields = np.array([h[s] for h in H])
                for h in (B.full, B.ab, B.ba):
                    order = B.order[id(h)]
                    ref = XR.plane(fields[order], [w[i] for i in order], t)
                    assert np.array_equal(_u32(inj, N, lib.ps_excur_fetch_counts, h, k, s), ref['C']), (k, s)
                    hi, lo, wt = (np.empty(M, dtype=np.uint32) for _ in range(3))
                    L.check(lib.ps_excur_fetch_bounds(h, k, s, *[a.ctypes.data_as(U32P) for a in (hi, lo, wt)]))
                    assert np.array_equal(hi, ref['hi']) and np.array_equal(lo, ref['lo']), (k, s)
                    assert wt.tolist() == [w[i] for i in order]
                    for what, key in ((0, 'above'), (1, 'below'), (2, 'contour')):
                        got = _f64(inj, N, lib.ps_excur_map, h, k, s, what)
                        assert np.array_equal(got, ref[key]), (k, s, key)
                        for level in (0.9, 1.0):
                            assert np.array_equal(got >= level, ref[key] >= level)
                    if h is B.ab:
                        continue
                    words = np.empty((M, nword), dtype=np.uint64)
                    for m in range(M):
                        L.check(lib.ps_excur_fetch_mask(h, m, k, s, words[m].ctypes.data_as(U64P)))
                    bad = np.flatnonzero((words != ref['words']).any(1))
                    assert bad.size == 0, (k, s, [mem[order[i]][:3:2] for i in bad])
                    assert not (words[:, -1] >> np.uint64(1)).any()                   # the pad bits of the last word
                    if h is B.full:
                        empty += int((~words.any(1)).sum())
                        full += int((ref['B'].all(1)).sum())
                        if k == 0 and s == 0:
                            assert (words[:, -1] == 1).sum() >= 10                       # the tail cell alone in its word
        # not vacuous: empty masks, full masks, two identical members
        assert empty > 100 and full >= 5
        assert np.array_equal(H[0], H[1])
    finally:
        B.close()


# ---- ps_range -----------------------------------------------------------------------------------------------------------

def _range_rows(inj, h, M, nslot):
    L, lib = inj.L, inj.lib
    J = len(CF.FRACTIONS)
    lam, n = np.empty((M, J, nslot)), np.empty((M, J, nslot), dtype=np.int64)
    Q, E, wt = np.empty((M, nslot), dtype=object), np.empty((M, nslot), dtype=np.int64), None
    for s in range(nslot):
        q, e = np.empty(M, dtype=np.uint64), np.empty(M, dtype=np.int32)
        L.check(lib.ps_range_fetch_mass(h, s, q.ctypes.data_as(U64P), L.p_i32(e)))
        Q[:, s], E[:, s] = [int(x) for x in q], e
        for j in range(J):
            a, c, wt = np.empty(M), np.empty(M, dtype=np.uint32), np.empty(M, dtype=np.uint32)
            L.check(lib.ps_range_fetch_members(h, j, s, L.p_f64(a), c.ctypes.data_as(U32P), wt.ctypes.data_as(U32P)))
            lam[:, j, s], n[:, j, s] = a, c
    return lam, n, Q, E, wt.tolist()


def _check_range(inj, N, h, ref, order, weights, names):
    lib = inj.lib
    lam, n, Q, E, wt = _range_rows(inj, h, len(order), 2)
    assert wt == [weights[i] for i in order]
    for got, key in ((lam, 'lam'), (n, 'n'), (Q, 'Q'), (E, 'E')):
        want = ref[key][order]
        bad = [names[order[i]] for i in range(len(order)) if not np.array_equal(got[i], want[i])]
        assert not bad, (key, bad, got, want)
    W = float(sum(weights[i] for i in order))
    for j in range(len(CF.FRACTIONS)):
        for s in range(2):
            assert np.array_equal(_u32(inj, N, lib.ps_range_fetch_counts, h, j, s), ref['counts'][j, s]), (j, s)
            assert np.array_equal(_f64(inj, N, lib.ps_range_prob, h, j, s), ref['counts'][j, s].astype(np.float64) / W), (j, s)


@pytest.mark.parametrize('N', CF.SIZES)
def test_range_levels_cells_and_masses(N):
    inj = CF.Injector(N)
    L, lib = inj.L, inj.lib
    mem = CF.range_members(N)
    names, w = [m[0] for m in mem], _weights(mem)
    fields = [CF.history(m[1], m[2], m[4]) for m in mem]
    frac = L.f64(CF.FRACTIONS)

    def create(out):
        return lib.ps_range_create(inj.dev, N, 2, len(CF.FRACTIONS), L.p_f64(frac), out)
    h = L._VP()
    assert lib.ps_range_create(inj.dev, N, 2, 2, L.p_f64(L.f64([0.5, 1.0])), C.byref(h)) == L.PS_ERR_BAD_ARG and not h
    B = _Built(inj, 'range', create, mem)
    try:
        ref = RR.accumulate(fields, w, CF.FRACTIONS)
        for h in (B.full, B.ab, B.ba):
            _check_range(inj, N, h, ref, B.order[id(h)], w, names)
        # every field as the only member of a handle
        inj2 = CF.Injector(N)
        one = L._VP()
        L.check(create(C.byref(one)))
        try:
            for i, m in enumerate(mem):
                L.check(lib.ps_range_reset(one))
                inj2.inject(m[1])
                L.check(lib.ps_range_add(one, inj2.s._h, *inj2.slots(m[2], m[4]), m[3]))
                alone = RR.accumulate(fields[i:i + 1], w[i:i + 1], CF.FRACTIONS)
                _check_range(inj2, N, one, alone, [0], w[i:i + 1], names[i:i + 1])
        finally:
            lib.ps_range_destroy(one)
            inj2.close()
        # not vacuous, from the device's rows
        lam, n, Q, E, _wt = _range_rows(inj, B.full, len(mem), 2)
        at = {name: i for i, name in enumerate(names)}
        z = at['zero']
        assert np.isinf(lam[z]).all() and not n[z].any() and Q[z].tolist() == [0, 0]
        assert lam[at['plateau2'], 1, 0] == 2.0 and n[at['plateau2'], :, 0].tolist() == [100, 100, 300, 300]
        assert lam[at['plateau2_odd'], 1, 0] == 0.5 + 2.0 ** -36 and n[at['plateau2_odd'], :, 0].tolist() == [1, 3, 3, 3]
        assert n[at['all_equal'], :, 0].tolist() == [N * N] * 4 and n[at['full'], :, 1].tolist() == [N * N] * 4
        assert lam[at['span36'], 3, 0] == 2.0 ** -20 and n[at['span36'], 3, 0] == 81 and E[at['span36'], 0] == 16
        assert E[at['pow2_max'], 0] == 5 and E[at['below_pow2_max'], 0] == 4 and E[at['subnormal_max'], 0] == -1061
        assert E[at['tiny'], 0] == -997 and E[at['big'], 0] == 996 and Q[at['subnormal_max'], 0] > 2 ** 36
        assert n[at['first_cell'], :, 0].tolist() == [1] * 4 and n[at['tail_cell'], :, 0].tolist() == [1] * 4
    finally:
        B.close()

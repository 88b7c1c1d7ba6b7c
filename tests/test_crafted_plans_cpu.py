"""The crafted plans of crafted_plans.py, without a GPU: the zoo holds every case it is there for, the numpy
restatements of the rules of ps_rank_* and ps_contrast_* equal a per-cell loop over Python floats, every altered rule
changes the reference on the zoo, and the restated moments lie where crafted_plans.py says against exact rationals.

Altered rules and smooth fields (printed by test_every_altered_rule_changes_the_reference; bump_plans / bump_pairs
are one Gaussian bump scaled per plan, under three profiles of which one has a slot of zeros, as most of a model's
domain is zero).  At both sizes and every P the bump is blind to three of the twelve: `>` for `>=` at a threshold, the
coverage rows counting the tail item's missing second cell, and gain with b <= t: it has no value on a threshold and
nothing in the tail cell.  It does tell the other nine, and fewer are hidden than one might expect: a slot of zeros is
a P-fold tie and a d == 0 everywhere, so a tie that goes to the lowest index or to every holder and d >= 0 for d > 0
show on any field with zeros in it, and sole with n >= 1, all with n >= P - 1, the regret against the other plans, the
last plan left out of the maximum, a pair whose second cell takes the first one's values and a second chunk written to
slot - chunk change smooth fields as well.  What the bump cannot do is tell them *at the values where kernels go
wrong*: a tie above zero, a one-ulp regret, a subset on a threshold; those are what the zoo is counted for above.
"""
import numpy as np
import pytest

import crafted_fields as CF
import crafted_plans as CP


def _masks(a, hi, lo):
    """the subsets, as bit masks, of the cells whose plans all hold hi or lo"""
    cells = np.flatnonzero(((a == hi) | (a == lo)).all(0))
    return cells, ((a[:, cells] == hi) * (1 << np.arange(a.shape[0]))[:, None]).sum(0)


@pytest.mark.parametrize('N', CP.SIZES)
@pytest.mark.parametrize('P', CP.PLANS)
def test_the_plan_zoo_holds_what_it_is_for(N, P):
    n, at, mem = N * N, CP.layout(N, P), CP.plan_members(N, P)
    assert len(mem) >= 5 and [m[3] for m in mem] == list(CP.WEIGHTS) and sum(CP.WEIGHTS) == 16
    assert np.array_equal(mem[0][1], mem[1][1]) and mem[0][2] == mem[1][2] and not mem[-1][1].any()
    a = mem[0][1].reshape(P, n)
    # every tie structure at every m: n_max takes every value, every non-empty subset holds the maximum somewhere,
    # the regrets include one ulp of m, m / 2 and m itself
    for i, m in enumerate(CP.tie_m(0)):
        blk = a[:, at['tie', i]:at['tie', i] + 2 ** P - 1]
        assert (blk.max(0) == m).all()
        hold = blk == m
        assert set(hold.sum(0)) == set(range(1, P + 1))
        assert len(set(((hold * (1 << np.arange(P))[:, None]).sum(0)).tolist())) == 2 ** P - 1
    kinds = set()
    for i, m in enumerate(CP.tie_m(0)):
        reg = set((a.max(0) - a)[:, at['tie', i]:at['tie', i] + 2 ** P - 1].ravel().tolist())
        assert reg <= {0.0, m - np.nextafter(m, 0), m / 2, m}
        kinds |= {(i, 'ulp' if x == m - np.nextafter(m, 0) else x / m) for x in reg}
        assert P == 2 or len(reg) == 4                  # two plans have two cells with a loser per m: two kinds each
    assert {(0, 'ulp'), (1, 'ulp'), (0, 1.0), (1, 0.5)} <= kinds
    # every subset at, and just above, every threshold against the value just below it
    assert {k for k, up in CP.THR_BLOCKS if up == 0} == set(range(4)) and {k for k, up in CP.THR_BLOCKS if up} == set(range(3))
    for t in CP.THR4:
        below, _t, above = CF.around(t)
        for hi in (t, above) if t in CF.THR else (t,):
            cells, masks = _masks(a, hi, below)
            k0 = at['thr', CP.THR4.index(t), int(hi != t)]
            inside = (cells >= k0) & (cells < k0 + 2 ** P)
            cells, masks = cells[inside], masks[inside]
            assert set(masks.tolist()) == set(range(2 ** P)), (t, hi)
            # the two cells a thread owns carry different subsets
            first = cells[(cells % 2 == 0) & np.isin(cells + 1, cells)]
            assert first.size >= 2 ** (P - 1) - 1
            lookup = dict(zip(cells.tolist(), masks.tolist()))
            assert all(lookup[c] != lookup[c + 1] for c in first.tolist())
    # placement: odd starts; the row-end copy has one pair on two rows, the wave-end copy ends a 128-cell wave, the
    # tail copy ends in the tail cell, and all three hold the short block
    sb = CP.short_block(P)
    assert all(v % 2 == 1 for v in at.values())
    e = at['row_end'] + 5
    assert e % 2 == 0 and e // N + 1 == (e + 1) // N
    assert (at['wave_end'] + 5) % 128 == 0 and at['tail'] + CP.SHORT == n and (n - 1) % 128 == 0
    for where in ('row_end', 'wave_end', 'tail'):
        assert np.array_equal(a[:, at[where]:at[where] + CP.SHORT], sb)
    assert sb[:, 5].tolist() != sb[:, 6].tolist() and sb[:, 4].tolist() != sb[:, 5].tolist()
    assert a[P - 1, n - 1] == 10.0 and (a[:P - 1, n - 1] == np.nextafter(10.0, 0)).all()
    # member 3: of the last 140 cells only the tail cell holds anything, so it is alone in its wave and its block
    f3 = mem[3][1].reshape(P, n)
    assert f3[:, n - 1].any() and not f3[:, n - 140:n - 1].any()
    # the rotation moves every plan's values on: member 2's plan j is member 0's plan j + 1 outside the HOT cells
    hot = CP.hot_cells(N, P)
    cold = np.setdiff1d(np.arange(at['thr', 0, 0], at['hot']), hot)
    f2 = mem[2][1].reshape(P, n)
    assert np.array_equal(f2[:, cold], np.roll(a, -1, axis=0)[:, cold])
    # HOT: the regret of plan 1 is 1e6 (1 + tiny) in the first five members
    r = np.array([(m[1].reshape(P, n).max(0) - m[1].reshape(P, n)[1])[hot] for m in mem[:5]])
    assert (abs(r / 1e6 - 1) < 1e-9).all() and (np.ptp(r, axis=0) > 0).all() and np.array_equal(r[0], r[1])
    # most of a member is zero in every plan (P = 8 at N = 65 fills 3400 of 4225 cells: 2^P subsets, eight times)
    live = max(int(m[1].any(0).sum()) for m in mem)
    assert live <= 3500 and (live < n // 3 or (N, P) in ((65, 7), (65, 8)))
    # no two neighbouring slots share an entry, nor do the slots s and s - chunk, and five slots are the entries
    assert [CP.entry_of(s) for s in range(5)] == list(range(5))
    assert all(CP.entry_of(s) != CP.entry_of(s + 1) for s in range(31))
    c = CP.rank_chunk(P)
    assert all(CP.entry_of(s) != CP.entry_of(s - c) for s in range(c, 32))
    assert [CP.rank_chunk(p) for p in CP.PLANS] == [32, 32, 28, 24, 20, 18, 16]


@pytest.mark.parametrize('N', CP.SIZES)
def test_the_pair_zoo_holds_what_it_is_for(N):
    n, at, mem, cases = N * N, CP.pair_layout(N), CP.pair_members(N), CP.pair_cases()
    L = cases.shape[1]
    have = set(map(tuple, cases.T.tolist()))
    for t in CF.THR:
        lo = np.nextafter(t, 0)
        assert {(t, lo), (lo, t), (t, t)} <= have
    d = cases[0] - cases[1]
    assert (d == 0).sum() >= 5 and ((d == 0) & (cases[0] > 0)).sum() >= 5
    for m in (25.0, 1e300, CP.SUBNORMAL):
        ulp = m - np.nextafter(m, 0)
        assert {ulp, -ulp} <= set(d.tolist())
    assert 1e16 - 1.0 in d.tolist() and 1e16 - 1.0 == 1e16                          # the difference rounds
    a = mem[0][1].reshape(2, n)
    e = at['row_end'] + 5
    assert all(v % 2 == 1 for v in at.values()) and e % 2 == 0 and e // N + 1 == (e + 1) // N
    assert (at['wave_end'] + 5) % 128 == 0 and at['tail'] + L == n
    for where in at:
        assert np.array_equal(a[:, at[where]:at[where] + L], cases)
    assert a[:, n - 1].any() and cases[:, 5].tolist() != cases[:, 6].tolist()
    # the sequence: d changes sign from member to member, a negative d repeats, the loguniform member, the zero one
    D = np.array([CP.values(m, 0)[0] - CP.values(m, 0)[1] for m in mem])
    assert ((D[1] < 0) & (D[2] > 0)).any() and ((D[2] > 0) & (D[4] < 0)).any()
    assert np.array_equal(D[0], D[1]) and (D[0] < 0).sum() >= 20 and not D[-1].any()
    mean_after_two = CP.contrast_reference(N)[0]['mom']['first2'][0]
    assert np.array_equal(mean_after_two, D[0])
    with np.errstate(over='ignore'):
        signs = np.sign(np.array([CF.welford(D[:k], CP.WEIGHTS[:k], False)[0] for k in range(1, 6)]))
    assert ((signs.min(0) < 0) & (signs.max(0) > 0)).sum() >= 10                     # the mean crosses zero
    f3 = mem[3][1].reshape(2, n)
    lu = f3[0, :CP.PAIR_LOG]
    assert (lu > 0).sum() > 900 and sorted(lu.tolist()) == sorted(f3[1, :CP.PAIR_LOG].tolist()) and (lu != f3[1, :CP.PAIR_LOG]).sum() > 900
    assert f3[:, n - 1].any() and not f3[:, n - 140:n - 1].any()


# ---- the numpy restatements against a loop over Python floats ---------------------------------------------------------

def _rank_cell(col, thr):
    """one cell with max, ==, >= and - alone -> (best [P], regret [P], per threshold (sole [P], any, all), reach [K][P])"""
    m = max(col)
    n_max = sum(1 for x in col if x == m)
    best = [x == m and n_max == 1 for x in col]
    reg = [m - x for x in col]
    per = []
    for t in thr:
        c = sum(1 for x in col if x >= t)
        per.append(([x >= t and c == 1 for x in col], c >= 1, c == len(col)))
    return best, reg, per


@pytest.mark.parametrize('P', (2, 5, 8))
def test_rank_restatement_equals_a_loop_over_python_floats(P):
    N = 65
    n, K = N * N, len(CP.THR4)
    seen = 0
    for mem in CP.plan_members(N, P):
        for e in range(CP.NENTRY):
            a = CP.values(mem, e)
            got = CP.rank_planes(a, CP.THR4)
            live = np.flatnonzero(a.any(0))
            dead = np.setdiff1d(np.arange(n), live)
            # a cell of zeros: a P-fold tie at regret 0, below every threshold; checked once
            best, reg, per = _rank_cell([0.0] * P, CP.THR4)
            assert not any(best) and not any(reg) and not any(s or y or z for so, y, z in per for s in so)
            assert not got['best'][:, dead].any() and not got['reg'][:, dead].any() and not got['sole'][:, :, dead].any()
            assert not got['any'][:, dead].any() and not got['all'][:, dead].any()
            rows = [[0] * K for _ in range(P)]
            for c in live.tolist():
                col = a[:, c].tolist()
                best, reg, per = _rank_cell(col, CP.THR4)
                assert got['best'][:, c].tolist() == best and got['reg'][:, c].tolist() == reg, (mem[0], e, c)
                for k, (sole, any_, all_) in enumerate(per):
                    assert got['sole'][k, :, c].tolist() == sole and got['any'][k, c] == any_ and got['all'][k, c] == all_
                    for j in range(P):
                        rows[j][k] += col[j] >= CP.THR4[k]
                seen += 1
            assert got['rows'].tolist() == rows
    assert seen > 5000


def test_contrast_restatement_equals_a_loop_over_python_floats():
    N = 65
    K = len(CP.THR4)
    seen = 0
    for mem in CP.pair_members(N):
        for e in range(CP.NENTRY):
            ab = CP.values(mem, e)
            got = CP.contrast_planes(ab, CP.THR4)
            rows = [[0] * K, [0] * K]
            for c in range(N * N):
                a, b = ab[:, c].tolist()
                d = a - b
                assert got['d'][c] == d and got['pos'][c] == (d > 0) and got['neg'][c] == (d < 0)
                for k, t in enumerate(CP.THR4):
                    assert got['gain'][k, c] == (a >= t and b < t) and got['loss'][k, c] == (b >= t and a < t)
                    rows[0][k] += a >= t
                    rows[1][k] += b >= t
                seen += int(a != 0 or b != 0)
            assert got['rows'].tolist() == rows
    assert seen > 3000


# ---- every altered rule changes the reference -------------------------------------------------------------------------

def _same(x, y):
    return all(np.array_equal(x[k], y[k]) for k in x)


def _told(members, planes, rule):
    return [m[0] + ':' + m[2] + ':%d' % e for m in members for e in range(CP.NENTRY)
            if not _same(planes(CP.values(m, e), CP.THR4), planes(CP.values(m, e), CP.THR4, rule))]


def _chunk_told(members, P, S):
    """the any_0 planes of a handle of S slots, the true launch against the one that writes to slot - chunk"""
    ent = [sum(m[3] * CP.rank_planes(CP.values(m, e), CP.THR4)['any'][0].astype(np.int64) for m in members)
           for e in range(CP.NENTRY)]
    true, alt = CP.assemble(ent, S), CP.assemble(ent, S, CP.rank_chunk(P))
    return any(not np.array_equal(x, y) for x, y in zip(true, alt))


@pytest.mark.parametrize('N', CP.SIZES)
def test_every_altered_rule_changes_the_reference(N):
    blind = []
    for P in (CP.PLANS if N == 65 else (8,)):
        zoo, bump = CP.plan_members(N, P), CP.bump_plans(N, P)
        for rule, text in CP.RANK_RULES.items():
            if rule == 'chunk':
                S = CP.rank_chunk(P) + 1
                if S > 32:          # two and three plans fit 32 slots, the cap, in one launch: the rule cannot occur
                    continue
                told, smooth = _chunk_told(zoo, P, S), _chunk_told(bump, P, S)
            else:
                told, smooth = _told(zoo, CP.rank_planes, rule), _told(bump, CP.rank_planes, rule)
            assert told, (P, text)
            if not smooth:
                blind.append('rank P = %d: %s' % (P, text))
    zoo, bump = CP.pair_members(N), CP.bump_pairs(N)
    for rule, text in CP.CONTRAST_RULES.items():
        assert _told(zoo, CP.contrast_planes, rule), text
        if not _told(bump, CP.contrast_planes, rule):
            blind.append('contrast: ' + text)
    print('N = %d: smooth bumps cannot tell these altered rules from the true ones:' % N)
    for b in blind:
        print('   ', b)
    want = ['rank P = %d: %s' % (P, CP.RANK_RULES[rule]) for P in (CP.PLANS if N == 65 else (8,))
            for rule in ('gt', 'tail_twice')] + ['contrast: ' + CP.CONTRAST_RULES[r] for r in ('gt', 'gain_le', 'tail_twice')]
    assert blind == want
    assert len(set(CP.RANK_RULES) | set(CP.CONTRAST_RULES)) == 12


# ---- the restated moments against the exact ones ----------------------------------------------------------------------

def test_restated_moments_against_the_exact_moments():
    worst = [0.0, 0.0]
    plain_differs = inf_cells = first2 = 0
    for N in CP.SIZES:
        moms = [(CP.contrast_reference(N), None)] + [(CP.rank_reference(N, P), P) for P in CP.PLANS]
        for ref, P in moms:
            for ent in ref:
                for mom in (ent['mom'] if P else [ent['mom']]):
                    at = mom['at']
                    for key in ('plain', 'fused', 'ab', 'ba'):
                        mean, M2 = mom[key][0][at], mom[key][1][at]
                        assert (M2 >= 0).all()
                        em, eq = CP.moment_errors(mean.tolist(), M2.tolist(), mom['exact'])
                        worst = [max(worst[0], em), max(worst[1], eq)]
                    assert np.array_equal(mom['plain'][0], mom['fused'][0])
                    plain_differs += int((mom['plain'][1] != mom['fused'][1]).sum())
                    inf_cells += int(np.isinf(mom['fused'][1]).sum())
                    first2 += int(mom['first2'][1].any())
    print('restated regret and difference moments vs exact: mean %.4f, M2 %.4f units' % tuple(worst))
    # two identical members leave M2 == 0 everywhere; the fused M2 is not the plain one; the ties at 1e300 overflow
    assert first2 == 0 and plain_differs > 1000 and inf_cells > 100
    assert CP.MEAN_ERR / 2 <= worst[0] <= 2 * CP.MEAN_ERR and CP.M2_ERR / 2 <= worst[1] <= 2 * CP.M2_ERR


def test_fma_and_exact_moments_take_what_the_plans_need():
    inf = float('inf')
    assert CF.fma(3e300, 1e300, 0.0) == inf and CF.fma(-3e300, 1e300, 0.0) == -inf and CF.fma(2.0, 3.0, inf) == inf
    assert CF.fma(1e-300, 1e-300, 0.0) == 0.0 and CF.fma(3.0, 1.0 / 3.0, -1.0) == -2.0 ** -54
    V = np.array([[1.5, -2.0], [-0.5, -2.0], [2.0, 4.0]])
    mean, M2, um, uq = CF.exact_moments(V, [1, 2, 1])
    F = CF.Fraction
    assert mean.tolist() == [F(5, 8), F(-1, 2)] and M2.tolist() == [F(4 * 27 - 25, 16), F(27)]
    assert um.tolist() == [F(2, 2 ** 53), F(4, 2 ** 53)] and uq.tolist() == [F(27, 4 * 2 ** 53), F(28, 2 ** 53)]


# ---- the release plans ------------------------------------------------------------------------------------------------

def test_ring_and_shifts():
    N = 9
    f = CP.ring(N)
    border = np.ones((N, N), dtype=bool)
    border[1:-1, 1:-1] = False
    assert (f[border] > 0).all() and len(set(f[f > 0].tolist())) == int((f > 0).sum())
    for plan in CP.ring_plans(N):
        want = np.zeros((N, N))
        for dr, dc, amount in plan:
            for r in range(N):
                for c in range(N):
                    if 0 <= r - dr < N and 0 <= c - dc < N:
                        want[r, c] = want[r, c] + amount * f[r - dr, c - dc]
        assert np.array_equal(CP.sites_expected(f, plan), want)
        # what a flat-index shift would bring in from the neighbouring row is not there
        dr, dc, _a = plan[0]
        if len(plan) == 1 and dc:
            flat = np.zeros(N * N)
            k = dr * N + dc
            src = f.ravel()
            flat[max(k, 0):N * N + min(k, 0)] = src[max(-k, 0):N * N - max(k, 0)]
            assert not np.array_equal(flat.reshape(N, N), want)

"""CPU tests of the core-range maps: the restatement of the ps_range statements in tests/range_ref.py against a
sort-and-cumulate on Python integers, ties, single cells, empty slots, the exponent's edges, tiny fields (the
scalbn path), scale invariance, the invariants of the level, the device's radix route restated for several pass
widths, and the host side of predictive.RangeMaps: check_core_range, the area quantiles, the merge order of the
member tables as the driver relies on it.  No device."""
import math
from fractions import Fraction

import numpy as np
import pytest

from range_ref import (accumulate, brute_levels, exponent, integer_mass, member_levels, needed_mass, radix_levels)

FR = [0.5, 0.95]
FR4 = [0.1, 0.5, 0.9, 0.99]


def _field(n, seed, zero_share=0.0, spread=6.0):
    rng = np.random.default_rng(seed)
    f = np.exp(rng.normal(0.0, spread, (n, n)))
    f[rng.random((n, n)) < zero_share] = 0.0
    return f


def _check_invariants(field, fractions):
    lam, n, Q, E, sets = member_levels(field, fractions)
    q, Q2, E2 = integer_mass(field)
    assert (Q, E) == (Q2, E2)
    v = np.asarray(field)
    for j, p in enumerate(fractions):
        need = needed_mass(p, Q)
        assert Fraction(need) >= Fraction(float(p)) * Q > Fraction(need - 1)
        inside = int(q[v >= lam[j]].sum(dtype=np.uint64))
        open_ = int(q[v > lam[j]].sum(dtype=np.uint64))
        assert inside >= need > open_, (j, inside, need, open_)
        assert (v == lam[j]).any() and n[j] == int((v >= lam[j]).sum()) == int(sets[j].sum())
        if j:
            assert lam[j] <= lam[j - 1] and not (sets[j - 1] & ~sets[j]).any()
    return lam, n, Q, E, sets


@pytest.mark.parametrize('n,seed,zero_share', [(5, 1, 0.0), (5, 2, 0.6), (9, 3, 0.0), (9, 4, 0.7), (9, 5, 0.9),
                                               (16, 6, 0.3)])
def test_levels_match_a_sort_and_cumulate_on_python_integers(n, seed, zero_share):
    f = _field(n, seed, zero_share)
    for fr in (FR, FR4, [2.0 ** -40], [1.0 - 2.0 ** -53]):
        lam, cells, Q, E, _sets = _check_invariants(f, fr)
        blam, bn, bQ, bE = brute_levels(f, fr)
        assert lam.tolist() == blam and cells.tolist() == bn and (Q, E) == (bQ, bE)


def test_a_plateau_at_the_level_enters_whole():
    f = np.zeros((6, 6))
    f[0, :3] = [8.0, 4.0, 4.0]
    f[1:3, :] = 1.0                  # a plateau of 12 cells, mass 12 of 28
    lam, n, Q, E, sets = _check_invariants(f, [0.5, 0.6, 0.99])
    assert E == 3 and Q == 28 << 33
    assert lam.tolist() == [4.0, 1.0, 1.0] and n.tolist() == [3, 15, 15]      # 16/28 >= 0.5; then the plateau
    assert sets[1].sum() == 15 and np.array_equal(sets[1], sets[2])
    assert brute_levels(f, [0.5, 0.6, 0.99])[:2] == ([4.0, 1.0, 1.0], [3, 15, 15])


def test_a_single_live_cell_is_its_own_level_for_every_fraction():
    f = np.zeros((5, 5))
    f[3, 1] = 0.37
    lam, n, Q, E, sets = member_levels(f, FR4 + [1.0 - 2.0 ** -53])
    assert np.all(lam == 0.37) and np.all(n == 1) and E == -2 and Q == int(0.37 * 2.0 ** 38)
    assert sets.sum() == 5 and sets[:, 3, 1].all()


def test_an_empty_slot_counts_nothing():
    for f in (np.zeros((5, 5)), -np.ones((4, 4)), np.full((3, 3), np.nan)):
        lam, n, Q, E, sets = member_levels(f, FR)
        assert np.all(np.isinf(lam)) and np.all(lam > 0) and not n.any() and (Q, E) == (0, 0) and not sets.any()
    acc = accumulate([[np.zeros((5, 5)), _field(5, 7)]], [3], FR)
    assert not acc['counts'][:, 0].any() and acc['counts'][:, 1].max() == 3
    assert radix_levels(np.zeros((5, 5)), FR) == ([math.inf, math.inf], 0, 0)
    f = _field(5, 7)
    g = f.copy()
    g[0, 0], g[1, 1] = np.inf, -np.inf                  # a cell that is not finite has no mass and lies in no set
    f[0, 0] = f[1, 1] = 0.0
    a, b = member_levels(f, FR4), member_levels(g, FR4)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not b[4][:, 0, 0].any()
    assert brute_levels(g, FR4) == brute_levels(f, FR4) and radix_levels(g, FR4) == radix_levels(f, FR4)


def test_the_exponent_at_a_power_of_two_and_its_lower_neighbour():
    assert exponent(4.0) == 2 and exponent(np.nextafter(4.0, 0.0)) == 1 and exponent(1.0) == 0
    assert exponent(np.nextafter(1.0, 0.0)) == -1 and exponent(5e-324) == -1074 and exponent(2.0 ** -1022) == -1022
    base = _field(9, 8, 0.3, spread=2.0)
    base = base / base.max()
    for top in (4.0, np.nextafter(4.0, 0.0)):
        f = base * 3.0
        f[4, 4] = top
        q, Q, E = integer_mass(f)
        assert E == exponent(top) and int(q.max()) == int(Fraction(float(top)) * Fraction(2) ** (36 - E)) < 2 ** 37
        assert int(q.max()) >= 2 ** 36
        _check_invariants(f, FR4)
        assert member_levels(f, FR4)[0].tolist() == brute_levels(f, FR4)[0]


def test_tiny_fields_go_through_scalbn_not_a_multiplication():
    f = _field(9, 9, 0.4, spread=3.0) * 1e-306
    f[0, 0] = 5e-324                              # the smallest subnormal: mass 0 unless the maximum is tiny too
    with np.errstate(over='ignore'):
        assert not np.isfinite(np.float64(2.0) ** np.float64(36 - exponent(f.max())))   # the factor overflows
    lam, n, Q, E, _sets = _check_invariants(f, FR4)
    assert E < -1000 and 2 ** 36 <= Q < 2 ** 62
    assert lam.tolist() == brute_levels(f, FR4)[0] == radix_levels(f, FR4)[0]
    g = np.zeros((5, 5))
    g[1, 1:4] = [5e-324, 1e-323, 1.5e-323]         # a subnormal maximum: E from its leading bit
    lam, n, Q, E, _sets = _check_invariants(g, [0.5, 0.8])
    assert E == -1073 and Q == (1 + 2 + 3) << 35 and lam.tolist() == [1.5e-323, 1e-323] and n.tolist() == [1, 2]
    assert radix_levels(g, [0.5, 0.8]) == ([1.5e-323, 1e-323], Q, E)


def test_scaling_the_field_by_a_power_of_two_leaves_every_set_unchanged():
    f = _field(9, 10, 0.5)
    lam, n, Q, E, sets = member_levels(f, FR4)
    for k in (-600, -17, 1, 40, 600):
        lam2, n2, Q2, E2, sets2 = member_levels(np.ldexp(f, k), FR4)
        assert np.array_equal(sets, sets2) and np.array_equal(n, n2) and E2 == E + k
        assert np.array_equal(lam2, np.ldexp(lam, k))
        assert Q2 == Q or k < -500                # the masses are the same integers unless values turn subnormal


@pytest.mark.parametrize('bits', [4, 8, 10, 11, 12])
def test_the_radix_route_gives_the_same_level_for_any_pass_width(bits):
    fields = [_field(9, 11, 0.5), _field(12, 12, 0.0, spread=0.01), _field(5, 13, 0.8), np.ldexp(_field(7, 14), -1040)]
    plateau = np.ones((6, 6))
    plateau[0, 0] = 3.0
    for f in fields + [plateau]:
        for fr in (FR, FR4, [2.0 ** -40, 1.0 - 2.0 ** -53]):
            lam, _n, Q, E, _sets = member_levels(f, fr)
            assert radix_levels(f, fr, bits) == (lam.tolist(), Q, E)


def test_needed_mass_is_the_exact_ceiling():
    assert needed_mass(0.5, 7) == 4 and needed_mass(0.5, 8) == 4 and needed_mass(0.1, 10) == 2   # 0.1 > 1/10
    assert needed_mass(0.3, 10) == 3                                                               # 0.3 < 3/10
    assert needed_mass(5e-324, 2 ** 61) == 1 and needed_mass(1.0 - 2.0 ** -53, 2 ** 61) == 2 ** 61 - 2 ** 8


def test_check_core_range_refuses_before_any_evaluation():
    from parasitoids_amd.predictive import check_core_range, check_range_fractions, posterior_predictive
    assert check_core_range([0.5, 0.95]) == ([0.5, 0.95], [0.5, 0.9])
    assert check_core_range(dict(fractions=(0.25,), levels=[1.0, 0.1]), days=[0, 3]) == ([0.25], [1.0, 0.1])
    for bad in ([0.0, 0.5], [0.5, 1.0], [float('nan')], [0.95, 0.5], [0.5, 0.5], [0.1, 0.2, 0.3, 0.4, 0.5], [],
                ['a'], 0.5, [-0.1], [float('inf')]):
        with pytest.raises(ValueError):
            check_core_range(bad)
        with pytest.raises(ValueError):
            check_core_range(dict(fractions=bad))
    for bad in (dict(levels=[0.5]), dict(fractions=[0.5], level=[0.5]), dict(fractions=[0.5], levels=[0.0]),
                dict(fractions=[0.5], levels=[1.5]), dict(fractions=[0.5], levels=[]),
                dict(fractions=[0.5], levels=['x'])):
        with pytest.raises(ValueError):
            check_core_range(bad)
    for days in ([], [3, 1], [-1, 2], list(range(33))):
        with pytest.raises(ValueError):
            check_core_range([0.5], days=days)
    with pytest.raises(ValueError):
        check_range_fractions([0.5, float('nan')])

    def never(theta):
        raise AssertionError('evaluated')
    trace = (np.zeros((3, 1)), ['x'])
    with pytest.raises(ValueError, match='evaluate'):
        posterior_predictive(None, trace, evaluate=never, core_range=[0.5])
    with pytest.raises(ValueError, match='fraction'):
        posterior_predictive(None, trace, core_range=[0.5, 1.5])
    with pytest.raises(ValueError, match='days'):
        posterior_predictive(None, trace, core_range=[0.5], days=[2, 1])


def test_area_is_the_weighted_mean_and_lower_quantiles_of_the_cell_counts():
    from parasitoids_amd.predictive import range_area, weighted_lower_quantile
    cells, w = [10, 40, 20, 30], [1, 1, 6, 2]
    a = range_area(cells, w, 25.0, (0.05, 0.5, 0.95), day=4)
    assert a['day'] == 4 and a['mean'] == (10 + 40 + 120 + 60) / 10 * 25.0
    assert a['quantiles'] == [10 * 25.0, 20 * 25.0, 40 * 25.0]
    assert a['quantiles'] == [float(weighted_lower_quantile(cells, w, p)) * 25.0 for p in (0.05, 0.5, 0.95)]
    assert a['radius_mean'] == math.sqrt(a['mean'] / math.pi)
    assert a['radius_quantiles'] == [math.sqrt(x / math.pi) for x in a['quantiles']]
    assert set(a) == {'day', 'mean', 'quantiles', 'radius_mean', 'radius_quantiles'}
    assert range_area([5, 5], [3, 4], 2.0, [1.0])['quantiles'] == [10.0]
    with pytest.raises(ValueError):
        range_area([], [], 1.0)
    with pytest.raises(ValueError):
        range_area([1], [1], 1.0, [0.0])


def test_member_tables_follow_the_merge_order_and_counts_do_not():
    fields = [[_field(7, 20 + m, 0.4), _field(7, 30 + m, 0.4)] for m in range(4)]
    w = [1, 3, 2, 5]
    whole = accumulate(fields, w, FR)
    a, b = accumulate(fields[:2], w[:2], FR), accumulate(fields[2:], w[2:], FR)
    assert np.array_equal(a['counts'] + b['counts'], whole['counts'])
    assert np.array_equal(b['counts'] + a['counts'], whole['counts'])
    for key in ('lam', 'n', 'Q', 'E'):
        assert np.array_equal(np.concatenate([a[key], b[key]]), whole[key])
        swapped = np.concatenate([b[key], a[key]])
        assert np.array_equal(swapped, np.concatenate([whole[key][2:], whole[key][:2]]))
    assert whole['counts'].max() <= sum(w) and (whole['counts'][0] <= whole['counts'][1]).all()

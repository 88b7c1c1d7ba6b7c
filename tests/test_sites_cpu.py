"""CPU tests of the release plans (predictive.ReleaseSites): metres to cells, every refusal of the plain-Python
checks, which (group, output) pairs are "not released yet", posterior_predictive refusing a bad plan before
any evaluation, and the numpy reference (sites_ref) against a case worked out by hand."""
import types

import numpy as np
import pytest

from sites_ref import plan_fields, shifted


def _model(ndays=6, R=64, **kw):
    """what the checks read of a PopModel"""
    m = types.SimpleNamespace(rad_dist=10000.0, rad_res=R, days=list(range(100, 100 + ndays)), r_number=130000,
                              prob_model=False, device=None)
    m.__dict__.update(kw)
    return m


def test_metres_become_cells_with_north_up():
    from parasitoids_amd.predictive import check_sites, site_groups
    res = 10000.0 / 64                                     # 156.25 m
    got = check_sites([(0, 0, 1), (2 * res, 3 * res, 0.5), (-res, -4 * res, 2.0, 3), (0.49 * res, 0.51 * res, 1e-3),
                       (1.5 * res, 2.5 * res, 1.0)], 10000.0, 64)
    assert [(s['drow'], s['dcol']) for s in got] == [(0, 0), (-3, 2), (4, -1), (-1, 0), (-2, 2)]   # half to even
    assert [s['lag'] for s in got] == [0, 0, 3, 0, 0] and got[2]['amount'] == 2.0 and got[1]['east'] == 2 * res
    assert site_groups(got) == [(0, [0, 1, 3, 4]), (3, [2])]
    # east moves the column up, north moves the row down: the cell convention of Data_Import.LocInfo
    assert check_sites([(1000.0, 0.0, 1)], 10000.0, 100)[0]['dcol'] == 10
    assert check_sites([(0.0, 1000.0, 1)], 10000.0, 100)[0]['drow'] == -10
    edge = check_sites([(20000.0, -20000.0, 1)], 10000.0, 64)[0]
    assert (edge['drow'], edge['dcol']) == (128, 128)      # |offset| = N - 1 is the last one allowed
    assert 'drow' not in check_sites([(1e9, 0, 1)], None, None)[0]      # no model: no cells, no offset check


@pytest.mark.parametrize('sites, match', [
    ([], 'release sites'),
    ([(0, 0, 1)] * 33, 'release sites'),
    (5, 'must be a list'),
    ([(0, 0)], 'expected'),
    ([(0, 0, 1, 0, 0)], 'expected'),
    ([(0, 0, 0.0)], 'amount'),
    ([(0, 0, -1.0)], 'amount'),
    ([(0, 0, float('nan'))], 'amount'),
    ([(0, 0, float('inf'))], 'amount'),
    ([(float('inf'), 0, 1)], 'not finite'),
    ([(0, 0, 'x')], 'numbers'),
    ([(0, 0, 1, 1.5)], 'whole number'),
    ([(0, 0, 1, -1)], 'negative'),
    ([(0, 0, 1, 1), (0, 0, 1, 2)], 'smallest lag must be 0'),
    ([(0, 0, 1, k) for k in range(9)], 'different release days'),
    ([(20000.0 + 156.25, 0, 1)], 'beyond the 129 x 129 domain'),       # dcol = 129 = N
    ([(0, -(20000.0 + 156.25), 1)], 'beyond the 129 x 129 domain'),    # drow = 129
])
def test_bad_sites_are_refused(sites, match):
    from parasitoids_amd.predictive import check_sites
    with pytest.raises(ValueError, match=match):
        check_sites(sites, 10000.0, 64)


def test_the_limits_themselves_pass():
    from parasitoids_amd.predictive import check_site_days, check_sites, site_groups
    assert len(check_sites([(0, 0, 1)] * 32, 10000.0, 64)) == 32
    assert len(site_groups(check_sites([(0, 0, 1, k) for k in range(8)], 10000.0, 64))) == 8
    assert check_site_days(range(32)) == list(range(32))


def test_days_of_a_plan():
    from parasitoids_amd.predictive import check_site_days
    assert check_site_days([0, 2, 5], 6) == [0, 2, 5]
    for bad, match in (([], 'output days'), (range(33), 'output days'), ([2, 2], 'strictly increasing'),
                       ([3, 1], 'strictly increasing'), ([-1, 0], 'strictly increasing'), ([0, 6], 'asks for day 6'),
                       (['x'], 'model days'), (3, 'model days')):
        with pytest.raises(ValueError, match=match):
            check_site_days(bad, 6)


def test_slot_planning_marks_groups_that_are_not_released_yet():
    from parasitoids_amd.predictive import site_slots
    assert site_slots([0, 2, 3], [0, 1, 2, 3, 5]) == [[0, 1, 2, 3, 5],
                                                      [None, None, 0, 1, 3],
                                                      [None, None, None, 0, 2]]
    assert site_slots([0, 4], [4]) == [[4], [0]]           # released on the output day itself: its day 0
    with pytest.raises(ValueError, match='beyond the last output day'):
        site_slots([0, 4], [0, 3])


def test_lagged_models_are_checked():
    from parasitoids_amd.predictive import check_lagged
    base = _model()
    ok = _model(days=base.days[2:])
    assert check_lagged(base, [0], None) == {}
    assert check_lagged(base, [0, 2], {2: ok, 4: None}) == {2: ok}
    with pytest.raises(ValueError, match=r'no model for the release 2 days'):
        check_lagged(base, [0, 2], {})
    with pytest.raises(ValueError, match=r'no model for the release 2 days'):
        check_lagged(base, [0, 2], {3: ok})
    with pytest.raises(ValueError, match=r'not over the base model'):
        check_lagged(base, [0, 2], {2: _model(days=base.days[1:])})
    with pytest.raises(ValueError, match=r'not over the base model'):
        check_lagged(base, [0, 2], {2: _model()})
    for name, other in (('rad_dist', 8000.0), ('rad_res', 128), ('r_number', 1.0), ('prob_model', True),
                        ('device', 1)):
        with pytest.raises(ValueError, match=r'lagged\[2\]\.' + name):
            check_lagged(base, [0, 2], {2: _model(days=base.days[2:], **{name: other})})
    with pytest.raises(ValueError, match="beyond the model's 6 days"):
        check_lagged(base, [0, 6], {6: ok})


def test_the_plan_argument_of_posterior_predictive():
    from parasitoids_amd.predictive import sites_plan
    sites, days, lags = sites_plan(dict(sites=[(0, 0, 0.6), (2000, 0, 0.4), (0, -2000, 0.5, 4)]), _model(ndays=6))
    assert days == list(range(6)) and lags == [0, 4] and [s['dcol'] for s in sites] == [0, 13, 0]
    assert sites_plan(dict(sites=[(0, 0, 1)], days=[1, 3]))[1:] == ([1, 3], [0])
    assert sites_plan(dict(sites=[(0, 0, 1)]))[1] is None            # no model: the days are not known yet
    for bad, match in (([(0, 0, 1)], 'sites must be dict'), (dict(days=[0]), 'sites must be dict'),
                       (dict(sites=[(0, 0, 1)], when=3), 'sites must be dict'),
                       (dict(sites=[(0, 0, 1), (0, 0, 1, 6)]), "beyond the model's 6 days"),
                       (dict(sites=[(0, 0, 1), (0, 0, 1, 4)], days=[0, 3]), 'beyond the last output day'),
                       (dict(sites=[(0, 0, 1)], days=[0, 6]), 'asks for day 6'),
                       (dict(sites=[(0, 0, 1)], days=list(range(33))), 'output days'),
                       (dict(sites=[(20200.0, 0, 1)]), 'beyond the 129 x 129 domain')):
        with pytest.raises(ValueError, match=match):
            sites_plan(bad, _model(ndays=6))


def test_posterior_predictive_refuses_a_bad_plan_before_evaluating():
    from parasitoids_amd.predictive import posterior_predictive
    calls = []
    trace = np.zeros((3, 1))

    def evaluate(theta):
        calls.append(theta)
        return None
    for sites in ([(0, 0, 1)], dict(sites=[]), dict(sites=[(0, 0, -1.0)]), dict(sites=[(0, 0, 1, 1)]),
                  dict(sites=[(0, 0, 1)], days=[3, 3]), dict(sites=[(0, 0, 1)], days=list(range(33))),
                  dict(sites=[(0, 0, 1), (0, 0, 1, 5)], days=[0, 4])):
        with pytest.raises(ValueError, match='sites must be|release sites|amount|smallest lag|increasing|output days|'
                                             'beyond the last output day'):
            posterior_predictive(None, (trace, ['x']), evaluate=evaluate, sites=sites)
    # with a model at hand also what only the model can tell: a lag beyond its days, a site outside its domain
    for sites in (dict(sites=[(0, 0, 1), (0, 0, 1, 6)]), dict(sites=[(0, 0, 1)], days=[0, 6]),
                  dict(sites=[(0, 30000.0, 1)])):
        with pytest.raises(ValueError, match="beyond the model's 6 days|asks for day 6|beyond the 129 x 129 domain"):
            posterior_predictive(_model(ndays=6), (trace, ['x']), evaluate=evaluate, sites=sites)
    assert not calls


def test_shift_cannot_wrap():
    f = np.arange(1.0, 26.0).reshape(5, 5)
    assert np.array_equal(shifted(f, 0, 0), f)
    east = shifted(f, 0, 2)                                # two columns to the east: the last two columns are gone
    assert np.array_equal(east[:, 2:], f[:, :3]) and not east[:, :2].any()
    assert east.sum() < f.sum()
    flat = np.roll(f.ravel(), 2).reshape(5, 5)             # the flat-index shift puts them onto the next row's west end
    assert flat[1, 0] == f[0, 3] and east[1, 0] == 0.0
    nw = shifted(f, -1, -3)
    assert np.array_equal(nw[:4, :2], f[1:, 3:]) and not nw[4].any() and not nw[:, 2:].any()
    assert not shifted(f, 5, 0).any() and not shifted(f, 0, -5).any()
    assert shifted(f, 4, -4)[4, 0] == f[0, 4] and np.count_nonzero(shifted(f, 4, -4)) == 1


def test_reference_against_a_hand_computed_case():
    """5 x 5, three output days, two sites on day 0 and one released a day later from a model of its own"""
    a = np.zeros((3, 5, 5))
    a[0, 2, 2] = 8.0                                       # the release, then a plume drifting east
    a[1, 2, 2], a[1, 2, 3] = 4.0, 2.0
    a[2, 2, 2], a[2, 2, 3], a[2, 2, 4] = 2.0, 2.0, 1.0
    b = np.zeros((2, 5, 5))                                # the later release: other wind, drifting south
    b[0, 2, 2] = 8.0
    b[1, 2, 2], b[1, 3, 2] = 3.0, 5.0
    sites = [(0, 0, 1.0, 0), (-1, 1, 0.5, 0), (2, 0, 0.25, 1)]
    Y = plan_fields({0: a, 1: b}, sites, [0, 1, 2])
    want = np.zeros((3, 5, 5))
    want[0, 2, 2], want[0, 1, 3] = 8.0, 4.0                # day 0: the first two sites alone
    want[1, 2, 2], want[1, 2, 3] = 4.0, 2.0
    want[1, 1, 3], want[1, 1, 4] = 2.0, 1.0
    want[1, 4, 2] = 2.0                                    # the later site's day 0, two rows south
    want[2, 2, 2], want[2, 2, 3], want[2, 2, 4] = 2.0, 2.0, 1.0
    want[2, 1, 3], want[2, 1, 4] = 1.0, 1.0                # its east-most cell (1, 5) has left the domain
    want[2, 4, 2] = 0.75                                   # and the later site's (5, 2) has left in the south
    assert np.array_equal(Y, want)
    assert Y[2].sum() < a[2].sum() + 0.5 * a[2].sum() + 0.25 * b[1].sum()
    # only the outputs asked for, in their order; a site released on the output day shows its day 0
    assert np.array_equal(plan_fields({0: a, 1: b}, sites, [1]), want[1:2])
    assert np.array_equal(plan_fields({0: a, 1: b}, sites, [0, 2]), want[[0, 2]])
    # the sum is taken site by site in the order given, product and sum rounded separately
    c = np.full((1, 1, 1), 0.1)
    got = plan_fields({0: c}, [(0, 0, 3.0, 0), (0, 0, 0.7, 0), (0, 0, 1e-17, 0)], [0])
    assert got[0, 0, 0] == (0.0 + 3.0 * 0.1) + 0.7 * 0.1 + 1e-17 * 0.1

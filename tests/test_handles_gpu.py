"""GPU tests of the lifetime of the fifteen classes that own one handle of the C library (_handle._Handle): each is
opened on the device, used once and closed, by hand and by `with`; afterwards it holds no handle and a second close
does nothing.  A SpreadSummary fed before all that and one fed after it hold the same planes bit for bit: no handle
that came and went touched the model's records or another handle's memory.  No closed handle is handed to the library.
R = 128, 6 days, one evaluation (the first member of test_arrival_gpu.py)."""
import numpy as np
import pytest

from test_arrival_gpu import MEMBERS, THR, _evaluate, _pop_model

pytestmark = pytest.mark.gpu

DAYS = [0, 2, 5]


@pytest.fixture(scope='module')
def pm():
    model = _pop_model()
    _evaluate(model, MEMBERS[0])
    yield model
    model.close()


def _sources(pm):
    """two projections and two plans with the same outputs, applied to the evaluation"""
    from parasitoids_amd import predictive as PP
    out = {'project': [PP.Projection(pm, w, [0, 1, 4]) for w in ([[1, 0, 1], [0, 0, 0], [0, 2, 0]],
                                                                 [[0, 1, 1], [0, 0, 0], [3, 0, 0]])],
           'sites': [PP.ReleaseSites(pm, s, DAYS) for s in ([(0, 0, 1.0), (1000, -500, 0.5)], [(-800, 300, 1.5)])]}
    for pair in out.values():
        for src in pair:
            src.apply()
    return out


def _cases(pm, src):
    """(name, open, use once) of every class, from the model and over a fields source"""
    from parasitoids_amd import laplace as LA
    from parasitoids_amd import mcmc
    from parasitoids_amd import predictive as PP
    theta = [m[2] for m in mcmc.MODEL_BLOCK]
    proj, plan = src['project'][0], src['sites'][0]
    add = lambda o: o.add(2)                               # noqa: E731
    apply_ = lambda o: o.apply()                           # noqa: E731
    return [
        ('SpreadSummary', lambda: PP.SpreadSummary(pm, DAYS, THR), add),
        ('SpreadSummary.for_projection', lambda: PP.SpreadSummary.for_projection(proj, THR), add),
        ('SpreadHistogram', lambda: PP.SpreadHistogram(pm, DAYS), add),
        ('SpreadHistogram.for_projection', lambda: PP.SpreadHistogram.for_projection(plan), add),
        ('ArrivalMaps', lambda: PP.ArrivalMaps(pm, THR, DAYS), add),
        ('ArrivalMaps.for_projection', lambda: PP.ArrivalMaps.for_projection(plan, THR), add),
        ('PeakMaps', lambda: PP.PeakMaps(pm, THR, DAYS), add),
        ('PeakMaps.for_projection', lambda: PP.PeakMaps.for_projection(proj, THR), add),
        ('ExcursionMaps', lambda: PP.ExcursionMaps(pm, THR, DAYS), add),
        ('ExcursionMaps.for_projection', lambda: PP.ExcursionMaps.for_projection(plan, THR), add),
        ('RangeMaps', lambda: PP.RangeMaps(pm, [0.5, 0.95], DAYS), add),
        ('RangeMaps.for_projection', lambda: PP.RangeMaps.for_projection(proj, [0.5]), add),
        ('Projection', lambda: PP.Projection(pm, [[1, 1]], [1, 2]), apply_),
        ('ReleaseSites', lambda: PP.ReleaseSites(pm, [(0, 0, 1.0)], DAYS), apply_),
        ('PlanContrast of projections', lambda: PP.PlanContrast(*src['project'], THR), add),
        ('PlanContrast of plans', lambda: PP.PlanContrast(*src['sites'], THR), add),
        ('SensitivityMaps', lambda: PP.SensitivityMaps(pm, ['sig_x', 'lam'], DAYS), lambda o: o.add(theta, 2)),
        ('SensitivityMaps.for_projection', lambda: PP.SensitivityMaps.for_projection(plan, ['lam']),
         lambda o: o.add(theta, 2)),
        ('MonteCarloError', lambda: PP.MonteCarloError(pm, 3, DAYS, THR), add),
        ('MonteCarloError.for_projection', lambda: PP.MonteCarloError.for_projection(proj, 3, THR), add),
        ('ReweightedSummary', lambda: PP.ReweightedSummary(pm, ['a', 'b'], DAYS, THR), lambda o: o.add([0.0, -1.0], 2)),
        ('ReweightedSummary.for_projection', lambda: PP.ReweightedSummary.for_projection(plan, ['a'], THR),
         lambda o: o.add([-0.5], 2)),
        ('CatchFields', lambda: PP.CatchFields(pm, [(2, 0.01), (5, 0.02, 2)]), apply_),
        ('CatchFields.for_projection', lambda: PP.CatchFields.for_projection(plan, [(2, 0.01)]), apply_),
        ('InformationFields', lambda: PP.InformationFields(pm, [(2, 0.01), (5, 0.02, 1)]), apply_),
        ('InformationFields.for_projection', lambda: PP.InformationFields.for_projection(proj, [(0, 0.01)]), apply_),
        ('LinearisedSpread', lambda: LA.LinearisedSpread(pm, DAYS, 2, THR, ['sig_x', 'lam']),
         lambda o: (o.set_center(), o.add(1, 0.25))),
    ]


def _planes(summary):
    return np.array([summary.fetch_slot(s, what) for s in range(len(DAYS)) for what in range(2 + len(THR))])


def test_every_class_opens_is_used_once_and_closes_and_leaves_the_others_alone(pm):
    from parasitoids_amd import predictive as PP
    with PP.SpreadSummary(pm, DAYS, THR) as first:
        first.add(2)
        before = _planes(first)
        src = _sources(pm)
        cases = _cases(pm, src)
        assert len({name.split('.')[0].split(' ')[0] for name, _open, _use in cases}) == 15
        for name, open_, use in cases:
            obj = open_()
            assert obj._h and obj._h.value, name
            use(obj)
            obj.close()
            assert not obj._h and obj._h.value is None, name
            obj.close()                                    # harmless
            assert not obj._h, name
            with open_() as obj:
                assert obj._h, name
                use(obj)
            assert not obj._h, name
        for pair in src.values():
            for s in pair:
                s.close()
                assert not s._h
        pm.solver.sync()
        with PP.SpreadSummary(pm, DAYS, THR) as second:
            second.add(2)
            after = _planes(second)
        assert np.array_equal(_planes(first), before)
        assert before.tobytes() == after.tobytes()
        assert first.members == 1 and first.total_weight == 2.0
    assert not first._h

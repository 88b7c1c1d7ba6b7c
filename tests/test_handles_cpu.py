"""CPU tests of the seventeen classes that own one handle of the C library (sixteen in parasitoids_amd.predictive and
laplace.LinearisedSpread): what each sends to the library, what it returns and what it refuses on the host.  No
device and no library: tests/golden/make_handle_trace.py puts a recording stand-in in `_lib._lib` and walks every
class through its life -- construction from the model and through every for_projection it has, one add or apply on
each path, merge, reset, the counters, profile, one accessor per fetch symbol, close twice, the `with` form, a create
the library refuses, and the refusals that never reach the library.  The expected trace
(tests/golden/handle_calls_trace.json) was recorded before the classes got their shared base (_handle._Handle), and
NeighbourhoodFields and ProximityFields before the field sources got theirs (_handle._FieldSource), so every symbol, argument, returned value, exception type and text here is the one the copied classes gave."""
import importlib.util
import json
import os

import pytest

from parasitoids_amd import _lib as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _recorder():
    spec = importlib.util.spec_from_file_location('make_handle_trace', os.path.join(GOLDEN, 'make_handle_trace.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()


@pytest.fixture(scope='module')
def traces():
    before = L._lib
    got = json.loads(REC.dumps(REC.record()))          # through JSON, as the fixture went
    assert L._lib is before                            # the stand-in is gone again
    with open(REC.FIXTURE) as f:
        return got, json.load(f)


def _scenarios():
    return ['%s over %s' % (name, over or 'the model') for name, spec in REC.specs().items() for over in spec['over']]


def test_fixture_covers_every_class_and_source(traces):
    got, want = traces
    assert list(got) == list(want) == _scenarios()
    assert len(REC.specs()) == 17
    # per class no larger than the driver's trace allowed the first fifteen
    driver = os.path.getsize(os.path.join(GOLDEN, 'predictive_driver_trace.json'))
    assert os.path.getsize(REC.FIXTURE) * 15 < driver * len(REC.specs())


@pytest.mark.parametrize('scenario', _scenarios())
def test_calls_values_and_refusals(traces, scenario):
    got, want = traces
    assert [s[0] for s in got[scenario]] == [s[0] for s in want[scenario]]
    for g, w in zip(got[scenario], want[scenario]):
        assert g == w, '%s, step %r' % (scenario, w[0])


@pytest.mark.parametrize('scenario', _scenarios())
def test_refused_create_leaves_no_handle_and_close_is_idempotent(traces, scenario):
    got, _want = traces
    steps = {s[0]: s for s in got[scenario]}
    label, calls, _value, error = steps['create refused']
    assert error[0] == 'HipError' and error[2] is False            # the object was found and holds no handle
    assert [c[0] for c in calls if c[0].endswith('_destroy')] == []
    assert steps['close'][2] == [None, False]
    assert [c[0].rsplit('_', 1)[1] for c in steps['close'][1]] == ['destroy']
    if 'close again' in steps:
        assert steps['close again'][1:] == [[], [None, False]]
        assert steps['with'][2] == [True, False]


def test_weight_and_model_both_wrong_reach_no_library():
    """Given both a weight below 1 and a model that is not evaluated far enough, the copied classes differed in
    which ValueError came; with the shared base the weight is refused first everywhere.  Nothing reaches the
    library and nothing is added either way -- the one case the trace leaves out."""
    from parasitoids_amd import predictive as PP
    shared = hasattr(PP.SpreadSummary, '_call')            # False for the copied classes the fixture was recorded from
    text = 'weight must be a positive integer' if shared else 'weight must be a positive integer|the last evaluation'
    with REC.stand_in() as lib:
        pm = REC.model()
        made = [PP.SpreadSummary(pm), PP.SpreadHistogram(pm), PP.ArrivalMaps(pm, [0.5]), PP.PeakMaps(pm),
                PP.ExcursionMaps(pm, [0.5]), PP.RangeMaps(pm, [0.5]), PP.MonteCarloError(pm, 3)]
        sens = PP.SensitivityMaps(pm, ['lam'])
        pm._nd = 3
        lib.calls = []
        for acc in made:
            with pytest.raises(ValueError, match=text):
                acc.add(0)
        with pytest.raises(ValueError, match=text):
            sens.add(REC.THETA, 0)
        assert sens.moments.W == 0 and sens.moments.members == 0
        assert lib.calls == []
        for acc in made + [sens]:
            acc.close()

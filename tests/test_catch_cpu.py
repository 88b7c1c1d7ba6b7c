"""CPU tests of the catch-probability maps: the numpy restatement of the kernel's statements (catch_ref) against
mpmath at 60 digits, the driver argument's checks, the required-rate step function and the command line's trap
parser.  No device is touched."""
import os

import numpy as np
import pytest

import catch_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (1, 2, 3, 5, 8, 16)


def _sweep(n):
    rng = np.random.default_rng(100 + n)
    return np.concatenate([10.0 ** rng.uniform(-12, 3, 160), rng.uniform(0, 40, 160),
                           [n, np.nextafter(float(n), 0.0), np.nextafter(float(n), 100.0), 700.0, 745.0, 746.0, 1e4]])


@pytest.mark.parametrize('n', COUNTS)
def test_the_restatement_against_mpmath(n):
    mu = _sweep(n)
    y = catch_ref.catch_value(mu, n)
    assert y.dtype == np.float64 and y.shape == mu.shape
    assert ((y >= 0.0) & (y <= 1.0)).all()
    err = catch_ref.rel_errors(y, mu, n)          # relative; absolute where the exact value is below 1e-290
    k = int(err.argmax())
    print('n = %d: largest error %.3g at mu = %.17g' % (n, err[k], mu[k]))
    assert err.max() <= 1e-14
    zero = catch_ref.catch_value(np.array([0.0, -0.0]), n)
    assert np.array_equal(zero, [0.0, 0.0]) and not np.signbit(zero).any()
    assert catch_ref.catch_value(np.array([1e4]), n)[0] == 1.0


def test_fields_restatement_uses_one_rounded_product():
    v = np.array([[0.0, 1e-8, 0.3], [2.5, 40.0, 1e3]])
    got = catch_ref.catch_fields(v, [0.5, 3.0], [1, 4])
    assert got.shape == (2, 2, 3)
    assert np.array_equal(got[1], catch_ref.catch_value(3.0 * v, 4))
    assert got[0, 0, 0] == 0.0 and got[1, 0, 0] == 0.0
    with pytest.raises(ValueError):
        catch_ref.catch_value(v, 17)


def test_check_catch_refusals():
    from parasitoids_amd.predictive import check_catch
    ok = check_catch(dict(traps=[(1, 0.5), (3, 2.0, 4)], levels=(0.5, 0.95)), 6)
    assert ok['traps'] == [(1, 0.5, 1), (3, 2.0, 4)] and ok['levels'] == [0.5, 0.95] and ok['emergence'] is None
    assert ok['given'] == {'traps': [[1, 0.5], [3, 2.0, 4]], 'levels': [0.5, 0.95]}
    assert check_catch(dict(traps=[(5, 1.0, 16)]), 6)['levels'] == [0.5, 0.95]
    bad = [dict(traps=[]),
           dict(traps=[(1, 0.5)] * 33),
           dict(traps=[(6, 0.5)]),                       # the model has days 0..5
           dict(traps=[(-1, 0.5)]),
           dict(traps=[(1.5, 0.5)]),
           dict(traps=[(1, 0.0)]),
           dict(traps=[(1, -2.0)]),
           dict(traps=[(1, float('inf'))]),
           dict(traps=[(1, float('nan'))]),
           dict(traps=[(1, 0.5, 0)]),
           dict(traps=[(1, 0.5, 17)]),
           dict(traps=[(1, 0.5, 2.5)]),
           dict(traps=[(1, 0.5, 1, 1)]),
           dict(traps=[(1, 0.5)], levels=(0.0, 0.5)),
           dict(traps=[(1, 0.5)], levels=(0.5, 1.5)),
           dict(traps=[(1, 0.5)], levels=(0.9, 0.5)),
           dict(traps=[(1, 0.5)], levels=(0.5, 0.5)),
           dict(traps=[(1, 0.5)], emergence=[(20, 0.5)]),  # the key without emergence=
           dict(traps=[(1, 0.5)], other=1),
           dict(levels=(0.5,)),
           [(1, 0.5)]]
    for arg in bad:
        with pytest.raises(ValueError):
            check_catch(arg, 6)
    with pytest.raises(ValueError, match='evaluate'):
        check_catch(dict(traps=[(1, 0.5)]), 6, evaluate=lambda theta: None)
    # the emergence key: a listed emergence day that carries weight
    em = dict(collection_day=6, obs_days=[19, 21, 24])
    got = check_catch(dict(traps=[(1, 0.5)], emergence=[(21, 0.2, 2)]), 6, em)
    assert got['emergence'] == [(21, 0.2, 2)]
    with pytest.raises(ValueError, match='emergence day'):
        check_catch(dict(traps=[(1, 0.5)], emergence=[(20, 0.2)]), 6, em)


def test_posterior_predictive_refuses_before_any_evaluation():
    from parasitoids_amd.predictive import posterior_predictive
    calls = []

    def evaluate(theta):
        calls.append(theta)
        return None
    chain = (np.zeros((3, 1)), ['x'])
    with pytest.raises(ValueError, match='evaluate'):
        posterior_predictive(None, chain, evaluate=evaluate, catch=dict(traps=[(1, 0.5)]))
    with pytest.raises(ValueError, match='count'):
        posterior_predictive(None, chain, catch=dict(traps=[(1, 0.5, 17)]))
    with pytest.raises(ValueError, match='emergence='):
        posterior_predictive(None, chain, catch=dict(traps=[(1, 0.5)], emergence=[(20, 1.0)]))
    assert not calls


def test_required_rate_is_a_step_function_over_the_listed_ladder():
    from parasitoids_amd.predictive import required_rate
    #         day rate n   -- the ladder of (2, n = 1) is listed out of order, with a tie at 4.0
    traps = [(2, 4.0, 1), (2, 0.5, 1), (3, 0.1, 1), (2, 1.0, 1), (2, 0.2, 2), (2, 4.0, 1)]
    means = [np.array([0.99, 0.96, 0.90, 0.2]),      # rate 4
             np.array([0.95, 0.40, 0.30, 0.1]),      # rate 0.5
             np.array([1.00, 1.00, 1.00, 1.0]),      # another day: ignored
             np.array([0.97, 0.95, 0.50, 0.1]),      # rate 1
             np.array([1.00, 1.00, 1.00, 1.0]),      # another count: ignored
             np.array([0.99, 0.96, 0.96, 0.2])]      # rate 4 once more: either may answer
    got = required_rate(traps, means, 2, 1, 0.95)
    assert np.array_equal(got[:3], [0.5, 1.0, 4.0]) and np.isnan(got[3])
    assert np.array_equal(required_rate(traps, means, 3, 1, 0.5), [0.1] * 4)
    assert np.array_equal(required_rate(traps, means, 2, 2, 1.0), [0.2] * 4)
    # a non-monotone ladder still answers with the smallest rate that reaches the level
    odd = required_rate([(0, 1.0, 1), (0, 2.0, 1)], [np.array([0.9]), np.array([0.1])], 0, 1, 0.5)
    assert odd[0] == 1.0
    with pytest.raises(ValueError):
        required_rate(traps, means, 4, 1, 0.5)


def test_the_trap_parser_round_trips():
    from parasitoids_amd.predictive import check_traps, format_traps, parse_traps
    text = '3,0.5;3,2.0,4;17,1e-06,16'
    traps = parse_traps(text)
    assert traps == [(3, 0.5), (3, 2.0, 4), (17, 1e-06, 16)]
    assert parse_traps(format_traps(traps)) == traps
    assert parse_traps(' 3 , 0.5 ; ') == [(3, 0.5)]
    assert check_traps(traps) == [(3, 0.5, 1), (3, 2.0, 4), (17, 1e-06, 16)]
    for bad in ('3', '3,0.5,1,2', 'a,0.5', '3,0.5,x', '2.5,1'):
        with pytest.raises(ValueError):
            parse_traps(bad)
    # the script documents and wires the flags
    src = open(os.path.join(ROOT, 'scripts', 'run_predictive.py')).read()
    for flag in ('--catch', '--catch-levels', '--catch-emergence', 'catch_ms_per_member'):
        assert flag in src

"""CPU tests of the trap information maps: the numpy restatement of the kernels' statements (gain_ref) against
mpmath at 60 digits, the properties of the gain on a synthetic ensemble (zeros, the cap, identical members, the
coarsening order, the two-member closed form), the driver argument's checks and the layout of the save file.  No
device is touched."""
import json
import os

import numpy as np
import pytest

import gain_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YMAX = (0, 1, 3, 7, 15)


def _sweep(ymax):
    rng = np.random.default_rng(200 + ymax)
    n = float(ymax + 1)
    return np.concatenate([10.0 ** rng.uniform(-12, 3, 160), rng.uniform(0, 40, 160),
                           [n, np.nextafter(n, 0.0), 700.0, 745.0, 746.0, 1e4, 5e-324, 1e-300]])


@pytest.mark.parametrize('ymax', YMAX)
def test_the_restatement_against_mpmath(ymax):
    mu = _sweep(ymax)
    planes = gain_ref.apply(mu, ymax)
    assert planes.dtype == np.float64 and planes.shape == (ymax + 3, mu.size)
    assert ((planes[:-1] >= 0.0) & (planes[:-1] <= 1.0)).all()
    assert (planes[-1] >= 0.0).all() and (planes[-1] <= np.log(ymax + 2)).all()
    rel, abs_h = gain_ref.errors(planes, mu, ymax)    # relative; absolute where the exact value is below 1e-290
    k = np.unravel_index(int(rel.argmax()), rel.shape)
    print('ymax = %d: class planes %.3g (plane %d at mu = %.17g), h %.3g (at mu = %.17g)'
          % (ymax, rel.max(), k[0], mu[k[1]], abs_h.max(), mu[int(abs_h.argmax())]))
    assert rel.max() <= 1e-14
    assert abs_h.max() <= 1e-14
    # the stated edges: every plane +0.0 where mu is not > 0; the sure branch from 800 on
    zero = gain_ref.apply(np.array([0.0, -0.0]), ymax)
    assert not zero.any() and not np.signbit(zero).any()
    sure = gain_ref.apply(np.array([1e4]), ymax)[:, 0]
    want = np.zeros(ymax + 3)
    want[0] = want[ymax + 1] = 1.0
    assert np.array_equal(sure, want)
    # the classes of a live cell sum to 1
    live = (mu > 0) & (mu < 700)
    total = (1.0 - planes[0, live]) + planes[1:ymax + 2, live].sum(axis=0)
    assert np.abs(total - 1.0).max() <= 1e-14


def test_fields_restatement_uses_one_rounded_product():
    v = np.array([[0.0, 1e-8, 0.3], [2.5, 40.0, 1e3]])
    got = gain_ref.fields(v, 3.0, 4)
    assert got.shape == (7, 2, 3)
    assert np.array_equal(got, gain_ref.apply(3.0 * v, 4))
    assert not got[:, 0, 0].any()
    with pytest.raises(ValueError):
        gain_ref.apply(v, 16)


def _ensemble(identical=False):
    """40 members with integer weights 1..8 and lognormal densities over 2000 cells, 100 of them empty in every
    member"""
    rng = np.random.default_rng(7)
    w = rng.integers(1, 9, 40)
    v = np.exp(rng.normal(0.0, 2.0, (40, 2000)))
    v[:, :100] = 0.0
    if identical:
        v[:] = v[0]
    return v, w


def _gain(v, w, rate, ymax):
    planes = [gain_ref.fields(m, rate, ymax) for m in v]
    return gain_ref.finish(gain_ref.weighted_mean(planes, w))


def test_the_gain_on_a_synthetic_ensemble():
    v, w = _ensemble()
    assert set(w) <= set(range(1, 9)) and v.shape == (40, 2000) and (v[:, 100:] > 0).all()
    cap = gain_ref.cap(w)
    assert 0 < cap <= np.log(40) + 1e-15
    by_ymax = {}
    for ymax in (0, 3, 7):
        G, HY, HYM = by_ymax[ymax] = _gain(v, w, 0.7, ymax)
        assert not G[:100].any() and not np.signbit(G[:100]).any()         # exactly +0.0 where every member is empty
        assert not HY[:100].any() and not HYM[:100].any()
        assert (G >= 0.0).all() and (G <= cap).all()
        assert G.max() > 0.05
        assert (HY <= np.log(ymax + 2) + 1e-15).all()
    # coarsening cannot add information
    assert (by_ymax[0][0] <= by_ymax[3][0] + 1e-12).all()
    assert (by_ymax[3][0] <= by_ymax[7][0] + 1e-12).all()
    assert (by_ymax[7][0] - by_ymax[0][0]).max() > 1e-3


@pytest.mark.parametrize('ymax', (0, 3, 15))
def test_identical_members_carry_no_information(ymax):
    v, w = _ensemble(identical=True)
    G, HY, HYM = _gain(v, w, 0.7, ymax)
    print('ymax = %d: largest |HY - HYM| %.3g' % (ymax, np.abs(HY - HYM).max()))
    assert np.abs(HY - HYM).max() <= 1e-12
    assert G.max() <= 1e-12


def test_two_members_against_the_closed_form():
    rng = np.random.default_rng(11)
    v = np.exp(rng.normal(0.0, 2.0, (2, 500)))
    v[0, :50] = 0.0                                  # one member empty: the trap tells which is true
    G, _HY, _HYM = _gain(v, [3, 3], 0.4, 0)

    def Hb(p):
        with np.errstate(divide='ignore', invalid='ignore'):
            h = -(np.where(p > 0, p * np.log(p), 0.0) + np.where(p < 1, (1 - p) * np.log1p(-p), 0.0))
        return h
    a, b = -np.expm1(-0.4 * v[0]), -np.expm1(-0.4 * v[1])
    want = Hb((a + b) / 2) - (Hb(a) + Hb(b)) / 2
    assert np.abs(G - want).max() <= 1e-12
    assert G.max() <= np.log(2) and G[:50].max() > 0.1


def test_check_information_refusals():
    from parasitoids_amd.predictive import check_information, check_info_traps
    ok = check_information(dict(traps=[(1, 0.5), (3, 2.0, 7)]), 6)
    assert ok['traps'] == [(1, 0.5, 0), (3, 2.0, 7)]
    assert ok['given'] == {'traps': [[1, 0.5], [3, 2.0, 7]]}
    assert check_information(dict(traps=[(5, 1.0, 15), (0, 1.0, 11)]), 6)['traps'][0] == (5, 1.0, 15)   # 18 + 14 planes
    assert len(check_info_traps([(1, 0.5)] * 10)) == 10                                               # 30 planes
    bad = [dict(traps=[]),
           dict(traps=[(1, 0.5)] * 11),                  # 33 planes
           dict(traps=[(5, 1.0, 15), (0, 1.0, 12)]),     # 18 + 15 planes
           dict(traps=[(6, 0.5)]),                       # the model has days 0..5
           dict(traps=[(-1, 0.5)]),
           dict(traps=[(1.5, 0.5)]),
           dict(traps=[(1, 0.0)]),
           dict(traps=[(1, -2.0)]),
           dict(traps=[(1, float('inf'))]),
           dict(traps=[(1, float('nan'))]),
           dict(traps=[(1, 0.5, -1)]),
           dict(traps=[(1, 0.5, 16)]),
           dict(traps=[(1, 0.5, 2.5)]),
           dict(traps=[(1, 0.5, 1, 1)]),
           dict(traps=[(1, 0.5)], levels=(0.5,)),
           dict(),
           [(1, 0.5)]]
    for arg in bad:
        with pytest.raises(ValueError):
            check_information(arg, 6)
    with pytest.raises(ValueError, match='evaluate'):
        check_information(dict(traps=[(1, 0.5)]), 6, evaluate=lambda theta: None)


def test_posterior_predictive_refuses_before_any_evaluation():
    from parasitoids_amd.predictive import posterior_predictive
    calls = []

    def evaluate(theta):
        calls.append(theta)
        return None
    chain = (np.zeros((3, 1)), ['x'])
    with pytest.raises(ValueError, match='evaluate'):
        posterior_predictive(None, chain, evaluate=evaluate, information=dict(traps=[(1, 0.5)]))
    with pytest.raises(ValueError, match='ymax'):
        posterior_predictive(None, chain, information=dict(traps=[(1, 0.5, 16)]))
    with pytest.raises(ValueError, match='planes'):
        posterior_predictive(None, chain, information=dict(traps=[(1, 0.5, 15), (1, 0.5, 15)]))
    assert not calls


class _FakeSummary():
    members, total_weight = 3, 6.0


class _FakeInformation():
    """what save_information reads of an InformationPosterior, over restated maps"""

    def __init__(self, traps, v, w):
        self.traps, self.weights, self.summary, self.given = traps, list(w), _FakeSummary(), None
        self._m = [gain_ref.weighted_mean([gain_ref.fields(m, t[1], t[2]) for m in v], w) for t in traps]
        self._r = [gain_ref.finish(m) for m in self._m]
        self.cap = gain_ref.cap(w)

    def gain(self, e):
        return self._r[e][0]

    def entropy(self, e):
        return self._r[e][1]

    def pmf(self, e, y):
        return 1.0 - self._m[e][0] if y == 0 else self._m[e][y]


def test_the_save_file_layout(tmp_path):
    from scipy import sparse
    from parasitoids_amd.predictive import save_information, weight_entropy
    rng = np.random.default_rng(3)
    v = np.exp(rng.normal(0.0, 2.0, (3, 9, 9)))
    v[:, :4] = 0.0
    traps = [(2, 0.5, 0), (4, 1.5, 2)]
    info = _FakeInformation(traps, v, [1, 2, 3])
    block = save_information(str(tmp_path / 'd' / 'pp_information'), info, cell_area=4.0)
    f = np.load(str(tmp_path / 'd' / 'pp_information.npz'))
    assert list(f['days']) == [2, 4] and list(f['rates']) == [0.5, 1.5] and list(f['ymax']) == [0, 2]
    want = {'days', 'rates', 'ymax'}
    for e, t in enumerate(traps):
        for name in ['gain', 'entropy', 'd0'] + ['p%d' % y for y in range(1, t[2] + 2)]:
            want |= {'i%d_%s_%s' % (e, name, part) for part in ('data', 'ind', 'indptr')}
    assert set(f.files) == want

    def csr(key):
        return sparse.csr_matrix((f[key + '_data'], f[key + '_ind'], f[key + '_indptr']), shape=(9, 9)).toarray()
    for e, t in enumerate(traps):
        for key, m in [('i%d_gain' % e, info.gain(e)), ('i%d_entropy' % e, info.entropy(e)),
                       ('i%d_d0' % e, 1.0 - info.pmf(e, 0)), ('i%d_p%d' % (e, t[2] + 1), info.pmf(e, t[2] + 1))]:
            assert np.array_equal(csr(key), np.where(m >= 1e-8, m, 0.0)), key
        assert not csr('i%d_d0' % e)[:4].any()                          # nothing stored where every member is empty
    assert block['traps'] == [list(t) for t in traps] and block['members'] == 3 and block['total_weight'] == 6.0
    assert block['cap'] == info.cap == weight_entropy([1, 2, 3]) and block['units'] == 'nats'
    for e, out in enumerate(block['outputs']):
        g = info.gain(e)
        assert out['trap'] == list(traps[e]) and out['max_gain'] == float(g.max())
        assert out['half_area'] == float((g >= 0.5 * g.max()).sum() * 4.0)
    json.dumps(block)
    assert weight_entropy([5]) == 0.0 and abs(weight_entropy([2, 2]) - np.log(2)) <= 1e-15


def test_the_script_documents_and_wires_the_flag():
    src = open(os.path.join(ROOT, 'scripts', 'run_predictive.py')).read()
    for flag in ('--information', 'information_ms_per_member', 'accumulate_ms_per_member'):
        assert flag in src

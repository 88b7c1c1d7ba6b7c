"""CPU tests of the proximity maps (predictive.ProximityFields / ProximityPosterior, ps_prox_*): the numpy restatement
(prox_ref) against scipy's exact Euclidean distance transform, every refusal of check_proximity, the default ladder,
radius() on a stub histogram, the layout of the saved file with a stub posterior, that the metres are strictly
monotone in the squared distance, the driver's wiring, and the host emulation of the device logic
(tests/host/prox_emul.cpp over csrc/ps_prox_core.h) under the sanitizers."""
import os
import subprocess
import types

import numpy as np
import pytest

import prox_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('density', [0.002, 0.05, 0.6])
def test_the_restatement_against_scipy(density):
    from scipy import ndimage
    N = 67
    rng = np.random.default_rng(int(density * 1000))
    s = rng.random((N, N)) < density
    assert s.any() and not s.all()
    for side_set in (s, ~s):
        dist, idx = ndimage.distance_transform_edt(~side_set, return_indices=True)    # to the nearest zero of ~S
        yy, xx = np.mgrid[:N, :N]
        want = (yy - idx[0]) ** 2 + (xx - idx[1]) ** 2
        got = prox_ref.d2(side_set)
        assert got.dtype == np.uint32 and np.array_equal(got.astype(np.int64), want)
        assert np.array_equal(np.sqrt(got.astype(np.float64)), dist)                  # bit for bit
        assert np.array_equal(got == 0, side_set)
        assert np.array_equal(prox_ref.metres(got, 25.0), dist * 25.0)


def test_the_restatement_on_the_crafted_sets():
    N = 65
    seen = {name: prox_ref.d2(s) for name, s in prox_ref.crafted(N)}
    F = prox_ref.far2(N)
    assert F == 2 * 64 * 64 + 1
    assert (seen['empty'] == F).all() and (seen['whole'] == 0).all()
    assert seen['corner0'][N - 1, N - 1] == F - 1 and seen['corner3'][0, 0] == F - 1
    assert seen['centre'][0, 0] == 2 * 32 * 32 and seen['centre'][32, 32] == 0
    assert np.array_equal(seen['column63'], np.broadcast_to((np.arange(N) - 63) ** 2, (N, N)))
    assert np.array_equal(seen['column64'], np.broadcast_to((np.arange(N) - 64) ** 2, (N, N)))
    assert (seen['equidistant'][:, 32] == (np.arange(N) - 32) ** 2 + 25).all()
    assert set(np.unique(seen['checkerboard'])) == {0, 1}
    ring = dict(prox_ref.crafted(N))['ring']
    inside = prox_ref.d2(~ring)
    assert inside[32, 32] == 0 and inside[0, 0] == 0          # the hole and the ground outside are not in the ring
    # the depth of a ring cell counts the hole and the outer ground, never the domain's edge
    assert inside.max() == inside[ring].max() and 0 < inside.max() < (N // 3) ** 2
    v = prox_ref.as_field(ring, 2.0)
    assert np.array_equal(prox_ref.reached(v, 2.0), ring) and np.array_equal(prox_ref.reached(v, 2.0, 'in'), ~ring)
    plane, m = prox_ref.field(v, 2.0, 'to', 156.25)
    assert np.array_equal(plane, seen['ring']) and m[0, 0] == np.sqrt(np.float64(plane[0, 0])) * 156.25


def test_check_proximity_and_its_refusals():
    from parasitoids_amd.predictive import check_proximity, check_prox_windows, parse_prox_windows
    got = check_proximity([(1, 2), (3, 10.0, 'in')], 6, 25.0)
    assert got['windows'] == [(1, 2.0, 'to'), (3, 10.0, 'in')] and got['radii_m'] == [] and got['levels'] is None
    assert got['ladder'] is None and got['given']['windows'] == [[1, 2.0, 'to'], [3, 10.0, 'in']]
    got = check_proximity(dict(windows=[(5, 1.0)], radii_m=[100, 400, 1600], levels=(0.05, 0.5), ladder=[25, 50, 100]))
    assert got['radii_m'] == [100.0, 400.0, 1600.0] and got['levels'] == [0.05, 0.5] and got['ladder'] == [25.0, 50.0, 100.0]
    bad = [
        [(6, 1.0)],                                   # a day the model has not
        [(1, 0.0)], [(1, -1.0)], [(1, float('nan'))], [(1, float('inf'))],      # t not finite or <= 0
        [(1, 1.0, 'from')], [(1,)], [(1, 1.0, 'to', 3)], [('a', 1.0)], [(1.5, 1.0)], [(-1, 1.0)],
        [], None, 3,
        [(1, 1.0)] * 33,                              # more than 32 windows
        dict(), dict(radii_m=[100]), dict(windows=[(1, 1.0)], other=1),
        dict(windows=[(1, 1.0)], radii_m=[100, 200, 300, 400]),                 # the fourth threshold is taken
        dict(windows=[(1, 1.0)], radii_m=[200, 100]), dict(windows=[(1, 1.0)], radii_m=[100, 100]),
        dict(windows=[(1, 1.0)], radii_m=[0.0]), dict(windows=[(1, 1.0)], radii_m=[-5.0]),
        dict(windows=[(1, 1.0)], radii_m=[float('inf')]), dict(windows=[(1, 1.0)], radii_m=[float('nan')]),
        dict(windows=[(1, 1.0)], ladder=[50, 25]), dict(windows=[(1, 1.0)], ladder=[0.0, 25]),
        dict(windows=[(1, 1.0)], ladder=[25, float('inf')]), dict(windows=[(1, 1.0)], ladder=[25, 25]),
        dict(windows=[(1, 1.0)], ladder=[25]),
        dict(windows=[(1, 1.0)], levels=[0.0]), dict(windows=[(1, 1.0)], levels=[1.5]),
    ]
    for arg in bad:
        with pytest.raises(ValueError):
            check_proximity(arg, 6, 25.0)
    assert len(check_prox_windows([(d, 1.0) for d in range(32)])) == 32         # 32 windows on 32 days fit
    with pytest.raises(ValueError, match='33 windows'):
        check_proximity([(d, 1.0) for d in range(33)])
    with pytest.raises(ValueError, match='evaluate'):
        check_proximity([(1, 1.0)], 6, 25.0, evaluate=lambda theta: None)
    assert parse_prox_windows('3,10; 5,2.5,in;') == [(3, 10.0), (5, 2.5, 'in')]
    for text in ('5', '5,1,in,2', 'a,1', '5,x', '2.5,1'):
        with pytest.raises(ValueError):
            parse_prox_windows(text)
    src = open(os.path.join(ROOT, 'scripts', 'run_predictive.py')).read()
    for flag in ("'--proximity'", "'--proximity-radii'", "'--proximity-levels'", 'prox_col_ms_per_member'):
        assert flag in src


def test_the_default_ladder():
    from parasitoids_amd.predictive import bin_edges, default_ladder, prox_far
    far2, far_m = prox_far(801, 25.0)
    assert far2 == 2 * 800 * 800 + 1 and far_m == np.sqrt(np.float64(far2)) * 25.0
    lad = default_ladder(25.0, far_m)
    assert lad[0] == 25.0 and lad[4] == 50.0 and lad[8] == 100.0
    assert lad[-1] > far_m >= lad[-2] and 40 <= len(lad) <= 48
    assert np.allclose(np.array(lad[1:]) / np.array(lad[:-1]), 2.0 ** 0.25, rtol=1e-15)
    assert np.array_equal(bin_edges(edges=lad), np.array(lad))                   # a histogram takes it as it is
    small = default_ladder(156.25, prox_far(65, 156.25)[1])
    assert small[-1] > prox_far(65, 156.25)[1] >= small[-2]


def test_radius_reads_the_ladder_off_the_exceedance_at_the_edges():
    from parasitoids_amd.predictive import ProximityPosterior, ladder_radius
    edges = np.array([25.0, 50.0, 100.0, 200.0])
    # three cells: P(d >= edge) per edge
    exc = {25.0: [0.0, 1.0, 1.0], 50.0: [0.0, 0.6, 1.0], 100.0: [0.0, 0.5, 1.0], 200.0: [0.0, 0.04, 1.0]}
    asked = []

    class Hist():
        def exceedance(self, e, r):
            asked.append((e, r))
            return np.array([exc[r]])
    Hist.edges = edges
    post = ProximityPosterior.__new__(ProximityPosterior)
    post.windows, post.histogram = [(1, 1.0, 'to'), (2, 1.0, 'to')], Hist()
    got = post.radius(1, 0.5)
    assert np.array_equal(got, [[25.0, 100.0, np.nan]], equal_nan=True)
    assert sorted(asked) == [(1, r) for r in edges]
    assert np.array_equal(post.radius(1, 0.95), [[25.0, 200.0, np.nan]], equal_nan=True)
    assert np.array_equal(post.radius(1, 0.4), [[25.0, 50.0, np.nan]], equal_nan=True)
    want = np.full(3, np.nan)
    for r in edges[::-1]:                       # the loop over the ladder
        want = np.where(1.0 - np.array(exc[r]) >= 0.97, r, want)
    assert np.array_equal(ladder_radius(edges, lambda r: np.array(exc[r]), 0.97), want, equal_nan=True)
    for bad in (0.0, 1.5):
        with pytest.raises(ValueError):
            post.radius(1, bad)
    with pytest.raises(ValueError):
        post.radius(2, 0.5)
    post.histogram = None
    with pytest.raises(ValueError, match='histogram'):
        post.radius(1, 0.5)


def _csr(f, key, N):
    from scipy import sparse
    return sparse.csr_matrix((f[key + '_data'], f[key + '_ind'], f[key + '_indptr']), shape=(N, N)).toarray()


def test_the_saved_file_with_a_stub_posterior(tmp_path):
    from parasitoids_amd.predictive import save_proximity
    N = 9
    rng = np.random.default_rng(4)
    planes = {}

    def plane(*key):
        return planes.setdefault(key, rng.random((N, N)))
    post = types.SimpleNamespace(
        windows=[(1, 2.0, 'to'), (3, 10.0, 'in')], radii_m=[100.0, 400.0], levels=[0.05, 0.5], ladder=[25.0, 50.0, 100.0],
        far_m=283.0, summary=types.SimpleNamespace(members=4, total_weight=9.0),
        mean=lambda e: plane('mean', e) * 100, sd=lambda e: plane('sd', e), nearer=lambda e, k: plane('near', e, k),
        quantile=lambda e, p: plane('q', e, p) * 50, empty_share=lambda e: [0.25, 0.0][e])
    block = save_proximity(str(tmp_path / 'out' / 'pp_prox'), post, 625.0)
    f = np.load(str(tmp_path / 'out' / 'pp_prox.npz'))
    assert list(f['days']) == [1, 3] and list(f['thresholds']) == [2.0, 10.0] and list(f['sides']) == ['to', 'in']
    assert list(f['radii_m']) == [100.0, 400.0] and list(f['ladder']) == [25.0, 50.0, 100.0]
    assert float(f['far_m']) == 283.0 and list(f['empty_share']) == [0.25, 0.0]
    for e in range(2):
        for key, m in (('x%d' % e, planes['mean', e] * 100), ('x%d_sd' % e, planes['sd', e]),
                       ('x%d_pnear0' % e, planes['near', e, 0]), ('x%d_pnear1' % e, planes['near', e, 1]),
                       ('x%d_q5' % e, planes['q', e, 0.05] * 50), ('x%d_q50' % e, planes['q', e, 0.5] * 50)):
            assert np.array_equal(_csr(f, key, N), np.where(m >= 1e-8, m, 0.0)), key
    assert block['windows'] == [[1, 2.0, 'to'], [3, 10.0, 'in']] and block['radii_m'] == [100.0, 400.0]
    assert block['members'] == 4 and block['total_weight'] == 9.0 and block['far_m'] == 283.0
    assert block['levels'] == [0.05, 0.5]
    for e, out in enumerate(block['outputs']):
        assert out['window'] == list(post.windows[e]) and out['empty_share'] == [0.25, 0.0][e]
        assert out['area'] == [float((planes['near', e, k] >= 0.5).sum() * 625.0) for k in range(2)]
    post.levels = None
    block = save_proximity(str(tmp_path / 'out' / 'bare'), post)
    assert block['outputs'][0]['area'] == [None, None]
    assert 'x0_q50_data' not in np.load(str(tmp_path / 'out' / 'bare.npz')).files


@pytest.mark.parametrize('cell_m', [25.0, 156.25, 10000.0 / 300, 1.0])
def test_the_metres_are_strictly_monotone_in_the_squared_distance(cell_m):
    r2 = np.arange(2 * 800 * 800 + 2, dtype=np.uint32)
    m = prox_ref.metres(r2, cell_m)
    assert (np.diff(m) > 0).all() and m[0] == 0.0


def test_the_driver_is_wired_and_builds_nothing_unasked():
    from parasitoids_amd import predictive as PR
    for kind in ('days', 'sites'):
        order = PR.FEED_ORDER[kind]
        assert order.index('proximity') == order.index('neighbourhood') + 1        # right after the neighbourhood
    assert 'proximity' not in PR.FEED_ORDER['projection'] and 'proximity' not in PR.FEED_ORDER['compare']
    assert 'proximity' in PR.ACCUMULATORS and PR.BUILD['proximity'] is PR._build_proximity
    q = types.SimpleNamespace(px_plan=None)
    fs = PR._FieldSet().fed_from('days', object(), owns=False, proximity=None)
    assert PR.BUILD['proximity'](fs, q) is None and fs.proximity is None
    assert PR.BUILD['proximity'](PR._FieldSet().fed_from('days', object(), owns=False), q) is None
    chain = (np.zeros((3, len(PR.model_names()))), PR.model_names())
    res = PR.posterior_predictive(None, chain, evaluate=lambda theta: None)
    assert res.proximity is None
    assert PR.ProximityFields.fields_kind == 'prox' and PR.ProximityFields._prefix == 'ps_prox'
    calls = []
    small = (np.zeros((3, 1)), ['x'])
    with pytest.raises(ValueError, match='evaluate'):
        PR.posterior_predictive(None, small, evaluate=lambda theta: calls.append(theta), proximity=[(1, 1.0)])
    with pytest.raises(ValueError, match='finite and > 0'):
        PR.posterior_predictive(None, small, proximity=[(1, 0.0)])
    with pytest.raises(ValueError, match='windows'):
        PR.posterior_predictive(None, small, proximity=dict(days=[1]))
    pm = types.SimpleNamespace(days=list(range(6)), rad_dist=10000.0, rad_res=400)
    with pytest.raises(ValueError, match='6 days'):
        PR.posterior_predictive(pm, small, proximity=[(6, 1.0)])
    with pytest.raises(ValueError, match='at most 3'):
        PR.posterior_predictive(pm, small, proximity=dict(windows=[(1, 1.0)], radii_m=[1, 2, 3, 4]))
    assert not calls
    # refused before the model is looked at
    with pytest.raises(ValueError, match='finite and > 0'):
        PR.ProximityFields(types.SimpleNamespace(), [(1, -1.0)])
    with pytest.raises(ValueError, match='33 windows'):
        PR.ProximityFields(types.SimpleNamespace(), [(1, 1.0)] * 33)


def test_the_header_the_signatures_and_the_sources_agree():
    import re
    from parasitoids_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'parasitoid_hip.h')).read()
    declared = set(re.findall(r'\b(ps_[a-z0-9]+_[a-z0-9_]*prox[a-z0-9_]*|ps_prox_[a-z0-9_]+)\s*\(', header))
    want = {'ps_prox_' + n for n in ('create', 'set_strip', 'apply', 'apply_project', 'apply_sites', 'fetch', 'fetch_d2',
                                     'gather', 'info', 'prof', 'destroy')}
    want |= {'ps_%s_add_prox' % a for a in ('summary', 'hist', 'mcerr', 'wsum')}
    assert declared == want
    assert want <= set(_lib.SIGNATURES)
    mk = open(os.path.join(ROOT, 'parasitoids_amd', 'csrc', 'Makefile')).read()
    assert 'ps_prox.hip' in mk
    core = open(os.path.join(ROOT, 'parasitoids_amd', 'csrc', 'ps_prox_core.h')).read()
    assert '-ffast-math' not in mk                 # the square root of the field stays correctly rounded
    assert 'prox_col_search' in core and 'prox_row_dist' in core


def _emulator(tmp_path, flags, name):
    exe = str(tmp_path / name)
    src = os.path.join(ROOT, 'tests', 'host', 'prox_emul.cpp')
    built = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-pthread'] + flags + ['-o', exe, src],
                           capture_output=True, text=True)
    return exe, built


def test_host_emulation_of_the_device_logic_under_the_sanitizers(tmp_path):
    """both passes of ps_prox_core.h as the kernels run them -- the set as flat 64-bit words, the row distance from
    the words, the column search over staged strips of 64 down to 1 columns -- on 8 threads, on the crafted sets and
    on random masks of three densities, both sides, at N = 63, 64, 65 and 130, against the emulator's own brute force.
    Built with the address and the undefined-behaviour sanitizer; a child process."""
    exe, built = _emulator(tmp_path, ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'], 'emul_asan')
    assert built.returncode == 0, built.stderr[-2000:]
    out = subprocess.run([exe, '63', '64', '65', '130'], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith('ok '), (out.stdout[-2000:], out.stderr[-2000:])
    assert int(out.stdout.split()[1]) == 2 * (16 + 17 + 18 + 18)      # sides x the sets of each size


def test_host_emulation_under_the_thread_sanitizer(tmp_path):
    """the same program built with -fsanitize=thread, where this compiler links it and its runtime starts"""
    exe, built = _emulator(tmp_path, ['-fsanitize=thread'], 'emul_tsan')
    if built.returncode != 0:
        pytest.skip('this compiler does not link -fsanitize=thread')
    out = subprocess.run([exe, '63', '65'], capture_output=True, text=True)
    if out.returncode != 0 and 'FATAL: ThreadSanitizer' in out.stderr and 'FAIL' not in out.stdout:
        pytest.skip('the thread sanitizer does not start here: %s' % out.stderr.strip().splitlines()[0])
    assert out.returncode == 0 and out.stdout.startswith('ok '), (out.stdout[-2000:], out.stderr[-2000:])

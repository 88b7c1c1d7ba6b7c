"""CPU tests of the pathway maps (predictive.PathwayMaps, ps_pathway_*): the numpy restatement (pathway_ref) against
a patch-by-patch version in plain Python over a flood fill on the crafted sequences, what each sequence is there for,
the argument checks and the driver's refusals, the arithmetic of the foci and area posteriors on hand-made rows, the
layout of the saved file with a stub handle, and the host emulation of the device logic (tests/host/pathway_emul.cpp
over csrc/ps_pathway_core.h and csrc/ps_patch_core.h) under the sanitizers."""
import json
import os
import subprocess
import types

import numpy as np
import pytest

import pathway_ref as W
import patch_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('N', [17, 33])
@pytest.mark.parametrize('connectivity', [4, 8])
def test_the_restatement_matches_a_plain_python_version_on_the_crafted_sequences(N, connectivity):
    seen = {}
    for name, f, anchors in W.sequences(N):
        assert f.shape == (W.NSLOT, N, N) and set(np.unique(f)) <= {0.0, 1.0, 2.0, 3.0}, name
        for t in P.SHAPE_THR:
            state, rows = W.classify(f, t, connectivity, anchors)
            fstate, frows = W.flood_classify(f, t, connectivity, anchors)
            assert np.array_equal(state, fstate) and np.array_equal(rows, frows), (name, t)
            # a cell is classed in the first slot that holds it, and never again
            first = np.argmax(f >= t, axis=0)
            ever = (f >= t).any(axis=0)
            assert np.array_equal(state > 0, ever), (name, t)
            for s in range(W.NSLOT):
                assert rows[s, :3].sum() == (ever & (first == s)).sum(), (name, t, s)
            for j in range(3):
                assert rows[:, j].sum() == (state == j + 1).sum(), (name, t, j)
            seen[name, t] = rows.tolist()
    # what each sequence is there for, at the threshold that shows it: rows of (front, jump, secondary, foci)
    c4 = connectivity == 4
    assert seen['empty', 0.5] == [[0, 0, 0, 0]] * 4
    assert seen['grow', 0.5] == [[25, 0, 0, 0], [24, 0, 0, 0], [32, 0, 0, 0], [40, 0, 0, 0]]
    assert seen['grow', 2.5] == [[1, 0, 0, 0], [8, 0, 0, 0], [16, 0, 0, 0], [24, 0, 0, 0]]
    assert seen['jump_grow_merge', 0.5] == [[9, 6, 0, 1], [0, 0, 6, 0], [2, 0, 0, 0], [5, 0, 0, 0]]
    assert seen['jump_grow_merge', 1.5] == [[9, 6, 0, 1], [0, 0, 6, 0], [2, 0, 0, 0], [0, 0, 0, 0]]
    assert seen['jump_grow_merge', 2.5] == [[9, 1, 0, 1], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert seen['two_foci_diagonal', 0.5] == ([[9, 0, 0, 0], [0, 8, 0, 2], [0, 0, 0, 0], [0, 0, 2, 0]] if c4 else
                                              [[9, 0, 0, 0], [4, 4, 0, 1], [0, 0, 0, 0], [2, 0, 0, 0]])
    assert seen['dropout_reenter', 0.5] == [[9, 6, 0, 1], [0, 0, 0, 0], [0, 0, 5, 0], [0, 4, 0, 1]]
    assert seen['anchor_late', 0.5] == [[0, 6, 0, 1], [9, 0, 0, 0], [16, 0, 0, 0], [24, 0, 0, 0]]
    assert seen['origin_wins', 0.5] == [[9, 6, 0, 1], [7, 0, 0, 0], [3, 0, 0, 0], [0, 0, 0, 0]]
    assert seen['two_anchors', 0.5] == [[18, 0, 0, 0], [0, 9, 0, 1], [3, 0, 0, 0], [0, 0, 0, 0]]
    assert seen['ring_island', 0.5] == [[32, 0, 0, 0], [0, 1, 0, 1], [0, 0, 2, 0], [2, 0, 0, 0]]
    assert seen['edge_next_row', 0.5] == [[9, 0, 0, 0], [0, 2, 0, 2], [0, 0, 2, 0], [0, 0, 0, 0]]
    assert seen['last', 0.5] == [[9, 0, 0, 0], [0, 0, 0, 0], [0, 1, 0, 1], [0, 0, 0, 0]]
    # the states of the dropped focus stay: its six cells are jump at the end, the re-entered ground secondary
    for name, f, anchors in W.sequences(N):
        if name == 'dropout_reenter':
            state, _rows = W.classify(f, 0.5, connectivity, anchors)
            c = N // 2
            assert (state[c + 4:c + 6, c - 6:c - 3] == 2).all() and (state == 3).sum() == 5
        if name == 'two_anchors':                  # without the second anchor the corner blob is a focus
            _s, rows = W.classify(f, 0.5, connectivity, anchors[:1])
            assert rows.tolist() == [[9, 9, 0, 1], [0, 9, 0, 1], [0, 0, 3, 0], [0, 0, 0, 0]]


def test_rows_follow_the_members_and_planes_do_not():
    seqs = [s for s in W.sequences(17) if len(s[2]) == 1]
    fields, anchors = [f for _n, f, _a in seqs], seqs[0][2]
    w = [1 + i % 3 for i in range(len(fields))]
    whole = W.accumulate(fields, w, P.SHAPE_THR, 4, anchors)
    a = W.accumulate(fields[:4], w[:4], P.SHAPE_THR, 4, anchors)
    b = W.accumulate(fields[4:], w[4:], P.SHAPE_THR, 4, anchors)
    for key in W.CLASSES:
        assert np.array_equal(a[key] + b[key], whole[key]) and np.array_equal(b[key] + a[key], whole[key])
    assert np.array_equal(np.concatenate([a['rows'], b['rows']]), whole['rows'])
    for k, t in enumerate(P.SHAPE_THR):            # the three classes partition the cells ever reached
        ever = sum(wi * (f >= t).any(axis=0) for f, wi in zip(fields, w))
        assert np.array_equal(whole['front'][k] + whole['jump'][k] + whole['secondary'][k], ever)
    flood = W.accumulate(fields, w, P.SHAPE_THR, 8, anchors, W.flood_classify)
    fast = W.accumulate(fields, w, P.SHAPE_THR, 8, anchors)
    assert all(np.array_equal(flood[key], fast[key]) for key in W.CLASSES + ('rows',))


def test_check_pathways_and_the_driver_refuse_before_any_evaluation():
    from parasitoids_amd.predictive import PathwayMaps, check_pathway_anchors, check_pathways, posterior_predictive
    assert check_pathways([1, 10]) == ([1.0, 10.0], 4, None, [0.05, 0.5, 0.95])
    assert check_pathways([1, 10], days=range(3)) == ([1.0, 10.0], 4, [0, 1, 2], [0.05, 0.5, 0.95])
    assert check_pathways(dict(thresholds=(2.5,), connectivity=8, days=[0, 3], levels=[1.0, 0.1])) == \
        ([2.5], 8, [0, 3], [1.0, 0.1])
    for bad in ([0.0, 1.0], [-1.0], [float('nan')], [float('inf')], [10, 1], [1, 1], [1, 2, 3, 4, 5], [], ['a'], 1.0):
        with pytest.raises(ValueError):
            check_pathways(bad)
        with pytest.raises(ValueError):
            check_pathways(dict(thresholds=bad))
        with pytest.raises(ValueError):
            PathwayMaps(None, bad)                   # refused before the model is touched
    for bad in (dict(connectivity=8), dict(thresholds=[1], conn=8), dict(thresholds=[1], connectivity=5),
                dict(thresholds=[1], connectivity='8'), dict(thresholds=[1], connectivity=True),
                dict(thresholds=[1], levels=[0.0]), dict(thresholds=[1], levels=[1.5]),
                dict(thresholds=[1], days=[3, 1]), dict(thresholds=[1], days=[]), dict(thresholds=[1], days=[-1, 2]),
                dict(thresholds=[1], days=list(range(33)))):
        with pytest.raises(ValueError):
            check_pathways(bad)
    with pytest.raises(ValueError):
        PathwayMaps(None, [1.0], connectivity=5)
    for days in ([], [3, 1], [-1, 2], list(range(33))):
        with pytest.raises(ValueError):
            check_pathways([1.0], days=days)
    with pytest.raises(ValueError, match='not among'):
        check_pathways(dict(thresholds=[1.0], days=[0, 7]), days=[0, 1, 2])
    assert check_pathway_anchors(None, 17) == [(8, 8)]
    assert check_pathway_anchors([(0, 16), [3.0, 2]], 17) == [(0, 16), (3, 2)]
    for bad in ([], [(0, 17)], [(-1, 0)], [(17, 0)], [(1, 2, 3)], 5, [(0, 0)] * 33, ['ab', 'c']):
        with pytest.raises(ValueError):
            check_pathway_anchors(bad, 17)
    with pytest.raises(ValueError, match='release plan'):
        PathwayMaps.for_projection(types.SimpleNamespace(fields_kind='project'), [1.0])

    def never(theta):
        raise AssertionError('evaluated')
    from parasitoids_amd import mcmc
    names = [m[0] for m in mcmc.MODEL_BLOCK]
    chain = (np.zeros((3, len(names))), names)
    model = types.SimpleNamespace(days=list(range(6)), rad_dist=10000.0, rad_res=64,
                                  evaluate=lambda *a, **k: never(None))
    with pytest.raises(ValueError, match='pathways= needs the device'):
        posterior_predictive(None, chain, evaluate=never, pathways=[1.0])
    # after the existing checks: of two bad arguments the other one is reported
    with pytest.raises(ValueError, match='fraction'):
        posterior_predictive(None, chain, core_range=[0.5, 1.5], pathways=[2.0, 1.0])
    with pytest.raises(ValueError, match='PopModel'):
        posterior_predictive(None, chain, pathways=[2.0, 1.0])
    with pytest.raises(ValueError, match='patch thresholds'):
        posterior_predictive(model, chain, patches=[2.0, 1.0], pathways=[2.0, 1.0])
    with pytest.raises(ValueError, match='pathway thresholds must be strictly increasing'):
        posterior_predictive(model, chain, pathways=[2.0, 1.0])
    with pytest.raises(ValueError, match='connectivity'):
        posterior_predictive(model, chain, pathways=dict(thresholds=[1.0], connectivity=5))
    with pytest.raises(ValueError, match='day 6 is not among them'):
        posterior_predictive(model, chain, pathways=dict(thresholds=[1.0], days=[0, 6]))
    with pytest.raises(ValueError, match='days'):
        posterior_predictive(model, chain, pathways=[1.0], days=[2, 1])


def test_without_pathways_nothing_is_built_and_the_feed_order_keeps_its_place():
    from parasitoids_amd import predictive as PR
    for kind in ('days', 'sites'):
        order = PR.FEED_ORDER[kind]
        assert order[order.index('patches') + 1] == 'pathways', kind
    assert 'pathways' not in PR.FEED_ORDER['projection'] and 'pathways' not in PR.FEED_ORDER['compare']
    assert 'pathways' in PR.ACCUMULATORS and 'pathways' in PR.BUILD and 'pathways' in PR.FEED
    fs = PR._FieldSet().fed_from('days', object(), owns=False)
    assert not PR.BUILD['pathways'](fs, types.SimpleNamespace(pw_thr=None)) and fs.pathways is None
    assert PR.ProjectedMaps(None, None, None, None).pathways is None
    chain = (np.zeros((3, len(PR.model_names()))), PR.model_names())
    q = types.SimpleNamespace(pop_model=None, chains=chain, burn=0, thin=1, days=None, thresholds=(), locinfo=None,
                              cell_area=None, seed=0, evaluate=lambda theta: None, quantiles=None, bins=PR.DEFAULT_BINS,
                              edges=None, arrival=None, arrival_levels=(0.5,), emergence=None, exposure=None, sites=None,
                              sensitivity=None, compare=None, mc_error=None, peak=None, excursion=None, reweight=None,
                              catch=None, information=None, core_range=None, patches=None, representative=None,
                              neighbourhood=None, modes=None, dependence=None, pathways=None)
    PR._check_request(q)
    assert q.pw_thr is None and q.pw_conn is None and q.pw_days is None and q.pw_levels is None
    res = PR.posterior_predictive(None, chain, evaluate=lambda theta: None)
    assert res.pathways is None and res.pathway_levels is None


def test_founded_and_area_arithmetic_on_hand_made_rows():
    from parasitoids_amd.predictive import PathwayMaps, pathway_founded, range_area, weighted_lower_quantile
    foci, w = [0, 2, 1, 0], [1, 1, 6, 2]
    got = pathway_founded(foci, w, (0.05, 0.5, 0.95))
    assert got == {'mean': (0 + 2 + 6 + 0) / 10, 'p_any': 0.7, 'quantiles': [0.0, 1.0, 2.0]}
    assert got['quantiles'] == [float(weighted_lower_quantile(foci, w, p)) for p in (0.05, 0.5, 0.95)]
    with pytest.raises(ValueError):
        pathway_founded([], [])
    # per member and day (front, jump, secondary, foci): two days
    rows = {1: ([10, 5, 7, 9], [0, 3, 2, 0], [0, 0, 0, 0], [0, 2, 1, 0]),
            4: ([4, 1, 0, 6], [0, 0, 0, 0], [0, 4, 3, 0], [0, 0, 0, 0])}

    class Stub(PathwayMaps):                           # the accessors over hand-made rows, no device
        def __init__(self):
            self.cell_area, self.days = 25.0, [1, 4]

        def _members(self, k, day):
            return tuple(np.array(r, np.uint32) for r in rows[day]) + (np.array(w, np.uint32),)
    S = Stub()
    assert S.founded(0) == got
    assert S.foci(0, 1).tolist() == foci and S.foci(0, 4).tolist() == [0, 0, 0, 0] and S.foci(0, 1).dtype == np.int64
    assert S.new_cells(0, 4, 'secondary').tolist() == [0, 4, 3, 0] and S.new_cells(0, 1, 'jump').tolist() == [0, 3, 2, 0]
    assert S.area(0, 'front') == range_area([14, 6, 7, 15], w, 25.0, (0.05, 0.5, 0.95))
    assert S.area(0, 'secondary')['mean'] == (0 + 4 + 18 + 0) / 10 * 25.0
    assert S.area(0, 'jump', [0.5])['quantiles'] == [2 * 25.0]
    with pytest.raises(ValueError):
        S.area(0, 'all')
    with pytest.raises(ValueError):
        S.new_cells(0, 1, 'main')
    assert S.weights.tolist() == w and S.weights.dtype == np.int64


def test_save_and_load_layout_with_a_stub_handle(tmp_path):
    from scipy import sparse
    from parasitoids_amd.predictive import pathway_founded, range_area, save_pathways
    N, days, thr, w = 17, [0, 2, 3, 5], [0.5, 2.5], [2, 1, 3]
    seqs = [s for s in W.sequences(N) if s[0] in ('jump_grow_merge', 'dropout_reenter', 'ring_island')]
    anchors = seqs[0][2]
    ref = W.accumulate([f for _n, f, _a in seqs], w, thr, 8, anchors)

    class Stub():
        thresholds, connectivity, members, total_weight, cell_area = thr, 8, 3, 6.0, 4.0

        def __init__(self):
            self.days, self.anchors = days, anchors
            self.weights = np.array(w, dtype=np.int64)

        def prob(self, k, which):
            return ref[which][k] / 6.0

        def _members(self, k, d):
            return tuple(ref['rows'][:, k, days.index(d), f].astype(np.uint32) for f in range(4)) + (np.array(w, np.uint32),)
    block = save_pathways(str(tmp_path / 'x' / 'pp_pathway'), Stub(), (0.5,))
    want = {'days', 'pathway_weights', 'pathway_thresholds', 'pathway_connectivity', 'pathway_days', 'pathway_anchors'}
    want |= {'pathway_' + name for name in W.ROW}
    with np.load(str(tmp_path / 'x' / 'pp_pathway.npz')) as fz:
        for k in range(2):
            for which in W.CLASSES:
                name = 'window_p%s%d' % (which, k)
                got = sparse.csr_matrix((fz[name + '_data'], fz[name + '_ind'], fz[name + '_indptr']),
                                        shape=(N, N)).toarray()
                assert np.array_equal(got, ref[which][k] / 6.0), name
                want |= {'%s_%s' % (name, t) for t in ('data', 'ind', 'indptr')}
        assert set(fz.files) == want
        for f, name in enumerate(W.ROW):
            a = fz['pathway_' + name]
            assert a.shape == (2, 4, 3) and a.dtype == np.uint32
            assert np.array_equal(a, ref['rows'][:, :, :, f].transpose(1, 2, 0)), name
        assert fz['pathway_weights'].tolist() == w and fz['pathway_thresholds'].tolist() == thr
        assert int(fz['pathway_connectivity']) == 8 and fz['pathway_days'].tolist() == days
        assert fz['pathway_anchors'].tolist() == [[8, 8]] and fz['days'].tolist() == ['window']
    assert json.loads(json.dumps(block)) == block
    assert block['thresholds'] == thr and block['connectivity'] == 8 and block['days'] == days
    assert block['levels'] == [0.5] and block['members'] == 3 and block['total_weight'] == 6.0
    assert block['anchors'] == [[8, 8]] and block['cell_area'] == 4.0
    for k in range(2):
        rec = block['pathways'][k]
        assert rec['founded'] == pathway_founded(ref['rows'][:, k, :, 3].sum(axis=1), w, (0.5,))
        for j, which in enumerate(W.CLASSES):
            assert rec['area_' + which] == range_area(ref['rows'][:, k, :, j].sum(axis=1), w, 4.0, (0.5,))
    assert block['pathways'][0]['founded']['p_any'] == 1.0 and block['pathways'][0]['area_secondary']['mean'] > 0


def test_the_command_line_knows_the_pathway_options():
    text = open(os.path.join(ROOT, 'scripts', 'run_predictive.py')).read()
    for opt in ('--pathways', '--pathway-connectivity', '--pathway-levels'):
        assert "add_argument('%s'" % opt in text, opt


def _emulator(tmp_path, flags, name):
    exe = str(tmp_path / name)
    src = os.path.join(ROOT, 'tests', 'host', 'pathway_emul.cpp')
    built = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-pthread'] + flags + ['-o', exe, src],
                           capture_output=True, text=True)
    return exe, built


def test_host_emulation_of_the_device_logic_under_the_sanitizers(tmp_path):
    """link, flatten, flag and class of ps_patch_core.h and ps_pathway_core.h, slot by slot, thread by thread in a
    scrambled order and with 8 threads, on crafted and pseudo-random sequences, both connectivities, N = 17, 33 and a
    wave-and-one size, against the emulator's own flood fill and patch-by-patch classification; every loop capped at
    4 N N passes.  Built with the address and the undefined-behaviour sanitizer; a child process."""
    exe, built = _emulator(tmp_path, ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'], 'emul_asan')
    assert built.returncode == 0, built.stderr[-2000:]
    out = subprocess.run([exe, '17', '33', '65'], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith('ok '), (out.stdout[-2000:], out.stderr[-2000:])
    assert int(out.stdout.split()[1]) == 3 * 16 * 2 * 2 * 2      # sizes, sequences, connectivities, orders, runs


def test_host_emulation_under_the_thread_sanitizer(tmp_path):
    """the same program built with -fsanitize=thread, where this compiler links it and its runtime starts"""
    exe, built = _emulator(tmp_path, ['-fsanitize=thread'], 'emul_tsan')
    if built.returncode != 0:
        pytest.skip('this compiler does not link -fsanitize=thread')
    out = subprocess.run([exe, '17', '33'], capture_output=True, text=True)
    if out.returncode != 0 and 'FATAL: ThreadSanitizer' in out.stderr and 'FAIL' not in out.stdout:
        pytest.skip('the thread sanitizer does not start here: %s' % out.stderr.strip().splitlines()[0])
    assert out.returncode == 0 and out.stdout.startswith('ok '), (out.stdout[-2000:], out.stderr[-2000:])

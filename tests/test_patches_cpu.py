"""CPU tests of the patch maps (predictive.PatchMaps, ps_patch_*): the numpy restatement (patch_ref) against a flood
fill in plain Python on the crafted shapes, the argument checks, the arithmetic of the patch-count posterior and of
the areas on hand-made rows, the layout of the saved file with a stub handle, the driver's refusals, and the host
emulation of the device logic (tests/host/patch_emul.cpp over csrc/ps_patch_core.h) under the sanitizers."""
import json
import os
import subprocess
import types

import numpy as np
import pytest

import patch_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('N', [17, 33])
@pytest.mark.parametrize('connectivity', [4, 8])
def test_the_restatement_matches_a_flood_fill_on_the_crafted_shapes(N, connectivity):
    seen = {}
    for name, f in P.shapes(N):
        assert set(np.unique(f)) <= {0.0, 1.0, 2.0, 3.0}, name
        for t in P.SHAPE_THR:
            mask = f >= t
            lab = P.labels(mask, connectivity)
            assert np.array_equal(lab, P.flood_labels(mask, connectivity)), (name, t)
            assert np.array_equal(lab >= 0, mask)
            got = P.member(f, t, connectivity)
            want = P.member(f, t, connectivity, P.flood_labels)
            assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
            row, main, sat = got
            assert np.array_equal(main | sat, mask) and not (main & sat).any()
            assert row['cells'] == mask.sum() and row['main_cells'] == main.sum()
            if row['npatch']:
                assert main.ravel()[row['main_label']] and not main.ravel()[:row['main_label']].any()
            else:
                assert row == dict(npatch=0, cells=0, main_cells=0, main_label=P.NONE, sat_cells_max=0)
            seen[name, t] = row
    # what each shape is there for, at the threshold that shows it
    half = (N * N + 1) // 2
    assert seen['empty', 0.5]['npatch'] == 0
    assert seen['full', 0.5] == dict(npatch=1, cells=N * N, main_cells=N * N, main_label=0, sat_cells_max=0)
    assert seen['first', 0.5]['main_label'] == 0 and seen['last', 0.5]['main_label'] == N * N - 1
    assert seen['checkerboard', 0.5]['npatch'] == (half if connectivity == 4 else 1)
    assert seen['spiral', 0.5]['npatch'] == 1 and seen['spiral', 0.5]['cells'] > N * N // 3
    assert seen['spiral', 1.5]['npatch'] > 2
    assert seen['comb', 0.5]['npatch'] == 1 and seen['comb', 0.5]['main_label'] == 0
    assert seen['comb', 1.5]['npatch'] == 1 + (N + 3) // 4             # the last row, and every other tooth's top
    for name, label in (('equal_left_first', N + 1), ('equal_right_first', N + 8)):
        assert seen[name, 2.5] == dict(npatch=2, cells=12, main_cells=6, main_label=label, sat_cells_max=6)
        assert seen[name, 1.5]['npatch'] == 3 and seen[name, 1.5]['sat_cells_max'] == 6
    for name in ('diagonal', 'antidiagonal'):
        assert seen[name, 0.5]['npatch'] == (2 if connectivity == 4 else 1)
    assert seen['ring_island', 0.5] == dict(npatch=2, cells=25, main_cells=24, main_label=2 * N + 2, sat_cells_max=1)
    for name in ('edge_next_row', 'edge_two_rows'):                    # the linear index does not wrap
        assert seen[name, 0.5] == dict(npatch=2, cells=2, main_cells=1, main_label=4 * N - 1, sat_cells_max=1)
    assert seen['last_row_col', 0.5] == dict(npatch=2, cells=2 * N, main_cells=2 * N - 1, main_label=N - 1,
                                             sat_cells_max=1)


def test_rows_follow_the_members_and_planes_do_not():
    fields = [np.array([f]) for _name, f in P.shapes(17)]
    w = [1 + i % 3 for i in range(len(fields))]
    whole = P.accumulate(fields, w, P.SHAPE_THR, 4)
    a, b = P.accumulate(fields[:5], w[:5], P.SHAPE_THR, 4), P.accumulate(fields[5:], w[5:], P.SHAPE_THR, 4)
    for key in ('main', 'sat'):
        assert np.array_equal(a[key] + b[key], whole[key]) and np.array_equal(b[key] + a[key], whole[key])
    for key in P.FIELDS:
        assert np.array_equal(np.concatenate([a[key], b[key]]), whole[key])
    exceed = sum(wi * (f >= t) for f, wi in zip(fields, w) for t in [P.SHAPE_THR[0]])
    assert np.array_equal(whole['main'][0] + whole['sat'][0], exceed)


def test_check_patches_and_the_driver_refuse_before_any_evaluation():
    from parasitoids_amd.predictive import PatchMaps, check_patches, posterior_predictive
    assert check_patches([1, 10]) == ([1.0, 10.0], 4, [0.05, 0.5, 0.95])
    assert check_patches(dict(thresholds=(2.5,), connectivity=8, levels=[1.0, 0.1]), days=[0, 3]) == ([2.5], 8, [1.0, 0.1])
    for bad in ([0.0, 1.0], [-1.0], [float('nan')], [float('inf')], [10, 1], [1, 1], [1, 2, 3, 4, 5], [], ['a'], 1.0):
        with pytest.raises(ValueError):
            check_patches(bad)
        with pytest.raises(ValueError):
            check_patches(dict(thresholds=bad))
        with pytest.raises(ValueError):
            PatchMaps(None, bad)                     # refused before the model is touched
    for bad in (dict(connectivity=8), dict(thresholds=[1], conn=8), dict(thresholds=[1], connectivity=5),
                dict(thresholds=[1], connectivity=6), dict(thresholds=[1], connectivity='8'),
                dict(thresholds=[1], connectivity=True), dict(thresholds=[1], levels=[0.0]),
                dict(thresholds=[1], levels=[1.5]), dict(thresholds=[1], levels=['x'])):
        with pytest.raises(ValueError):
            check_patches(bad)
    with pytest.raises(ValueError):
        PatchMaps(None, [1.0], connectivity=5)
    for days in ([], [3, 1], [-1, 2], list(range(33))):
        with pytest.raises(ValueError):
            check_patches([1.0], days=days)

    def never(theta):
        raise AssertionError('evaluated')
    from parasitoids_amd import mcmc
    names = [m[0] for m in mcmc.MODEL_BLOCK]
    chain = (np.zeros((3, len(names))), names)
    model = types.SimpleNamespace(days=list(range(6)), rad_dist=10000.0, rad_res=64,
                                  evaluate=lambda *a, **k: never(None))
    with pytest.raises(ValueError, match='patches= needs the device'):
        posterior_predictive(None, chain, evaluate=never, patches=[1.0])
    # after the existing checks: of two bad arguments the other one is reported
    with pytest.raises(ValueError, match='fraction'):
        posterior_predictive(None, chain, core_range=[0.5, 1.5], patches=[2.0, 1.0])
    with pytest.raises(ValueError, match='different model'):
        posterior_predictive(model, (np.zeros((3, 1)), ['x']), patches=[2.0, 1.0])
    with pytest.raises(ValueError, match='PopModel'):
        posterior_predictive(None, chain, patches=[2.0, 1.0])
    with pytest.raises(ValueError, match='strictly increasing'):
        posterior_predictive(model, chain, patches=[2.0, 1.0])
    with pytest.raises(ValueError, match='connectivity'):
        posterior_predictive(model, chain, patches=dict(thresholds=[1.0], connectivity=5))
    with pytest.raises(ValueError, match='days'):
        posterior_predictive(model, chain, patches=[1.0], days=[2, 1])
    with pytest.raises(ValueError, match='arrival'):       # an existing check comes first
        posterior_predictive(model, chain, arrival=[2.0, 1.0], patches=[2.0, 1.0])


def test_number_and_area_arithmetic_on_hand_made_rows():
    from parasitoids_amd.predictive import (PatchMaps, patch_number, patch_satellite_share, range_area,
                                            weighted_lower_quantile)
    npatch, w = [1, 0, 3, 2], [1, 1, 6, 2]            # the second member holds nothing
    n = patch_number(npatch, w, (0.05, 0.5, 0.95), day=2)
    assert n == {'day': 2, 'mean': (1 + 0 + 18 + 4) / 10, 'p_fragmented': 0.8, 'p_empty': 0.1,
                 'quantiles': [0.0, 3.0, 3.0]}
    assert n['quantiles'] == [float(weighted_lower_quantile(npatch, w, p)) for p in (0.05, 0.5, 0.95)]
    with pytest.raises(ValueError):
        patch_number([], [])
    cells, main = np.array([10, 0, 40, 20]), np.array([10, 0, 30, 15])
    assert patch_satellite_share(cells, main, w) == (0.0 * 1 + 0.25 * 6 + 0.25 * 2) / 9
    assert patch_satellite_share([0, 0], [0, 0], [1, 2]) is None

    class Stub(PatchMaps):                             # the accessors over hand-made rows, no device
        def __init__(self):
            self.cell_area, self.days = 25.0, [2]

        def _members(self, k, day):
            u = np.uint32
            return (np.array(npatch, u), cells.astype(u), main.astype(u), np.array([3, 0xffffffff, 0, 7], u),
                    np.array([0, 0, 6, 5], u), np.array(w, u))
    S = Stub()
    assert S.number(0, 2) == n
    assert S.patches(0, 2).tolist() == npatch and S.main_label(0, 2).tolist() == [3, -1, 0, 7]
    assert S.main_label(0, 2).dtype == np.int64 and S.largest_satellite(0, 2).tolist() == [0, 0, 6, 5]
    assert S.area(0, 2, 'main') == range_area(main, w, 25.0, (0.05, 0.5, 0.95), 2)
    assert S.area(0, 2, 'satellite')['mean'] == (0 + 0 + 60 + 10) / 10 * 25.0
    assert S.area(0, 2, 'all', [0.5])['quantiles'] == [40 * 25.0]
    with pytest.raises(ValueError):
        S.area(0, 2, 'both')
    assert S.weights.tolist() == w and S.weights.dtype == np.int64


def test_save_and_load_layout_with_a_stub_handle(tmp_path):
    from scipy import sparse
    from parasitoids_amd.predictive import patch_number, patch_satellite_share, save_patches
    N, days, thr, w = 17, [0, 3], [1.0, 2.0], [2, 1, 3]
    fields = [np.array([f, g]) for (_n, f), (_m, g) in zip(P.shapes(N)[4:7], P.shapes(N)[9:12])]
    ref = P.accumulate(fields, w, thr, 8)

    class Stub():
        thresholds, connectivity, members, total_weight, cell_area = thr, 8, 3, 6.0, 4.0

        def __init__(self):
            self.days = days

        def prob(self, k, d, which):
            return ref['main' if which == 'main' else 'sat'][k, days.index(d)] / 6.0

        def _members(self, k, d):
            return tuple(ref[name][:, k, days.index(d)].astype(np.uint32) for name in P.FIELDS) + (np.array(w, np.uint32),)
    block = save_patches(str(tmp_path / 'x' / 'pp_patch'), Stub(), (0.5,))
    want = {'days', 'patch_weights', 'patch_thresholds', 'patch_connectivity', 'patch_days'}
    want |= {'patch_' + name for name in P.FIELDS}
    with np.load(str(tmp_path / 'x' / 'pp_patch.npz')) as fz:
        for s, d in enumerate(days):
            for k in range(2):
                for tag, key in (('pmain', 'main'), ('psat', 'sat')):
                    name = '%d_%s%d' % (d, tag, k)
                    got = sparse.csr_matrix((fz[name + '_data'], fz[name + '_ind'], fz[name + '_indptr']),
                                            shape=(N, N)).toarray()
                    assert np.array_equal(got, ref[key][k, s] / 6.0), name
                    want |= {'%s_%s' % (name, t) for t in ('data', 'ind', 'indptr')}
        assert set(fz.files) == want
        for name in P.FIELDS:
            a = fz['patch_' + name]
            assert a.shape == (2, 2, 3) and a.dtype == (np.int64 if name == 'main_label' else np.uint32)
            wanted = np.where(ref[name] == P.NONE, -1, ref[name]) if name == 'main_label' else ref[name]
            assert np.array_equal(a, wanted.transpose(1, 2, 0)), name
        assert fz['patch_weights'].tolist() == w and fz['patch_thresholds'].tolist() == thr
        assert int(fz['patch_connectivity']) == 8 and fz['patch_days'].tolist() == days
    assert json.loads(json.dumps(block)) == block
    assert block['thresholds'] == thr and block['connectivity'] == 8 and block['days'] == days
    assert block['levels'] == [0.5] and block['members'] == 3 and block['total_weight'] == 6.0
    for k in range(2):
        for s, d in enumerate(days):
            rec = patch_number(ref['npatch'][:, k, s], w, (0.5,), d)
            assert block['number'][k][s] == {
                'day': d, 'p_fragmented': rec['p_fragmented'], 'mean_patches': rec['mean'],
                'quantiles': rec['quantiles'], 'p_empty': rec['p_empty'],
                'satellite_share': patch_satellite_share(ref['cells'][:, k, s], ref['main_cells'][:, k, s], w)}


def _emulator(tmp_path, flags, name):
    exe = str(tmp_path / name)
    src = os.path.join(ROOT, 'tests', 'host', 'patch_emul.cpp')
    built = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-pthread'] + flags + ['-o', exe, src],
                           capture_output=True, text=True)
    return exe, built


def test_host_emulation_of_the_device_logic_under_the_sanitizers(tmp_path):
    """link, flatten, sizes and pick of ps_patch_core.h, thread by thread in a scrambled order and with 8 threads
    joining concurrently, on every crafted shape, both connectivities, N = 17 and 33 and a wave-and-one size, against
    the emulator's own flood fill; every loop capped at 4 N N passes.  Built with the address and the
    undefined-behaviour sanitizer."""
    exe, built = _emulator(tmp_path, ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'], 'emul_asan')
    assert built.returncode == 0, built.stderr[-2000:]
    out = subprocess.run([exe, '17', '33', '65'], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith('ok '), (out.stdout[-2000:], out.stderr[-2000:])
    assert int(out.stdout.split()[1]) == 3 * 15 * 2 * 3 * 2      # sizes, shapes, connectivities, orders, runs


def test_host_emulation_under_the_thread_sanitizer(tmp_path):
    """the same program built with -fsanitize=thread, where this compiler links it and its runtime starts"""
    exe, built = _emulator(tmp_path, ['-fsanitize=thread'], 'emul_tsan')
    if built.returncode != 0:
        pytest.skip('this compiler does not link -fsanitize=thread')
    out = subprocess.run([exe, '17', '33'], capture_output=True, text=True)
    if out.returncode != 0 and 'FATAL: ThreadSanitizer' in out.stderr and 'FAIL' not in out.stdout:
        pytest.skip('the thread sanitizer does not start here: %s' % out.stderr.strip().splitlines()[0])
    assert out.returncode == 0 and out.stdout.startswith('ok '), (out.stdout[-2000:], out.stderr[-2000:])

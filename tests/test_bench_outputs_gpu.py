"""`bench.py --dump-outputs DIR` writes what the timed chain computed in its last stack: the per-day
statistics and the day solutions at a fixed sample of cells -- the same numbers a caller gets from
`chain_stats` / `chain_solution` of a solver that ran the same stack."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dumped_outputs_are_the_chain_results(tmp_path):
    R, K, nd = 200, 201, 4
    out = tmp_path / 'dump'
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3',
                        '--warmup', '1', '--rad-res', str(R), '--kshape', str(K), '--ndays', str(nd),
                        '--dump-outputs', str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d['steps'] == 3 and d['warmup'] == 1 and d['unit'] == 'grid-days/s' and d['dtype'] == 'f64'
    assert d['value'] > 0 and abs(d['value'] - nd / (d['ms_per_step'] * 1e-3)) < 0.01 * d['value']
    assert 'roofline' not in d and 'cpu_baseline' not in d          # --full only
    stats = np.load(out / 'day_stats.npy')
    samples = np.load(out / 'day_samples.npy')
    assert stats.dtype == np.float64 and samples.dtype == np.float64
    assert stats.shape == (nd, 5) and samples.shape[0] == nd
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 * 1024 * 1024

    import bench
    from parasitoids_amd import hip_lib, synthetic
    state, kernels, _ = synthetic.make_stack(R=R, K=K, ndays=nd, seed=20240613)
    s = hip_lib.HipSolve(state, [K, K], mode='fast', chain_only=True)
    s.set_kernels(kernels)
    for _ in range(1 + 3):                     # the bench's warmup and timed steps, in the same order
        s.set_state(state)
        s.run_chain(0, nd, negval=1e-8, scale=1.0, renorm=True)
    st = s.chain_stats(0, nd)
    rows, cols = bench.dump_cells(2 * R + 1)
    for day in range(nd):
        want = [st[day].nnz, st[day].sum, st[day].delta, st[day].padmax, st[day].flag]
        np.testing.assert_allclose(stats[day], want, rtol=1e-12, atol=1e-15)
        sol = s.chain_solution(day, st[day], fmt='csr')
        np.testing.assert_allclose(samples[day], np.asarray(sol[rows, cols]).ravel(), rtol=0, atol=1e-12)
    assert samples.max() > 0
    s.close()

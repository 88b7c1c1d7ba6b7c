"""Every FFT size and pipeline of the day chain on BROADBAND inputs against an exact reference.

The other GPU tests above a 360-point torus feed the chain Gaussian (or smooth real-wind) day kernels,
whose spectrum is below 1e-6 in over 90 % of the frequency bins (pinned in test_sparse_chain_ref_cpu.py):
they verify the low frequencies of each transform.  Here states and kernels are 3..8 points -- flat
spectra, every bin carries weight -- and the reference is the exact chain of sparse convolutions
(sparse_chain_ref.exact_chain, longdouble on triplets, nothing shared with the library).  Sparse inputs
also sit on the edges of the zero-skipping logic: live-row ranges of kernels and states, the staging
capacity of the two-role column pass, the quiet pad rows, the compact-kernel route; PS_POISON (conftest)
turns a read of a row that the writing side skipped into a NaN.

Checks per run (tolerances as in test_random_small_chains_against_oracle / test_auto_mode_routes):
every day flag and nnz equal to the reference, sum + delta * nnz == 1 to 1e-12, the RAW record (gather
with no threshold) at all support cells and as many random other cells to 1e-13; the whole field
(dense) to 1e-13 on every day for N <= 2600 and on the last day at any size; the thresholded solution
of the last day to 1e-12.  Each run prints its worst error (pytest -s)."""
import numpy as np
import pytest

import sparse_chain_ref as SR

pytestmark = pytest.mark.gpu

KNOBS = ('PS_TPIPE', 'PS_NO_DIRECT', 'PS_NO_RS', 'PS_WIDE_MIN_N', 'PS_NO_FOLD_FUSE', 'PS_FUSED_DAYS')


@pytest.fixture(scope='module')
def hip_lib():
    from parasitoids_amd import hip_lib
    return hip_lib


def _set_knobs(monkeypatch, **env):
    """The library reads the environment when a solver is created."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _dense_err(s, d, day):
    got = s.dense(0, d)
    got[day.rows, day.cols] -= day.vals.astype(np.float64)
    return max(got.max(), -got.min())        # NaN propagates


def _check_run(s, ref, label):
    """All checks of one finished run_chain against the exact reference; prints the worst error."""
    from parasitoids_amd import _lib as L
    N, nd = s.dom_len, len(ref)
    st = s.chain_stats(0, nd)
    rng = np.random.default_rng(N + nd)
    bad = []
    worst = 0.0

    def check(what, d, err, tol):
        nonlocal worst
        err = float(err)
        if not err < tol:                    # a NaN fails
            bad.append('%s day %d: %.3e (tolerance %g)' % (what, d, err, tol))
        worst = max(worst, err) if err == err else float('nan')

    for d, (day, x) in enumerate(zip(ref, st)):
        if bool(x.flag) != day.flag:
            bad.append('flag day %d: %s, reference %s' % (d, bool(x.flag), day.flag))
        if x.nnz != day.nnz:
            bad.append('nnz day %d: %d, reference %d' % (d, x.nnz, day.nnz))
        if not abs(x.sum + x.delta * x.nnz - 1.0) < 1e-12:
            bad.append('sum + delta nnz day %d: 1 %+.3e' % (d, x.sum + x.delta * x.nnz - 1.0))
        rows, cols, want = SR.check_cells(day, N, rng)
        got = s.gather(L.REC_CHAIN, d, rows, cols, negval=-1.0)   # nothing is below -1: the raw record
        check('gather', d, np.abs(got - want).max(), 1e-13)
        if N <= 2600 or d == nd - 1:
            check('dense', d, _dense_err(s, d, day), 1e-13)
    sol = s.chain_solution(nd - 1, st[nd - 1]).tocsr()
    check('solution', nd - 1, abs(sol - SR.sol_csr(ref[-1], N)).max(), 1e-12)
    print('BROADBAND %s fft=%d N=%d days=%d flags=%s worst=%.2e' % (
        label, s.fft_len, N, nd, ''.join('01'[d.flag] for d in ref), worst))
    assert not bad, label + ': ' + '; '.join(bad)
    return worst


def _run(hip_lib, state, K, kernels, ref, label, mode, full_column=None, fft_len=None, chain_only=False):
    s = hip_lib.HipSolve(state, [K, K], mode=mode, chain_only=chain_only)
    try:
        if fft_len is not None:
            assert s.fft_len == fft_len, (label, s.fft_len)
        s.set_kernels(kernels)
        s.run_chain(renorm=True)
        _check_run(s, ref, label)
        if full_column is not None:
            assert s.full_column == full_column, label
        return s
    finally:
        s.close()


# ------------------------------------------------------------------ (a) every register-resident size, fast mode
@pytest.mark.parametrize('L', SR.rs_sizes(), ids=str)
def test_every_register_resident_size_broadband(hip_lib, monkeypatch, L):
    """Fast mode with the fast torus equal to the reference torus (N + K // 2 == L, so the result must equal
    the exact chain to round-off), per size a clean six-day chain (wide, band, wide, one-sided, wide, wide:
    speculative windows of 2 and 4 days, chained passes) and a flagged three-day chain (single-day passes,
    predicated re-transform, deferred column half), through the default route, the full-column pipeline,
    the tiled pipeline, and exact mode (register-resident rows behind the tiled column passes)."""
    from parasitoids_amd import _lib
    geo = {}
    for chain in ('clean', 'edge'):
        N, K, state, kernels = SR.fast_geometry(L, chain)
        ref = SR.exact_chain(state, kernels, N)
        assert any(d.flag for d in ref) == (chain == 'edge')
        geo[chain] = (state, K, kernels, ref)
        _set_knobs(monkeypatch)
        assert _lib.load().ps_fast_size(N, K) == L
    for tag, chain, mode, env, fc in (('default', 'clean', 'fast', {}, None),
                                      ('full-column', 'clean', 'fast', {'PS_TPIPE': '1'}, True),
                                      ('full-column', 'edge', 'fast', {'PS_TPIPE': '1'}, None),
                                      ('tiled', 'edge', 'fast', {'PS_TPIPE': '0'}, False),
                                      ('exact', 'edge', 'exact', {}, None)):
        _set_knobs(monkeypatch, **env)
        _run(hip_lib, *geo[chain], 'a L=%d %s-%s-%s' % (L, mode, tag, chain), mode, full_column=fc, fft_len=L)


# ------------------------------------------------------------------ (b) every register-resident size, fold mode
# Sizes at which no domain within 20 steps below L - 3m gives fft_len == L with the full-column pipeline
# (each with its reason).  A size that is neither hit nor listed here fails.
FOLD_UNREACHABLE = {}


@pytest.mark.parametrize('L', SR.rs_sizes(), ids=str)
def test_every_register_resident_size_broadband_fold(hip_lib, monkeypatch, L):
    """Fold mode (linear convolution on the FFT size L >= N + 3m, folded back onto the reference torus): three
    flagged days of wide kernels from the corners of the domain (truncation inside the next row pass), and a
    clean four-day chain."""
    _set_knobs(monkeypatch, PS_TPIPE='1')
    m = SR.fold_m(L)
    K = 2 * m + 1
    hit = None
    for step in range(21):
        N = L - 3 * m - 2 * step
        _, state, _ = SR.fold_geometry(L, N, 'edge')
        s = hip_lib.HipSolve(state, [K, K], mode='fold', chain_only=True)
        try:
            ok = s.fft_len == L and s.full_column
        finally:
            s.close()
        if ok:
            hit = N
            break
    if L in FOLD_UNREACHABLE:
        assert hit is None, 'size %d is reachable: take it out of FOLD_UNREACHABLE' % L
        return
    assert hit is not None, 'fold mode never ran on FFT size %d' % L
    N = hit
    for chain in ('edge', 'clean'):
        _, state, kernels = SR.fold_geometry(L, N, chain)
        ref = SR.exact_chain(state, kernels, N)
        assert any(d.flag for d in ref) == (chain == 'edge')
        _run(hip_lib, state, K, kernels, ref, 'b L=%d fold-%s' % (L, chain), 'fold', full_column=True, fft_len=L,
             chain_only=True)


# ------------------------------------------------------------------ (c) below and beside the register-resident sizes
@pytest.mark.parametrize('N,K,nd,direct', SR.AWKWARD_CASES, ids=lambda v: str(v))
def test_awkward_pads_broadband(hip_lib, monkeypatch, N, K, nd, direct):
    """Exact mode on the pads of test_chain_with_flags_at_awkward_sizes (N + K // 2 is the stated P with N odd as
    it is), a prime pad and the reference torus of the full-size workload: wide kernels from the corners of the
    domain; then band kernels, which are compact.  Where the column transform is split into short sub-passes
    (`direct`) they take the direct-sum first column sub-pass -- asserted -- and run once more with
    PS_NO_DIRECT=1 through the FFT sub-pass; at 1021 (no split) and 5121 (second sub-pass of 569 points) there
    is no direct route and one band run covers what there is."""
    P = N + K // 2
    assert P in (1300, 2574, 1551, 1021, 5121) and N % 2 == 1
    state, chains = SR.awkward_geometry(N, K, nd)
    runs = [('wide', {}), ('band', {})] + ([('band', {'PS_NO_DIRECT': '1'})] if direct else [])
    for kind, env in runs:
        kernels = chains[kind]
        ref = SR.exact_chain(state, kernels, N)
        if kind == 'wide':
            assert ref[0].flag
        _set_knobs(monkeypatch, **env)
        s = hip_lib.HipSolve(state, [K, K], mode='exact')
        try:
            assert s.mode == 'exact' and s.fft_len == P
            s.set_kernels(kernels)
            s.run_chain(renorm=True)
            _check_run(s, ref, 'c P=%d exact-%s%s' % (P, kind, '-nodirect' if env else ''))
            if kind == 'band':
                assert s.kernels_direct == (direct and not env)
        finally:
            s.close()


@pytest.mark.parametrize('start,wide_min_n,routes', [('edge', '0', [1, 1, 1, 1]), ('edge', None, [2, 2, 2, 2]),
                                                     ('late', '0', [0, 0, 1, 1]), ('late', None, [0, 0, 2, 2])])
def test_auto_mode_routes_broadband(hip_lib, monkeypatch, start, wide_min_n, routes):
    """PS_MODE_AUTO at N = 301, K = 101 (P = 351 = 3^3 13), every route it has for days whose pad mass is either
    nothing or far above the threshold: 0 the fast-torus front (the clean prefix of the 'late' chain), 1 the wide
    fast-torus helper (flagged days, with PS_WIDE_MIN_N=0 so that this small domain gets one), 2 the fold child
    (the same flagged days with PS_WIDE_MIN_N at its default, where a domain below 1500 cells has no wide helper).
    (The fourth hand-over, wide helper -> fold child on a dusty day, needs pad mass between 1e-15 and 1e-8, which
    the exact reference rules out; test_auto_mode_routes covers it.)"""
    N, K = SR.AUTO_N, SR.AUTO_K
    state, kernels = SR.auto_geometry(start)
    ref = SR.exact_chain(state, kernels, N)
    assert [d.flag for d in ref] == [r != 0 for r in routes]
    _set_knobs(monkeypatch, **({} if wide_min_n is None else {'PS_WIDE_MIN_N': wide_min_n}))
    s = hip_lib.HipSolve(state, [K, K], mode='auto', chain_only=True)
    try:
        assert s.mode == 'auto'
        s.set_kernels(kernels)
        s.run_chain(renorm=True)
        label = 'c P=351 auto-%s-%s' % (start, 'wide' if wide_min_n else 'child')
        _check_run(s, ref, label)
        got = s.auto_route(0, len(ref)).tolist()
        print('BROADBAND %s auto_route=%s' % (label, got))
        assert got == routes
    finally:
        s.close()

"""The first chained window of a run transforms the state's columns itself: after a set_state only the row half
of the state's transform is enqueued, and role A of the two-role pass (k_colfull_dual<..., true>) runs the
column half in its idle first slot.  Against the separate forward column launch (PS_NO_STATE_FUSE=1): records,
flags and statistics bit for bit, the per-call API with a pending state, and the launch counts."""
import ctypes as C
import functools

import numpy as np
import pytest
from scipy import sparse

pytestmark = pytest.mark.gpu

ND = 8
KNOB = 'PS_NO_STATE_FUSE'
# (R, K, FFT size, PS_FAST_SIZE or None)
#   3360 = 16 x 15 x 14: the smallest two-role size; its remainder of 145 columns (1681 = 6 x 256 + 145) is not split
#   3584: 1793 columns = 7 x 256 + 1, one tail column (its state column goes through the short forward launch)
#   3600 = 16 x 15 x 15: 1801 columns, a remainder of 9
SIZES = [(1200, 1601, 3360, None), (1300, 1801, 3584, None), (1300, 1801, 3600, 3600)]
STATES = ['centre', 'flagging', 'random', 'edge_rows', 'edge_rows_device']


@pytest.fixture(scope='module')
def hip_lib():
    from parasitoids_amd import hip_lib
    return hip_lib


@functools.lru_cache(maxsize=None)
def _kernels(R, K):
    from parasitoids_amd import synthetic
    _, kernels, _ = synthetic.make_stack(R=R, K=K, ndays=ND, seed=11, sigma=(15.0, 40.0), shift=40)
    return tuple(kernels)


def _state(name, R):
    N = 2 * R + 1
    if name == 'centre':
        return sparse.coo_matrix(([1.0], ([R], [R])), shape=(N, N))
    if name == 'flagging':      # raises the boundary flag inside the fused window: recovery with no initial spectrum in memory
        return sparse.coo_matrix(([1.0], ([N - 71], [N - 71])), shape=(N, N))
    if name == 'random':
        rng = np.random.default_rng(5)
        st = sparse.coo_matrix((rng.random(80) + 0.1, (rng.integers(2, 40, 80), rng.integers(R - 30, R + 30, 80))), shape=(N, N))
        st.sum_duplicates()
        return (st / st.sum()).tocoo()
    # entries in the first and in the last row of the domain: the live-row range clipped at both ends
    rows = np.array([0, 0, R, N - 1, N - 1])
    cols = np.array([R - 7, R + 12, R, R - 3, R + 9])
    return sparse.coo_matrix((np.array([0.15, 0.2, 0.3, 0.25, 0.1]), (rows, cols)), shape=(N, N))


def _set_state(s, name, R):
    st = _state(name, R)
    if name != 'edge_rows_device':
        s.set_state(st)
        return
    # device triplets of an N x N "kernel": no row range is known, all N rows are live
    from parasitoids_amd import _lib as L
    N = 2 * R + 1
    hip = _hip_runtime()
    bufs = []
    try:
        for arr in (st.row.astype(np.int32), st.col.astype(np.int32), st.data.astype(np.float64)):
            arr = np.ascontiguousarray(arr)
            ptr = C.c_void_p()
            assert hip.hipMalloc(C.byref(ptr), C.c_size_t(arr.nbytes)) == 0
            bufs.append(ptr)
            assert hip.hipMemcpy(ptr, C.c_void_p(arr.ctypes.data), C.c_size_t(arr.nbytes), 1) == 0   # host to device
        L.check(s._lib.ps_solver_set_state_device(s._h, bufs[0], bufs[1], bufs[2], int(st.nnz), N))   # (synchronises)
    finally:
        for ptr in bufs:
            hip.hipFree(ptr)


def _hip_runtime():
    """the HIP runtime the library itself is linked against, as this process has it loaded"""
    from parasitoids_amd import _lib
    _lib.load()
    with open('/proc/self/maps') as f:
        for line in f:
            if 'libamdhip64' in line:
                return C.CDLL(line.split()[-1])
    raise RuntimeError('libamdhip64 is not loaded')


def _solver(hip_lib, monkeypatch, knob, R, K, fft, fast):
    monkeypatch.setenv('PS_TPIPE', '1')
    monkeypatch.delenv(KNOB, raising=False)
    monkeypatch.delenv('PS_FAST_SIZE', raising=False)
    if knob:
        monkeypatch.setenv(KNOB, '1')
    if fast:
        monkeypatch.setenv('PS_FAST_SIZE', str(fast))
    N = 2 * R + 1
    s = hip_lib.HipSolve(sparse.coo_matrix(([1.0], ([R], [R])), shape=(N, N)), [K, K], mode='fast', chain_only=True)
    assert s.fft_len == fft and s.full_column
    assert s.get_option(KNOB) == (1.0 if knob else 0.0)
    s.set_kernels(list(_kernels(R, K)))
    s.run_chain(renorm=True)        # clean first run: the next one opens with one 8-day window
    assert not any(x.flag for x in s.chain_stats(0, ND))
    return s


def _collect(s):
    st = s.chain_stats(0, ND)
    return [s.dense(0, d) for d in range(ND)], [(x.flag, x.nnz, x.sum, x.delta, x.padmax) for x in st]


def _same(a, b):
    assert a[1] == b[1]
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize('name', STATES)
@pytest.mark.parametrize('R,K,fft,fast', SIZES)
def test_state_fused_window_is_bit_identical(hip_lib, monkeypatch, R, K, fft, fast, name):
    """set_state + run_chain with one hinted 8-day window, default against PS_NO_STATE_FUSE=1: every day's record
    np.array_equal, every day's (flag, nnz, sum, delta, padmax) equal.  The fused stack has no forward column
    launch of the state (class col_fwd_a); a run that flags inside the window recovers through one, from the
    flagged day's record, in both variants."""
    runs, fwd = {}, {}
    for knob in (False, True):
        s = _solver(hip_lib, monkeypatch, knob, R, K, fft, fast)
        try:
            _set_state(s, name, R)
            s.prof_enable(True, every=1)
            s.run_chain(renorm=True)
            runs[knob] = _collect(s)
            fwd[knob] = s.prof_launches()['col_fwd_a']
        finally:
            s.close()
    flagged = any(f for f, *_ in runs[True][1])
    if name == 'centre':
        assert not flagged
    if name == 'flagging':
        assert flagged
    assert fwd[True] == fwd[False] + 1, fwd          # the state's column launch: there with the knob, gone without
    if not flagged:
        assert fwd[False] == 0, fwd
    _same(runs[False], runs[True])


@pytest.mark.parametrize('R,K,fft,fast', SIZES[:1])
def test_pending_state_serves_the_per_call_api_and_a_second_run(hip_lib, monkeypatch, R, K, fft, fast):
    """A state that no run_chain has consumed yet: get_cursol, and fftconv2 + get_cursol, build its spectrum the
    usual way and give what they give with the knob set.  And a second run_chain without a new set_state goes on
    from the first one's final spectrum (written back by the fused pass) exactly as it does with the knob."""
    N = 2 * R + 1
    out = {}
    for knob in (False, True):
        s = _solver(hip_lib, monkeypatch, knob, R, K, fft, fast)
        try:
            got = []
            _set_state(s, 'random', R)
            got.append(s.get_cursol([N, N]).toarray())
            _set_state(s, 'edge_rows', R)
            s.fftconv2(_kernels(R, K)[0])
            got.append(s.get_cursol([N, N]).toarray())
            _set_state(s, 'centre', R)
            s.run_chain(renorm=True)
            first = _collect(s)
            s.run_chain(renorm=True)
            second = _collect(s)
            out[knob] = (got, first, second)
        finally:
            s.close()
    for a, b in zip(out[False][0], out[True][0]):
        assert np.array_equal(a, b)
    _same(out[False][1], out[True][1])
    _same(out[False][2], out[True][2])
    assert out[False][0][0].sum() > 0.5 and out[False][1][0][-1].sum() > 0.5

"""The persistent forward row pass over the live units of a kernel batch (k_row_fwd_rsp) against the
one-shot kernel it replaces there (PS_NO_FWD_PERSIST=1): records, flags and statistics bit for bit."""
import hashlib
import struct

import numpy as np
import pytest
from scipy import sparse

pytestmark = pytest.mark.gpu

ND = 8


@pytest.fixture(scope='module')
def hip_lib():
    from parasitoids_amd import hip_lib
    return hip_lib


def _kernels(R, K, seed):
    from parasitoids_amd import synthetic
    _, kernels, _ = synthetic.make_stack(R=R, K=K, ndays=ND, seed=seed, sigma=(15.0, 40.0), shift=40)
    return list(kernels)


def _stack_under_test(R, K):
    """Eight synthetic day kernels, three of them replaced by hand: a single entry at the centre (its
    torus row 0 shares a pair with a dead row), a blob confined to the top rows of the K x K box (one
    run of live units only), and an empty kernel (no live unit; last, because nothing survives it)."""
    kernels = _kernels(R, K, seed=11)
    M = K // 2
    kernels[3] = sparse.coo_matrix(([1.0], ([M], [M])), shape=(K, K))
    rr, cc = np.meshgrid(np.arange(0, 23), np.arange(M - 30, M + 31), indexing='ij')
    vv = np.exp(-((rr - 11.0) ** 2 + (cc - M) ** 2) / 90.0)
    kernels[5] = sparse.coo_matrix((vv.ravel() / vv.sum(), (rr.ravel(), cc.ravel())), shape=(K, K))
    kernels[7] = sparse.coo_matrix((K, K))
    return kernels


def _bits(x):
    return struct.pack('<d', float(x))


def _collect(s, first, count):
    st = s.chain_stats(first, count)
    stats = [(int(x.flag), int(x.nnz), _bits(x.sum), _bits(x.delta), _bits(x.padmax)) for x in st]
    recs = []
    for d in range(first, first + count):
        a = s.dense(0, d)
        recs.append((hashlib.sha1(a.tobytes()).hexdigest(), int(np.count_nonzero(a))))
    return stats, recs


def _run_variant(hip_lib, monkeypatch, env, R, K, fft, guard, kernels):
    for k in ('PS_NO_FWD_PERSIST', 'PS_KT_SPLIT'):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    N = 2 * R + 1
    state = sparse.coo_matrix(([1.0], ([R], [R])), shape=(N, N))
    s = hip_lib.HipSolve(state, [K, K], mode='fast', chain_only=True)
    try:
        assert s.fft_len == fft and s.full_column
        # another kernel set first: a live unit that the pass under test skipped would otherwise find
        # its right spectrum still in place from an earlier staging
        s.set_kernels(guard)
        s.run_chain(renorm=True)
        s.chain_stats(0, ND)
        out = {}
        s.set_state(state)
        s.set_kernels(kernels)
        s.run_chain(renorm=True)                    # first run on these kernels
        out['first'] = _collect(s, 0, ND)
        s.set_state(state)
        s.run_chain(renorm=True)                    # second run: hinted by the first
        out['second'] = _collect(s, 0, ND)
        s.set_state(state)
        s.run_chain(first=2, count=5, renorm=True)
        out['part'] = _collect(s, 2, 5)
        s.set_state(state)
        s.run_chain(first=7, count=1, renorm=True)  # a batch of one empty kernel: nothing to launch
        out['empty'] = _collect(s, 7, 1)
    finally:
        s.close()
    return out


# Row pairs per workgroup (NP) and units per 128-byte output line (KL = 4 / NP, 1 from NP = 3 on):
#   3360 = 16 x 15 x 14, 3584 = 16 x 16 x 14: four waves per pair, NP = 3, KL = 1
#   3456 = 16 x 18 x 12: five waves per pair, NP = 2, KL = 2 -- as the 5184-point headline size: list position
#          -> line -> unit inside it, the XCD remapping with KL > 1, dead units inside a live line walked past
#   1008 = 16 x 9 x 7: three waves per pair, NP = 4, KL = 1
# (NP = 1 sizes, 2800 or 5600 for instance, keep the one-shot kernel: test_row_fwd_live_cpu.py.)
@pytest.mark.parametrize('R,K,fft,np_want', [(1200, 1601, 3360, 3), (1300, 1801, 3584, 3), (1250, 1801, 3456, 2),
                                             (350, 401, 1008, 4)])
def test_persistent_kernel_row_pass_is_bit_identical(hip_lib, monkeypatch, R, K, fft, np_want):
    """Default (k_row_fwd_rsp over the live units) against PS_NO_FWD_PERSIST=1 (k_row_fwd_rs over the
    whole torus): every day's record must be equal bit for bit (np.array_equal; compared as digests of
    the arrays' bytes, which is no weaker), and so must (flag, nnz, sum, delta, padmax) -- for a first
    run, a second run that the first one hinted, a run over days 2..6, and a run over the one empty
    kernel.  At 3360 also with PS_KT_SPLIT=2: the later days' kernels are then staged in a second part
    (transform_kernels with slot0 > 0) on the low-priority stream."""
    import ctypes as C
    from parasitoids_amd import _lib
    np_got, persistent = C.c_int32(-1), C.c_int32(-1)
    assert _lib.load().ps_row_fwd_info(fft, C.byref(np_got), C.byref(persistent)) == 0
    assert (np_got.value, persistent.value) == (np_want, 1)
    monkeypatch.setenv('PS_TPIPE', '1')
    guard = _kernels(R, K, seed=23)
    kernels = _stack_under_test(R, K)
    variants = [('persist', {}), ('oneshot', {'PS_NO_FWD_PERSIST': '1'})]
    if fft == 3360:
        variants += [('persist_split', {'PS_KT_SPLIT': '2'}),
                     ('oneshot_split', {'PS_KT_SPLIT': '2', 'PS_NO_FWD_PERSIST': '1'})]
    runs = {tag: _run_variant(hip_lib, monkeypatch, env, R, K, fft, guard, kernels) for tag, env in variants}
    ref = runs['oneshot']
    # the comparison is about something: the days before the empty kernel hold mass
    assert all(nz > 0 for _, nz in ref['first'][1][:7])
    for tag, got in runs.items():
        for what in ('first', 'second', 'part', 'empty'):
            assert got[what][0] == ref[what][0], (tag, what, 'statistics')
            assert got[what][1] == ref[what][1], (tag, what, 'records')

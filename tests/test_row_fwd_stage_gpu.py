"""The persistent forward row pass over kernel batches in its three forms -- the default (workgroups of one row
pair, two per CU, at the two-pair sizes), workgroups of RsCfg::NP pairs (PS_NO_FWD_SOLO=1) and the staged kernel
(PS_FWD_STAGE=1, k_row_fwd_rsps: the next live unit's source rows copied HBM -> LDS while one is transformed) --
against the one-shot kernel (PS_NO_FWD_PERSIST=1): records, flags and statistics bit for bit."""
import ctypes as C
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


def _blob(K, r0, r1, c0, c1):
    """a bump over box rows r0..r1 and columns c0..c1 (inclusive), every entry positive; sum 1"""
    rr, cc = np.meshgrid(np.arange(r0, r1 + 1), np.arange(c0, c1 + 1), indexing='ij')
    vv = np.exp(-((rr - 0.5 * (r0 + r1)) ** 2 + (cc - 0.5 * (c0 + c1)) ** 2) / 90.0)
    return sparse.coo_matrix((vv.ravel() / vv.sum(), (rr.ravel(), cc.ravel())), shape=(K, K))


def _mix(K, parts):
    """weighted sum of kernels as one coo matrix (the mass stays near the centre, the edges carry a little)"""
    m = sum(w * p.tocsr() for w, p in parts).tocoo()
    return sparse.coo_matrix((m.data, (m.row, m.col)), shape=(K, K))


def _stack_under_test(R, K):
    """Eight synthetic day kernels, six of them replaced by hand.  From the persistent kernel's test: a single
    entry at the centre, a blob confined to the top rows of the box, an empty kernel (last: nothing survives it).
    For the staging area's edges: entries in box columns 0 and K - 1 (the first and the last double of a staged
    row, at either parity); live rows that start at an odd and at an even row (both parities of row * K); a blob
    in the last rows of the box, row and column K - 1 included, on day 6 -- the last day of the batches 0..6
    and 2..6, whose last row ends the staged source, so its copy is the one that must not run past the end."""
    kernels = _kernels(R, K, seed=11)
    M = K // 2
    centre = _blob(K, M - 12, M + 12, M - 12, M + 12)
    edge = sparse.coo_matrix((np.full(10, 0.1), (np.repeat(np.arange(M - 2, M + 3), 2), np.tile([0, K - 1], 5))), shape=(K, K))
    kernels[0] = _mix(K, [(0.98, centre), (0.02, edge)])
    odd = M - 41 if (M - 41) % 2 else M - 40
    kernels[1] = _blob(K, odd, M + 20, M - 30, M + 30)           # live rows from an odd row on
    kernels[2] = _blob(K, odd + 1, M + 21, M - 30, M + 30)       # ... from an even one
    kernels[3] = sparse.coo_matrix(([1.0], ([M], [M])), shape=(K, K))
    kernels[5] = _blob(K, 0, 22, M - 30, M + 30)
    kernels[6] = _mix(K, [(0.9, centre), (0.1, _blob(K, K - 23, K - 1, K - 31, K - 1))])
    kernels[7] = sparse.coo_matrix((K, K))
    assert kernels[1].row.min() % 2 == 1 and kernels[2].row.min() % 2 == 0
    assert kernels[0].col.min() == 0 and kernels[0].col.max() == K - 1
    assert kernels[6].row.max() == K - 1 and kernels[6].col[kernels[6].row == K - 1].max() == K - 1
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
    for k in ('PS_FWD_STAGE', 'PS_NO_FWD_SOLO', 'PS_NO_FWD_PERSIST', 'PS_KT_SPLIT'):
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
        s.run_chain(first=2, count=5, renorm=True)  # days 2..6: the last-rows blob ends the batch
        out['part'] = _collect(s, 2, 5)
        s.set_state(state)
        s.run_chain(first=0, count=7, renorm=True)  # days 0..6: the same, seven slots
        out['head'] = _collect(s, 0, 7)
        s.set_state(state)
        s.run_chain(first=7, count=1, renorm=True)  # a batch of one empty kernel: nothing to launch
        out['empty'] = _collect(s, 7, 1)
    finally:
        s.close()
    return out


# 3456 = 16 x 18 x 12: NP = 2, two units per output line, the headline's class; 60 KB of exchange buffers + 4 rows
#        of 15 KB
# 1008 = 16 x 9 x 7: NP = 4
# 3360 = 16 x 15 x 14: NP = 3; with K = 1601 the six staged rows (6 x 13 KB) do not fit beside the exchange
#        buffers: the launcher must fall back to the plain persistent kernel; with K = 1401 (6 x 11 KB) they do
@pytest.mark.parametrize('R,K,fft,np_want,staged_want', [(1250, 1801, 3456, 2, 1), (350, 401, 1008, 4, 1),
                                                         (1200, 1601, 3360, 3, 0), (1250, 1401, 3360, 3, 1)])
def test_staged_kernel_row_pass_is_bit_identical(hip_lib, monkeypatch, R, K, fft, np_want, staged_want):
    """PS_FWD_STAGE=1 (the staged kernel where ps_row_fwd_stage_info says it fits, else the fallback), the
    default and PS_NO_FWD_SOLO=1 (k_row_fwd_rsp with one and with NP pairs per workgroup; the same launch at the
    sizes with NP != 2) against PS_NO_FWD_PERSIST=1 (k_row_fwd_rs over the whole torus): every day's record must
    be equal bit for bit (compared as digests of the arrays' bytes), and so must (flag, nnz, sum, delta, padmax) -- for a first run, a second run that the first one hinted, runs over days
    2..6 and 0..6, and a run over the one empty kernel.  At 3360 also with PS_KT_SPLIT=2: the later days'
    kernels are then staged in a second part (transform_kernels with slot0 > 0)."""
    from parasitoids_amd import _lib
    lib = _lib.load()
    np_got, persistent, staged = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    assert lib.ps_row_fwd_info(fft, C.byref(np_got), C.byref(persistent)) == 0
    assert (np_got.value, persistent.value) == (np_want, 1)
    assert lib.ps_row_fwd_stage_info(fft, K, C.byref(staged)) == 0
    assert staged.value == staged_want
    monkeypatch.setenv('PS_TPIPE', '1')
    guard = _kernels(R, K, seed=23)
    kernels = _stack_under_test(R, K)
    variants = [('stage', {'PS_FWD_STAGE': '1'}), ('default', {}), ('oneshot', {'PS_NO_FWD_PERSIST': '1'})]
    if np_want == 2:
        variants += [('wide', {'PS_NO_FWD_SOLO': '1'})]
    if fft == 3360:
        variants += [('stage_split', {'PS_FWD_STAGE': '1', 'PS_KT_SPLIT': '2'})]   # (unstaged: test_row_fwd_live_gpu.py)
    runs = {tag: _run_variant(hip_lib, monkeypatch, env, R, K, fft, guard, kernels) for tag, env in variants}
    ref = runs['oneshot']
    # the comparison is about something: the days before the empty kernel hold mass
    assert all(nz > 0 for _, nz in ref['first'][1][:7])
    for tag, got in runs.items():
        for what in ('first', 'second', 'part', 'head', 'empty'):
            assert got[what][0] == ref[what][0], (tag, what, 'statistics')
            assert got[what][1] == ref[what][1], (tag, what, 'records')

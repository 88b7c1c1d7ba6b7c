"""The deferred check of a chain run's last speculation window (`PS_NO_DEFER_CHECK`).

A fast-mode run on the full-column pipeline returns with its last window of days enqueued but not yet
verified; the library verifies it -- and redoes the days behind a flag -- at the start of the next call
that reads or changes anything of the run.  `set_state` does not settle it, it copies the caller's
triplets into pinned staging and enqueues.  Everything a caller can see must be BIT-identical to the
same sequence of calls with `PS_NO_DEFER_CHECK=1` (the call returns with the last window verified).

Stack: the one of `test_window_hint_changes_nothing` (R = 400, K = 401, 20 days, FFT 1008, unit mass at
cell (p, p)).  On the CPU oracle (reference torus 1001) p = 400 raises no flag, p = 625 flags from day 15,
p = 650 from day 12, p = 770 from day 0; the device runs on the 1008 torus and may differ by a day near
the threshold, so every case asserts its premise from the `PS_NO_DEFER_CHECK=1` run's own flags."""
import types

import numpy as np
import pytest
from scipy import sparse

pytestmark = pytest.mark.gpu

R, K, ND = 400, 401, 20
N = 2 * R + 1
ENTRIES = ('chain_stats', 'dense', 'gather_multi', 'chain_solution', 'sync', 'prof_read',
           'set_kernels+run_chain', 'set_state+run_chain')


@pytest.fixture(scope='module')
def hip_lib():
    from parasitoids_amd import hip_lib
    return hip_lib


@pytest.fixture(scope='module')
def kernels():
    from parasitoids_amd import synthetic
    return synthetic.make_stack(R=R, K=K, ndays=ND, seed=7, sigma=(6.0, 12.0), shift=10)[1]


def unit(p):
    return sparse.coo_matrix(([1.0], ([p], [p])), shape=(N, N))


def make_solver(hip_lib, monkeypatch, kernels, no_defer, state=None):
    monkeypatch.setenv('PS_TPIPE', '1')
    monkeypatch.setenv('PS_RSP', '1')      # the persistent (batched) row kernel also below 1536 points
    if no_defer:
        monkeypatch.setenv('PS_NO_DEFER_CHECK', '1')
    else:
        monkeypatch.delenv('PS_NO_DEFER_CHECK', raising=False)
    s = hip_lib.HipSolve(unit(400) if state is None else state, [K, K], mode='fast', chain_only=True)
    assert s.fft_len == 1008 and s.full_column
    assert s.get_option('PS_NO_DEFER_CHECK') == float(no_defer)
    s.set_kernels(kernels)
    s.prof_enable(True, every=1)           # counts every launch of every run that follows
    return s


def collect(s):
    """every day's statistics, flags and record of the last run"""
    st = s.chain_stats(0, ND)
    return ([(x.flag, x.nnz, x.sum, x.delta, x.padmax) for x in st], [s.dense(0, d) for d in range(ND)])


def same(a, b, what):
    assert a[0] == b[0], what
    for d, (x, y) in enumerate(zip(a[1], b[1])):
        assert np.array_equal(x, y), (what, d)


def first_flag(stats):
    flags = [f for f, *_ in stats]
    return flags.index(1) if 1 in flags else -1


_flags = {}


def flags_of(hip_lib, monkeypatch, kernels, p):
    """first flagged day of the chain from cell (p, p), on a PS_NO_DEFER_CHECK=1 solver (-1: none)"""
    if p not in _flags:
        s = make_solver(hip_lib, monkeypatch, kernels, True, unit(p))
        s.run_chain(renorm=True)
        _flags[p] = first_flag(collect(s)[0])
        s.close()
    return _flags[p]


def sequence(hip_lib, monkeypatch, kernels, no_defer, p, hinted, entry):
    """[clean run from 400 that leaves the window hint,] run from p, `entry` called first after it
    returns, then one more run from 400 whose launches tell whether the hint survived"""
    s = make_solver(hip_lib, monkeypatch, kernels, no_defer)
    if hinted:
        s.run_chain(renorm=True)
        s.sync()
    s.set_state(unit(p))
    s.run_chain(renorm=True)               # returns with its last window pending (unless no_defer)
    seen = {'pending': s.deferred_info()['pending']}
    if entry == 'chain_stats':
        s.chain_stats(0, ND)
    elif entry == 'dense':
        s.dense(0, ND - 1)
    elif entry == 'gather_multi':
        s.gather_multi([0, 0], [ND - 1, ND // 2], [400, p], [400, p])
    elif entry == 'chain_solution':
        s.chain_solution(ND - 1, types.SimpleNamespace(delta=0.0, nnz=1))
    elif entry == 'sync':
        s.sync()
    elif entry == 'prof_read':
        s.prof_read()
    elif entry == 'set_kernels+run_chain':
        s.set_kernels(kernels)
        s.set_state(unit(400))
        s.run_chain(renorm=True)
    elif entry == 'set_state+run_chain':
        s.set_state(unit(p))
        s.run_chain(renorm=True)
    else:
        raise AssertionError(entry)
    seen['after_entry'] = s.deferred_info()
    a = collect(s)                         # the run from p, or the run `entry` itself made
    assert not s.deferred_info()['pending']
    s.set_state(unit(400))
    s.run_chain(renorm=True)
    b = collect(s)
    shape = (s.prof_days(), s.prof_launches())
    seen['end'] = s.deferred_info()
    s.close()
    return a, b, shape, seen


def check_sequence(hip_lib, monkeypatch, kernels, p, hinted, entry):
    ref = sequence(hip_lib, monkeypatch, kernels, True, p, hinted, entry)
    got = sequence(hip_lib, monkeypatch, kernels, False, p, hinted, entry)
    same(got[0], ref[0], (p, hinted, entry, 'run'))
    same(got[1], ref[1], (p, hinted, entry, 'next run'))
    assert got[2] == ref[2], (p, hinted, entry, got[2], ref[2])
    # PS_NO_DEFER_CHECK=1 never defers; uploads are staged either way
    assert not ref[3]['pending'] and ref[3]['end']['deferred'] == 0 and ref[3]['end']['staged_early'] == 0
    assert ref[3]['end']['staged_uploads'] >= 2
    return ref, got


def assert_deferred_with_late_flag(seen, entry):
    """the run from p returned with its check pending, `entry` settled it and found the flag"""
    assert seen['pending']
    assert not seen['after_entry']['pending']      # a run after a flag no longer speculates: nothing to defer
    assert seen['after_entry']['deferred'] >= 1 and seen['after_entry']['late_flags'] == 1
    if entry == 'set_state+run_chain':             # its kernel staging went in ahead of the recovery
        assert seen['after_entry']['staged_early'] == 1
    else:
        assert seen['after_entry']['staged_early'] == 0


@pytest.mark.parametrize('entry', ENTRIES)
def test_flag_in_the_last_window_unhinted(hip_lib, monkeypatch, kernels, entry):
    """fresh solver, windows 2, 4, 8, 6: the first flag sits in the last window (days 14-19)"""
    f = flags_of(hip_lib, monkeypatch, kernels, 625)
    assert f >= 14, f
    ref, got = check_sequence(hip_lib, monkeypatch, kernels, 625, False, entry)
    if '+' not in entry:
        assert first_flag(ref[0][0]) == f
    assert_deferred_with_late_flag(got[3], entry)


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('p', (625, 650, 770))
def test_flag_in_the_hinted_window(hip_lib, monkeypatch, kernels, p, entry):
    """after a clean run the next one is ONE 20-day window: any flag is found by the deferred check"""
    assert flags_of(hip_lib, monkeypatch, kernels, 400) == -1
    assert flags_of(hip_lib, monkeypatch, kernels, p) >= 0
    ref, got = check_sequence(hip_lib, monkeypatch, kernels, p, True, entry)
    assert_deferred_with_late_flag(got[3], entry)


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('p', (650, 400))
def test_entry_points_without_a_late_flag(hip_lib, monkeypatch, kernels, p, entry):
    """the first flag in an earlier un-hinted window (p = 650: found inside the call, nothing left to defer)
    and no flag at all (p = 400: the check is deferred, the entry point settles it and leaves the window hint,
    so the run that follows is ONE 20-day chained pass)"""
    f = flags_of(hip_lib, monkeypatch, kernels, p)
    ref, got = check_sequence(hip_lib, monkeypatch, kernels, p, False, entry)
    seen = got[3]
    if p == 650:
        assert 6 <= f <= 13, f
        assert not seen['pending'] and seen['end']['late_flags'] == 0
    else:
        assert f == -1
        assert seen['pending'] and seen['end']['late_flags'] == 0
        assert seen['after_entry']['pending'] == ('+' in entry)    # the run `entry` made is deferred in turn
        # un-hinted runs chain at most 6 days in the `_xn` class (windows 2, 4, 8, 6); a hinted one all 20
        assert ref[2][0]['col_inv_a_xn'] >= ND and got[2][0]['col_inv_a_xn'] >= ND
        if entry == 'set_state+run_chain':
            assert seen['after_entry']['staged_early'] == 1


@pytest.mark.parametrize('p', (650, 400))
def test_three_stacks_back_to_back(hip_lib, monkeypatch, kernels, p):
    """a flag in an earlier un-hinted window (found inside the call, nothing deferred), and no flag at all
    (every stack's last window deferred, settled by the next run_chain behind its kernel staging)"""
    f = flags_of(hip_lib, monkeypatch, kernels, p)
    if p == 650:
        assert 6 <= f <= 13, f
    else:
        assert f == -1
    runs = {}
    for no_defer in (True, False):
        s = make_solver(hip_lib, monkeypatch, kernels, no_defer)
        for _ in range(3):
            s.set_state(unit(p))
            s.run_chain(renorm=True)
        info = s.deferred_info()
        assert info['pending'] == (p == 400 and not no_defer)
        assert info['deferred'] == (3 if p == 400 and not no_defer else 0)
        assert info['staged_early'] == (2 if p == 400 and not no_defer else 0) and info['late_flags'] == 0
        runs[no_defer] = (collect(s), s.prof_days(), s.prof_launches())
        s.close()
    same(runs[False][0], runs[True][0], p)
    assert runs[False][1:] == runs[True][1:]
    assert first_flag(runs[True][0][0]) == f
    if p == 400:   # stacks two and three were hinted: one chained pass each
        assert runs[True][1]['col_inv_a_xn'] >= 2 * ND


def test_smaller_state_leaves_no_stale_rows(hip_lib, monkeypatch, kernels):
    """set_state clears only the rows the previous state occupied: a state on fewer rows finds the rest zero"""
    from parasitoids_amd import _lib as L
    rows = np.array([100, 250, 400, 550, 700])
    wide = sparse.coo_matrix((np.full(5, 0.2), (rows, rows[::-1])), shape=(N, N))
    narrow = sparse.coo_matrix(([0.5, 0.5], ([400, 401], [390, 410])), shape=(N, N))
    s = make_solver(hip_lib, monkeypatch, kernels, False, wide)
    s.run_chain(renorm=True)
    s.set_state(narrow)
    got_state = s.dense(L.REC_STATE, 0)
    s.run_chain(renorm=True)
    got = collect(s)
    s.set_state(sparse.coo_matrix((N, N)))          # an empty state: every row of the last one cleared
    empty_state = s.dense(L.REC_STATE, 0)
    s.close()
    fresh = make_solver(hip_lib, monkeypatch, kernels, False, narrow)
    ref_state = fresh.dense(L.REC_STATE, 0)
    fresh.run_chain(renorm=True)
    ref = collect(fresh)
    fresh.close()
    assert np.array_equal(got_state, narrow.toarray()) and np.array_equal(ref_state, got_state)
    assert not empty_state.any()
    same(got, ref, 'narrow state')


def test_set_state_owns_a_copy_of_the_callers_arrays(hip_lib, monkeypatch, kernels):
    """the triplets are staged before set_state returns: overwriting them right away changes nothing,
    even with a whole chain still queued ahead of the upload"""
    from parasitoids_amd import _lib as L
    ref = make_solver(hip_lib, monkeypatch, kernels, False, unit(410))
    ref.run_chain(renorm=True)
    want = collect(ref)
    ref.close()
    s = make_solver(hip_lib, monkeypatch, kernels, False)
    s.run_chain(renorm=True)                           # queued work ahead of the upload
    row, col, val = L.i32([410]), L.i32([410]), L.f64([1.0])
    before = s.deferred_info()
    assert before['pending']
    L.check(s._lib.ps_solver_set_state_coo(s._h, L.p_i32(row), L.p_i32(col), L.p_f64(val), 1))
    after = s.deferred_info()
    # the call neither settled the run ahead of it nor bypassed the staging
    assert after['pending'] and after['staged_uploads'] == before['staged_uploads'] + 1
    row[:] = 5
    col[:] = 790
    val[:] = 0.25
    s.run_chain(renorm=True)
    got = collect(s)
    s.close()
    same(got, want, 'staged upload')


def test_two_solvers_each_with_a_pending_check(hip_lib, monkeypatch, kernels):
    """the pending check lives on the handle: two solvers in one process, calls interleaved"""
    alone = {}
    for p in (625, 400):
        s = make_solver(hip_lib, monkeypatch, kernels, True)
        for _ in range(2):
            s.set_state(unit(p))
            s.run_chain(renorm=True)
        alone[p] = collect(s)
        s.close()
    a = make_solver(hip_lib, monkeypatch, kernels, False)
    b = make_solver(hip_lib, monkeypatch, kernels, False)
    for _ in range(2):
        a.set_state(unit(625))
        b.set_state(unit(400))
        a.run_chain(renorm=True)
        b.run_chain(renorm=True)
    assert b.deferred_info()['pending'] and b.deferred_info()['deferred'] == 2
    assert a.deferred_info()['late_flags'] == 1 and not a.deferred_info()['pending']
    got_b = collect(b)
    got_a = collect(a)
    a.close()
    b.close()
    same(got_a, alone[625], 'solver a')
    same(got_b, alone[400], 'solver b')


def test_close_with_a_check_pending(hip_lib, monkeypatch, kernels):
    s = make_solver(hip_lib, monkeypatch, kernels, False)
    s.set_state(unit(625))
    s.run_chain(renorm=True)
    s.set_state(unit(400))
    assert s.deferred_info()['pending']
    s.close()
    assert not s._h.value

"""The staging layout of the staged persistent forward row kernel (row_fwd_stage.h, walked through
ps_row_fwd_stage_walk / ps_row_fwd_stage_slot: host only, no device) against a plain loop over a source
buffer, and the LDS figures the launcher's fit test uses."""
import ctypes as C

import numpy as np
import pytest

MAX_LDS = 160 * 1024


def _walk(lib, K, rows, row, r, nstaged):
    """staging image after the copy of source row `row` into staged row r: source element index per double"""
    rs = lib.ps_row_fwd_stage_bytes(1, K) // 16            # doubles of one staged row
    image = np.full(nstaged * rs, -1, dtype=np.int64)
    assert lib.ps_row_fwd_stage_walk(K, rows, row, r, nstaged, image.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    return image, rs


@pytest.mark.parametrize('K', [1, 3, 5, 63, 125, 127, 129, 253, 255, 257, 401])
def test_every_slot_holds_its_element_and_no_chunk_reads_past_the_buffer(K):
    """A buffer of `rows` rows of K doubles (K odd, element 0 on a 16-byte boundary: rows alternate between the
    two parities).  For every row and column the slot of (row parity, column) holds exactly that element; every
    element the copy reads lies inside the buffer (the last row of a buffer with an odd number of doubles ends
    half a 16-byte word before a boundary: the clamp); the copy writes inside its own staged row only."""
    from parasitoids_amd import _lib
    lib = _lib.load()
    nstaged = 4
    for rows in sorted({1, 2, 3, min(K, 6), K, K + 1}):   # odd and even totals: both parities of the last row
        for row in range(rows):
            r = row % nstaged
            image, rs = _walk(lib, K, rows, row, r, nstaged)
            e = (row * K) & 1
            slots = np.array([lib.ps_row_fwd_stage_slot(K, r, e, c) for c in range(K)], dtype=np.int64)
            assert np.array_equal(slots, r * rs + e + np.arange(K))           # a plain image of the aligned span
            assert np.array_equal(image[slots], row * K + np.arange(K)), (K, rows, row)
            written = np.flatnonzero(image >= 0)
            assert written.min() >= r * rs and written.max() < (r + 1) * rs
            assert image.max() < rows * K, (K, rows, row)                    # nothing read past rows * K
            assert image[written].min() >= row * K - e                       # ... nor before the aligned start
    assert lib.ps_row_fwd_stage_slot(K, 0, 0, K) < 0 and lib.ps_row_fwd_stage_slot(K, 0, 2, 0) < 0
    assert lib.ps_row_fwd_stage_walk(K + 1, 4, 0, 0, 4, None) < 0                # even K, no image


def test_staged_bytes_and_the_launchers_fit_test():
    """bytes(NP, K): 2 NP rows in whole 1 KB chunks of 128 doubles, one double of room for the parity.  The
    kernel's LDS is the exchange buffers of the size (the same for every K) plus that, and the launcher stages
    exactly when it is at most 160 KB.  Headline figures: 16 x 18 x 18, NP = 2, K = 2049."""
    from parasitoids_amd import _lib
    lib = _lib.load()
    for np_, K in [(1, 1), (2, 127), (2, 129), (4, 401), (3, 1601), (2, 2049)]:
        assert lib.ps_row_fwd_stage_bytes(np_, K) == 2 * np_ * ((K + 1 + 127) // 128) * 1024
    assert lib.ps_row_fwd_stage_bytes(2, 2049) == 4 * 17408 == 69632
    assert lib.ps_row_fwd_stage_lds(5184, 2049) == 89856 + 69632 == 159488 <= MAX_LDS
    sizes = {1008: 4, 3360: 3, 3456: 2, 3584: 3, 4608: 2, 5184: 2}
    for fft, np_want in sizes.items():
        n, p = C.c_int32(-1), C.c_int32(-1)
        assert lib.ps_row_fwd_info(fft, C.byref(n), C.byref(p)) == 0 and (n.value, p.value) == (np_want, 1)
        base = lib.ps_row_fwd_stage_lds(fft, 1) - lib.ps_row_fwd_stage_bytes(np_want, 1)
        assert base > 0
        for K in (1, 65, 401, 1279, 1281, 1407, 1409, 1535, 1537, 1601, 1801, 2049, 2305, 4097):
            lds = lib.ps_row_fwd_stage_lds(fft, K)
            assert lds == base + lib.ps_row_fwd_stage_bytes(np_want, K)
            staged = C.c_int32(-1)
            assert lib.ps_row_fwd_stage_info(fft, K, C.byref(staged)) == 0
            assert staged.value == (1 if lds <= MAX_LDS else 0), (fft, K)
    # the cases of the GPU test
    for fft, K, want in [(3456, 1801, 1), (1008, 401, 1), (3360, 1601, 0), (3360, 1401, 1), (5184, 2049, 1)]:
        staged = C.c_int32(-1)
        assert lib.ps_row_fwd_stage_info(fft, K, C.byref(staged)) == 0 and staged.value == want, (fft, K)
    # one pair per workgroup: these sizes keep the one-shot kernel, nothing is staged
    for fft in (2800, 5600, 6912, 8400):
        staged = C.c_int32(-1)
        assert lib.ps_row_fwd_stage_info(fft, 801, C.byref(staged)) == 0 and staged.value == 0
        assert lib.ps_row_fwd_stage_lds(fft, 801) == 0
    assert lib.ps_row_fwd_stage_info(810, 65, None) < 0       # no register-resident kernels at this size
    assert lib.ps_row_fwd_stage_info(5184, 0, None) < 0

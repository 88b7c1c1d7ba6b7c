"""The unit list of the persistent forward row pass over kernel batches (row_live_units.h, exported as
ps_row_live_units: host only, no device) against a brute-force enumeration of the row map over all
torus rows."""
import ctypes as C

import numpy as np
import pytest


def _src_map(P, M, r):
    """map_wrap(M, P): torus row -> source row of the K x K box (K = 2 M + 1), -1 = zero row"""
    src = np.full(r.shape, -1, dtype=np.int64)
    src[r < M + 1] = r[r < M + 1] + M
    src[r >= P - M] = r[r >= P - M] - (P - M)
    return src


def _brute(P, M, NP, ranges):
    """(day, unit) of every unit with a live row, in list order: days ascending, units ascending"""
    r = np.arange(P)
    src = _src_map(P, M, r)
    out = []
    for d, (lo, hi) in enumerate(ranges):
        live = (src >= 0) & (src >= lo) & (src <= hi)
        for u in np.unique(r[live] // (2 * NP)):
            out.append((d, int(u)))
    return out


def _units(lib, P, M, NP, ranges):
    rng = np.ascontiguousarray(np.asarray(ranges, dtype=np.int32).reshape(-1))
    nd = len(ranges)
    i32p = C.POINTER(C.c_int32)
    total = lib.ps_row_live_units(P, M, NP, nd, rng.ctypes.data_as(i32p), None, None, 0)
    assert total >= 0
    day = np.full(total + 1, -7, dtype=np.int32)
    unit = np.full(total + 1, -7, dtype=np.int32)
    again = lib.ps_row_live_units(P, M, NP, nd, rng.ctypes.data_as(i32p), day.ctypes.data_as(i32p),
                                  unit.ctypes.data_as(i32p), total)
    assert again == total
    assert day[total] == -7 and unit[total] == -7          # nothing written past `cap`
    return total, list(zip(day[:total].tolist(), unit[:total].tolist()))


def _ranges(K):
    M = K // 2
    return [
        (1, 0),                    # empty kernel (lo > hi)
        (M, M),                    # one entry at the centre: torus row 0, its pair's other row dead
        (M - 1, M - 1),            # torus row P - 1
        (0, 0), (K - 1, K - 1),    # the box's first and last rows
        (3, M - 2),                # entirely below the centre (upper end of the torus)
        (2, M - 1),
        (M + 1, K - 4),            # entirely above it
        (M, K - 3),
        (M - 5, M + 6),            # spanning the centre, odd and even edges: units straddle the range
        (M - 4, M + 5),
        (M - 1, M),
        (M - 8, M + 8), (M - 7, M + 7),
        (0, K - 1),                # the full box
        (5, 4),                    # empty again
    ]


@pytest.mark.parametrize('P', [1008, 3584, 5184])
@pytest.mark.parametrize('NP', [1, 2, 4])
def test_live_unit_list_matches_brute_force(P, NP):
    from parasitoids_amd import _lib
    lib = _lib.load()
    for K in (9, 65, 401, min(1801, (P - 1) // 2 * 2 - 1), P if P % 2 else P - 1):
        M = K // 2
        assert 2 * M + 1 <= P
        ranges = _ranges(K) if K >= 33 else [(1, 0), (M, M), (M - 1, M - 1), (0, K - 1), (1, K - 2), (M - 2, M + 1)]
        want = _brute(P, M, NP, ranges)
        total, got = _units(lib, P, M, NP, ranges)
        assert total == len(want)
        assert got == want, (P, NP, K)
        # every live pair is covered exactly once, and no unit is without a live row
        assert len(set(got)) == len(got)
        src = _src_map(P, M, np.arange(P))
        for d, (lo, hi) in enumerate(ranges):
            live_rows = np.flatnonzero((src >= lo) & (src <= hi) & (src >= 0))
            units_d = [u for dd, u in got if dd == d]
            assert set((live_rows // 2 // NP).tolist()) == set(units_d)
        # one day at a time gives the same units as the batch
        for d, rg in enumerate(ranges):
            _, one = _units(lib, P, M, NP, [rg])
            assert [u for _, u in one] == [u for dd, u in got if dd == d]


def test_live_unit_list_rejects_bad_arguments():
    from parasitoids_amd import _lib
    lib = _lib.load()
    i32p = C.POINTER(C.c_int32)
    rng = np.array([0, 4], dtype=np.int32)
    assert lib.ps_row_live_units(8, 4, 2, 1, rng.ctypes.data_as(i32p), None, None, 0) < 0   # box larger than the torus
    assert lib.ps_row_live_units(64, 4, 0, 1, rng.ctypes.data_as(i32p), None, None, 0) < 0
    assert lib.ps_row_live_units(64, 4, 2, 1, None, None, None, 0) < 0
    assert lib.ps_row_live_units(64, 4, 2, 1, rng.ctypes.data_as(i32p), None, None, 3) < 0  # cap without arrays
    assert lib.ps_row_live_units(64, 4, 2, 0, None, None, None, 0) == 0


def test_which_sizes_take_the_persistent_kernel():
    """Row pairs per workgroup of the forward row kernels, and the rule of the launcher: kernel batches go to
    the persistent kernel at the sizes with two or more pairs per workgroup; the one-pair sizes (seven waves
    and more per pair) keep the one-shot kernel."""
    from parasitoids_amd import _lib
    lib = _lib.load()
    want = {1008: (4, 1), 3360: (3, 1), 3456: (2, 1), 3584: (3, 1), 4608: (2, 1), 5184: (2, 1),
            2800: (1, 0), 5600: (1, 0), 6912: (1, 0), 8400: (1, 0)}
    for fft, (np_want, persistent_want) in want.items():
        n, p = C.c_int32(-1), C.c_int32(-1)
        assert lib.ps_row_fwd_info(fft, C.byref(n), C.byref(p)) == 0
        assert (n.value, p.value) == (np_want, persistent_want), fft
    assert lib.ps_row_fwd_info(810, None, None) < 0          # no register-resident kernels at this size

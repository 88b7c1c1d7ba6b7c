"""Exact reference for day chains with SPARSE states and kernels, and seeded generators for them.

Why sparse: a kernel of 4..8 points has a flat spectrum (no frequency bin of the transform is
negligible), where the Gaussian day kernels of `synthetic.make_stack` leave more than 90 % of the bins
below 1e-6 -- so a wrong twiddle, digit-reversal slot or exchange address shows in the field values.
And the chain of sparse convolutions is a few thousand products, summed here in `np.longdouble` on COO
triplets: exact to the last bit of a double at any torus size, in milliseconds, with no FFT and
nothing shared with the library under test.

The chain follows `oracle.calcsol.get_solutions` (CalcSol.py:140-201): per day the linear convolution
of the state with the day kernel (kernel centre at K // 2), truncated to the domain [0, N)^2; the flag
says whether anything fell outside; the next day continues from the RAW truncated field (thresholding
only shapes the returned solution); the solution is `oracle.model.r_small_vals(prob_model=True)`.

On the reference torus P = N + K // 2 everything outside the domain lands in the pad, so the flag of
the oracle (pad maximum > 1e-8) and "anything fell outside" agree as long as no nonzero is anywhere
near 1e-8, and then every solver mode (exact / fold / fast / auto) must give this chain to round-off:
there is no sub-threshold pad mass whose treatment could differ between the tori.  `exact_chain`
therefore ASSERTS that every nonzero of every day's field is >= MIN_VALUE = 1e-6.
"""
import os
import re
from collections import namedtuple

import numpy as np
from scipy import sparse

LD = np.longdouble
MIN_VALUE = 1e-6      # 100 x the 1e-8 threshold: thresholding, nnz and the flag are unambiguous

Day = namedtuple('Day', 'rows cols vals flag keep sol_vals nnz sum delta')
Day.__doc__ = """One chain day of the exact reference.
rows, cols, vals: the raw truncated field (sorted by cell, vals in longdouble);
flag: mass fell outside the domain; keep: mask of the cells r_small_vals keeps (not below negval; here all
of them); sol_vals: r_small_vals(prob_model=True) values at the kept cells; nnz, sum: count and sum of the
kept raw values; delta = (1 - sum) / nnz."""


def _triplets(A):
    A = sparse.coo_matrix(A)
    A.sum_duplicates()
    return A.row.astype(np.int64), A.col.astype(np.int64), A.data.astype(LD), A.shape


def exact_chain(state, kernels, N, negval=1e-8):
    """state: sparse N x N; kernels: sparse, odd square shapes (each its own K).  -> [Day]"""
    r, c, v, shape = _triplets(state)
    assert shape == (N, N)
    days = []
    for B in kernels:
        kr, kc, kv, ks = _triplets(B)
        assert ks[0] == ks[1] and ks[0] % 2 == 1
        m = ks[0] // 2
        rr = (r[:, None] + kr[None, :] - m).ravel()
        cc = (c[:, None] + kc[None, :] - m).ravel()
        vv = (v[:, None] * kv[None, :]).ravel()
        inside = (rr >= 0) & (rr < N) & (cc >= 0) & (cc < N)
        flag = bool((~inside).any())
        key, inv = np.unique(rr[inside] * N + cc[inside], return_inverse=True)
        v = np.zeros(len(key), dtype=LD)
        np.add.at(v, inv.ravel(), vv[inside])          # equal cells are summed, in longdouble
        r, c = key // N, key % N
        assert len(v) == 0 or v.min() >= MIN_VALUE, 'reference field has a nonzero below %g: %g' % (MIN_VALUE, v.min())
        keep = ~(v < negval)
        nnz = int(keep.sum())
        tot = v[keep].sum()
        delta = (1 - tot) / nnz if nnz else LD(0)
        days.append(Day(r, c, v, flag, keep, v[keep] + delta, nnz, tot, delta))
    return days


def raw_dense(day, N):
    out = np.zeros((N, N))
    out[day.rows, day.cols] = day.vals.astype(np.float64)
    return out


def sol_csr(day, N):
    return sparse.csr_matrix((day.sol_vals.astype(np.float64), (day.rows[day.keep], day.cols[day.keep])), shape=(N, N))


# ------------------------------------------------------------------ generators (all seeded)
def _weights(rng, n):
    w = rng.uniform(0.8, 1.2, n)
    return w / w.sum()


def sparse_kernel(rng, K, T, kind):
    """T-point kernel of shape K x K, weights uniform in (0.8, 1.2) normalised to 1.
    'wide'       the four corners of the support plus T - 4 random cells: every row is between live rows,
                 the solver cannot treat the kernel as compact;
    'band'       rows within +-2 of the centre, columns anywhere: compact (direct-sum route);
    'one_sided'  all rows strictly above the centre."""
    m = K // 2
    if kind == 'wide':
        assert T >= 4
        cells = {(0, 0), (0, K - 1), (K - 1, 0), (K - 1, K - 1)}
        rows, cols = (0, K), (0, K)
    elif kind == 'band':
        cells = set()
        rows, cols = (max(0, m - 2), min(K, m + 3)), (0, K)
    elif kind == 'one_sided':
        assert m >= 1
        cells = set()
        rows, cols = (0, m), (0, K)
    else:
        raise ValueError(kind)
    assert (rows[1] - rows[0]) * (cols[1] - cols[0]) >= T
    while len(cells) < T:
        cells.add((int(rng.integers(*rows)), int(rng.integers(*cols))))
    cells = sorted(cells)
    return sparse.coo_matrix((_weights(rng, T), ([a for a, _ in cells], [b for _, b in cells])), shape=(K, K))


def clean_state(rng, N, margin):
    """3 distinct points within +-margin of the centre."""
    R = N // 2
    assert 1 <= margin <= R
    cells = set()
    while len(cells) < 3:
        cells.add((R + int(rng.integers(-margin, margin + 1)), R + int(rng.integers(-margin, margin + 1))))
    cells = sorted(cells)
    return sparse.coo_matrix((_weights(rng, 3), ([a for a, _ in cells], [b for _, b in cells])), shape=(N, N))


def edge_state(rng, N):
    """The corners of the state's live range: (0, 0), (N-1, N-1), the centre, and one point ten
    cells from two edges."""
    R = N // 2
    assert N >= 25
    cells = [(0, 0), (10, N - 11), (R, R), (N - 1, N - 1)]
    return sparse.coo_matrix((_weights(rng, 4), ([a for a, _ in cells], [b for _, b in cells])), shape=(N, N))


# ------------------------------------------------------------------ geometries of the GPU tests
def rs_sizes():
    """Sizes served by the register-resident row kernels, parsed from fft_rs_sizes.h; the list has as
    many entries as the header has X( lines."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, 'parasitoids_amd', 'csrc', 'fft_rs_sizes.h')).read()
    sizes = [16 * int(a) * int(b) for a, b in re.findall(r'^\s*X\((\d+), (\d+)\)', txt, flags=re.M)]
    assert len(sizes) == len(re.findall(r'^\s*X\(', txt, flags=re.M)) and len(set(sizes)) == len(sizes)
    return sorted(sizes)


def odd_le(x):
    n = int(np.floor(x))
    return n if n % 2 else n - 1


CLEAN_KINDS = ('wide', 'band', 'wide', 'one_sided', 'wide', 'wide')


def fast_geometry(L, chain):
    """Fast mode with the fast torus equal to the reference torus: m odd, K = 2m + 1, N = L - m, so
    that N + K // 2 == L with N odd.  -> (N, K, state, kernels)
    'clean': m <= L / 16, six 4-point days (wide, band, wide, one_sided, wide, wide) from three points
             within +-(R - 6m - 2) of the centre: nothing can leave the domain;
    'edge':  m <= L / 6, three wide 8-point days from `edge_state`: the first day already flags."""
    rng = np.random.default_rng([L, 0 if chain == 'clean' else 1])
    if chain == 'clean':
        m = odd_le(L / 16)
        kinds, T = CLEAN_KINDS, 4
    else:
        m = odd_le(L / 6)
        kinds, T = ('wide',) * 3, 8
    K, N = 2 * m + 1, L - m
    state = clean_state(rng, N, N // 2 - 6 * m - 2) if chain == 'clean' else edge_state(rng, N)
    return N, K, state, [sparse_kernel(rng, K, T, k) for k in kinds]


def fold_m(L):
    return odd_le(L / 9)


def fold_geometry(L, N, chain):
    """Fold mode: m <= L / 9, K = 2m + 1, N = L - 3m less the even step the test's size search took (the
    linear convolution N + 3m fits the FFT size L).  -> (K, state, kernels)
    'edge':  three wide 8-point days of shape K from `edge_state`;
    'clean': four 4-point days (wide, band, wide, one_sided) of the smaller shape 2mc + 1, mc the largest odd
             number <= (R - 2) / 5, from three points within +-(R - 4mc - 2) of the centre.  (With the full shape
             K the domain of 6m cells could not hold four wide days: the corners alone travel 4m > R.)"""
    m = fold_m(L)
    K = 2 * m + 1
    rng = np.random.default_rng([L, N, 2 if chain == 'clean' else 3])
    if chain == 'clean':
        R = N // 2
        mc = odd_le((R - 2) / 5)
        assert 1 <= mc <= m
        state = clean_state(rng, N, R - 4 * mc - 2)
        return K, state, [sparse_kernel(rng, 2 * mc + 1, 4, k) for k in CLEAN_KINDS[:4]]
    return K, edge_state(rng, N), [sparse_kernel(rng, K, 8, 'wide') for _ in range(3)]


# (N, K, days, direct): exact-mode pads below and beside the register-resident sizes; `direct`: the column
# transform is split into sub-passes of at most 255 points, so compact kernels take the direct-sum sub-pass
AWKWARD_CASES = [
    (1201, 199, 4, True),       # P = 1300 = 2^2 5^2 13: split columns, radix 13
    (2301, 547, 4, True),       # P = 2574 = 2 3^2 11 13: both sub-passes generic
    (1401, 301, 4, True),       # P = 1551 = 3 11 47: split, generic
    (901, 241, 4, False),       # P = 1021, prime: one wave-cooperative radix, no split
    (4097, 2049, 2, False),     # P = 5121 = 9 x 569, the reference torus of the benchmarked workload: L2 = 569 > 255
]


def awkward_geometry(N, K, nd):
    """`edge_state` and two chains of 8-point kernels: wide, band.  -> state, {kind: kernels}"""
    rng = np.random.default_rng([N, K])
    state = edge_state(rng, N)
    return state, {kind: [sparse_kernel(rng, K, 8, kind) for _ in range(nd)] for kind in ('wide', 'band')}


AUTO_N, AUTO_K = 301, 101     # P = 351 = 3^3 13 is not 7-smooth: chain-only callers get PS_MODE_AUTO


def auto_geometry(start):
    """Four wide 8-point days on the 301 domain with K = 101 (m = 50).  -> state, kernels
    'edge': `edge_state`, every day flags: no day is left to the fast-torus front;
    'late': three points within +-48 of the centre: two days (+-100) stay inside, the third and fourth spill --
            a clean prefix, then the hand-over."""
    rng = np.random.default_rng([AUTO_N, AUTO_K, start == 'late'])
    R = AUTO_N // 2
    state = clean_state(rng, AUTO_N, R - 2 * (AUTO_K // 2) - 2) if start == 'late' else edge_state(rng, AUTO_N)
    return state, [sparse_kernel(rng, AUTO_K, 8, 'wide') for _ in range(4)]


def check_cells(day, N, rng):
    """The reference support plus as many random other cells (expected 0) -> rows, cols, expected."""
    n = len(day.rows)
    key = set((day.rows * N + day.cols).tolist())
    extra = []
    while len(extra) < n:
        k = int(rng.integers(0, N * N))
        if k not in key:
            key.add(k)
            extra.append(k)
    extra = np.array(extra, dtype=np.int64)
    rows = np.concatenate([day.rows, extra // N])
    cols = np.concatenate([day.cols, extra % N])
    return rows, cols, np.concatenate([day.vals.astype(np.float64), np.zeros(len(extra))])

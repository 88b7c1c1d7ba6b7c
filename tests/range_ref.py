"""The core-range statements of include/parasitoid_hip.h (ps_range_*) restated in numpy and Python integers, line
by line, for the tests.  One member and slot: a field v [N, N]; a cell whose value is not > 0 has mass 0 and lies in
no set; neither does a cell that is not finite.
    vmax = max v;  not (vmax > 0): empty, lambda_j = +inf, n_j = 0, Q = 0, E = 0
    E = floor(log2 vmax) from frexp;  q(c) = floor(ldexp(v(c), 36 - E)) as an integer (< 2^37, exact)
    Q = sum q;  need_j = the smallest integer >= p_j Q, p_j as the exact Fraction of the double
    lambda_j = the largest x with sum of q over {v >= x} >= need_j;  B_j = {v >= lambda_j};  n_j = |B_j|
"""
import math
from fractions import Fraction

import numpy as np


def exponent(vmax):
    """floor(log2 vmax) of a double > 0, from the exponent field"""
    return math.frexp(float(vmax))[1] - 1


def integer_mass(field):
    """(q [..] uint64, Q int, E int) of one field; all zero where nothing is > 0"""
    v = np.asarray(field, dtype=np.float64)
    live = (v > 0) & np.isfinite(v)
    if not live.any():
        return np.zeros(v.shape, dtype=np.uint64), 0, 0
    E = exponent(v[live].max())
    q = np.zeros(v.shape, dtype=np.uint64)
    q[live] = np.floor(np.ldexp(v[live], 36 - E)).astype(np.uint64)
    return q, int(q.sum(dtype=np.uint64)), E


def needed_mass(p, Q):
    """the smallest integer >= p Q, p at its exact binary value"""
    x = Fraction(float(p)) * Q
    return -((-x.numerator) // x.denominator)


def member_levels(field, fractions):
    """-> (lam [J] float64, n [J] int64, Q int, E int, sets [J, ...] bool) of one member and slot"""
    v = np.asarray(field, dtype=np.float64)
    J = len(fractions)
    q, Q, E = integer_mass(v)
    lam = np.full(J, np.inf)
    n = np.zeros(J, dtype=np.int64)
    sets = np.zeros((J,) + v.shape, dtype=bool)
    if Q == 0:
        return lam, n, 0, 0, sets
    live = (v > 0) & np.isfinite(v)
    vv, qq = v[live], q[live]
    order = np.argsort(-vv, kind='stable')
    vs = vv[order]
    cum = np.cumsum(qq[order], dtype=np.uint64)       # < 2^62: exact
    for j, p in enumerate(fractions):
        need = needed_mass(p, Q)
        at = int(np.searchsorted(cum, np.uint64(need), side='left'))     # the first position with cum >= need
        lam[j] = vs[at]
        sets[j] = live & (v >= lam[j])
        n[j] = int(sets[j].sum())
    return lam, n, Q, E, sets


def accumulate(fields, weights, fractions):
    """fields: per member [nslot, N, N]; integer weights -> dict(counts [J, nslot, N, N] int64, lam [M, J, nslot],
    n [M, J, nslot] int64, Q [M, nslot] (Python ints in an object array), E [M, nslot] int64)"""
    M, J = len(fields), len(fractions)
    nslot = len(fields[0])
    counts = np.zeros((J, nslot) + np.asarray(fields[0][0]).shape, dtype=np.int64)
    lam = np.zeros((M, J, nslot))
    n = np.zeros((M, J, nslot), dtype=np.int64)
    Q = np.zeros((M, nslot), dtype=object)
    E = np.zeros((M, nslot), dtype=np.int64)
    for m, (F, w) in enumerate(zip(fields, weights)):
        for s in range(nslot):
            lam[m, :, s], n[m, :, s], Q[m, s], E[m, s], sets = member_levels(F[s], fractions)
            counts[:, s] += int(w) * sets
    return {'counts': counts, 'lam': lam, 'n': n, 'Q': Q, 'E': E}


def brute_levels(field, fractions):
    """the same levels by a sort-and-cumulate on Python integers alone (small fields): -> (lam [J], n [J], Q, E)"""
    vals = [float(x) for x in np.asarray(field, dtype=np.float64).ravel() if 0 < x < math.inf]
    if not vals:
        return [math.inf] * len(fractions), [0] * len(fractions), 0, 0
    E = exponent(max(vals))
    mass = {}
    for x in vals:
        fx = Fraction(x) * Fraction(2) ** (36 - E)
        mass[x] = mass.get(x, 0) + fx.numerator // fx.denominator
    Q = sum(mass.values())
    lam, n = [], []
    for p in fractions:
        need = needed_mass(p, Q)
        run = 0
        for x in sorted(mass, reverse=True):       # distinct values from the top: a tie enters whole
            run += mass[x]
            if run >= need:
                lam.append(x)
                n.append(sum(1 for y in vals if y >= x))
                break
    return lam, n, Q, E


def radix_levels(field, fractions, bits=10):
    """the levels by the device's route (csrc/ps_range.hip), for any pass width: key = pattern(v) -
    pattern(2^(E - 36)) over the cells with mass, most significant digit first; per pass the integer mass per digit
    among the keys that match the prefix, and the prefix takes the largest digit d at which the mass above the
    prefix's range plus the mass of the digits >= d reaches the need; the need by the 128-bit product of the
    53-bit significand with Q -> (lam [J], Q, E)"""
    v = np.asarray(field, dtype=np.float64).ravel()
    v = v[(v > 0) & np.isfinite(v)]
    if v.size == 0:
        return [math.inf] * len(fractions), 0, 0
    pat = v.view(np.uint64)
    E = exponent(v[pat.argmax()])                   # positive doubles order as their patterns
    base = int(np.array([math.ldexp(1.0, E - 36)]).view(np.uint64)[0])     # 0 where 2^(E - 36) underflows
    keep = pat >= np.uint64(base)
    keys = [int(x) - base for x in pat[keep]]
    q = [int(math.floor(math.ldexp(float(x), 36 - E))) for x in v[keep]]
    Q = sum(q)
    passes = -(-60 // bits)
    lam = []
    for p in fractions:
        f, e = math.frexp(float(p))
        m, k = int(math.ldexp(f, 53)), 53 - e
        prod = m * Q                                 # < 2^128
        need = (prod >> k) + (1 if prod & ((1 << k) - 1) else 0)
        prefix, above = 0, 0
        for ps in range(passes):
            hi, lo = bits * (passes - ps), bits * (passes - ps - 1)
            hist = [0] * (1 << bits)
            for key, mass in zip(keys, q):
                if key >> hi == prefix:
                    hist[(key >> lo) & ((1 << bits) - 1)] += mass
            tail = 0
            for d in range((1 << bits) - 1, -1, -1):
                if above + tail + hist[d] >= need:
                    prefix, above = (prefix << bits) | d, above + tail
                    break
                tail += hist[d]
        lam.append(float(np.array([prefix + base], dtype=np.uint64).view(np.float64)[0]))
    return lam, Q, E

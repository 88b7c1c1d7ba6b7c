"""numpy reference of the excursion semantics of ps_excur_* / predictive.ExcursionMaps for one plane (one
threshold, one slot), from the members' fields of any shape, flattened in C order: the masks as little-endian
packed uint64 words including the pad up to 64 cells, the weighted counts, the members' bounds with the two
sentinels, the integer numerators A+ / A- / Ac as int64 by a plain loop over the members, the three functions,
the region map and the areas.  Shared by the CPU and GPU excursion tests."""
import numpy as np

NONE = 0xffffffff          # lo of a member whose mask is empty


def bits(fields, t):
    """fields: [M, *shape] -> [M, ncell] bool: B_m(c) = [v_m(c) >= t], flattened"""
    X = np.asarray(fields, dtype=np.float64)
    return X.reshape(X.shape[0], -1) >= float(t)


def pack(B):
    """[M, ncell] bool -> [M, nword] uint64 ('<u8'): bit l of word j is cell 64 j + l, the pad bits 0"""
    B = np.asarray(B, dtype=bool)
    M, n = B.shape
    pitch = (n + 63) // 64 * 64
    padded = np.zeros((M, pitch), dtype=np.uint8)
    padded[:, :n] = B
    return np.packbits(padded, axis=1, bitorder='little').view('<u8')


def counts(B, weights):
    """[ncell] int64: C(c) = sum_m w_m B_m(c)"""
    w = np.asarray(weights, dtype=np.int64)
    return (np.asarray(B, dtype=np.int64) * w[:, None]).sum(0)


def bounds(B, C):
    """(hi [M], lo [M]) int64: hi_m = max{C(c) : B_m(c) = 0} (0 if none), lo_m = min{C(c) : B_m(c) = 1} (NONE)"""
    hi = np.zeros(len(B), dtype=np.int64)
    lo = np.full(len(B), NONE, dtype=np.int64)
    for m, b in enumerate(np.asarray(B, dtype=bool)):
        if (~b).any():
            hi[m] = max(0, int(C[~b].max()))
        if b.any():
            lo[m] = int(C[b].min())
    return hi, lo


def numerators(C, hi, lo, weights):
    """(A+, A-, Ac) int64 [ncell], one member at a time"""
    w = np.asarray(weights, dtype=np.int64)
    W = int(w.sum())
    C = np.asarray(C, dtype=np.int64)
    u = np.minimum(C, W - C)
    Ap = np.zeros(C.shape, dtype=np.int64)
    Am = np.zeros(C.shape, dtype=np.int64)
    Ac = np.zeros(C.shape, dtype=np.int64)
    for m in range(len(w)):
        Ap += w[m] * (hi[m] < C)
        Am += w[m] * (lo[m] > C)
        Ac += w[m] * ((hi[m] < W - u) & (lo[m] > u))
    Ap[C == 0] = 0
    Ac[2 * u >= W] = 0
    return Ap, Am, Ac


def functions(C, hi, lo, weights):
    """(F+, F-, Fc) float64 [ncell]: (double)A / (double)W"""
    W = float(int(np.asarray(weights, dtype=np.int64).sum()))
    return tuple(A.astype(np.float64) / W for A in numerators(C, hi, lo, weights))


def plane(fields, weights, t):
    """everything of one plane from the members' fields -> dict(B, words, C, hi, lo, above, below, contour), the
    maps in the fields' own shape"""
    X = np.asarray(fields, dtype=np.float64)
    B = bits(X, t)
    C = counts(B, weights)
    hi, lo = bounds(B, C)
    Fp, Fm, Fc = functions(C, hi, lo, weights)
    shape = X.shape[1:]
    return {'B': B, 'words': pack(B), 'C': C.reshape(shape), 'hi': hi, 'lo': lo, 'above': Fp.reshape(shape),
            'below': Fm.reshape(shape), 'contour': Fc.reshape(shape)}


def region(above, below, level):
    """int8: +1 on {F+ >= level}, -1 on {F- >= level}, 0 elsewhere (0.5 < level <= 1: never both)"""
    return (above >= level).astype(np.int8) - (below >= level).astype(np.int8)


def areas(above, below, contour, levels, cell_area):
    return [{'level': float(p), 'above': float(int((above >= p).sum())) * cell_area,
             'below': float(int((below >= p).sum())) * cell_area,
             'band': float(int((contour < p).sum())) * cell_area} for p in levels]

"""The numpy restatement of the neighbourhood fields (ps_nbhd_*, predictive.NeighbourhoodFields):
Z(y, x) = max of v over the cells of the domain with (y' - y)^2 + (x' - x)^2 <= r2.  The output starts from the
centre cell and takes np.maximum with every clipped shifted view, one per offset of the disc: cells outside the
domain never take part, nothing wraps.  A maximum is exact, so the device must return these bits."""
import math

import numpy as np


def window_cells(radius_m, cell_m):
    """(r2, H, ncells): rho = radius_m / cell_m, r2 = floor(rho^2 + 1e-9), H = floor(sqrt(r2))"""
    rho = float(radius_m) / float(cell_m)
    r2 = int(math.floor(rho * rho + 1e-9))
    return r2, math.isqrt(r2), len(disc_offsets(r2))


def disc_offsets(r2):
    """[(dy, dx)] of the disc, row by row"""
    H = math.isqrt(int(r2))
    return [(dy, dx) for dy in range(-H, H + 1) for dx in range(-H, H + 1) if dy * dy + dx * dx <= r2]


def disc_footprint(r2):
    """the disc as a (2H + 1) x (2H + 1) boolean array"""
    H = math.isqrt(int(r2))
    fp = np.zeros((2 * H + 1, 2 * H + 1), dtype=bool)
    for dy, dx in disc_offsets(r2):
        fp[dy + H, dx + H] = True
    return fp


def neighbourhood_max(v, r2):
    """Z of the square field v"""
    v = np.asarray(v, dtype=np.float64)
    n0, n1 = v.shape
    out = v.copy()
    for dy, dx in disc_offsets(r2):
        if abs(dy) >= n0 or abs(dx) >= n1:
            continue                  # the shifted view is empty: no cell of the domain lies there
        # out[y, x] takes v[y + dy, x + dx] wherever both lie in the domain
        ys = slice(max(-dy, 0), n0 - max(dy, 0))
        xs = slice(max(-dx, 0), n1 - max(dx, 0))
        yv = slice(max(dy, 0), n0 - max(-dy, 0))
        xv = slice(max(dx, 0), n1 - max(-dx, 0))
        np.maximum(out[ys, xs], v[yv, xv], out=out[ys, xs])
    return out

"""Generator of g10_bvn_mp.npz: stamps of get_mvn_cdf_values from the high-precision reference
(tests/bvn_ref.py, mpmath) at every correlation class of the device's BVU and on both sides of every
class boundary.  Needs mpmath, numpy; nothing from the library, the oracle or the reference project.

    python tests/golden/make_bvn_mp.py [-j PROCESSES]

Per case k (arrays indexed by case):
    inputs[k]  = cell, mu_x, mu_y, sigma_x, sigma_y, rho      (float64, taken as exact by the reference)
    kind[k]    = index into KINDS
    H[k]       = support half width of the square rule
    margin[k]  = min |1 - P(square) - 1e-3| over h in {H - 1, H}: how far the support decision is from
                 its threshold (asserted >= 1e-6 here, so that H is not a matter of round-off)
    masses[offsets[k]:offsets[k + 1]] = the (2H+1)^2 cell masses, row-major in the orientation of
                 get_mvn_cdf_values, rounded to float64
"""
import argparse
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bvn_ref  # noqa: E402

# 0; just under / on every class boundary of the device's rule (0.3: 3 -> 6 node pairs, 0.75: 6 -> 10,
# 0.925: second branch); deep in the second branch
RHOS = (0.0, 0.2999, -0.2999, 0.3, -0.3, 0.7499, -0.7499, 0.75, -0.75, 0.9249, -0.9249, 0.925, -0.925,
        0.99, -0.99, 0.999, -0.999)

# kind: cell, mu / cell, sigma / cell.  Half widths: 3.3 (|rho| -> 1) to 3.5 (rho = 0) times the larger
# sigma, less half a cell
KINDS = ('centred', 'off_centre', 'anisotropic', 'coarse', 'fine')
SHAPES = {
    'centred': (62.5, (0.0, 0.0), (0.85, 0.85)),          # H = 3
    'off_centre': (25.0, (0.31, -0.27), (0.8, 0.9)),      # H = 3, mu a fraction of a cell, both signs
    'anisotropic': (10.0, (-0.12, 0.2), (0.27, 0.9)),     # H = 3, sigma_y = 3.33 sigma_x
    'coarse': (160.0, (0.05, 0.2), (0.6, 0.62)),          # H = 2, cell ~ 1.6 sigma
    'fine': (2.0, (-0.45, 0.1), (1.75, 1.6)),             # H = 6
}
MAX_H = 8
MIN_MARGIN = 1e-6


def cases():
    out = []
    for rho in RHOS:
        for ki, kind in enumerate(KINDS):
            cell, mu, sg = SHAPES[kind]
            out.append((ki, np.array([cell, mu[0] * cell, mu[1] * cell, sg[0] * cell, sg[1] * cell, rho])))
    return out


def one(case):
    ki, c = case
    H, rows, margin = bvn_ref.stamp_mp(c[0], (c[1], c[2]), c[3], c[4], c[5])
    return H, np.array([[float(v) for v in row] for row in rows]), float(margin)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('-j', type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument('-o', default=os.path.join(HERE, 'g10_bvn_mp.npz'))
    args = ap.parse_args()
    cs = cases()
    with multiprocessing.Pool(args.j) as pool:
        res = pool.map(one, cs, chunksize=1)
    off = [0]
    for (ki, c), (H, m, margin) in zip(cs, res):
        assert H <= MAX_H, (KINDS[ki], c, H)
        assert margin >= MIN_MARGIN, (KINDS[ki], c, H, margin)
        if KINDS[ki] == 'coarse':
            assert H <= 2, (c, H)
        if KINDS[ki] == 'fine':
            assert 6 <= H <= 8, (c, H)
        off.append(off[-1] + m.size)
    np.savez(args.o,
             inputs=np.array([c for _, c in cs]), kind=np.array([ki for ki, _ in cs], dtype=np.int32),
             kinds=np.array(KINDS), H=np.array([r[0] for r in res], dtype=np.int32),
             margin=np.array([r[2] for r in res]), offsets=np.array(off, dtype=np.int64),
             masses=np.concatenate([r[1].ravel() for r in res]), dps=np.int32(bvn_ref.DPS))
    print('%d cases, H %d..%d, smallest margin %.3g, %d masses -> %s' % (
        len(cs), min(r[0] for r in res), max(r[0] for r in res), min(r[2] for r in res), off[-1], args.o))


if __name__ == '__main__':
    main()

"""numpy reference of the release-plan arithmetic of ps_sites_* / predictive.ReleaseSites: per output day the sum
over the release days in ascending lag and over each day's sites in the order given of amount * the translated
field, Y[e] = Y[e] + a * shifted(f_lag[D_e - lag]), from +0.0, product and sum rounded separately in float64.
The translation is built with slices, so it cannot wrap: what leaves an edge is gone.  Shared by the CPU and
GPU release-plan tests ("the reference")."""
import numpy as np


def shifted(f, drow, dcol):
    """out[r, c] = f[r - drow, c - dcol] where both indices lie inside f, else 0"""
    f = np.asarray(f, dtype=np.float64)
    n0, n1 = f.shape
    out = np.zeros_like(f)
    if abs(drow) >= n0 or abs(dcol) >= n1:
        return out
    out[max(drow, 0):n0 + min(drow, 0), max(dcol, 0):n1 + min(dcol, 0)] = \
        f[max(-drow, 0):n0 + min(-drow, 0), max(-dcol, 0):n1 + min(-dcol, 0)]
    return out


def plan_fields(fields, sites, days):
    """fields: {lag: [model day of that release's own model, N, N]}; sites: [(drow, dcol, amount, lag), ...];
    days: output days counted from the first release -> [len(days), N, N] float64"""
    shape = np.asarray(fields[0]).shape[1:]
    Y = np.zeros((len(days),) + shape, dtype=np.float64)
    for lag in sorted({s[3] for s in sites}):
        for drow, dcol, amount, site_lag in sites:
            if site_lag != lag:
                continue
            for e, D in enumerate(days):
                if D < lag:
                    continue                       # not released yet
                Y[e] = Y[e] + float(amount) * shifted(fields[lag][D - lag], drow, dcol)
    return Y

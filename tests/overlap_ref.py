"""Reference of the representative-member semantics of ps_overlap_* / predictive.RepresentativeMembers, written
apart from the product code: the pair table as an integer matrix product of the members' bits (excur_ref.bits),
everything else by plain Python loops over Python integers.  Shared by the CPU and GPU tests.

Setting: one plane (threshold, day) of an ExcursionMaps; members m = 0..M-1 in add order, B_m the cells whose mask
bit is 1 (pad bits are 0 and do not count), integer weight w_m >= 1, W = sum w_m.
  I[i][j] = |B_i & B_j|, the diagonal n_i = |B_i|;  Cs(c) = sum_m s_m bit_m(c)
  out_ij = n_i - I_ij;  i lies in j (eps)  <=>  1000 out_ij <= e n_i, e = round(1000 eps); an empty set in every set
  in_i = sum_j w_j [i in j], cont_i = sum_j w_j [j in i], both with j = i;  depth_i = min(in_i, cont_i)
  median: the largest depth, among equals the smallest index
  central set: the shortest prefix of the members sorted by (-depth, index) with 1000 cum >= round(1000 central) W
  band: +1 where Cs == Wc, 0 where 0 < Cs < Wc, -1 where Cs == 0, Cs of the central set with s = w
  d_ij = n_i + n_j - 2 I_ij
  scenarios: weighted k-medoids, cost(Med) = sum_i w_i min_{m in Med} d_im, by PAM.  BUILD: argmin_m sum_i w_i d_im,
    then the candidate that lowers the cost most, among equals the smallest index.  SWAP: over every (medoid
    position, other member) the swap with the largest strict improvement, among equals the smallest position, then
    the smallest member, until none improves.  A member goes to its nearest medoid, among equals the medoid with the
    smallest index; clusters by descending weight, then medoid index.
  plane 'all': I summed over the days."""
import itertools

import numpy as np

import excur_ref


def table(B):
    """[M, ncell] bool -> [M, M] int64"""
    B = np.asarray(B, dtype=bool).astype(np.int64)
    return B @ B.T


def table_of_fields(fields, t):
    """members' fields [M, *shape] at threshold t -> [M, M] int64"""
    return table(excur_ref.bits(fields, t))


def subset_counts(B, sel):
    """[ncell] int64: sum_m sel[m] B_m(c)"""
    B = np.asarray(B, dtype=bool)
    out = np.zeros(B.shape[1], dtype=np.int64)
    for m, s in enumerate(sel):
        out += int(s) * B[m]
    return out


def depth(I, weights, e):
    """(depth, in, cont) as lists of ints; e = round(1000 eps)"""
    M = len(weights)
    n = [int(I[i][i]) for i in range(M)]
    inside = [[1000 * (n[i] - int(I[i][j])) <= e * n[i] for j in range(M)] for i in range(M)]
    w_in = [sum(int(weights[j]) for j in range(M) if inside[i][j]) for i in range(M)]
    w_cont = [sum(int(weights[j]) for j in range(M) if inside[j][i]) for i in range(M)]
    return [min(a, b) for a, b in zip(w_in, w_cont)], w_in, w_cont


def median(d):
    best = 0
    for i in range(1, len(d)):
        if d[i] > d[best]:
            best = i
    return best


def central(d, weights, c):
    """c = round(1000 central)"""
    W = sum(int(w) for w in weights)
    order = sorted(range(len(d)), key=lambda i: (-d[i], i))
    out, cum = [], 0
    for m in order:
        out.append(m)
        cum += int(weights[m])
        if 1000 * cum >= c * W:
            return out
    return out


def band(B, weights, members, shape):
    sel = [int(weights[m]) if m in members else 0 for m in range(len(weights))]
    Cs, Wc = subset_counts(B, sel), sum(sel)
    return np.where(Cs == Wc, 1, np.where(Cs == 0, -1, 0)).astype(np.int8).reshape(shape)


def distance(I):
    M = len(I)
    return [[int(I[i][i]) + int(I[j][j]) - 2 * int(I[i][j]) for j in range(M)] for i in range(M)]


def cost(D, weights, med):
    return sum(int(weights[i]) * min(D[i][m] for m in med) for i in range(len(weights)))


def pam(D, weights, K):
    """(medoids in BUILD order, cost)"""
    M = len(weights)
    med = [min(range(M), key=lambda m: (cost(D, weights, [m]), m))]
    while len(med) < K:
        med.append(min((m for m in range(M) if m not in med), key=lambda m: (cost(D, weights, med + [m]), m)))
    cur = cost(D, weights, med)
    while True:
        best = None
        for p in range(K):
            for c in range(M):
                if c in med:
                    continue
                trial = cost(D, weights, med[:p] + [c] + med[p + 1:])
                if trial < cur and (best is None or trial < best[0]):
                    best = (trial, p, c)
        if best is None:
            return med, cur
        cur, med[best[1]] = best[0], best[2]


def k_medoids(D, weights, K):
    """dict(medoids, assignment, cluster_weight, cost, costs_by_k) with the clusters in reported order"""
    M = len(weights)
    runs = [pam(D, weights, k) for k in range(1, K + 1)]
    med = sorted(runs[-1][0])
    near = [min(range(K), key=lambda c: (D[i][med[c]], med[c])) for i in range(M)]
    weight = [sum(int(weights[i]) for i in range(M) if near[i] == c) for c in range(K)]
    order = sorted(range(K), key=lambda c: (-weight[c], med[c]))
    return {'medoids': [med[c] for c in order], 'assignment': [order.index(near[i]) for i in range(M)],
            'cluster_weight': [weight[c] for c in order], 'cost': runs[-1][1], 'costs_by_k': [r[1] for r in runs]}


def exhaustive(D, weights, K):
    """the smallest cost over every set of K medoids"""
    return min(cost(D, weights, list(med)) for med in itertools.combinations(range(len(weights)), K))


def jaccard(I):
    M = len(I)
    out = np.ones((M, M))
    for i in range(M):
        for j in range(M):
            u = int(I[i][i]) + int(I[j][j]) - int(I[i][j])
            if u > 0:
                out[i, j] = int(I[i][j]) / u
    return out


def check_plane(rep, k, day, I, B_by_day, weights, eps=0.02, cen=0.5, K=3):
    """every host output of a RepresentativeMembers `rep` on plane (k, day) against this reference: I the reference
    table of the plane, B_by_day {day of the maps: [M, ncell] bool} for the band and the scenario maps"""
    M = len(weights)
    W = sum(int(w) for w in weights)
    e, c = int(round(1000 * eps)), int(round(1000 * cen))
    got = rep.pairs(k, day)
    assert np.array_equal(np.asarray(got).astype(np.int64), I), (k, day)
    d, w_in, w_cont = depth(I, weights, e)
    gd, gi, gc = rep.depth_counts(k, day)
    assert gd.dtype == gi.dtype == gc.dtype == np.int64
    assert gd.tolist() == d and gi.tolist() == w_in and gc.tolist() == w_cont, (k, day)
    assert np.array_equal(rep.depth(k, day), np.asarray(d, dtype=np.float64) / float(W))
    assert rep.median(k, day) == median(d)
    cm = central(d, weights, c)
    assert rep.central(k, day) == cm
    K = min(K, M)
    want = k_medoids(distance(I), weights, K)
    sc = rep.scenarios(k, day, K)
    assert sc['medoids'] == want['medoids'] and list(sc['assignment']) == want['assignment']
    assert sc['cluster_weight'] == want['cluster_weight'] and sc['cost'] == want['cost']
    assert sc['costs_by_k'] == want['costs_by_k']
    assert sc['share'] == [cw / float(W) for cw in want['cluster_weight']]
    assert np.array_equal(rep.jaccard(k, day), jaccard(I))
    shape = (rep.N, rep.N)
    for dm, B in B_by_day.items():
        b = rep.band(k, dm, day)
        assert b.dtype == np.int8 and np.array_equal(b, band(B, weights, cm, shape)), (k, day, dm)
        for cl in range(K):
            members = [i for i in range(M) if want['assignment'][i] == cl]
            sel = [int(weights[i]) if i in members else 0 for i in range(M)]
            m = rep.scenario_map(k, dm, cl, day, K)
            assert np.array_equal(m, (subset_counts(B, sel) / float(sum(sel))).reshape(shape)), (k, day, dm, cl)
    return {'depth': d, 'median': median(d), 'central': cm, 'scenarios': want}

"""The ensemble modes restated in numpy, one statement of include/parasitoid_hip.h (ps_modes_*) and of
predictive.mode_decomposition / separated / score_drivers per function.

  X = v (raw) or sqrt(v), the IEEE square root
  mu = (sum_m w_m X_m) / W: acc += w_m * X_m over m in add order, one division
  A_m = X_m - mu (centred) or X_m
  G_ij = sum_c A_i(c) A_j(c), here the dot of the fp64 anomalies taken in np.longdouble (64-bit significand: a
    product of two fp64 rounds at 2^-64, so its error is 2^-11 of one fp64 rounding per term)
  out_k = sum_m coef_km A_m: out += coef * A_m over m in add order
  the decomposition through the SVD of Y = diag(sqrt(w / W)) A: Y = U S V^T, lambda_k = s_k^2, u_k the columns of U,
    e_k the rows of V^T; the sign rule makes the entry of u_k of largest magnitude positive (smallest index first)
"""
import numpy as np


def transform(v, name):
    v = np.asarray(v, dtype=np.float64)
    return np.sqrt(v) if name == 'sqrt' else v.copy()


def mean(X, weights):
    """X [M, ...] -> the weighted mean plane, by the loop"""
    acc = np.zeros(np.asarray(X[0]).shape, dtype=np.float64)
    W = 0
    for x, w in zip(X, weights):
        acc += float(w) * np.asarray(x, dtype=np.float64)
        W += int(w)
    return acc / float(W)


def anomalies(X, weights, centred=True):
    X = np.asarray(X, dtype=np.float64)
    if not centred:
        return X.copy()
    mu = mean(X, weights)
    return np.array([x - mu for x in X])


def table(A):
    """[M, M] longdouble: the dot of every pair of anomalies"""
    A = np.asarray(A, dtype=np.float64)
    L = A.reshape(len(A), -1).astype(np.longdouble)
    M = len(L)
    G = np.zeros((M, M), dtype=np.longdouble)
    for i in range(M):
        for j in range(i, M):
            G[i, j] = G[j, i] = np.dot(L[i], L[j])
    return G


def table_bound(G, ncell):
    """2 P 2^-53 sqrt(G_ii G_jj): gamma_P of any summation order through Cauchy-Schwarz, twice for the reference's
    own rounding"""
    d = np.sqrt(np.diagonal(np.asarray(G, dtype=np.float64)))
    return 2.0 * ncell * 2.0 ** -53 * d[:, None] * d[None, :]


def combine(A, coef):
    """[K, ...]: out_k += coef[k, m] * A_m over m in order"""
    A = np.asarray(A, dtype=np.float64)
    coef = np.asarray(coef, dtype=np.float64)
    out = np.zeros((coef.shape[0],) + A.shape[1:], dtype=np.float64)
    for k in range(coef.shape[0]):
        for m in range(A.shape[0]):
            out[k] += coef[k, m] * A[m]
    return out


def sign_rule(u):
    """u or -u: the entry of largest magnitude positive, among equal magnitudes the one of smallest index"""
    best = 0
    for i in range(len(u)):
        if abs(u[i]) > abs(u[best]):
            best = i
    return -np.asarray(u) if u[best] < 0 else np.asarray(u)


def decomposition(A, weights, count):
    """through the SVD of the sqrt(w / W)-weighted centred anomalies A [M, P] -> dict(eigenvalues, explained,
    total_variance, vectors [M, K], scores [M, K], patterns [K, P] of unit norm), K = count, nothing dropped"""
    A = np.asarray(A, dtype=np.float64).reshape(len(A), -1)
    w = np.asarray(weights, dtype=np.float64)
    W = w.sum()
    Y = np.sqrt(w / W)[:, None] * A
    U, s, Vt = np.linalg.svd(Y, full_matrices=False)
    lam = s * s
    K = count
    vec = np.zeros((len(w), K))
    pat = np.zeros((K, A.shape[1]))
    for k in range(K):
        u = sign_rule(U[:, k])
        flip = 1.0 if np.array_equal(u, U[:, k]) else -1.0
        vec[:, k] = u
        pat[k] = flip * Vt[k]
    scores = np.zeros((len(w), K))
    for m in range(len(w)):
        for k in range(K):
            scores[m, k] = vec[m, k] * np.sqrt(W / w[m])
    return {'eigenvalues': lam[:K], 'explained': lam[:K] / lam.sum(), 'total_variance': lam.sum(), 'vectors': vec,
            'scores': scores, 'patterns': pat, 'spectrum': lam}


def n_eff(weights):
    s1 = s2 = 0.0
    for w in weights:
        s1 += float(w)
        s2 += float(w) ** 2
    return s1 * s1 / s2


def separated(eigenvalues, weights):
    lam = [float(v) for v in eigenvalues]
    ne = n_eff(weights)
    out = []
    for k in range(len(lam)):
        err = lam[k] * (2.0 / ne) ** 0.5
        ok = True
        if k > 0 and not lam[k - 1] - lam[k] > err:
            ok = False
        if k + 1 < len(lam) and not lam[k] - lam[k + 1] > err:
            ok = False
        out.append(ok)
    return out


def score_drivers(scores, thetas, weights):
    """[K, P]: the weighted correlation of score k with parameter p by the loop; 0 where either never moves"""
    z = np.asarray(scores, dtype=np.float64)
    th = np.asarray(thetas, dtype=np.float64)
    w = [float(v) for v in weights]
    W = sum(w)
    out = np.zeros((z.shape[1], th.shape[1]))
    for k in range(z.shape[1]):
        for p in range(th.shape[1]):
            mz = sum(w[m] * z[m, k] for m in range(len(w))) / W
            mt = sum(w[m] * th[m, p] for m in range(len(w))) / W
            szz = sum(w[m] * (z[m, k] - mz) ** 2 for m in range(len(w))) / W
            stt = sum(w[m] * (th[m, p] - mt) ** 2 for m in range(len(w))) / W
            szt = sum(w[m] * (z[m, k] - mz) * (th[m, p] - mt) for m in range(len(w))) / W
            if len(set(th[:, p].tolist())) > 1 and szz > 0 and stt > 0:
                out[k, p] = szt / (szz * stt) ** 0.5
    return out

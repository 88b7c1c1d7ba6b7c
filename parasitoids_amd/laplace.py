"""MAP fit and normal (Laplace) approximation of the reference's Bayesian model, with delta-method
spread maps built on the device -- the counterpart of Bayes_MAP.py (`MAP_run` :484-519, `norm_run`
:521-566: pymc.MAP and pymc.NormApprox over the model of Bayes_Run.py).

  free parameters     the 14 continuous model parameters of mcmc.MODEL_BLOCK, xi, em_obs_prob,
                      grid_obs_prob, A_collected and every sent_obs_probs_k; n_periods is held at its
                      start value, as Bayes_MAP.py:144-147 does ("pymc.MAP can only take float values").
                      Bayes_MAP's `sprd_factor` (:200-205) is not part of this project's model
                      (Bayes_Run.py:175 sets it to None), so it is left out.
  steps               PRIOR_EPS: the `prior_eps` table of Bayes_MAP.py:101-191
  objective           mcmc.log_prior + mcmc.loglik_parts_stats; model evaluations are cached by the exact
                      bytes of the model parameters, so a point that moves only nuisance parameters costs
                      no evaluation (as the sampler's scalar steps reuse its expected observations)
  find_map            outer search over the model block in unconstrained coordinates (scipy Powell), the
                      nuisance block profiled on the host for each model evaluation (L-BFGS-B)
  normal_approx       central-difference Hessian in the natural parameters (as NormApprox), C = (-H)^-1;
                      the axis stencil evaluations feed a LinearisedSpread (ps_linspread_*,
                      csrc/ps_linspread.hip): per day and cell the sensitivities dU/dtheta_i, then the
                      delta-method variance J' Sigma J of the model block and normal exceedances

`evaluate=` injects the expected observations of a model evaluation (mcmc.Sampler's hook): every host
path then runs without a device, and no spread maps are built.
"""
import ctypes as C
import json
import math
import os
import time

import numpy as np

from . import _lib as L
from . import mcmc
from . import predictive as PP
from ._handle import _Handle

NEGVAL = PP.NEGVAL
NEG_INF = float('-inf')

# finite-difference steps (`prior_eps`, Bayes_MAP.py:101-191) in mcmc.MODEL_BLOCK order; None: held fixed
PRIOR_EPS = [
    ('g_aw', 0.05),        # Bayes_MAP.py:121
    ('g_bw', 0.1),         # :123
    ('f_a1', 0.1),         # :107
    ('f_b1_p', 0.05),      # :111
    ('f_a2', 0.1),         # :109
    ('f_b2_p', 0.05),      # :116
    ('sig_x', 1.0),        # :126
    ('sig_y', 1.0),        # :128
    ('corr_p', 0.01),      # :130
    ('sig_x_l', 1.0),      # :136
    ('sig_y_l', 1.0),      # :138
    ('corr_l_p', 0.005),   # :140
    ('lam', 0.01),         # :105
    ('n_periods', None),   # :147 held at its start value
    ('mu_r', 0.05),        # :146
]
NUISANCE_EPS = [0.05, 0.0005, 0.0005]   # xi :150, em_obs_prob :158, grid_obs_prob :161
A_COLLECTED_EPS = 10.0                  # :175
SENT_EPS = 0.0005                       # :191

# supports of the priors (mcmc.MODEL_BLOCK): Gamma (0, inf), Beta (0, 1), TruncatedNormal [a, b], Normal
_MODEL_SUPPORT = {'g_aw': (0, math.inf), 'g_bw': (0, math.inf), 'f_a1': (0, 9), 'f_b1_p': (0, math.inf),
                  'f_a2': (15, 24), 'f_b2_p': (0, math.inf), 'sig_x': (0, math.inf), 'sig_y': (0, math.inf),
                  'corr_p': (0, 1), 'sig_x_l': (0, math.inf), 'sig_y_l': (0, math.inf), 'corr_l_p': (0, 1),
                  'lam': (0, 1), 'n_periods': (0, math.inf), 'mu_r': (-math.inf, math.inf)}

FREE_MODEL = [i for i, (_n, e) in enumerate(PRIOR_EPS) if e is not None]   # MODEL_BLOCK indices
FREE_MODEL_NAMES = [PRIOR_EPS[i][0] for i in FREE_MODEL]
_NP = mcmc.MODEL_BLOCK.index(next(m for m in mcmc.MODEL_BLOCK if m[0] == 'n_periods'))
HELD_STEP = 1e-3       # a step shrunk below HELD_STEP * prior_eps holds the parameter


# ------------------------------------------------------------------ the device accumulator
class LinearisedSpread(_Handle):
    '''Delta-method spread of `pop_model`'s days around one evaluation (ps_linspread_*).  days: model
    days (0 = release day) to keep, default all; nparam: sensitivities kept (<= 16); thresholds: up to 4
    population densities whose exceedance probability under the normal approximation is kept; names:
    optional parameter names for `sensitivity`.'''
    _prefix, _noun, _prof_pairs = 'ps_linspread', 'spread', 2

    def __init__(self, pop_model, days=None, nparam=len(FREE_MODEL), thresholds=(), names=None):
        self.days = list(range(len(pop_model.days)) if days is None else days)
        if not self.days or min(self.days) < 0:
            raise ValueError('days must be a non-empty list of model days >= 0')
        self.nparam = int(nparam)
        self.names = list(FREE_MODEL_NAMES if names is None and self.nparam == len(FREE_MODEL) else
                          (names or range(self.nparam)))
        self.thresholds = [float(t) for t in thresholds]
        self._attach(pop_model)
        thr = L.f64(self.thresholds if self.thresholds else [0.0])
        self._create(len(self.days), self.nparam, len(self.thresholds), L.p_f64(thr))
        self._set_source(None, self.days)

    def set_center(self):
        '''centre = the last evaluation's days (enqueued on the solver's stream)'''
        self._from_model('set_center')

    def add(self, param, coef):
        '''J[param] += coef * the last evaluation's days (enqueued on the solver's stream)'''
        self._from_model('add', head=(int(param), float(coef)))

    def finalize(self, F):
        '''Sigma = F F' (F: nparam x rank): per cell variance and exceedances'''
        F = L.f64(np.atleast_2d(F))
        if F.ndim != 2 or F.shape[0] != self.nparam:
            raise ValueError('F must be %d x rank, got %s' % (self.nparam, F.shape))
        self._call('finalize', self.nparam, F.shape[1], L.p_f64(F))

    def reset(self):
        self._call('reset')

    def info(self):
        '''(centre set, finalized, adds per parameter)'''
        c, f = C.c_int32(), C.c_int32()
        adds = np.zeros(self.nparam, dtype=np.int64)
        self._call('info', C.byref(c), C.byref(f), L.p_i64(adds))
        return bool(c.value), bool(f.value), adds

    def _fetch(self, day, what):
        return self.fetch_slot(self._slot_of(day), what)

    def fetch_slot(self, slot, what):
        '''raw access by slot index (0 centre, 1 variance, 2 + k exceedance, 16 + i sensitivity)'''
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('fetch', int(slot), int(what), L.p_f64(out))
        return out

    def mean(self, day):
        return self._fetch(day, 0)

    def variance(self, day):
        return self._fetch(day, 1)

    def sd(self, day):
        return np.sqrt(self.variance(day))

    def exceedance(self, day, k):
        '''P(population >= thresholds[k]) per cell under the normal approximation'''
        if not 0 <= k < len(self.thresholds):
            raise ValueError('threshold %r of %d' % (k, len(self.thresholds)))
        return self._fetch(day, 2 + k)

    def sensitivity(self, day, name):
        '''J_i = dU/dtheta_i per cell; name: a parameter name or index'''
        i = self.names.index(name) if not isinstance(name, (int, np.integer)) else int(name)
        if not 0 <= i < self.nparam:
            raise ValueError('parameter %r of %d' % (name, self.nparam))
        return self._fetch(day, 16 + i)

    def profile(self, enable=None):
        '''HIP-event time of the add and finalize launches; enable switches it'''
        return dict(zip(('add_ms', 'add_launches', 'finalize_ms', 'finalize_launches'), self._profile(enable)))


# ------------------------------------------------------------------ the objective
def free_names(locinfo):
    '''names of the free parameters, in the order of every vector here'''
    return (FREE_MODEL_NAMES + [m[0] for m in mcmc.NUISANCE] + ['A_collected']
            + ['sent_obs_probs_{}'.format(k) for k in locinfo.sent_ids])


def start_point(locinfo, cell_area, start=None):
    '''(model block [15], nuisance vector [4 + fields]) of a start: None (the sampler's initial
    values), a model-block vector, or a full point in mcmc.Sampler.names() order'''
    areas = mcmc.field_areas(locinfo, cell_area)
    theta = np.array([m[2] for m in mcmc.MODEL_BLOCK], dtype=np.float64)
    z = np.concatenate([[m[2] for m in mcmc.NUISANCE], [min(mcmc.A_COLLECTED_INIT, 0.5 * float(areas.min()))],
                        mcmc.initial_sent_obs_probs(locinfo, cell_area)]).astype(np.float64)
    if start is not None:
        s = np.asarray(start, dtype=np.float64).ravel()
        nb = len(mcmc.MODEL_BLOCK)
        if s.size == nb:
            theta = s.copy()
        elif s.size == nb + z.size:
            theta, z = s[:nb].copy(), s[nb:].copy()
        else:
            raise ValueError('start has %d values: %d (model block) or %d (full point) expected'
                             % (s.size, nb, nb + z.size))
    return theta, z


def start_from_chain(paths, locinfo=None):
    '''the highest-logp row of one or more `Sampler.save` chains (the first such row in chain order),
    as a full point in mcmc.Sampler.names() order (the sentinel fields in locinfo.sent_ids order, or
    the first file's without locinfo)'''
    if isinstance(paths, (str, os.PathLike)):
        paths = [paths]
    best, best_lp = None, NEG_INF
    want = [m[0] for m in mcmc.MODEL_BLOCK] + [m[0] for m in mcmc.NUISANCE] + ['A_collected']
    sent = None if locinfo is None else ['sent_obs_probs_{}'.format(k) for k in locinfo.sent_ids]
    for p in paths:
        trace, names, src = PP.load_chain(p)
        with np.load(src if src.endswith('.npz') else src + '.npz', allow_pickle=False) as f:
            logp = np.asarray(f['logp'], dtype=np.float64)
        if sent is None:
            sent = [n for n in names if n.startswith('sent_obs_probs_')]
        cols = PP._columns(names, want + sent)
        if not len(logp):
            continue
        r = int(np.argmax(logp))
        if logp[r] > best_lp:
            best, best_lp = trace[r, cols].copy(), float(logp[r])
    if best is None:
        raise ValueError('no chain rows to start from')
    return best


class Posterior():
    '''The joint log density over the free parameters (free_names order) in natural coordinates:
    mcmc.log_prior + the observation log likelihood, with n_periods held.  Model evaluations are
    cached by the exact bytes of the model block; `on_evaluate(key)` runs right after each successful
    one (while its days are still in the solver's records).'''

    def __init__(self, pop_model, locinfo, cell_area, n_periods, evaluate=None, ndays=None, on_evaluate=None):
        self.pm = pop_model
        self.li = locinfo
        self.areas = mcmc.field_areas(locinfo, cell_area)
        self.n_periods = float(n_periods)
        self.ndays = ndays
        self._evaluate_fn = evaluate
        self.on_evaluate = on_evaluate
        self.names = free_names(locinfo)
        self.nm = len(FREE_MODEL)
        self.evaluations = 0
        self.failed = 0
        self._cache = {}
        lo = [_MODEL_SUPPORT[n][0] for n in FREE_MODEL_NAMES] + [0.0, 0.0, 0.0, 0.0] + [0.0] * len(locinfo.sent_ids)
        hi = ([_MODEL_SUPPORT[n][1] for n in FREE_MODEL_NAMES] + [math.inf, 1.0, 1.0, float(self.areas.min())]
              + [1.0] * len(locinfo.sent_ids))
        self.lo, self.hi = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
        self.eps = np.array([PRIOR_EPS[i][1] for i in FREE_MODEL] + NUISANCE_EPS + [A_COLLECTED_EPS]
                            + [SENT_EPS] * len(locinfo.sent_ids), dtype=np.float64)

    def theta(self, xm):
        '''model block [15] from the free model parameters'''
        t = np.empty(len(mcmc.MODEL_BLOCK), dtype=np.float64)
        t[FREE_MODEL] = xm
        t[_NP] = self.n_periods
        return t

    def _evaluate(self, theta):
        if self._evaluate_fn is not None:
            return self._evaluate_fn(theta)
        try:
            self.pm.evaluate(*mcmc.model_args(theta), ndays=self.ndays, want_stats=False)
        except (AssertionError, ValueError):
            return None
        except L.HipError as e:
            if e.code not in mcmc._PARAMETER_ERRORS:      # device errors stop the run
                raise
            return None
        return mcmc.expected_observations(self.pm, self.li)

    def stats(self, theta):
        '''lik_stats of the model evaluation at `theta` (cached), None where it fails'''
        key = theta.tobytes()
        if key in self._cache:
            return self._cache[key]
        self.evaluations += 1
        exp = self._evaluate(theta)
        st = None if exp is None else mcmc.lik_stats(exp, self.li)
        self._cache[key] = st
        if st is None:
            self.failed += 1
        elif self.on_evaluate is not None:
            self.on_evaluate(key)
        return st

    def split(self, x):
        x = np.asarray(x, dtype=np.float64)
        return self.theta(x[:self.nm]), x[self.nm:self.nm + 3], float(x[self.nm + 3]), x[self.nm + 4:]

    def nuisance_logp(self, st, z):
        '''log density of the nuisance block z = (xi, em, grid, A, sent...) given one evaluation's
        statistics: their priors + the observation log likelihood (no model prior)'''
        nuis, A, sp = z[:3], float(z[3]), z[4:]
        lp = sum(m[1](v) for m, v in zip(mcmc.NUISANCE, nuis))
        if lp == NEG_INF:
            return NEG_INF, NEG_INF
        lc = mcmc.collection_logprior(A, sp, self.areas)
        if lc == NEG_INF:
            return NEG_INF, NEG_INF
        ll = sum(mcmc.loglik_parts_stats(st, nuis, sp))
        return lp + lc + ll, ll

    def parts(self, x):
        '''(joint log density, log likelihood) at x; the model is evaluated only where the prior is finite'''
        theta, nuis, A, sp = self.split(x)
        lp = mcmc.log_prior(theta, nuis, A, sp, self.areas)
        if lp == NEG_INF:
            return NEG_INF, NEG_INF
        st = self.stats(theta)
        if st is None:
            return NEG_INF, NEG_INF
        ll = sum(mcmc.loglik_parts_stats(st, nuis, sp))
        return lp + ll, ll

    def logp(self, x):
        return self.parts(x)[0]


# ------------------------------------------------------------------ finite differences
def stencil_steps(x, lo, hi, eps):
    '''per parameter the step: eps, shrunk to half the distance to the nearer bound of the support
    where x +- eps would leave it; 0 (held) where that is below HELD_STEP * eps'''
    x, lo, hi, eps = (np.asarray(a, dtype=np.float64) for a in (x, lo, hi, eps))
    h = eps.copy()
    dist = np.minimum(x - lo, hi - x)
    shrink = h >= dist
    h[shrink] = 0.5 * dist[shrink]
    h[~(h >= HELD_STEP * eps)] = 0.0         # NaN / negative distances hold the parameter too
    return h


def hessian(f, x, h):
    '''Central-difference Hessian and gradient of f at x (as pymc.NormApprox):
        H_ii = (f(x + h_i) - 2 f(x) + f(x - h_i)) / h_i^2
        H_ij = (f(x+h_i+h_j) - f(x+h_i-h_j) - f(x-h_i+h_j) + f(x-h_i-h_j)) / (4 h_i h_j)
        g_i  = (f(x + h_i) - f(x - h_i)) / (2 h_i)
    Rows and columns with h_i = 0 stay 0.  Points in a fixed order: x, then x + h_i, x - h_i for every i,
    then the four corners of every pair i < j.  -> (H, g, f(x))'''
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    d = x.size
    act = [i for i in range(d) if h[i] != 0.0]
    f0 = f(x)
    fp, fm = np.zeros(d), np.zeros(d)
    for i in act:
        xp = x.copy()
        xp[i] += h[i]
        fp[i] = f(xp)
        xm = x.copy()
        xm[i] -= h[i]
        fm[i] = f(xm)
    H = np.zeros((d, d))
    g = np.zeros(d)
    for i in act:
        H[i, i] = (fp[i] - 2.0 * f0 + fm[i]) / (h[i] * h[i])
        g[i] = (fp[i] - fm[i]) / (2.0 * h[i])
    for a, i in enumerate(act):
        for j in act[a + 1:]:
            c = []
            for si, sj in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                xc = x.copy()
                xc[i] += si * h[i]
                xc[j] += sj * h[j]
                c.append(f(xc))
            H[i, j] = H[j, i] = (c[0] - c[1] - c[2] + c[3]) / (4.0 * h[i] * h[j])
    return H, g, f0


def axis_point(x, h, i, sign):
    '''the stencil point x + sign h_i e_i, computed as hessian() computes it'''
    xs = np.asarray(x, dtype=np.float64).copy()
    if sign > 0:
        xs[i] += h[i]
    else:
        xs[i] -= h[i]
    return xs


# ------------------------------------------------------------------ coordinates of the search
def _to_u(x, lo, hi):
    u = np.empty_like(x)
    for i, (v, a, b) in enumerate(zip(x, lo, hi)):
        if math.isinf(a) and math.isinf(b):
            u[i] = v
        elif math.isinf(b):
            u[i] = math.log(v - a)
        else:
            p = (v - a) / (b - a)
            u[i] = math.log(p) - math.log1p(-p)
    return u


def _from_u(u, lo, hi):
    x = np.empty_like(u)
    for i, (v, a, b) in enumerate(zip(u, lo, hi)):
        if math.isinf(a) and math.isinf(b):
            x[i] = v
        elif math.isinf(b):
            x[i] = a + math.exp(min(v, 700.0))
        else:
            x[i] = a + (b - a) / (1.0 + math.exp(-max(min(v, 700.0), -700.0)))
    return x


# ------------------------------------------------------------------ results
def _write_text(fname, lines):
    d = os.path.dirname(str(fname))
    if d and not os.path.exists(d):
        os.makedirs(d)
    with open(fname, 'w') as fobj:
        for line in lines:
            fobj.write(line + '\n')


class MapResult():
    '''What find_map returns (the fields MAP_run reports, Bayes_MAP.py:491-502): `k` free stochastic
    values, `logp` the joint log density at the estimate (= `logp_at_max`), `lnL` the log likelihood
    there, `AIC` = 2 (k - lnL), `estimates` {name: value}; besides `x` (free_names order), `theta` (the
    model block with n_periods), `point` (mcmc.Sampler.names() order), `logp_start`, `evaluations`,
    `failed`, `seconds`.'''

    def __init__(self, names, x, theta, point, logp, lnL, logp_start, evaluations, failed, seconds, n_periods,
                 message=''):
        self.names, self.x, self.theta, self.point = list(names), x, theta, point
        self.k = len(self.names)
        self.logp = self.logp_at_max = float(logp)
        self.lnL = float(lnL)
        self.AIC = 2.0 * (self.k - self.lnL)
        self.logp_start = float(logp_start)
        self.evaluations, self.failed, self.seconds = int(evaluations), int(failed), float(seconds)
        self.n_periods = float(n_periods)
        self.message = message
        self.estimates = dict(zip(self.names, (float(v) for v in x)))

    def lines(self):
        '''the lines of MAP_run's result file (Bayes_MAP.py:507-516), in its order'''
        out = ['Time elapsed: {}'.format(self.seconds),
               'Free stochastic variables: {}'.format(self.k),
               'Joint log-probability of model: {}'.format(self.logp),
               'Max joint log-probability of model: {}'.format(self.logp_at_max),
               'Maximum log-likelihood: {}'.format(self.lnL),
               "Akaike's Information Criterion {}".format(self.AIC),
               '---------------Variable estimates---------------']
        return out + ['{} = {}'.format(n, v) for n, v in self.estimates.items()]

    def save(self, outname, params=None):
        '''outname.txt (MAP_run's file), outname.npz (names, x, theta, point), outname.json (params and
        provenance) -> the three paths'''
        outname = str(outname)
        _write_text(outname + '.txt', self.lines())
        np.savez(outname + '.npz', names=np.array(self.names), x=self.x, theta=self.theta, point=self.point,
                 n_periods=self.n_periods)
        meta = PP.params_dict(params)
        meta['map'] = {'k': self.k, 'logp': self.logp, 'lnL': self.lnL, 'AIC': self.AIC,
                       'logp_start': self.logp_start, 'evaluations': self.evaluations, 'failed': self.failed,
                       'seconds': self.seconds, 'n_periods_held': self.n_periods, 'message': self.message}
        with open(outname + '.json', 'w') as fobj:
            json.dump(meta, fobj, default=str)
        return outname + '.txt', outname + '.npz', outname + '.json'


class NormalResult():
    '''What normal_approx returns: `mu` (free_names order), `C` = (-H)^-1 (held rows / columns 0), `H`,
    `steps` (the h_i used; 0 = held at a bound), `held` (names), `grad` (the stencil's gradient at mu), `pd`
    (whether -H over the free parameters is positive definite) and its `eigenvalues`, `logp` / `lnL` /
    `AIC` at mu, `F` (the factor of the model-block covariance the maps use: Sigma = F F'), `spread` (a
    LinearisedSpread, None without a device), `evaluations`, `failed`, `seconds` {stage: s}.'''

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.k = len(self.names)
        self.logp_at_max = self.logp
        self.AIC = 2.0 * (self.k - self.lnL)

    @property
    def variances(self):
        return np.diag(self.C).copy()

    def lines(self):
        '''the lines of norm_run's result file (Bayes_MAP.py:548-561), in its order'''
        out = ['Time elapsed: {}'.format(sum(self.seconds.values())),
               'Free stochastic variables: {}'.format(self.k),
               'Joint log-probability of model: {}'.format(self.logp),
               'Max joint log-probability of model: {}'.format(self.logp_at_max),
               "Akaike's Information Criterion {}".format(self.AIC),
               '---------------Variable estimates---------------',
               'Estimated means: ']
        out += ['{} = {}'.format(n, v) for n, v in zip(self.names, self.mu)]
        out += ['Estimated variances: ']
        out += ['{} = {}'.format(n, v) for n, v in zip(self.names, np.diag(self.C))]
        return out

    def save(self, outname, params=None):
        '''outname.txt (norm_run's file), outname.npz (names, mu, C, H, steps, grad, pd, eigenvalues, F),
        outname.json (params, provenance, the pd note) and, with spread maps, outname_maps.npz in the
        Run.save_result layout: per day `{day}_data/_ind/_indptr` of the centre, `{day}_sd_*` and
        `{day}_pexc{k}_*` (predictive.save_maps) -> the paths written'''
        outname = str(outname)
        _write_text(outname + '.txt', self.lines())
        np.savez(outname + '.npz', names=np.array(self.names), mu=self.mu, C=self.C, H=self.H, steps=self.steps,
                 grad=self.grad, pd=np.array(self.pd), eigenvalues=self.eigenvalues, F=self.F,
                 n_periods=self.n_periods)
        paths = [outname + '.txt', outname + '.npz']
        s = self.spread
        if s is not None:
            maps = []
            for d in s.days:
                label = s.pm.days[d] if d < len(s.pm.days) else d
                day_maps = [('', s.mean(d)), ('_sd', s.sd(d))]
                day_maps += [('_pexc%d' % k, s.exceedance(d, k)) for k in range(len(s.thresholds))]
                maps.append((label, day_maps))
            PP.save_maps(outname + '_maps', maps)
            paths.append(outname + '_maps.npz')
        meta = PP.params_dict(params)
        meta['normal_approx'] = {
            'k': self.k, 'logp': self.logp, 'lnL': self.lnL, 'AIC': self.AIC, 'pd': bool(self.pd),
            'covariance': 'inverse of -H' if self.pd else
                          '-H is not positive definite: pseudo-inverse with its negative eigenvalues clipped',
            'held': self.held, 'evaluations': self.evaluations, 'failed': self.failed, 'seconds': self.seconds,
            'n_periods_held': self.n_periods,
            'thresholds': None if s is None else s.thresholds, 'days': None if s is None else s.days}
        with open(outname + '.json', 'w') as fobj:
            json.dump(meta, fobj, default=str)
        paths.append(outname + '.json')
        return paths


# ------------------------------------------------------------------ MAP
def _profile_nuisance(post, st, z0, maxiter):
    '''max over the nuisance block of the joint density given one evaluation (L-BFGS-B in unconstrained
    coordinates from z0) -> (value, z); never worse than z0'''
    from scipy.optimize import minimize
    lo, hi = post.lo[post.nm:], post.hi[post.nm:]
    v0 = post.nuisance_logp(st, z0)[0]

    def fun(u):
        v = post.nuisance_logp(st, _from_u(u, lo, hi))[0]
        return -v if math.isfinite(v) else 1e300
    best_v, best_z = v0, z0
    try:
        u0 = _to_u(z0, lo, hi)
        if np.all(np.isfinite(u0)):
            r = minimize(fun, u0, method='L-BFGS-B', options={'maxiter': maxiter, 'ftol': 1e-15, 'gtol': 1e-9})
            z = _from_u(r.x, lo, hi)
            v = post.nuisance_logp(st, z)[0]
            if v > best_v:
                best_v, best_z = v, z
    except (ValueError, OverflowError):
        pass
    return best_v, best_z


def find_map(pop_model, locinfo, cell_area, start=None, maxeval=400, evaluate=None, ndays=None, inner_maxiter=200):
    '''Maximum a posteriori estimate (MAP_run, Bayes_MAP.py:484-519).  The 14 free model parameters
    are searched in unconstrained coordinates (log for Gamma priors, logit for Beta, scaled logit for
    TruncatedNormal) by scipy's Powell method with at most `maxeval` model evaluations; for each
    evaluation the nuisance block is profiled on the host, from the best point so far.  start: None, a model-block vector or a full
    point (start_from_chain).  Deterministic for a given start.  -> MapResult'''
    from scipy.optimize import minimize
    t0 = time.perf_counter()
    theta0, z0 = start_point(locinfo, cell_area, start)
    n_periods = float(round(theta0[_NP]))
    theta0[_NP] = n_periods
    post = Posterior(pop_model, locinfo, cell_area, n_periods, evaluate=evaluate, ndays=ndays)
    x0 = np.concatenate([theta0[FREE_MODEL], z0])
    lp0, ll0 = post.parts(x0)
    best = {'v': lp0, 'll': ll0, 'x': x0}
    lo, hi = post.lo[:post.nm], post.hi[:post.nm]
    prof = {}

    def value(xm):
        key = xm.tobytes()
        if key in prof:
            return prof[key]
        theta = post.theta(xm)
        lpm = sum(m[1](v) for m, v in zip(mcmc.MODEL_BLOCK, theta))
        v = NEG_INF
        if lpm > NEG_INF:
            st = post.stats(theta)
            if st is not None:
                vz, z = _profile_nuisance(post, st, best['x'][post.nm:], inner_maxiter)
                if vz > NEG_INF:
                    x = np.concatenate([xm, z])
                    lp, ll = post.parts(x)
                    v = lp
                    if lp > best['v']:
                        best.update(v=lp, ll=ll, x=x)
        prof[key] = v
        return v

    message = ''
    u0 = _to_u(x0[:post.nm], lo, hi)
    if not np.all(np.isfinite(u0)):
        raise ValueError('the start lies on the boundary of a prior support')
    if maxeval > 0:
        value(x0[:post.nm].copy())

        def fun(u):
            if post.evaluations >= maxeval:
                v = prof.get(_from_u(u, lo, hi).tobytes(), NEG_INF)
            else:
                v = value(_from_u(u, lo, hi))
            return -v if math.isfinite(v) else 1e300
        r = minimize(fun, u0, method='Powell', options={'maxfev': 4 * maxeval, 'xtol': 1e-8, 'ftol': 1e-12})
        message = str(r.message)
    x = best['x']
    theta = post.theta(x[:post.nm])
    point = np.concatenate([theta, x[post.nm:]])
    return MapResult(post.names, x, theta, point, best['v'], best['ll'], lp0, post.evaluations, post.failed,
                     time.perf_counter() - t0, n_periods, message)


# ------------------------------------------------------------------ normal approximation
def _covariance(H, h):
    '''C = (-H)^-1 over the parameters with h != 0 (held rows / columns 0) -> (C, pd, eigenvalues of -H)'''
    d = H.shape[0]
    free = np.flatnonzero(h != 0.0)
    A = -H[np.ix_(free, free)]
    w, V = np.linalg.eigh(A)
    C = np.zeros((d, d))
    pd = bool(np.all(np.isfinite(A)))
    if pd:
        try:
            Lc = np.linalg.cholesky(A)
            inv = np.linalg.solve(Lc.T, np.linalg.solve(Lc, np.eye(len(free))))
            C[np.ix_(free, free)] = 0.5 * (inv + inv.T)
        except np.linalg.LinAlgError:
            pd = False
    if not pd:
        wi = np.where(w > 0, 1.0 / np.where(w > 0, w, 1.0), 0.0)
        inv = (V * wi) @ V.T
        C[np.ix_(free, free)] = 0.5 * (inv + inv.T)
    return C, pd, w


def model_factor(C, nm, pd):
    '''F with F F' = the model-block submatrix of C (the marginal covariance of the model parameters):
    its Cholesky factor when C is positive definite, else the eigen-factor with negative eigenvalues
    clipped.  Held (zero) rows stay zero.'''
    S = C[:nm, :nm]
    F = np.zeros((nm, nm))
    live = np.flatnonzero(np.diag(S) != 0.0)
    Sl = S[np.ix_(live, live)]
    if pd and live.size:
        try:
            F[np.ix_(live, np.arange(live.size))] = np.linalg.cholesky(Sl)
            return F
        except np.linalg.LinAlgError:
            pass
    if live.size:
        w, V = np.linalg.eigh(Sl)
        F[np.ix_(live, np.arange(live.size))] = V * np.sqrt(np.clip(w, 0.0, None))
    return F


def normal_approx(pop_model, locinfo, cell_area, at=None, days=None, thresholds=(), evaluate=None, ndays=None,
                  spread=True, profile=False):
    '''Normal approximation of the posterior at `at` (norm_run, Bayes_MAP.py:521-566; pymc.NormApprox):
    the central-difference Hessian H of the joint log density in the natural parameters with the
    prior_eps steps (shrunk near a bound, held on it), C = (-H)^-1.  at: a MapResult, None (the start
    point), a model-block vector or a full point.  The model x model block costs 1 + 2 m + 2 m (m - 1)
    evaluations for m free model parameters (393 at m = 14); points that move only nuisance parameters
    reuse them.  With a device (no `evaluate`) and `spread`, the MAP evaluation sets the centre of a
    LinearisedSpread over `days`, each axis evaluation theta +- h_i e_i adds +-1/(2 h_i) times its days
    to J_i, and the maps are finalised with the factor of the model-block covariance.  -> NormalResult'''
    secs = {}
    t0 = time.perf_counter()
    if isinstance(at, MapResult):
        theta, z = at.theta.copy(), at.x[len(FREE_MODEL):].copy()
    else:
        theta, z = start_point(locinfo, cell_area, at)
    n_periods = float(round(theta[_NP]))
    theta[_NP] = n_periods
    post = Posterior(pop_model, locinfo, cell_area, n_periods, evaluate=evaluate, ndays=ndays)
    nm = post.nm
    x = np.concatenate([theta[FREE_MODEL], z])
    h = stencil_steps(x, post.lo, post.hi, post.eps)
    S = None
    if spread and evaluate is None and pop_model is not None:
        S = LinearisedSpread(pop_model, days, nm, thresholds)
        if profile:
            S.profile(True)
        center = post.theta(x[:nm]).tobytes()
        axis = {}
        for i in range(nm):
            if h[i] != 0.0:
                axis[post.theta(axis_point(x, h, i, 1)[:nm]).tobytes()] = (i, 0.5 / h[i])
                axis[post.theta(axis_point(x, h, i, -1)[:nm]).tobytes()] = (i, -0.5 / h[i])

        def hook(key):
            if key == center:
                S.set_center()
            elif key in axis:
                S.add(*axis[key])
        post.on_evaluate = hook
    try:
        secs['setup'] = time.perf_counter() - t0
        t1 = time.perf_counter()
        H, g, f0 = hessian(post.logp, x, h)
        secs['stencil'] = time.perf_counter() - t1
        if not np.all(np.isfinite(H)) or not math.isfinite(f0):
            bad = [post.names[i] for i in range(len(x)) if not np.all(np.isfinite(H[i]))]
            raise ValueError('the log density is not finite on the stencil (failed evaluations: %d; rows %s)'
                             % (post.failed, bad))
        C, pd, w = _covariance(H, h)
        F = model_factor(C, nm, pd)
        t1 = time.perf_counter()
        if S is not None:
            S.finalize(F)
            S.profile()           # synchronises: the finalize is in the stage's time
        secs['finalize'] = time.perf_counter() - t1
    except BaseException:
        if S is not None:
            S.close()
        raise
    _lp, ll = post.parts(x)
    held = [post.names[i] for i in range(len(x)) if h[i] == 0.0]
    return NormalResult(names=post.names, mu=x, C=C, H=H, steps=h, grad=g, pd=pd, eigenvalues=w, held=held,
                        logp=f0, lnL=ll, F=F, spread=S, evaluations=post.evaluations, failed=post.failed,
                        seconds=secs, n_periods=n_periods)

"""GPU test of the posterior predictive driver as a whole: one call with every option on against calls with the
options in groups.  An accumulator sees the same adds whatever else is fed beside it, so every map it exposes has to
be the same, bit for bit, in the call with everything and in the group that holds it -- the raw moments and counts
taken from the accumulators here, and every array of every file PredictiveResult.save writes.  Kalbar wind, 6 days,
R = 64, the two chains of test_peak_gpu.py; one model, and two models on two threads."""
import os
import warnings

import numpy as np
import pytest

from test_peak_gpu import _chain
from test_sites_gpu import _pop_model

pytestmark = pytest.mark.gpu

R = 64
RES_M = 10000.0 / R


def _options(chains):
    return dict(
        quantiles=[0.5], arrival=[1.0, 10.0], sensitivity=['sig_x', 'mu_r'], mc_error=dict(batches=4),
        peak=[1.0, 10.0], excursion=[1.0], core_range=[0.5, 0.95],
        reweight={'trap': dict(probes=[(0, 0, 1, 'count', 1e-3, 3), (3000, 0, 2, 'found', 0.5)]),
                  'flat': dict(log_weights=[np.zeros(len(t)) for t, _n in chains]), 'options': dict(min_ess=0)},
        catch=dict(traps=[(1, 0.5), (3, 2.0, 3)], levels=(0.5, 0.95), emergence=[(19, 0.5), (24, 2.0, 3)]),
        information=dict(traps=[(1, 0.01), (3, 1.0, 3)]),
        emergence=dict(collection_day=6, obs_days=[19, 21, 24]), exposure=[2, 4],
        sites=dict(sites=[(0.0, 0.0, 0.6), (13 * RES_M, 6 * RES_M, 0.5, 2)], days=[0, 1, 3, 5]),
        compare=dict(sites=[(0.0, 0.0, 1.0), (-5 * RES_M, 3 * RES_M, 0.3, 3)]))


# every option is in some group, none holds them all, and what needs two options (the plan's own peak, the catch's
# own Monte Carlo error, a projection's histogram, ...) finds both in one of them
GROUPS = (
    ('sites', 'compare', 'quantiles', 'arrival', 'peak', 'excursion', 'core_range', 'sensitivity'),
    ('sites', 'emergence', 'catch', 'information', 'reweight', 'mc_error'),
    ('emergence', 'exposure', 'quantiles', 'sensitivity', 'reweight', 'mc_error'),
)


def _raw(res):
    """{key: array} of the unthresholded maps of every accumulator of a result"""
    out = {}

    def summary(tag, s, keys):
        for d in keys:
            out[tag, d, 'mean'], out[tag, d, 'var'] = s.mean(d), s.variance(d)
            for k in range(len(s.thresholds)):
                out[tag, d, 'exc', k] = s.exceedance(d, k)

    def reweighted(tag, rw, keys):
        for name in rw.scenarios:
            for d in keys:
                out[tag, name, d, 'mean'], out[tag, name, d, 'var'] = rw.mean(name, d), rw.variance(name, d)

    def mc(tag, m, keys):
        for d in keys:
            out[tag, d, 'mean'], out[tag, d, 'mcse'], out[tag, d, 'ess'] = m.mean(d), m.mcse(d), m.ess(d)
            if m.rhat is not None:
                out[tag, d, 'rhat'] = m.rhat[d]

    def catch(tag, cp):
        keys = list(range(len(cp.traps)))
        summary(tag + '.summary', cp.summary, keys)
        if cp.reweight is not None:
            reweighted(tag + '.reweight', cp.reweight, keys)
        if cp.mc_error is not None:
            mc(tag + '.mc_error', cp.mc_error, keys)

    def information(tag, ip):
        for e in range(len(ip.traps)):
            out[tag, e, 'gain'], out[tag, e, 'entropy'] = ip.gain(e), ip.entropy(e)
            out[tag, e, 'conditional'] = ip.conditional(e)
            if ip.reweight is not None:
                for name in ip.reweight.scenarios:
                    out[tag, e, 'gain', name] = ip.gain(e, scenario=name)
        out[tag, 'weights'] = np.array(ip.weights)

    def one(tag, src, keys, arrival_keys):
        summary(tag + 'summary', src.summary, keys)
        if src.histogram is not None:
            for d in keys:
                out[tag + 'histogram', d] = src.histogram.counts(d)
        if src.arrival is not None:
            for d in arrival_keys:
                for k in range(len(src.arrival.thresholds)):
                    out[tag + 'arrival', k, d] = src.arrival.counts(k, d)
        if src.sensitivity is not None:
            S = src.sensitivity
            for d in keys:
                out[tag + 'sens', d, 'mean'], out[tag + 'sens', d, 'var'] = S.mean(d), S.variance(d)
                for n in S.params:
                    out[tag + 'sens', d, n] = S.covariance(d, n)
        if src.mc_error is not None:
            mc(tag + 'mc_error', src.mc_error, keys)
        if src.reweight is not None:
            reweighted(tag + 'reweight', src.reweight, keys)
        if src.catch is not None:
            catch(tag + 'catch', src.catch)
        if getattr(src, 'information', None) is not None:
            information(tag + 'information', src.information)

    one('', res, res.summary.days, res.summary.days)
    for name in ('emergence', 'exposure', 'sites'):
        pr = getattr(res, name)
        if pr is not None:
            one(name + '.', pr, list(range(len(pr.labels))), pr.labels)
    X = res.contrast
    if X is not None:
        for e in range(len(X.labels)):
            out['contrast', e, 'mean'], out['contrast', e, 'var'] = X.mean(e), X.variance(e)
            out['contrast', e, 'ppos'], out['contrast', e, 'pneg'] = X.prob_positive(e), X.prob_negative(e)
    return out


def _files(res, folder):
    """{(file, key): array} of everything save() writes as .npz"""
    os.makedirs(folder)
    res.save(os.path.join(folder, 'pp'))
    out = {}
    for name in sorted(os.listdir(folder)):
        if name.endswith('.npz'):
            with np.load(os.path.join(folder, name)) as f:
                for key in f.files:
                    out[name, key] = f[key]
    return out


def _close(res):
    for name in ('summary', 'histogram', 'arrival', 'sensitivity', 'mc_error', 'peak', 'excursion', 'reweight',
                 'catch', 'information', 'core_range', 'emergence', 'exposure', 'sites', 'contrast'):
        acc = getattr(res, name)
        if acc is not None:
            acc.close()


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind in 'fc':
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize('nmodels', [1, 2])
def test_everything_at_once_equals_the_options_in_groups(nmodels, tmp_path):
    from parasitoids_amd import predictive as PR
    trace, names = _chain([2, 1, 3, 1, 2])
    chains = [(trace[:5], names), (trace[5:], names)]       # the run of three is cut in two: 2 + 1 + 2 | 1 + 1 + 2
    options = _options(chains)
    assert set().union(*GROUPS) == set(options) and all(set(g) != set(options) for g in GROUPS)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        models = [_pop_model(R=R, mode='exact') for _ in range(nmodels)]
        pm = models if nmodels > 1 else models[0]
        res = PR.posterior_predictive(pm, chains, thresholds=[1.0, 10.0], cell_area=RES_M ** 2, **options)
        assert res.failed == 0 and res.evaluations == 6 and res.summary.total_weight == 9
        raw_all, files_all = _raw(res), _files(res, str(tmp_path / 'all'))
        _close(res)
        seen_raw, seen_files = set(), set()
        for g, group in enumerate(GROUPS):
            part = PR.posterior_predictive(pm, chains, thresholds=[1.0, 10.0], cell_area=RES_M ** 2,
                                           **{name: options[name] for name in group})
            raw, files = _raw(part), _files(part, str(tmp_path / ('group%d' % g)))
            _close(part)
            assert len(raw) > 50 and len(files) > 50
            for got, want, what in ((raw, raw_all, 'map'), (files, files_all, 'file')):
                for key, arr in got.items():
                    assert key in want, (what, group, key)
                    if what == 'file' and key[1] == 'days':      # the labels of the file's maps: of the group's only
                        assert set(arr.tolist()) <= set(want[key].tolist()), (group, key)
                        continue
                    assert _same(arr, want[key]), (what, group, key)
            seen_raw |= set(raw)
            seen_files |= set(files)
    # every map and every saved array of the call with everything was compared in some group
    assert seen_raw == set(raw_all)
    assert seen_files == set(files_all)
    for m in models:
        m.close()

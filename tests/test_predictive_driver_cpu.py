"""CPU tests of the wiring of predictive.posterior_predictive: which accumulators it builds per chain, what it feeds
every member to and in which order, how it merges the chains and what it closes.  No device and no library: every
class and function the driver names in parasitoids_amd.predictive is replaced by a recording stub, the checks of the
arguments stay the real ones.  The expected traces (tests/golden/predictive_driver_trace.json) were recorded with
`record()` below from the driver as it was before it became table-driven; the module only uses names that exist
there, so the same file runs against both.

A stub records its construction and every evaluate, apply, add, reserve, merge and close with the arguments.  It
raises Misuse when it is used after its own close, and when it is applied, added to or reserved while the source it
was built from is closed (a merge reads the accumulators only: the driver has always merged the catch posteriors
after closing their fields).  Names do not depend on the order of construction: chain, class, source and a digest of
the other arguments, numbered only among equals (the two Monte Carlo error sequences of a chain)."""
import contextlib
import hashlib
import json
import os
import threading
import warnings

import numpy as np
import pytest

from parasitoids_amd import _lib as L
from parasitoids_amd import mcmc
from parasitoids_amd import predictive as PP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'predictive_driver_trace.json')
ACCUMULATORS = ('SpreadSummary', 'SpreadHistogram', 'ArrivalMaps', 'SensitivityMaps', 'PeakMaps', 'PeakPosterior',
                'ExcursionMaps', 'RangeMaps', 'MonteCarloError', 'ReweightedSummary', 'CatchFields', 'CatchPosterior',
                'InformationFields', 'InformationPosterior', 'Projection', 'ReleaseSites', 'PlanContrast')
NDAYS = 6
FAILS = 1            # the member (its number along _chain) whose evaluation raises ValueError, of the two chains


class Misuse(Exception):
    pass


def _chain(run_lengths):
    """runs of identical model parameters around the sampler's start values (as tests/test_peak_gpu.py)"""
    names = [m[0] for m in mcmc.MODEL_BLOCK]
    base = np.array([m[2] for m in mcmc.MODEL_BLOCK], dtype=np.float64)
    rows = []
    for n, length in enumerate(run_lengths):
        t = base.copy()
        t[names.index('sig_x')] += 6.0 * n
        rows += [t] * length
    return np.array(rows), names


def _member(theta):
    names = [m[0] for m in mcmc.MODEL_BLOCK]
    return int(round((theta[names.index('sig_x')] - mcmc.MODEL_BLOCK[names.index('sig_x')][2]) / 6.0))


def _chains(cut=5, runs=(2, 1, 3, 1, 2)):
    trace, names = _chain(runs)
    return [(trace[:cut], names), (trace[cut:], names)]      # 2 + 1 + 2 | 1 + 1 + 2


def _canon(x):
    if isinstance(x, (Stub, Model)):
        return '@' + x.name
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, (np.floating, np.integer)):
        return x.item()
    if isinstance(x, dict):
        return {str(k): _canon(v) for k, v in sorted(x.items(), key=lambda kv: str(kv[0]))}
    if isinstance(x, (list, tuple, range)):
        return [_canon(v) for v in x]
    return x


class World():
    """what one call of the driver did"""

    def __init__(self, fail_at=None, hip_at=None, fails=FAILS):
        self.fails = fails           # the member whose evaluation raises ValueError
        self.lock = threading.RLock()
        self.objects = []            # every stub, in the order of construction
        self.events = []             # (chain, name, method, args, kwargs)
        self.merges = {}             # name -> the names merged into it, in order
        self.pools = []              # pool_mc_error's arguments
        self.lagged = []             # (lags,) of every lagged_models call
        self.lagged_models = []
        self.built = 0               # constructions by the driver itself
        self.fail_at = fail_at       # the construction that raises
        self.hip_at = hip_at         # the evaluation of a base model that raises a HipError that is no parameter's
        self.evaluated = 0
        self.stride = 1
        self.counts = {}

    def construct(self):
        with self.lock:
            self.built += 1
            if self.built == self.fail_at:
                raise RuntimeError('construction %d fails' % self.built)

    def numbered(self, name):
        with self.lock:
            k = self.counts.get(name, 0)
            self.counts[name] = k + 1
        return '%s#%d' % (name, k) if k else name

    def event(self, chain, name, method, args, kwargs):
        with self.lock:
            self.events.append([chain, name, method, _canon(args), _canon(kwargs)])


class Model():
    """a PopModel: days, rad_dist, rad_res and a recording evaluate"""

    def __init__(self, world, index=0, root=None, lag=0):
        self.world, self.index, self.root, self.lag = world, index, root or self, lag
        self.name = 'lag%d' % lag if lag else 'pm'
        self.days = ['d%d' % d for d in range(lag, NDAYS)]
        self.rad_dist, self.rad_res = 8000.0, 8
        self.device = None
        self.chains_done = 0
        self.closed = False
        self.closes = 0

    def chain_now(self):
        return self.root.index + self.world.stride * self.root.chains_done

    def evaluate(self, *args, **kwargs):
        w = self.world
        if self.closed:
            raise Misuse('%s evaluated after close' % self.name)
        w.event(self.chain_now(), self.name, 'evaluate', args, kwargs)
        if not self.lag:
            with w.lock:
                w.evaluated += 1
                if w.evaluated == w.hip_at:
                    raise L.HipError(999, 'no parameter\'s fault')
            if args[0] == w.fails:
                raise ValueError('member %d does not evaluate' % w.fails)

    def close(self):
        self.closes += 1
        self.closed = True


class Stub():
    composite = {'CatchPosterior': 'fields', 'InformationPosterior': 'fields', 'PeakPosterior': 'maps'}

    def setup(self, world, cname, args, kwargs, inner=False):
        if not inner:
            world.construct()
        self.world, self.cname = world, cname
        self.sources = [a for a in args[:2 if cname == 'PlanContrast' else 1] if isinstance(a, (Stub, Model))]
        self.root = self.sources[0].root if self.sources else None
        self.chain = args[1] if cname == '_ReweightFeed' else self.root.chain_now()
        rest = _canon([args[len(self.sources):], kwargs])
        digest = hashlib.sha1(json.dumps(rest, sort_keys=True).encode()).hexdigest()[:8]
        self.name = world.numbered('c%d:%s(%s|%s)' % (self.chain, cname, ','.join(s.name for s in self.sources), digest))
        self.made = [cname, [s.name for s in self.sources], rest]
        self.closed, self.closes, self.owned = False, 0, []
        base = cname.split('.')[0]
        if base == 'SpreadSummary':
            self.days = list(range(NDAYS) if len(args) < 2 or args[1] is None else args[1])
        if base == 'ReleaseSites':
            self.days = list(args[2])
        if base in self.composite:
            setattr(self, self.composite[base], args[0])
            self.owned.append(args[0])
            self.given = None
            self.reweight = None
            self.traps, self.weights, self.cap = [], [], 0.0
        if base == 'CatchPosterior':
            self.mc_error = None
            if (args[2] if len(args) > 2 else kwargs.get('mc_batch')):
                self.mc_error = []
                for _half in range(2):
                    s = Stub()
                    s.setup(world, 'MonteCarloError.for_projection', (args[0], 'inner'), {}, inner=True)
                    self.mc_error.append(s)
        if base == '_ReweightFeed':
            self.rows = [[] for _ in args[0]['names']]
        with world.lock:
            world.objects.append(self)

    def _use(self, method, args, kwargs, needs_source=True):
        if self.closed:
            raise Misuse('%s: %s after close' % (self.name, method))
        if needs_source and any(s.closed for s in self.sources):
            raise Misuse('%s: %s while its source is closed' % (self.name, method))
        self.world.event(self.chain, self.name, method, args, kwargs)

    def apply(self, *args, **kwargs):
        self._use('apply', args, kwargs)

    def add(self, *args, **kwargs):
        self._use('add', args, kwargs)

    def reserve(self, *args, **kwargs):
        self._use('reserve', args, kwargs)

    def evaluate_lagged(self, *args, **kwargs):
        self._use('evaluate_lagged', args, kwargs)

    def log_weights(self, pm, first, length):
        self._use('log_weights', (pm, first, length), {})
        for rows in self.rows:
            rows.extend([0.0] * length)
        return [float(10 * first + j) for j in range(len(self.rows))]

    def merge(self, other):
        if self.closed or other.closed:
            raise Misuse('%s: merge of %s after close' % (self.name, other.name))
        with self.world.lock:
            self.world.merges.setdefault(self.name, []).append(other.name)

    def finish(self):
        pass

    def describe(self):
        return {'plan': self.made[2]}

    def members(self, name):
        return 1

    def skipped(self, name):
        return 0

    def log_total_weight(self, name):
        return 0.0

    def release(self):
        """what close does, also to what a composite owns (as the real ones: closing twice is harmless there)"""
        self.closed = True
        m = getattr(self, 'mc_error', None)
        for o in self.owned + (list(m) if isinstance(m, list) else [m] if isinstance(m, Stub) else []):
            o.release()

    def close(self):
        self.closes += 1
        self.release()


def _stub_class(world, cname):
    class S(Stub):
        def __init__(self, *args, **kwargs):
            self.setup(world, cname, args, kwargs)

        @classmethod
        def for_projection(cls, *args, **kwargs):
            self = cls.__new__(cls)
            self.setup(world, cname + '.for_projection', args, kwargs)
            return self
    S.__name__ = S.__qualname__ = cname
    return S


@contextlib.contextmanager
def _installed(world):
    """the driver's names in parasitoids_amd.predictive and mcmc replaced by the world's stubs"""
    new = {name: _stub_class(world, name) for name in ACCUMULATORS + ('_ReweightFeed',)}

    def lagged_models(pm, lags, wind_data=None):
        world.construct()
        with world.lock:
            world.lagged.append(_canon(lags))
            made = {int(lag): Model(world, root=pm, lag=int(lag)) for lag in lags if lag}
            world.lagged_models += list(made.values())
        return made

    def pool_mc_error(pairs):
        seqs = [s for pair in pairs for s in pair]
        with world.lock:
            world.pools.append([[s.name for s in pair] for pair in pairs])
        for s in seqs[1:]:
            seqs[0].merge(s)
            s.close()
        seqs[0].rhat = None
        return seqs[0]
    real_runs = PP._evaluate_runs

    def evaluate_runs(pm, *args, **kwargs):
        try:
            return real_runs(pm, *args, **kwargs)
        finally:
            if pm is not None:
                pm.chains_done += 1             # what the thread of this model builds next is the next chain's
    new.update(lagged_models=lagged_models, pool_mc_error=pool_mc_error, _evaluate_runs=evaluate_runs)
    old = {name: getattr(PP, name) for name in new}
    old_mcmc = (mcmc.model_args, mcmc.expected_observations)
    for name, v in new.items():
        setattr(PP, name, v)
    mcmc.model_args = lambda theta: (_member(theta),)
    mcmc.expected_observations = lambda pm, locinfo: True
    try:
        yield
    finally:
        for name, v in old.items():
            setattr(PP, name, v)
        mcmc.model_args, mcmc.expected_observations = old_mcmc


def everything(chains=None):
    """every option of the driver at once"""
    chains = chains or _chains()
    return dict(
        days=[0, 1, 3, 5], thresholds=[1.0, 10.0], quantiles=[0.5], arrival=[1.0, 10.0], sensitivity=['sig_x', 'mu_r'],
        mc_error=dict(batches=4), peak=[1.0, 10.0], excursion=dict(thresholds=[1.0], levels=(0.9,)),
        reweight={'trap': dict(probes=[(0, 0, 1, 'count', 1e-3, 3)]),
                  'flat': dict(log_weights=[np.zeros(len(t)) for t, _n in chains]), 'options': dict(min_ess=0)},
        catch=dict(traps=[(1, 0.5), (3, 2.0, 3)], levels=(0.5,), emergence=[(19, 0.5)]),
        information=dict(traps=[(1, 0.01), (3, 1.0, 3)]), core_range=[0.5, 0.95],
        emergence=dict(collection_day=6, obs_days=[19, 21, 24]), exposure=[2, 4],
        sites=dict(sites=[(0.0, 0.0, 0.6), (2000.0, 1000.0, 0.5, 2)], days=[0, 1, 3, 5]),
        compare=dict(sites=[(0.0, 0.0, 1.0), (-1000.0, 0.0, 0.3, 3)]))


def run(kwargs, nmodels=1, chains=None, fail_at=None, hip_at=None, fails=FAILS):
    """one call of the driver in a world of stubs -> (world, result or None, exception or None)"""
    world = World(fail_at, hip_at, fails)
    chains = chains or _chains()
    world.stride = nmodels if nmodels > 1 and len(chains) > 1 else 1
    models = [Model(world, p) for p in range(nmodels)]
    res = err = None
    with _installed(world), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        try:
            res = PP.posterior_predictive(models if nmodels > 1 else models[0], chains, **kwargs)
        except Exception as e:
            err = e
    return world, res, err


def trace(world):
    """what is compared with the golden file: per chain the calls in order, the reserves and the constructions sorted,
    per object the merges in order, the pooled sequences and the lags of the lagged models"""
    chains = sorted({e[0] for e in world.events} | {o.chain for o in world.objects})
    return {
        'calls': {str(c): [e[1:] for e in world.events if e[0] == c and e[2] != 'reserve'] for c in chains},
        'reserved': {str(c): sorted(json.dumps(e[1:]) for e in world.events if e[0] == c and e[2] == 'reserve')
                     for c in chains},      # part of a chain's setup, whose order is free
        'constructions': {str(c): sorted(json.dumps([o.name, o.made], sort_keys=True) for o in world.objects
                                         if o.chain == c) for c in chains},
        'merges': {name: others for name, others in sorted(world.merges.items())},
        'pools': sorted(json.dumps(p) for p in world.pools),
        'lagged': sorted({json.dumps(l) for l in world.lagged}),
    }


SUBSETS = {
    'nothing': dict(thresholds=[1.0]),
    'sites': dict(sites=dict(sites=[(0.0, 0.0, 0.6), (2000.0, 1000.0, 0.5, 2)], days=[0, 1, 3, 5])),
    'emergence_catch': dict(emergence=dict(collection_day=6, obs_days=[19, 21, 24]),
                            catch=dict(traps=[(1, 0.5)], emergence=[(19, 0.5), (24, 2.0, 3)])),
    # one chain whose first run straddles its Monte Carlo half boundary (5 rows: the half begins at row 2)
    'straddle': dict(thresholds=[1.0], mc_error=dict(batches=4), emergence=dict(collection_day=6),
                     catch=dict(traps=[(1, 0.5)])),
}
STRADDLE = [_chain([3, 2])]


def _evaluate(theta):
    return None


# pairs of bad arguments along the driver's order of checks: the first of the pair has to be the one reported
REFUSALS = [
    dict(core_range=[1.5], arrival=[-1.0]),
    dict(core_range=[0.5], evaluate=_evaluate, information='traps'),
    dict(information='traps', evaluate=_evaluate, reweight={'a': dict(log_weights=[[0.0]])}),
    dict(information=dict(traps=[(9, 1.0)]), catch=dict(traps=[])),
    dict(catch=dict(traps=[(1, -1.0)]), reweight={}),
    dict(reweight={'a': dict(log_weights=[[0.0]])}, evaluate=_evaluate, quantiles=[2.0]),
    dict(reweight={'a': dict(probes=[(0, 0, 9, 'count', 1.0, 1)])}, excursion=[]),
    dict(excursion=[-1.0], peak=[-1.0]),
    dict(peak=[-1.0], sites=dict()),
    dict(peak=[1.0], days=[3, 1], mc_error=dict(batches=3)),
    dict(mc_error=dict(batches=3), sensitivity=['nothing']),
    dict(mc_error=True, thresholds=[2.0, 1.0], quantiles=[0.0]),
    dict(sensitivity=['nothing'], quantiles=[2.0]),
    dict(quantiles=[0.5], edges=[1.0], arrival=[-1.0]),
    dict(arrival=[-1.0], emergence=dict()),
    dict(emergence=dict(collection_day=-1), sites=dict()),
    dict(exposure=[99], compare=dict(sites=[(0.0, 0.0, 1.0)])),
    dict(sites=dict(sites=[(0.0, 0.0, 1.0)], days=[1, 3]), catch=dict(traps=[(2, 1.0)]), compare=dict()),
    dict(compare=dict(sites=[(0.0, 0.0, 1.0)]), mc_error=dict(batches=40)),
    dict(sites=dict(sites=[(0.0, 0.0, 1.0)]), compare=dict(sites=[(0.0, 0.0, 1.0)]), thresholds=[],
         mc_error=dict(batches=40)),
    dict(reweight={'a': dict(log_weights=[[0.0], [0.0]])}, mc_error=dict(batches=40)),
    dict(mc_error=dict(batches=40), arrival=[1.0], days=[1, 1]),
]


def _refusal(kwargs):
    kwargs = dict(kwargs)
    have_model = kwargs.get('evaluate') is None
    world = World()
    with _installed(world), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        try:
            PP.posterior_predictive(Model(world) if have_model else None, _chains(), **kwargs)
        except Exception as e:
            assert world.built == 0 and not world.events, 'refused only after the work began'
            return [type(e).__name__, str(e)]
    return None


def _subset(name):
    if name == 'straddle':
        return run(SUBSETS[name], chains=STRADDLE, fails=None)
    return run(SUBSETS[name])


def record():
    """the golden traces, from the driver at hand"""
    out = {'all': trace(run(everything())[0]),
           'subsets': {name: trace(_subset(name)[0]) for name in SUBSETS},
           'refusals': [_refusal(kw) for kw in REFUSALS]}
    return out


@pytest.fixture(scope='module')
def gold():
    if not os.path.exists(GOLDEN):
        pytest.fail('%s is missing: it is recorded once, with record(), from the driver before the change under test; '
                    'this test does not write it' % GOLDEN)
    with open(GOLDEN) as fobj:
        return json.load(fobj)


def _same_trace(got, want):
    got = json.loads(json.dumps(got))
    for key in ('calls', 'reserved', 'constructions', 'merges', 'pools', 'lagged'):
        assert sorted(got[key]) == sorted(want[key]), key
        if isinstance(want[key], dict):
            for k in want[key]:
                assert got[key][k] == want[key][k], (key, k)
        else:
            assert got[key] == want[key], key


def _reachable(res):
    seen, todo = {}, [res]
    while todo:
        x = todo.pop()
        if id(x) in seen or isinstance(x, (str, bytes, int, float, np.ndarray, Model)) or x is None:
            continue
        seen[id(x)] = x
        if isinstance(x, dict):
            todo += list(x.values())
        elif isinstance(x, (list, tuple)):
            todo += list(x)
        elif hasattr(x, '__dict__'):
            todo += [v for k, v in vars(x).items() if k not in ('world', 'sources', 'root')]
    return {i for i, x in seen.items() if isinstance(x, Stub)}


def _check_lifetime(world, res=None):
    """every object the driver made is closed exactly once or, of a call that returned, in the result"""
    kept = _reachable(res) if res is not None else set()
    for o in world.objects:
        if o.cname == '_ReweightFeed':        # host lists only
            continue
        assert o.closes <= 1, '%s closed %d times' % (o.name, o.closes)
        assert o.closed or id(o) in kept, '%s is neither closed nor in the result' % o.name
    for m in world.lagged_models:
        assert m.closes == 1, 'lagged model %s of chain root %d closed %d times' % (m.name, m.root.index, m.closes)


def test_every_option_at_once_feeds_merges_and_closes_as_recorded(gold):
    world, res, err = run(everything())
    assert err is None, err
    _same_trace(trace(world), gold['all'])
    # the failed member is added nowhere: nothing but the evaluation carries its chain's second run
    calls = trace(world)['calls']['0']
    at = [i for i, c in enumerate(calls) if c[1] == 'evaluate' and c[0] == 'pm']
    assert len(at) == 3 and res.failed == 1 and res.evaluations == 6 and len(res.runs) == 5
    between = calls[at[1] + 1:at[2]]
    assert all(c[1] == 'evaluate' for c in between), between
    _check_lifetime(world, res)
    for name in ('summary', 'histogram', 'arrival', 'sensitivity', 'mc_error', 'peak', 'excursion', 'reweight', 'catch',
                 'information', 'core_range', 'emergence', 'exposure', 'sites', 'contrast', 'compare_plan',
                 'reweight_info', 'mc_plan'):
        assert getattr(res, name) is not None, name
    assert res.quantiles == [0.5] and res.excursion_levels == [0.9] and res.days == [0, 1, 3, 5]
    assert res.sites.information.given == {'traps': [[1, 0.01], [3, 1.0, 3]]} == res.information.given
    assert res.emergence.catch.given == res.catch.given and res.exposure.catch is None


def test_two_models_give_the_same_traces_per_chain(gold):
    world, res, err = run(everything(), nmodels=2)
    assert err is None, err
    got = trace(world)
    _same_trace(got, gold['all'])
    assert len(world.lagged) == 2 and len(world.lagged_models) == 4
    _check_lifetime(world, res)


@pytest.mark.parametrize('name', sorted(SUBSETS))
def test_subsets_of_the_options(gold, name):
    world, res, err = _subset(name)
    assert err is None, err
    _same_trace(trace(world), gold['subsets'][name])
    _check_lifetime(world, res)
    if name == 'straddle':      # the run of three rows goes 2 + 1 into the two sequences, of every pair of them
        adds = [c for c in trace(world)['calls']['0'] if 'MonteCarloError' in c[0] and c[1] == 'add']
        assert [c[2] for c in adds[:2]] == [[2], [1]] and len(adds) == 3 * 3


def test_of_two_bad_arguments_the_same_one_is_reported(gold):
    assert len(gold['refusals']) == len(REFUSALS)
    for kw, want in zip(REFUSALS, gold['refusals']):
        assert want is not None, kw
        assert _refusal(kw) == want, kw


def test_a_failing_construction_leaks_nothing():
    total = run(everything())[0].built
    assert total > 60
    for k in range(1, total + 1):
        world, res, err = run(everything(), fail_at=k)
        assert isinstance(err, RuntimeError) and str(err) == 'construction %d fails' % k, (k, err)
        _check_lifetime(world)
    world, res, err = run(everything(), nmodels=2, fail_at=total - 3)
    assert isinstance(err, RuntimeError)
    _check_lifetime(world)


def test_a_device_error_of_the_third_member_propagates_and_leaks_nothing():
    world, res, err = run(everything(), hip_at=3)
    assert isinstance(err, L.HipError) and err.code == 999
    assert world.evaluated == 3
    _check_lifetime(world)


if __name__ == '__main__':
    with open(GOLDEN, 'w') as fobj:
        json.dump(record(), fobj, indent=0, sort_keys=True)

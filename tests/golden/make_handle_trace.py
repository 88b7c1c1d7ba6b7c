"""Records tests/golden/handle_calls_trace.json: what the seventeen classes that own one handle of the C library
(sixteen in parasitoids_amd.predictive, laplace.LinearisedSpread) send to the library, what they return and what
they refuse, with no device and no library.  `_lib._lib` holds a recording stand-in while `record()` runs: every
ps_* symbol of `_lib.SIGNATURES` returns 0 and appends (symbol, arguments), the arguments decoded with the
signature -- scalars by value, handles as small integers, pointers as 'null' or 'set', numpy arrays handed to a
create / add / apply / merge / finalize / gather symbol with their contents.  A create writes a fresh id through
its out-pointer, an info or prof writes fixed numbers, every other output array is filled with 0, 1, 0, 1, ...

    python tests/golden/make_handle_trace.py        # rewrites the fixture

The fixture was recorded at the commit before the classes got their shared base, NeighbourhoodFields and
ProximityFields at the commit before the field sources got theirs; tests/test_handles_cpu.py re-records and compares.  The module only uses names that exist at both commits.  Where an add is given both a
weight below 1 and a model that is not evaluated far enough, the classes used to differ in which ValueError
came; no case here does both."""
import contextlib
import ctypes as C
import gc
import hashlib
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from parasitoids_amd import _lib as L                      # noqa: E402
from parasitoids_amd import laplace as LA                  # noqa: E402
from parasitoids_amd import mcmc                           # noqa: E402
from parasitoids_amd import predictive as PP               # noqa: E402

FIXTURE = os.path.join(HERE, 'handle_calls_trace.json')
INPUT_SYMBOLS = ('create', 'add', 'apply', 'merge', 'finalize', 'set_center', 'gather')
ATTRIBUTES = ('days', 'thresholds', 'fractions', 'live', 'nout', 'N', 'device', 'nbytes', 'fields_kind', '_slot',
              'in_days')
HAVE_AREA = ('ArrivalMaps', 'ExcursionMaps', 'RangeMaps', 'PlanContrast')     # the classes that state areas


class Library():
    """the stand-in for the loaded library"""

    def __init__(self):
        self.calls = []
        self.next_id = 1
        self.fail_create = False

    def __getattr__(self, name):
        if name not in L.SIGNATURES:
            raise AttributeError(name)
        fn = lambda *args: self._call(name, args)         # noqa: E731
        self.__dict__[name] = fn
        return fn

    def ps_last_error(self):
        return b''

    def _call(self, name, args):
        _res, types_ = L.SIGNATURES[name]
        assert len(args) == len(types_), (name, len(args), len(types_))
        verb = name.split('_', 2)[2]
        takes = verb.startswith(INPUT_SYMBOLS)
        writes = 2                                          # the k-th output of an info or prof reads k + 2
        rec = []
        for a, t in zip(args, types_):
            if t is L._VP:
                rec.append(None if a is None else 'h%d' % (a.value or 0))
            elif t is C.POINTER(L._VP):
                if verb == 'create':
                    if not self.fail_create:
                        a._obj.value = 100 + self.next_id
                        self.next_id += 1
                    rec.append('out')
                else:                                       # ps_mcerr_rhat: the handles of the sequences
                    rec.append('set')
            elif t in (C.c_int, C.c_int64, C.c_uint32):
                rec.append(int(a))
            elif t is C.c_double:
                rec.append(float(a))
            elif a is None:
                rec.append('null')
            else:
                arr = getattr(a, '_arr', None)              # the numpy array behind ndarray.ctypes.data_as
                if verb in ('info', 'prof'):
                    if arr is None:
                        a._obj.value = writes
                    else:
                        arr[...] = writes
                    writes += 1
                    rec.append('set')
                elif arr is not None and takes and not (verb == 'gather' and t is L._F64P):
                    rec.append(np.asarray(arr).ravel().tolist())
                else:
                    if arr is not None:
                        flat = arr.reshape(-1)
                        flat[...] = (np.arange(flat.size) % 2).astype(arr.dtype)
                    rec.append('set')
        self.calls.append([name] + rec)
        if verb == 'create' and self.fail_create:
            return L.PS_ERR_OOM
        return 0


def canon(x):
    if isinstance(x, np.ndarray):
        return '%s%s:%s' % (x.dtype.str[1:], list(x.shape), hashlib.sha1(np.ascontiguousarray(x).tobytes()).hexdigest()[:8])
    if isinstance(x, (np.floating, np.integer, np.bool_)):
        return x.item()
    if isinstance(x, float) and x != x:
        return 'nan'
    if isinstance(x, float) and x in (float('inf'), float('-inf')):
        return str(x)
    if isinstance(x, dict):
        return {str(k): canon(v) for k, v in x.items()}
    if isinstance(x, (list, tuple, range)):
        return [canon(v) for v in x]
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    return '<%s>' % type(x).__name__


def describe(obj):
    """the attributes every class keeps, and whether the handle is set"""
    out = {a: canon(getattr(obj, a)) for a in ATTRIBUTES if hasattr(obj, a)}
    if type(obj).__name__ in HAVE_AREA:
        out['cell_area'] = obj.cell_area
    out['_h'] = bool(obj._h)
    return out


def handle_of_failed(exc, cls):
    """whether the object whose construction raised `exc` holds a handle (it is a `self` of some frame)"""
    tb = exc.__traceback__
    found = None
    while tb is not None:
        me = tb.tb_frame.f_locals.get('self')
        if isinstance(me, cls):
            found = bool(me._h)
        tb = tb.tb_next
    return found


class Trace():
    def __init__(self, lib):
        self.lib = lib
        self.steps = []

    def do(self, label, fn, failed=None):
        """run one step and record [label, calls, value, error], trailing None left out: the error [type, text], of a
        refused construction also whether the object is left with a handle"""
        self.lib.calls = []
        out = value = error = None
        try:
            out = fn()
            value = describe(out) if hasattr(out, '_h') else canon(out)
        except Exception as e:
            error = [type(e).__name__, str(e)]
            if failed is not None:
                error.append(handle_of_failed(e, failed))
            e = None
        step = [label, self.lib.calls, value, error]
        while step[-1] is None:                             # [label, calls], [.., value] or [.., value, error]
            step.pop()
        self.steps.append(step)
        self.lib.calls = []
        return out


def model():
    return types.SimpleNamespace(rad_res=2, rad_dist=8.0, device=None, days=range(6), r_number=3.0, _nd=6,
                                 prob_model=None, solver=types.SimpleNamespace(_h=C.c_void_p(99)))


THETA = [m[2] for m in mcmc.MODEL_BLOCK]
SOURCES = {
    'project': lambda pm: PP.Projection(pm, [[1, 0, 1], [0, 0, 0], [0, 2, 0]], [0, 1, 4]),
    'sites': lambda pm: PP.ReleaseSites(pm, [(0, 0, 1), (4, 0, 2)], [0, 2, 3]),
    'peak': lambda pm: PP.PeakMaps(pm, [0.5], [1, 2, 4]),
    'catch': lambda pm: PP.CatchFields(pm, [(1, 0.5), (4, 0.25, 2)]),
    'gain': lambda pm: PP.InformationFields(pm, [(1, 0.5), (4, 0.25, 1)]),
}


def feed(src):
    """bring a source to the state an accumulator reads"""
    src.add(1) if src.fields_kind == 'peak' else src.apply()


# per class: the constructions (None: from the model), one use, the use with weight 0, the accessors (one per fetch
# symbol), the host-side refusals, whether it merges / resets / counts weight
def specs():
    S = {}
    S['SpreadSummary'] = dict(
        make=lambda pm, src: PP.SpreadSummary(pm, [0, 2, 5], [0.5]) if src is None else
        PP.SpreadSummary.for_projection(src, [0.5]),
        over=(None, 'project', 'sites', 'peak', 'catch', 'gain'), use=lambda o: o.add(2), zero=lambda o: o.add(0),
        access=[('mean', lambda o: o.mean(0)), ('sd', lambda o: o.sd(0)), ('exceedance', lambda o: o.exceedance(0, 0)),
                ('fetch_slot', lambda o: o.fetch_slot(0, 1))],
        refuse=[('day', lambda o: o.mean(77)), ('threshold', lambda o: o.exceedance(0, 1))])
    S['SpreadHistogram'] = dict(
        make=lambda pm, src: PP.SpreadHistogram(pm, [0, 2, 5], (1e-2, 1e2, 2)) if src is None else
        PP.SpreadHistogram.for_projection(src, None, [0.5, 1.0, 2.0]),
        over=(None, 'project', 'sites', 'peak'), use=lambda o: o.add(2), zero=lambda o: o.add(0),
        access=[('edges', lambda o: o.edges), ('counts', lambda o: o.counts(0)), ('quantile', lambda o: o.quantile(0, 0.5)),
                ('quantile_bounds', lambda o: o.quantile_bounds(0, 0.5)),
                ('exceedance', lambda o: o.exceedance(0, o.edges[1])), ('dead', lambda o: o.counts(1))],
        refuse=[('day', lambda o: o.counts(77)), ('level', lambda o: o.quantile(0, 0.0)),
                ('edge', lambda o: o.exceedance(0, 0.123))])
    S['ArrivalMaps'] = dict(
        make=lambda pm, src: PP.ArrivalMaps(pm, [0.5, 1.5], [0, 2, 5]) if src is None else
        PP.ArrivalMaps.for_projection(src, [0.5, 1.5]),
        over=(None, 'project', 'sites'), use=lambda o: o.add(2), zero=lambda o: o.add(0),
        access=[('counts', lambda o: o.counts(1, o.days[0])), ('never', lambda o: o.counts(0, None)),
                ('prob_by', lambda o: o.prob_by(0, o.days[-1])), ('quantile', lambda o: o.quantile(1, 0.5)),
                ('reached', lambda o: o.reached(1)), ('reached_area', lambda o: o.reached_area(0))],
        refuse=[('day', lambda o: o.prob_by(0, 77)), ('threshold', lambda o: o.counts(2, o.days[0])),
                ('level', lambda o: o.quantile(0, 1.5))])
    S['PeakMaps'] = dict(
        make=lambda pm, src: PP.PeakMaps(pm, [0.5, 1.5], [0, 2, 5]) if src is None else
        PP.PeakMaps.for_projection(src, [0.5, 1.5]),
        over=(None, 'project', 'sites'), use=lambda o: o.add(2), zero=lambda o: o.add(0),
        access=[('field', lambda o: o.field()), ('day_counts', lambda o: o.day_counts(o.days[0])),
                ('day_prob', lambda o: o.day_prob(o.days[-1])), ('day_quantile', lambda o: o.day_quantile(0.5)),
                ('duration_counts', lambda o: o.duration_counts(1, 0)), ('duration_prob', lambda o: o.duration_prob(0, 1)),
                ('duration_quantile', lambda o: o.duration_quantile(1, 0.5)),
                ('duration_mean', lambda o: o.duration_mean(0))],
        refuse=[('day', lambda o: o.day_prob(77)), ('threshold', lambda o: o.duration_mean(2)),
                ('duration', lambda o: o.duration_prob(0, 0)), ('level', lambda o: o.day_quantile(0.0))])
    S['ExcursionMaps'] = dict(
        make=lambda pm, src: PP.ExcursionMaps(pm, [0.5, 1.5], [0, 2, 5]) if src is None else
        PP.ExcursionMaps.for_projection(src, [0.5, 1.5]),
        over=(None, 'project', 'sites', 'peak'), use=lambda o: o.add(2), zero=lambda o: o.add(0),
        access=[('reserve', lambda o: o.reserve(8)), ('capacity', lambda o: o.capacity), ('nbytes', lambda o: o.nbytes),
                ('counts', lambda o: o.counts(1, o.days[0])), ('mask', lambda o: o.mask(0, 0, o.days[0])),
                ('bounds', lambda o: o.bounds(1, o.days[0])), ('above', lambda o: o.above(0, o.days[0])),
                ('contour', lambda o: o.contour(1, o.days[-1])), ('region', lambda o: o.region(0, o.days[0], 0.9)),
                ('areas', lambda o: o.areas(0, o.days[0], [0.9]))],
        refuse=[('day', lambda o: o.counts(0, 77)), ('threshold', lambda o: o.above(2, o.days[0])),
                ('level', lambda o: o.region(0, o.days[0], 0.5))])
    S['RangeMaps'] = dict(
        make=lambda pm, src: PP.RangeMaps(pm, [0.5, 0.95], [0, 2, 5]) if src is None else
        PP.RangeMaps.for_projection(src, [0.5, 0.95]),
        over=(None, 'project', 'sites'), use=lambda o: o.add(2), zero=lambda o: o.add(0),
        access=[('reserve', lambda o: o.reserve(8)), ('capacity', lambda o: o.capacity), ('nbytes', lambda o: o.nbytes),
                ('counts', lambda o: o.counts(1, o.days[0])), ('prob', lambda o: o.prob(0, o.days[-1])),
                ('range', lambda o: o.range(0, o.days[0])), ('weights', lambda o: o.weights),
                ('levels', lambda o: o.levels(1, o.days[0])), ('cells', lambda o: o.cells(0, o.days[0])),
                ('mass', lambda o: o.mass(o.days[0])), ('area', lambda o: o.area(0, o.days[0]))],
        refuse=[('day', lambda o: o.prob(0, 77)), ('fraction', lambda o: o.counts(2, o.days[0]))])
    S['Projection'] = dict(
        make=lambda pm, src: SOURCES['project'](pm), over=(None,), use=lambda o: o.apply(), zero=None,
        access=[('applies', lambda o: o.applies), ('field', lambda o: o.field(0)), ('dead', lambda o: o.field(1)),
                ('gather', lambda o: o.gather([0, 1], [2, 3]))],
        refuse=[('output', lambda o: o.field(3)), ('gather', lambda o: o.gather([0, 1], [2]))],
        merges=False, resets=False, weighs=False)
    S['ReleaseSites'] = dict(
        make=lambda pm, src: SOURCES['sites'](pm), over=(None,), use=lambda o: o.apply(), zero=None,
        access=[('applies', lambda o: o.applies), ('field', lambda o: o.field(1)),
                ('gather', lambda o: o.gather([0, 1], [2, 3])), ('describe', lambda o: o.describe()),
                ('models', lambda o: [lag for lag, _m in o.models()])],
        refuse=[('output', lambda o: o.field(3))], merges=False, resets=False, weighs=False)
    S['PlanContrast'] = dict(
        make=lambda pm, src: PP.PlanContrast(src[0], src[1], [0.5]), over=('project', 'sites'), pair=True,
        use=lambda o: o.add(2), zero=lambda o: o.add(0),
        access=[('mean', lambda o: o.mean(0)), ('sd', lambda o: o.sd(0)), ('prob_positive', lambda o: o.prob_positive(0)),
                ('gain', lambda o: o.gain(0, 0)), ('loss', lambda o: o.loss(0, 0)), ('counts', lambda o: o.counts(0, 3)),
                ('weights', lambda o: o.weights), ('coverage', lambda o: o.coverage(0)),
                ('coverage_difference', lambda o: o.coverage_difference(0))],
        refuse=[('output', lambda o: o.mean(3)), ('threshold', lambda o: o.gain(0, 1)), ('plane', lambda o: o.counts(0, 4))])
    S['SensitivityMaps'] = dict(
        make=lambda pm, src: PP.SensitivityMaps(pm, ['sig_x', 'lam'], [0, 2, 5]) if src is None else
        PP.SensitivityMaps.for_projection(src, ['sig_x', 'lam']),
        over=(None, 'project', 'sites'), use=lambda o: o.add(THETA, 2), zero=lambda o: o.add(THETA, 0),
        access=[('moments', lambda o: [o.moments.W, o.moments.members]), ('mean', lambda o: o.mean(0)),
                ('covariance', lambda o: o.covariance(0, 'lam')), ('dominant', lambda o: o.dominant(0)),
                ('fetch_slot', lambda o: o.fetch_slot(0, 2)), ('describe', lambda o: sorted(o.describe()))],
        refuse=[('day', lambda o: o.mean(77)), ('parameter', lambda o: o.covariance(0, 'mu_r')),
                ('theta', lambda o: o.add(THETA[:3], 1)), ('finalize', lambda o: o.finalize()),
                ('moments', lambda o: [o.moments.W, o.moments.members])])
    S['MonteCarloError'] = dict(
        make=lambda pm, src: PP.MonteCarloError(pm, 3, [0, 2, 5], [0.5]) if src is None else
        PP.MonteCarloError.for_projection(src, 3, [0.5]),
        over=(None, 'project', 'sites', 'catch'), use=lambda o: o.add(2), zero=lambda o: o.add(0),
        access=[('finish', lambda o: o.finish()), ('batches', lambda o: [o.batches, o.batch_weight, o.used_weight,
                                                                        o.open_weight, o.discarded_weight]),
                ('plane', lambda o: o.plane(0, 2)), ('counts', lambda o: o.counts(0, 0)), ('mean', lambda o: o.mean(0)),
                ('mcse', lambda o: o.mcse(0)), ('variance', lambda o: o.variance(0)), ('ess', lambda o: o.ess(0)),
                ('prob', lambda o: o.prob(0, 0)), ('prob_mcse', lambda o: o.prob_mcse(0, 0)),
                ('prob_ess', lambda o: o.prob_ess(0, 0))],
        refuse=[('day', lambda o: o.plane(77, 0)), ('threshold', lambda o: o.counts(0, 1))], weighs='members')
    S['ReweightedSummary'] = dict(
        make=lambda pm, src: PP.ReweightedSummary(pm, ['a', 'b'], [0, 2, 5], [0.5]) if src is None else
        PP.ReweightedSummary.for_projection(src, ['a', 'b'], [0.5]),
        over=(None, 'project', 'sites', 'peak', 'catch', 'gain'), use=lambda o: o.add([0.0, -1.0], 2),
        zero=lambda o: o.add([0.0, -1.0], 0),
        access=[('ref', lambda o: list(o.ref)), ('total_weight', lambda o: o.total_weight('a')),
                ('log_total_weight', lambda o: o.log_total_weight('b')), ('members', lambda o: o.members('b')),
                ('skipped', lambda o: o.skipped('a')), ('mean', lambda o: o.mean('a', 0)), ('sd', lambda o: o.sd('b', 0)),
                ('exceedance', lambda o: o.exceedance('a', 0, 0)), ('fetch_slot', lambda o: o.fetch_slot(1, 0, 1)),
                ('scale', lambda o: o.scale({'a': 1.0, 'b': -2.0}, 3))],
        refuse=[('day', lambda o: o.mean('a', 77)), ('scenario', lambda o: o.mean('c', 0)),
                ('threshold', lambda o: o.exceedance('a', 0, 1)), ('log_weights', lambda o: o.add([0.0], 1)),
                ('ref', lambda o: list(o.ref))], weighs=False)
    S['CatchFields'] = dict(
        make=lambda pm, src: SOURCES['catch'](pm) if src is None else PP.CatchFields.for_projection(src, [(0, 0.5), (2, 1.0, 3)]),
        over=(None, 'project', 'sites'), use=lambda o: o.apply(), zero=None,
        access=[('applies', lambda o: o.applies), ('field', lambda o: o.field(1)),
                ('gather', lambda o: o.gather([0, 1], [2, 3])), ('rates', lambda o: [o.rates, o.counts])],
        refuse=[('output', lambda o: o.field(2))], merges=False, resets=False, weighs=False)
    S['InformationFields'] = dict(
        make=lambda pm, src: SOURCES['gain'](pm) if src is None else
        PP.InformationFields.for_projection(src, [(0, 0.5), (2, 1.0, 2)]),
        over=(None, 'project', 'sites'), use=lambda o: o.apply(), zero=None,
        access=[('applies', lambda o: o.applies), ('plane', lambda o: o.plane(1, 'tail')),
                ('plane_index', lambda o: o.plane_index(1, 'h')), ('gather', lambda o: o.gather([0, 1], [2, 3])),
                ('result', lambda o: o.result(0, 'entropy')), ('shape', lambda o: [o.ntrap, o.ymax, o.base])],
        refuse=[('trap', lambda o: o.result(2, 'gain')), ('plane', lambda o: o.plane(0, 'p9')),
                ('what', lambda o: o.result(0, 'loss'))], merges=False, resets=False, weighs=False)
    S['NeighbourhoodFields'] = dict(
        make=lambda pm, src: PP.NeighbourhoodFields(pm, [(1, 4.0), (4, 0.0)]) if src is None else
        PP.NeighbourhoodFields.for_projection(src, [(0, 4.0), (2, 9.0)]),
        over=(None, 'project', 'sites'), use=lambda o: o.apply(), zero=None,
        access=[('applies', lambda o: o.applies), ('field', lambda o: o.field(1)),
                ('gather', lambda o: o.gather([0, 1], [2, 3])), ('set_skip', lambda o: o.set_skip(False)),
                ('discs', lambda o: [o.radii_m, o.r2, o.half, o.cells])],
        refuse=[('output', lambda o: o.field(2)), ('gather', lambda o: o.gather([0, 1], [2]))],
        merges=False, resets=False, weighs=False)
    S['ProximityFields'] = dict(
        make=lambda pm, src: PP.ProximityFields(pm, [(1, 0.5), (4, 0.25, 'in')]) if src is None else
        PP.ProximityFields.for_projection(src, [(0, 0.5, 'in'), (2, 1.0)]),
        over=(None, 'project', 'sites'), use=lambda o: o.apply(), zero=None,
        access=[('applies', lambda o: o.applies), ('strip', lambda o: o.strip), ('field', lambda o: o.field(1)),
                ('d2', lambda o: o.d2(0)), ('gather', lambda o: o.gather([0, 1], [2, 3])),
                ('set_strip', lambda o: o.set_strip(8)),
                ('sets', lambda o: [o.thresholds, o.sides, o.cell_m, o.far2, o.far_m])],
        refuse=[('output', lambda o: o.d2(2)), ('gather', lambda o: o.gather([0, 1], [2]))],
        merges=False, resets=False, weighs=False)
    S['LinearisedSpread'] = dict(
        make=lambda pm, src: LA.LinearisedSpread(pm, [0, 2, 5], 2, [0.5], ['sig_x', 'lam']), over=(None,),
        use=lambda o: (o.set_center(), o.add(1, 0.25)), zero=None,
        access=[('finalize', lambda o: o.finalize([[1.0], [0.5]])), ('info', lambda o: o.info()),
                ('mean', lambda o: o.mean(0)), ('sd', lambda o: o.sd(2)), ('exceedance', lambda o: o.exceedance(5, 0)),
                ('sensitivity', lambda o: o.sensitivity(0, 'lam')), ('fetch_slot', lambda o: o.fetch_slot(1, 16))],
        refuse=[('day', lambda o: o.mean(77)), ('threshold', lambda o: o.exceedance(0, 1)),
                ('parameter', lambda o: o.sensitivity(0, 2)), ('finalize', lambda o: o.finalize([[1.0]]))],
        merges=False, weighs=False)
    return S


def scenario(lib, name, spec, over):
    """every step of one class over one source of fields; the accessors and what they refuse over the model and
    over the first of the other sources only -- a further source changes the add's symbol and nothing behind it"""
    full = over in spec['over'][:2]
    t = Trace(lib)
    lib.next_id = 1
    pm = model()
    cls = getattr(PP, name, None) or getattr(LA, name)
    srcs = []
    if over is not None:
        srcs = [SOURCES[over](pm) for _ in range(2 if spec.get('pair') else 1)]
        for s in srcs:
            feed(s)
    src = None if over is None else (srcs if spec.get('pair') else srcs[0])
    make = lambda: spec['make'](pm, src)                  # noqa: E731
    obj = t.do('create', make)
    t.do('use', lambda: spec['use'](obj))
    if spec['zero'] is not None:
        t.do('weight 0', lambda: spec['zero'](obj))
    if over is None and name != 'PlanContrast':
        pm._nd = 3
        t.do('model of 3 days', lambda: spec['use'](obj))
        pm._nd = 6
    if spec.get('merges', True):
        other = make()
        t.do('merge', lambda: obj.merge(other))
        if full:                                            # a peer over other days, or other outputs
            other.days = other.labels = [0, 1]
            t.do('merge of different days', lambda: obj.merge(other))
        other.close()
    for label, fn in spec['access'] if full else ():
        t.do(label, lambda: fn(obj))
    for label, fn in spec['refuse'] if full else ():
        t.do('refused ' + label, lambda: fn(obj))
    weighs = spec.get('weighs', True) if full else False
    if weighs is True:
        t.do('total_weight', lambda: obj.total_weight)
    if weighs:
        t.do('members', lambda: obj.members)
    if full:
        t.do('profile(None)', lambda: obj.profile())
        t.do('profile(True)', lambda: obj.profile(True))
    if full and spec.get('resets', True):
        t.do('reset', lambda: obj.reset())
    t.do('close', lambda: (obj.close(), bool(obj._h)))
    if full:
        t.do('close again', lambda: (obj.close(), bool(obj._h)))

    def with_form():
        with make() as o:
            inside = bool(o._h)
        return inside, bool(o._h)
    if full:
        t.do('with', with_form)
    lib.fail_create = True
    t.do('create refused', make, failed=cls)
    lib.fail_create = False
    for s in srcs:
        s.close()
    return t.steps


@contextlib.contextmanager
def stand_in():
    lib = Library()
    saved = L._lib
    L._lib = lib
    try:
        yield lib
    finally:
        L._lib = saved


def record():
    out = {}
    with stand_in() as lib, np.errstate(all='ignore'):
        for name, spec in specs().items():
            for over in spec['over']:
                out['%s over %s' % (name, over or 'the model')] = scenario(lib, name, spec, over)
    gc.collect()
    return out


def dumps(trace):
    """one step per line"""
    lines = []
    for key, steps in trace.items():
        body = ',\n'.join(' ' + json.dumps(s, sort_keys=True, separators=(',', ':')) for s in steps)
        lines.append('%s: [\n%s\n]' % (json.dumps(key), body))
    return '{\n' + ',\n'.join(lines) + '\n}\n'


if __name__ == '__main__':
    with open(FIXTURE, 'w') as f:
        f.write(dumps(record()))
    print('%s: %d bytes' % (FIXTURE, os.path.getsize(FIXTURE)))

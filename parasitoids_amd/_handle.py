"""The base of every class that owns one ps_<x> handle of the C library: the accumulators and field sources of
`predictive` and `laplace.LinearisedSpread`.  `_Handle` holds what they all do alike -- the handle's lifetime, the
calls behind it, the counters of ps_<x>_info, profiling, the index checks -- and the two ways an add or an
apply reads its fields: the day records of the model's last evaluation, or the outputs of a fields source.  A class
states its `_prefix`, `_info_types`, `_prof_pairs` and `_noun`, calls `_attach` and `_create`, and keeps only what is
its own; `_Accumulator` adds reset, total_weight and members for those that sum weighted members, `_FieldSource`
what the sources of fields share.  HipSolve and WindModel are not of this kind: their handles are retargeted and
cached.
"""
import ctypes as C

import numpy as np

from . import _lib as L

NEGVAL = 1e-8          # r_small_vals threshold of the daily solutions (CalcSol.py:126-132)
MAX_PROJECT_IN = 32    # ps_project: the input records of one launch's descriptors


def _day_slots(days):
    '''record (kind, idx, use_delta) of every model day: day 0 the state, day d chain record d - 1'''
    kind = L.i32([L.REC_STATE if d == 0 else L.REC_CHAIN for d in days])
    idx = L.i32([0 if d == 0 else d - 1 for d in days])
    delta = L.i32([0 if d == 0 else 1 for d in days])
    return kind, idx, delta


def _day_scales(pm, days):
    '''(stat_scale, post_scale) per day: what PopModel.population applies to each record'''
    r = float(pm.r_number)
    return L.f64([1.0 if d == 0 else r for d in days]), L.f64([r if d == 0 else 1.0 for d in days])


def _check_evaluated(pm, days, what):
    nd = getattr(pm, '_nd', 0)
    if pm.solver is None or max(days) >= nd:
        raise ValueError('the last evaluation has %d days; the %s needs day %d' % (nd, what, max(days)))


def check_in_days(in_days):
    '''a projection's input days as a list of ints: 1..32 model days >= 0, strictly increasing'''
    d = [int(x) for x in in_days]
    if not 1 <= len(d) <= MAX_PROJECT_IN:
        raise ValueError('%d projection input days; 1..%d fit one launch' % (len(d), MAX_PROJECT_IN))
    if d[0] < 0 or any(b <= a for a, b in zip(d, d[1:])):
        raise ValueError('projection input days must be model days >= 0, strictly increasing: %r' % (d,))
    return d


class _Handle():
    _prefix = None         # 'ps_summary': the class's symbols are ps_summary_create, ps_summary_add, ...
    _info_types = (C.c_double, C.c_int64)      # the out-parameters of ps_<x>_info: total weight, members, ...
    _prof_pairs = 1        # the (ms, launches) pairs of ps_<x>_prof
    _noun = None           # what the class calls itself in its messages: 'summary'
    _proj = None           # the fields source an accumulator reads; None: the model's day records

    def __new__(cls, *args, **kwargs):
        self = super().__new__(cls)
        self._h = L._VP()              # empty until _create: close and __del__ are safe wherever a constructor raises
        return self

    def _attach(self, pop_model):
        '''the library and the grid facts of the model'''
        self._lib = L.load()
        self.pm = pop_model
        self.N = 2 * int(pop_model.rad_res) + 1
        self.device = L.default_device() if pop_model.device is None else int(pop_model.device)
        self.pitch = (self.N * self.N + 63) // 64 * 64
        self.cell_area = (float(pop_model.rad_dist) / int(pop_model.rad_res)) ** 2

    def _create(self, *args):
        L.check(getattr(self._lib, self._prefix + '_create')(self.device, self.N, *args, C.byref(self._h)))

    def _call(self, name, *args):
        L.check(getattr(self._lib, self._prefix + '_' + name)(self._h, *args))

    def close(self):
        if self._h:
            getattr(self._lib, self._prefix + '_destroy')(self._h)
            self._h = L._VP()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _info(self):
        out = [t() for t in self._info_types]
        self._call('info', *[C.byref(v) for v in out])
        return tuple(v.value for v in out)

    def _profile(self, enable):
        out = [t() for _ in range(self._prof_pairs) for t in (C.c_double, C.c_int64)]
        self._call('prof', -1 if enable is None else int(bool(enable)), *[C.byref(v) for v in out])
        return tuple(v.value for v in out)

    # ---------------------------------------------------------------- argument checks
    @staticmethod
    def _weight(weight):
        w = int(weight)
        if w < 1:
            raise ValueError('weight must be a positive integer')
        return w

    @staticmethod
    def _index(i, n, noun):
        if not 0 <= int(i) < n:
            raise ValueError('%s %r of %d' % (noun, i, n))
        return int(i)

    def _k(self, k):
        return self._index(k, len(self.thresholds), 'threshold')

    def _e(self, e):
        return self._index(e, self.nout, 'output')

    def _slot_of(self, day, noun=None):
        '''the device slot of a day; None for a projection's output without weight (zero throughout)'''
        if day not in self._slot:
            if self._proj is not None and day in self.days:
                return None
            raise ValueError('day %r is not in the %s %s' % (day, noun or self._noun, self.days))
        return self._slot[day]

    # ---------------------------------------------------------------- where an add or an apply reads its fields
    def _set_days(self, days):
        '''the descriptors of the model days `_from_model` reads, built once'''
        self._days = days
        self._kind, self._idx, self._delta = _day_slots(days)

    def _set_source(self, projection, days, keys=None):
        '''what an accumulator sums: `days` of the model, or (the labels of) the outputs of `projection`; one device
        slot per key, by default per day'''
        self._proj = projection
        self.days = days
        self._slot = {d: i for i, d in enumerate(days if keys is None else keys)}
        if projection is None:
            self._set_days(days)

    def _from_model(self, name, *tail, head=()):
        '''ps_<x>_<name> over the day records of the model's last evaluation'''
        pm = self.pm
        _check_evaluated(pm, self._days, self._noun)
        stat, post = _day_scales(pm, self._days)
        self._call(name, pm.solver._h, *head, len(self._days), L.p_i32(self._kind), L.p_i32(self._idx), L.p_f64(stat),
                   L.p_f64(post), L.p_i32(self._delta), NEGVAL, *tail)

    def _from_fields(self, name, source, *tail):
        '''ps_<x>_<name>_<kind> over the last apply of a fields source'''
        self._call(name + '_' + source.fields_kind, source._h, *tail)

    def _read(self, name, source, *tail):
        '''ps_<x>_<name> over `source`, or over the model's days where there is none'''
        if source is None:
            self._from_model(name, *tail)
        else:
            self._from_fields(name, source, *tail)


class _Accumulator(_Handle):
    '''a handle that sums members of integer weight: ps_<x>_info starts with the total weight and the members'''

    def reset(self):
        self._call('reset')

    @property
    def total_weight(self):
        return self._info()[0]

    @property
    def members(self):
        return self._info()[1]

    def _add(self, weight):
        '''the add that takes the weight and nothing else'''
        w = self._weight(weight)
        self._read('add', self._proj, w)


class _FieldSource(_Handle):
    '''a handle whose apply leaves `nout` fields on the device, those of `live` carrying weight, which the accumulators
    read through their for_projection: a projection, a release plan, or fields computed per item (a trap, a window)
    from one input each -- a model day, or an output of a projection or a plan.  A class of the last kind states the
    attribute its items live under (`_items`: 'traps'), the word its messages use (`_item`: 'trap'), its item check
    (`_check`), its input limit (`_max_in`) and `_setup(pop_model, inputs, nin)`, and gives `_from_days` and `_over`
    its own constructor and for_projection to keep their argument names.'''
    _items = _item = _check = _max_in = None
    _info_n = 4            # the out-parameters of ps_<x>_info; the applies are the last
    _source = None         # the projection or plan whose outputs an apply reads; None: the model's day records

    def _from_days(self, pop_model, items, days):
        '''the constructor: an item's first entry is a model day; days: the model days the handle reads, default the
        items' own'''
        items = self._check(items)
        setattr(self, self._items, items)
        used = sorted({t[0] for t in items})
        self.in_days = used if days is None else check_in_days(days)
        if len(self.in_days) > self._max_in:
            raise ValueError('%d input days; at most %d fit one handle' % (len(self.in_days), self._max_in))
        missing = [d for d in used if d not in self.in_days]
        if missing:
            raise ValueError('%s days %r are not among the days %r' % (self._item, missing, self.in_days))
        self._source = None
        self._setup(pop_model, [self.in_days.index(t[0]) for t in items], len(self.in_days))
        self._set_days(self.in_days)

    @classmethod
    def _over(cls, source, items, labels):
        '''for_projection: an item's first entry is the output label of `source` (labels: one per output, default a
        ReleaseSites' output days, else the output indices); an output without weight is refused'''
        self = cls.__new__(cls)
        items = cls._check(items, 'output')
        setattr(self, cls._items, items)
        if labels is None:
            labels = getattr(source, 'days', None) if source.fields_kind == 'sites' else None
        labels = list(range(source.nout)) if labels is None else [int(x) for x in labels]
        if len(labels) != source.nout:
            raise ValueError('%d labels for %d outputs' % (len(labels), source.nout))
        slot = {e: i for i, e in enumerate(source.live)}        # the source's device slot of every output
        inputs = []
        for t in items:
            if t[0] not in labels or labels.index(t[0]) not in slot:
                raise ValueError('%s %r: %d is not an output that carries weight (%r)' % (cls._item, t, t[0], labels))
            inputs.append(slot[labels.index(t[0])])
        self.in_days = None
        self._source = source
        self._setup(source.pm, inputs, len(source.live))
        return self

    def apply(self):
        '''The fields of the last evaluation of the model (enqueued on the solver's stream), or of the source's last
        apply (on the handle's stream); no host synchronisation; the outputs of the previous apply are
        overwritten.'''
        self._read('apply', self._source)

    @property
    def applies(self):
        '''the applies so far; of a release plan the complete passes over its groups'''
        n = C.c_int64()
        self._call('info', *[None] * (self._info_n - 1), C.byref(n))
        return n.value

    def field(self, e):
        '''[N, N] float64: output e of the last apply; zeros for an output without weight, which is kept off the
        device'''
        e = self._e(e)
        if e not in self.live:
            return np.zeros((self.N, self.N), dtype=np.float64)
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('fetch', self.live.index(e), L.p_f64(out))
        return out

    def gather(self, rows, cols):
        '''[nout, n] float64: every output of the last apply at the cells (rows[k], cols[k])'''
        rows, cols = L.i32(np.asarray(rows).ravel()), L.i32(np.asarray(cols).ravel())
        if rows.size != cols.size:
            raise ValueError('%d rows and %d columns' % (rows.size, cols.size))
        out = np.zeros((self.nout, rows.size), dtype=np.float64)
        got = out if len(self.live) == self.nout else np.zeros((len(self.live), rows.size), dtype=np.float64)
        self._call('gather', rows.size, L.p_i32(rows), L.p_i32(cols), L.p_f64(got))
        if got is not out:
            out[self.live] = got
        return out

    def profile(self, enable=None):
        '''HIP-event time of the apply launches: (total ms, launches) per timed pass; enable switches it'''
        return self._profile(enable)

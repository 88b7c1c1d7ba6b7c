"""Posterior predictive spread from MCMC chains (no reference counterpart: CompareToData.assess_fit
and Plot_Result show one run at a point estimate).

`SpreadSummary` accumulates, on the device, the per-cell weighted mean, variance and threshold
exceedance of the daily populations of many model evaluations (ps_summary_*, csrc/ps_summary.hip):
the value added for a cell is exactly what `PopModel.population(day)` holds there, 0 where it holds
nothing.  `posterior_predictive` feeds it from `mcmc.Sampler.save` chains -- one evaluation per run of
identical model parameters, weighted by the run's length -- and, given the site's observations,
draws replicated observations from the reference's Poisson model (Bayes_Run.py:344-433).
`SpreadHistogram` keeps, on the device, the per-cell weighted distribution of the same values on fixed
bin edges (ps_hist_*, csrc/ps_hist.hip): quantile maps with their exact brackets, and exceedance at any
bin edge chosen after the run.  `ArrivalMaps` keeps, on the device, per threshold and cell the weighted
distribution of the first listed day on which a member's value reaches the threshold, and per member the
number of cells reached by each day (ps_arrival_*, csrc/ps_arrival.hip): arrival probabilities and
arrival-day quantile maps, and the posterior of the reached area.  `Projection` applies, on the device, a
weight matrix along the time axis of one member's daily fields (ps_project_*, csrc/ps_project.hip): the
emergence the field data measure (`emergence_weights`, the matrix of Bayes_funcs.popdensity_to_emergence) and
the cumulative exposure (`exposure_weights`) as maps, which `SpreadSummary.for_projection` and
`SpreadHistogram.for_projection` accumulate per member -- the spread of a sum over days cannot be rebuilt
from the per-day moments.  `ReleaseSites` superposes, on the device, the translated fields of several release
sites and of releases on later days (ps_sites_*, csrc/ps_sites.hip) into the field of a whole release plan,
which the same accumulators and `ArrivalMaps.for_projection` take per member -- neither can the spread, the
quantiles, the arrival day or the reached area of a sum over sites be rebuilt from the per-site maps.
`SensitivityMaps` keeps, on the device, per cell the weighted co-moments between the same values and the model
parameters of the member behind them (ps_sens_*, csrc/ps_sens.hip; `ParamMoments` is the parameters' side on the
host): which parameter the spread at a cell comes from, as correlation maps, the share of the variance a linear
dependence on the parameters explains, and the dominant parameter -- a chain stores no fields, so this
covariance cannot be formed after the run.
`DependenceMaps` keeps, on the device, per cell the sums of the same values over the bins of each model parameter
(ps_depend_*, csrc/ps_depend.hip): the correlation ratio eta^2 of every cell on every parameter, which also sees a
dependence that is not linear -- the ring around the plume where the density first rises and then falls with the
diffusion scale, and the correlation is nearly 0.
`MonteCarloError` keeps, on the device, one sequence of members -- a chain, or half of one -- as batch means of
exactly b rows of weight (ps_mcerr_*, csrc/ps_mcerr.hip): the Monte Carlo standard error of the posterior mean and
of the exceedance probabilities, the effective sample size and, over several sequences, the split R-hat
(`split_rhat`) per cell -- they need the order of the chain at every cell, which no saved map keeps.
`PeakMaps` keeps, on the device, per member the peak of every cell's curve over the listed days and, over the
members, the weighted counts of the day of the peak and of the number of days at or above each threshold
(ps_peak_*, csrc/ps_peak.hip): the peak field feeds `SpreadSummary.for_projection` / `SpreadHistogram.for_projection`
(E[max], its spread and quantiles), the counts give peak-day and duration probabilities, quantile maps and the
mean duration -- max over days is not linear, so none of them can be rebuilt from the per-day maps.
`ExcursionMaps` keeps, on the device, per threshold and day the weighted exceedance counts and per member the bit
mask of the cells at or above the threshold (ps_excur_*, csrc/ps_excur.hip): the joint excursion sets "surely
reached" / "surely not reached" and the credible band of the contour between them (Bolin & Lindgren 2015) --
every other map is marginal in space and cannot say with which probability all cells of a region exceed at once.
`CatchFields` turns, on the device, one member's field into the probability that a trap of a given effort catches at
least n wasps at every cell (ps_catch_*, csrc/ps_catch.hip), under the Poisson model of the package's own likelihood;
`SpreadSummary.for_projection`, `MonteCarloError.for_projection` and `ReweightedSummary.for_projection` accumulate it
per member (`CatchPosterior`) -- the transform is not linear in the density, so no saved map gives it.
`InformationFields` turns one member's field into the whole class distribution of a described trap's count and its
entropy (ps_gain_*, csrc/ps_gain.hip); from the accumulated means the device forms the mutual information between the
count and the identity of the member (`InformationPosterior`): where a reading would change what we believe.
`RangeMaps` keeps, on the device, per mass fraction and day the weighted count of the members whose own
highest-density region holding that share of their wasps contains the cell, and per member the region's level, cell
count and integer mass (ps_range_*, csrc/ps_range.hip): the 50 % core and the 95 % range as probability maps and the
posterior of their area -- the level is each member's own, so no map cut at an absolute density gives them.
`PatchMaps` labels, on the device, the connected components of each member's set {v >= t} per threshold and day
(ps_patch_*, csrc/ps_patch.hip) and keeps the weighted count of the members whose main patch, or another patch, holds
the cell, and per member the number of patches and their sizes: is the reached area one front or separate foci?
`PathwayMaps` follows those patches through a member's days in order (ps_pathway_*, csrc/ps_pathway.hip) and keeps
the weighted count of the members that reached the cell by the front that grew from the release, as a founding cell
of a detached focus, or by the growth of such a focus, and per member and day the cells so classed and the foci founded.
`MemberOverlap` forms, on the device, the table of pairwise intersections of the members' reached sets from the masks
of an `ExcursionMaps`, and the count plane of any selection of members (ps_overlap_*, csrc/ps_overlap.hip);
`RepresentativeMembers` reads from it, in integers on the host, the inclusion depth of every member, the deepest
member, the central band and k-medoids scenarios -- which single outcome is typical, which no summary map can say.
`ReweightedExcursion` (`ExcursionMaps.reweighted`) gives, from the same masks and one log-weight per member, the
excursion functions under new findings (ps_wexcur_*, csrc/ps_wexcur.hip), for a scenario chosen after the run.
`NeighbourhoodFields` turns, on the device, one member's field into its largest value within a disc of each cell
(ps_nbhd_*, csrc/ps_nbhd.hip); the existing accumulators take it per member (`NeighbourhoodPosterior`): the
probability of at least t wasps somewhere within r metres, which no per-cell map gives.
`ProximityFields` turns, on the device, one member's field into the exact Euclidean distance from each cell to the
member's own ground with at least t wasps, or the depth inside it (ps_prox_*, csrc/ps_prox.hip); the existing
accumulators take it per member (`ProximityPosterior`): the mean, spread and quantiles of that distance and the
probability of such ground within any radius, which no map for one radius gives.
`OriginMaps` runs the other way (ps_origin_*, csrc/ps_origin.hip): given findings -- probes as `check_probes` takes
them -- the likelihood of every candidate origin cell at once, per member on the device, for a ladder of founding
numbers and release days; the posterior of the origin with the parameter uncertainty integrated out, and the
members' own evidence as row log-weights for `reweight=`.  Inference about the past: it recommends nothing.  With
`known=` the releases that are facts lie in the background of every finding, and `second_source()` says whether the
findings need a second source or the known releases explain them.
`wind_sequences` resamples the days of the wind record by a circular moving-block bootstrap and `posterior_predictive(
wind=...)` evaluates every run under each sequence, over one batch of day kernels per run (`PopModel.build_pool`,
`run_sequence`); `WeatherShare` keeps, on the device, the members in groups -- one parameter vector under several
sequences -- and splits every cell's variance into the part over the wind and the parameters' own (ps_nested_*,
csrc/ps_nested.hip): the one axis of uncertainty that no other map shows.
"""
import ctypes as C
import json
import os
import threading
import time
import types

import numpy as np

from . import Bayes_funcs as BF
from . import _lib as L
from . import mcmc
from ._handle import (MAX_PROJECT_IN, NEGVAL, _Accumulator, _FieldSource, _Handle, _check_evaluated, _day_scales,
                      _day_slots, check_in_days)

DEFAULT_BINS = (1e-8, 1e6, 16)   # NEGVAL .. above any r_number, 16 bins per decade: 225 edges
MAX_EDGES = 1024
MAX_ARRIVAL_SLOTS = 32     # ps_arrival: the day slots of one launch's descriptors
MAX_ARRIVAL_THRESHOLDS = 4
MAX_PROJECT_OUT = 32
MAX_SITES = 32             # ps_sites: the sites of one plan, its release days (groups) and its outputs
MAX_SITE_GROUPS = 8
MAX_SITE_OUT = 32


def _model_days(pop_model, days):
    '''the model days an accumulator keeps: `days`, default all of the model's'''
    days = list(range(len(pop_model.days)) if days is None else days)
    if not days or min(days) < 0:
        raise ValueError('days must be a non-empty list of model days >= 0')
    return days


class SpreadSummary(_Accumulator):
    '''Weighted per-cell moments of `pop_model`'s days over the members added.  days: model days
    (0 = release day) to keep, default all; thresholds: up to 4 population densities whose
    exceedance probability is kept.'''
    _prefix, _noun = 'ps_summary', 'summary'

    def __init__(self, pop_model, days=None, thresholds=()):
        self._setup(pop_model, _model_days(pop_model, days), thresholds, None)

    @classmethod
    def for_projection(cls, projection, thresholds=()):
        '''A summary of the outputs of `projection` (a Projection or a ReleaseSites), one slot per output: `add(weight)` accumulates the outputs of
        the projection's last `apply()`, and the accessors take the output index where the day-based summary
        takes a day.'''
        self = cls.__new__(cls)
        self._setup(projection.pm, list(range(projection.nout)), thresholds, projection)
        return self

    def _setup(self, pop_model, days, thresholds, projection):
        self.thresholds = [float(t) for t in thresholds]
        self._attach(pop_model)
        # slot of every day; of a projection the outputs that carry weight (the others are zero throughout)
        self._set_source(projection, days, projection and projection.live)
        thr = L.f64(self.thresholds if self.thresholds else [0.0])
        self._create(len(self._slot), len(self.thresholds), L.p_f64(thr))

    def add(self, weight=1):
        '''Accumulate the last evaluation of the model with integer weight >= 1 (enqueued on the
        solver's stream; no host synchronisation).  On a projection: its last apply, on the summary's stream.'''
        self._add(weight)

    def merge(self, other):
        '''self += other (same device, domain, days and thresholds)'''
        if list(other.days) != self.days or other._slot != self._slot:
            raise ValueError('summaries over different days')
        self._call('merge', other._h)

    def _fetch(self, day, what):
        slot = self._slot_of(day)
        if slot is None:                                          # an output without weight
            return np.zeros((self.N, self.N), dtype=np.float64)
        return self.fetch_slot(slot, what)

    def fetch_slot(self, slot, what):
        '''raw access by slot index (0 mean, 1 variance, 2 + k exceedance)'''
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
        '''P(population >= thresholds[k]) per cell'''
        if not 0 <= k < len(self.thresholds):
            raise ValueError('threshold %r of %d' % (k, len(self.thresholds)))
        return self._fetch(day, 2 + k)

    def profile(self, enable=None):
        '''HIP-event time of the accumulate launches: (total ms, launches); enable switches it'''
        return self._profile(enable)



def bin_edges(bins=DEFAULT_BINS, edges=None):
    '''The histogram's edge table e_0 < ... < e_B (float64, 2..1024 edges, every edge finite and > 0).
    edges: an explicit table; else bins = (lo, hi, per_decade):
    B = int(round(per_decade * log10(hi / lo))), edges = lo * 10 ** (arange(B + 1) / per_decade).'''
    if edges is None:
        try:
            lo, hi, per = bins
        except (TypeError, ValueError):
            raise ValueError('bins must be (lo, hi, per_decade), got %r' % (bins,))
        if not (np.isfinite(lo) and lo > 0):
            raise ValueError('bins: lo = %r must be finite and > 0' % (lo,))
        if not (np.isfinite(hi) and hi > lo):
            raise ValueError('bins: hi = %r must be finite and > lo = %r' % (hi, lo))
        if not (np.isfinite(per) and per >= 1):
            raise ValueError('bins: per_decade = %r must be >= 1' % (per,))
        B = int(round(per * np.log10(hi / lo)))
        if B + 1 > MAX_EDGES:
            raise ValueError('bins %r give %d edges, at most %d' % (tuple(bins), B + 1, MAX_EDGES))
        edges = lo * 10.0 ** (np.arange(B + 1) / per)
    e = np.array(edges, dtype=np.float64).ravel()
    if not 2 <= e.size <= MAX_EDGES:
        raise ValueError('%d edges; a histogram needs 2..%d' % (e.size, MAX_EDGES))
    if not np.all(np.isfinite(e)) or not np.all(e > 0):
        raise ValueError('every edge must be finite and > 0')
    if not np.all(np.diff(e) > 0):
        raise ValueError('edges must be strictly increasing')
    return e


def check_levels(quantiles):
    '''quantile levels as a list of floats, each in (0, 1]; ValueError otherwise'''
    levels = [float(p) for p in quantiles]
    bad = [p for p in levels if not 0.0 < p <= 1.0]
    if bad:
        raise ValueError('quantile levels must lie in (0, 1]: %r' % (bad,))
    return levels


def quantile_tag(p):
    '''the key suffix of level p: 0.05 -> q5, 0.5 -> q50, 0.025 -> q2p5'''
    return 'q' + ('%g' % (100 * p)).replace('.', 'p')


class SpreadHistogram(_Accumulator):
    '''Weighted per-cell histograms of `pop_model`'s days over the members added, on fixed bin edges
    (`bin_edges(bins, edges)`).  days: model days to keep, default all.  The value of a cell is the one
    SpreadSummary adds; bin b = searchsorted(edges, v, side='right'), b = 0 .. B + 1.'''
    _prefix, _noun, _prof_pairs = 'ps_hist', 'histogram', 2
    _info_types = (C.c_double, C.c_int64, C.c_int32)

    def __init__(self, pop_model, days=None, bins=DEFAULT_BINS, edges=None):
        self._setup(pop_model, _model_days(pop_model, days), bins, edges, None)

    @classmethod
    def for_projection(cls, projection, bins=DEFAULT_BINS, edges=None):
        '''Histograms of the outputs of `projection` (a Projection or a ReleaseSites), one slot per output: `add(weight)` accumulates the outputs
        of the projection's last `apply()`, and the accessors take the output index where the day-based
        histogram takes a day.'''
        self = cls.__new__(cls)
        self._setup(projection.pm, list(range(projection.nout)), bins, edges, projection)
        return self

    def _setup(self, pop_model, days, bins, edges, projection):
        self._edges = bin_edges(bins, edges)
        self.bins = None if edges is not None else tuple(float(b) for b in bins)
        self._attach(pop_model)
        # slot of every day; of a projection the outputs that carry weight (the others are zero throughout)
        self._set_source(projection, days, projection and projection.live)
        self.nbytes = len(self._slot) * self.pitch * (self._edges.size + 1) * 4   # count planes + range words
        self._create(len(self._slot), self._edges.size, L.p_f64(self._edges))

    @property
    def edges(self):
        return self._edges.copy()

    def add(self, weight=1):
        '''Accumulate the last evaluation of the model with integer weight >= 1 (enqueued on the
        solver's stream; no host synchronisation).'''
        self._add(weight)                # of a projection: its last apply, on the histogram's stream

    def merge(self, other):
        '''self += other (same device, domain, days and edges)'''
        if list(other.days) != self.days or other._slot != self._slot:
            raise ValueError('histograms over different days')
        self._call('merge', other._h)

    def counts(self, day):
        '''[B + 2, N, N] uint32: the weight of every bin per cell, bin 0 = W - the others'''
        s = self._slot_of(day)
        out = np.empty((self._edges.size + 1, self.N, self.N), dtype=np.uint32)
        if s is None:
            out[:] = 0
            out[0] = np.uint32(self.total_weight)
            return out
        for b in range(out.shape[0]):
            self._call('fetch_counts', s, b, out[b].ctypes.data_as(C.POINTER(C.c_uint32)))
        return out

    def _quantile(self, day, p, value, lower, upper):
        s = self._slot_of(day)
        if not 0.0 < float(p) <= 1.0:
            raise ValueError('quantile level %r is not in (0, 1]' % (p,))
        if s is None:                    # every member's value is 0: bin 0 = [0, e_0)
            for a, v in ((value, 0.0), (lower, 0.0), (upper, self._edges[0])):
                if a is not None:
                    a[:] = v
            return
        ptr = [None if a is None else L.p_f64(a) for a in (value, lower, upper)]
        self._call('quantile', s, float(p), *ptr)

    def quantile(self, day, p):
        '''N x N point map of the weighted lower quantile at level p (log-interpolated inside its bin)'''
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._quantile(day, p, out, None, None)
        return out

    def quantile_bounds(self, day, p):
        '''(lower, upper): the bin [lower, upper) that holds the exact weighted quantile at level p'''
        lo = np.empty((self.N, self.N), dtype=np.float64)
        hi = np.empty((self.N, self.N), dtype=np.float64)
        self._quantile(day, p, None, lo, hi)
        return lo, hi

    def exceedance(self, day, t):
        '''P(population >= t) per cell, exact; t must be one of the edges (ValueError otherwise)'''
        k = np.flatnonzero(self._edges == float(t))
        if k.size != 1:
            raise ValueError('threshold %r is not a bin edge; exceedance is exact only at the edges' % (t,))
        out = np.empty((self.N, self.N), dtype=np.float64)
        s = self._slot_of(day)
        if s is None:
            out[:] = 0.0
            return out
        self._call('exceed', s, int(k[0]), L.p_f64(out))
        return out

    def profile(self, enable=None):
        '''HIP-event time of the add and quantile launches: (add ms, adds, quantile ms, quantile
        launches); enable switches it'''
        return self._profile(enable)



def check_arrival_thresholds(thresholds):
    '''arrival thresholds as a list of floats: 1..4 of them, each finite and > 0, strictly increasing;
    ValueError otherwise'''
    try:
        thr = [float(t) for t in thresholds]
    except (TypeError, ValueError):
        raise ValueError('arrival thresholds must be numbers, got %r' % (thresholds,))
    if not 1 <= len(thr) <= MAX_ARRIVAL_THRESHOLDS:
        raise ValueError('%d arrival thresholds; 1..%d are kept' % (len(thr), MAX_ARRIVAL_THRESHOLDS))
    if not all(np.isfinite(t) and t > 0 for t in thr):
        raise ValueError('every arrival threshold must be finite and > 0: %r' % (thr,))
    if any(b <= a for a, b in zip(thr, thr[1:])):
        raise ValueError('arrival thresholds must be strictly increasing: %r' % (thr,))
    return thr


def check_arrival_days(days):
    '''arrival day slots as a list of ints: 1..32 model days >= 0, strictly increasing; ValueError otherwise'''
    d = [int(x) for x in days]
    if not 1 <= len(d) <= MAX_ARRIVAL_SLOTS:
        raise ValueError('%d arrival days; 1..%d fit one launch' % (len(d), MAX_ARRIVAL_SLOTS))
    if d[0] < 0 or any(b <= a for a, b in zip(d, d[1:])):
        raise ValueError('arrival days must be model days >= 0, strictly increasing: %r' % (d,))
    return d


def weighted_lower_quantile(values, weights, p):
    '''min{a : sum of w_m over a_m <= a >= p W}, compared as (double)(integer weight) >= p * (double)W; real
    (floating-point) weights are summed as they are, in the order of the sorted values, and W is the last entry of
    that running sum -- the sum taken in another order can differ from it by an ulp, and at p = 1 no entry would
    reach it'''
    v = np.asarray(values)
    w = np.asarray(weights)
    order = np.argsort(v, kind='stable')
    if w.dtype.kind == 'f':
        cw = np.cumsum(w[order])
        j = int(np.argmax(cw >= float(p) * cw[-1]))
        return v[order][j]
    w = w.astype(np.int64)
    cw = np.cumsum(w[order])
    j = int(np.argmax(cw.astype(np.float64) >= float(p) * float(w.sum())))
    return v[order][j]


def _output_labels(projection):
    '''the labels of the outputs of a fields source that carry weight, in ascending order: a plan's output days,
    else the output indices; the one output of a PeakMaps, whose `days` are those it peaks over, is 0'''
    if projection.fields_kind == 'peak':
        labels = [0]
    else:
        labels = list(getattr(projection, 'days', range(projection.nout)))
    return [labels[e] for e in projection.live]


class ArrivalMaps(_Accumulator):
    '''When `pop_model`'s members reach each cell: for thresholds t_0 < ... < t_{K-1} (1..4, finite, > 0)
    and the model days `days` (strictly increasing, at most 32, default all), per threshold and cell the
    weighted distribution of the arrival day a_k = the first listed day whose value (the one SpreadSummary
    adds) is >= t_k, "never" if none; and per member the cells reached by each day.  Counts are integers:
    the order of adds and merges changes no bit.'''
    _prefix, _noun, _prof_pairs = 'ps_arrival', 'arrival maps', 2

    def __init__(self, pop_model, thresholds, days=None):
        self.thresholds = check_arrival_thresholds(thresholds)
        self._setup(pop_model, None, check_arrival_days(range(len(pop_model.days)) if days is None else days))

    @classmethod
    def for_projection(cls, projection, thresholds):
        '''Arrival maps of the outputs of `projection` (a ReleaseSites or a Projection), the slots its outputs
        that carry weight in ascending order: `add(weight)` accumulates the outputs of its last `apply()`.
        `days` holds the output labels -- the plan's output days, or the projection's output indices -- and
        `reached_area` is the coverage curve of the plan.'''
        self = cls.__new__(cls)
        self.thresholds = check_arrival_thresholds(thresholds)
        self._setup(projection.pm, projection, check_arrival_days(_output_labels(projection)))
        return self

    def _setup(self, pop_model, projection, days):
        self._attach(pop_model)
        self._set_source(projection, days)
        self.nbytes = len(self.thresholds) * len(self.days) * self.pitch * 4     # the count planes
        self._create(len(self.days), len(self.thresholds), L.p_f64(L.f64(self.thresholds)))

    def add(self, weight=1):
        '''Accumulate the last evaluation of the model with integer weight >= 1 (enqueued on the
        solver's stream; no host synchronisation).  On a projection or a plan: its last apply, on the
        handle's stream.'''
        self._add(weight)

    def merge(self, other):
        '''self += other (same device, domain, days and thresholds); other's members follow self's'''
        if list(other.days) != self.days:
            raise ValueError('arrival maps over different days')
        self._call('merge', other._h)

    def counts(self, k, day):
        '''[N, N] uint32: the weight of the members whose arrival day at t_k is `day`; day=None: never'''
        s = len(self.days) if day is None else self._slot_of(day)
        out = np.empty((self.N, self.N), dtype=np.uint32)
        self._call('fetch_counts', self._k(k), s, out.ctypes.data_as(C.POINTER(C.c_uint32)))
        return out

    def prob_by(self, k, day):
        '''[N, N] float64: P(arrived at t_k by `day`) = C_k / W, C_k the weight of the arrivals up to `day`'''
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('prob', self._k(k), self._slot_of(day), L.p_f64(out))
        return out

    def quantile(self, k, p):
        '''[N, N] int32 map of model days: the first day whose C_k reaches p W ((double)C >= p * (double)W),
        -1 where even the last day falls short (not within the window)'''
        if not 0.0 < float(p) <= 1.0:
            raise ValueError('quantile level %r is not in (0, 1]' % (p,))
        slot = np.empty((self.N, self.N), dtype=np.int32)
        self._call('quantile', self._k(k), float(p), L.p_i32(slot))
        day = np.append(np.asarray(self.days, dtype=np.int32), np.int32(-1))
        return day[slot]          # slot -1 picks the appended -1

    def _reached(self):
        m = self.members
        cells = np.empty((m, len(self.thresholds), len(self.days)), dtype=np.uint32)
        w = np.empty(m, dtype=np.uint32)
        u32 = C.POINTER(C.c_uint32)
        self._call('fetch_reached', 0, m, cells.ctypes.data_as(u32), w.ctypes.data_as(u32))
        return cells, w

    def reached(self, k):
        '''(cells [members, days] int64, weights [members] int64): per member in add order the number of cells
        that reached t_k by each day'''
        k = self._k(k)
        cells, w = self._reached()
        return cells[:, k, :].astype(np.int64), w.astype(np.int64)

    def reached_area(self, k, levels=(0.05, 0.5, 0.95)):
        '''Per day the posterior of the area that reached t_k: [{'day', 'mean', 'quantiles', 'radius_mean',
        'radius_quantiles'}, ...].  Areas in m^2 (cells x (rad_dist / rad_res)^2): the weighted mean and the
        weighted lower quantiles min{a : sum of w_m over a_m <= a >= p W} at `levels`; radii sqrt(A / pi) in m.'''
        levels = check_levels(levels)
        cells, w = self.reached(k)
        W = int(w.sum())
        if W == 0:
            raise ValueError('nothing accumulated')
        out = []
        for s, d in enumerate(self.days):
            n = cells[:, s]
            mean = float(int((n * w).sum())) / float(W) * self.cell_area
            q = [float(weighted_lower_quantile(n, w, p)) * self.cell_area for p in levels]
            out.append({'day': d, 'mean': mean, 'quantiles': q, 'radius_mean': float(np.sqrt(mean / np.pi)),
                        'radius_quantiles': [float(np.sqrt(a / np.pi)) for a in q]})
        return out

    def profile(self, enable=None):
        '''HIP-event time of the add and map launches: (add ms, adds, map ms, map launches); enable
        switches it'''
        return self._profile(enable)



def check_peak_thresholds(thresholds):
    '''the duration thresholds of peak maps as a list of floats: 0..4 of them by the rules of
    check_arrival_thresholds; an empty list keeps the peak value and the peak day only'''
    try:
        thr = list(thresholds)
    except TypeError:
        raise ValueError('peak thresholds must be a list of numbers, got %r' % (thresholds,))
    return check_arrival_thresholds(thr) if thr else []


def check_peak(peak):
    '''the peak= argument of posterior_predictive -> (thresholds, levels): a list of thresholds, or
    dict(thresholds=[...], levels=(0.05, 0.5, 0.95)); ValueError otherwise'''
    levels = (0.05, 0.5, 0.95)
    if isinstance(peak, dict):
        unknown = set(peak) - {'thresholds', 'levels'}
        if unknown:
            raise ValueError('peak: unknown keys %r' % (sorted(unknown),))
        levels = peak.get('levels', levels)
        peak = peak.get('thresholds', ())
    return check_peak_thresholds(peak), check_levels(levels)


class PeakMaps(_Accumulator):
    '''The shape of each cell's curve over the listed days, per member and then over the members: the peak value
    m = max(+0.0, max_d v_d) (v_d the value SpreadSummary adds for day d), the peak day -- the first listed day
    that attains m, none where m == 0 -- and per threshold t_k (0..4, finite, > 0, strictly increasing) the number
    of listed days with v_d >= t_k.  On the device: the last member's peak field, the weighted counts of the peak
    day and of every duration.  The peak field is a fields source like a Projection's outputs (one output):
    SpreadSummary.for_projection(peak, thresholds) and SpreadHistogram.for_projection(peak, ...) accumulate it, so
    E[max], its spread, P(peak >= t) and its quantiles come from the existing accumulators.  A duration counts
    listed days: it is a number of days only where they are consecutive model days (`consecutive`).  Counts are
    integers: the order of adds and merges changes no bit.'''
    _prefix, _noun, _prof_pairs = 'ps_peak', 'peak maps', 2
    fields_kind = 'peak'         # the accumulators' entry points for the peak field: ps_*_add_peak
    nout = 1
    live = [0]

    def __init__(self, pop_model, thresholds=(), days=None):
        self.thresholds = check_peak_thresholds(thresholds)
        self._setup(pop_model, None, check_arrival_days(range(len(pop_model.days)) if days is None else days))

    @classmethod
    def for_projection(cls, projection, thresholds=()):
        '''Peak maps of the outputs of `projection` (a ReleaseSites or a Projection), the slots its outputs that
        carry weight in ascending order: `add(weight)` accumulates the outputs of its last `apply()`.  `days`
        holds the output labels -- the plan's output days, or the projection's output indices.'''
        self = cls.__new__(cls)
        self.thresholds = check_peak_thresholds(thresholds)
        self._setup(projection.pm, projection, check_arrival_days(_output_labels(projection)))
        return self

    def _setup(self, pop_model, projection, days):
        self._attach(pop_model)
        self._set_source(projection, days)
        self.consecutive = all(b == a + 1 for a, b in zip(self.days, self.days[1:]))
        self.nbytes = (1 + len(self.thresholds)) * len(self.days) * self.pitch * 4 + 2 * self.pitch * 8   # counts + peak field + map scratch
        thr = L.f64(self.thresholds if self.thresholds else [0.0])
        self._create(len(self.days), len(self.thresholds), L.p_f64(thr))

    def add(self, weight=1):
        '''Accumulate the last evaluation of the model with integer weight >= 1 (enqueued on the
        solver's stream; no host synchronisation).  On a projection or a plan: its last apply, on the
        handle's stream.'''
        self._add(weight)

    def merge(self, other):
        '''self += other (same device, domain, days and thresholds); the peak field stays self's'''
        if list(other.days) != self.days:
            raise ValueError('peak maps over different days')
        self._call('merge', other._h)

    def _n(self, n, lo):
        if not lo <= int(n) <= len(self.days):
            raise ValueError('duration %r is not in %d..%d' % (n, lo, len(self.days)))
        return int(n)

    def field(self):
        '''[N, N] float64: the peak field of the last member added'''
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('fetch_field', L.p_f64(out))
        return out

    def day_counts(self, day):
        '''[N, N] uint32: the weight of the members whose peak falls on `day`'''
        out = np.empty((self.N, self.N), dtype=np.uint32)
        self._call('fetch_day_counts', self._slot_of(day), out.ctypes.data_as(C.POINTER(C.c_uint32)))
        return out

    def day_prob(self, day):
        '''[N, N] float64: P(peaked by `day`) = C / W, C the weight of the peaks up to `day`'''
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('day_prob', self._slot_of(day), L.p_f64(out))
        return out

    def day_quantile(self, p):
        '''[N, N] int32 map of model days: the first day whose C reaches p W ((double)C >= p * (double)W), -1
        where even the last day falls short (too few members ever hold anything there)'''
        if not 0.0 < float(p) <= 1.0:
            raise ValueError('quantile level %r is not in (0, 1]' % (p,))
        slot = np.empty((self.N, self.N), dtype=np.int32)
        self._call('day_quantile', float(p), L.p_i32(slot))
        day = np.append(np.asarray(self.days, dtype=np.int32), np.int32(-1))
        return day[slot]          # slot -1 picks the appended -1

    def duration_counts(self, k, n):
        '''[N, N] uint32: the weight of the members with exactly n listed days at or above t_k, n in 0..len(days)'''
        out = np.empty((self.N, self.N), dtype=np.uint32)
        self._call('fetch_duration_counts', self._k(k), self._n(n, 0), out.ctypes.data_as(C.POINTER(C.c_uint32)))
        return out

    def duration_prob(self, k, n):
        '''[N, N] float64: P(at least n listed days at or above t_k), n in 1..len(days)'''
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('duration_prob', self._k(k), self._n(n, 1), L.p_f64(out))
        return out

    def duration_quantile(self, k, p):
        '''[N, N] int32: the smallest n in 0..len(days) whose cumulative weight reaches p W (same rule)'''
        if not 0.0 < float(p) <= 1.0:
            raise ValueError('quantile level %r is not in (0, 1]' % (p,))
        out = np.empty((self.N, self.N), dtype=np.int32)
        self._call('duration_quantile', self._k(k), float(p), L.p_i32(out))
        return out

    def duration_mean(self, k):
        '''[N, N] float64: the posterior mean of the listed days at or above t_k'''
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('duration_mean', self._k(k), L.p_f64(out))
        return out

    def profile(self, enable=None):
        '''HIP-event time of the add and map launches: (add ms, adds, map ms, map launches); enable
        switches it'''
        return self._profile(enable)



class PeakPosterior():
    '''The peak maps of one source as posterior_predictive fills and returns them: `maps` (PeakMaps), `summary`
    (SpreadSummary.for_projection of the peak field: E[max], its spread and P(peak >= t), output index 0),
    `histogram` (SpreadHistogram.for_projection of it, None without quantile levels) and `levels` (the levels of
    the saved peak-day and duration quantile maps).  `add` feeds the three in that order.'''

    def __init__(self, maps, thresholds=(), levels=(0.05, 0.5, 0.95), bins=None, edges=None):
        self.maps = maps
        self.levels = list(levels)
        self.summary = self.histogram = None
        try:
            self.summary = SpreadSummary.for_projection(maps, thresholds)
            if bins is not None or edges is not None:
                self.histogram = SpreadHistogram.for_projection(maps, bins, edges)
        except BaseException:
            self.close()
            raise

    def add(self, weight=1):
        self.maps.add(weight)
        self.summary.add(weight)
        if self.histogram is not None:
            self.histogram.add(weight)

    def merge(self, other):
        self.maps.merge(other.maps)
        self.summary.merge(other.summary)
        if self.histogram is not None:
            self.histogram.merge(other.histogram)

    def close(self):
        for a in (self.histogram, self.summary, self.maps):
            if a is not None:
                a.close()


def check_excursion_levels(levels):
    '''credible levels of the excursion regions as a list of floats, each in (0.5, 1] -- above 0.5 "surely
    reached" and "surely not reached" cannot hold at one cell; ValueError otherwise'''
    try:
        lv = [float(p) for p in levels]
    except (TypeError, ValueError):
        raise ValueError('excursion levels must be numbers, got %r' % (levels,))
    bad = [p for p in lv if not 0.5 < p <= 1.0]
    if bad or not lv:
        raise ValueError('excursion levels must lie in (0.5, 1], at least one: %r' % (bad or lv,))
    return lv


def check_excursion(excursion):
    '''the excursion= argument of posterior_predictive -> (thresholds, levels): a list of thresholds (1..4, by the
    rules of check_arrival_thresholds), or dict(thresholds=[...], levels=(0.9, 0.95)) with every level in
    (0.5, 1]; ValueError otherwise'''
    levels = (0.9, 0.95)
    if isinstance(excursion, dict):
        unknown = set(excursion) - {'thresholds', 'levels'}
        if unknown:
            raise ValueError('excursion: unknown keys %r' % (sorted(unknown),))
        if 'thresholds' not in excursion:
            raise ValueError('excursion: thresholds are needed')
        levels = excursion.get('levels', levels)
        excursion = excursion['thresholds']
    try:
        thr = list(excursion)
    except TypeError:
        raise ValueError('excursion thresholds must be a list of numbers, got %r' % (excursion,))
    return check_arrival_thresholds(thr), check_excursion_levels(levels)


def level_tag(p):
    '''the key suffix of credible level p: 0.95 -> l95, 0.975 -> l97p5'''
    return 'l' + ('%g' % (100 * p)).replace('.', 'p')


class ExcursionMaps(_Accumulator):
    '''Joint statements about where `pop_model`'s members hold >= t_k on a listed day (Bolin & Lindgren 2015, on
    the level sets of the marginal probability): thresholds t_0 < ... < t_{K-1} (1..4, finite, > 0), model days
    `days` (strictly increasing, at most 32, default all).  On the device per (k, day) the weighted count C of the
    members at or above t_k (W x SpreadSummary.exceedance) and per member the bit mask of the cells where it is.
    From them `above` F+ -- {F+ >= level} is the largest level set of C on which all cells hold >= t_k at the same
    time with probability >= level, "surely reached" -- its mirror image `below` F- ("surely not reached") and
    `contour` Fc, whose {Fc < level} is the credible band of the t_k-contour, the front.  Counts and bounds are
    integers: the order of adds and merges changes no bit of a map.'''
    _prefix, _noun = 'ps_excur', 'excursion maps'
    _info_types = (C.c_double, C.c_int64, C.c_int64, C.c_int64)      # weight, members, capacity, bytes

    ABOVE, BELOW, CONTOUR = 0, 1, 2

    def __init__(self, pop_model, thresholds, days=None):
        self.thresholds = check_arrival_thresholds(thresholds)
        self._setup(pop_model, None, check_arrival_days(range(len(pop_model.days)) if days is None else days))

    @classmethod
    def for_projection(cls, projection, thresholds):
        '''Excursion maps of the outputs of `projection` (a ReleaseSites, a Projection or a PeakMaps), the slots
        its outputs that carry weight in ascending order: `add(weight)` accumulates the outputs of its last
        `apply()` (the peak field of its last add).  `days` holds the output labels -- the plan's output days,
        or the output indices.'''
        self = cls.__new__(cls)
        self.thresholds = check_arrival_thresholds(thresholds)
        self._setup(projection.pm, projection, check_arrival_days(_output_labels(projection)))
        return self

    def _setup(self, pop_model, projection, days):
        self._attach(pop_model)
        self._set_source(projection, days)
        self.member_nbytes = len(self.thresholds) * len(self.days) * self.pitch // 8     # one member's masks
        self._create(len(self.days), len(self.thresholds), L.p_f64(L.f64(self.thresholds)))

    def reserve(self, n):
        '''room for n members' masks now, so that no add has to grow them'''
        self._call('reserve', int(n))

    def add(self, weight=1):
        '''Accumulate the last evaluation of the model with integer weight >= 1 (enqueued on the
        solver's stream; no host synchronisation unless the masks grow).  On a projection or a plan: its last
        apply, on the handle's stream.'''
        self._add(weight)

    def merge(self, other):
        '''self += other (same device, domain, days and thresholds); other's members follow self's'''
        if list(other.days) != self.days:
            raise ValueError('excursion maps over different days')
        self._call('merge', other._h)

    @property
    def capacity(self):
        '''the members the masks hold room for'''
        return self._info()[2]

    @property
    def nbytes(self):
        '''the device memory the handle holds now'''
        return self._info()[3]

    def counts(self, k, day):
        '''[N, N] uint32: the weight of the members at or above t_k on `day`'''
        out = np.empty((self.N, self.N), dtype=np.uint32)
        self._call('fetch_counts', self._k(k), self._slot_of(day), out.ctypes.data_as(C.POINTER(C.c_uint32)))
        return out

    def mask(self, member, k, day):
        '''[pitch / 64] uint64: the mask words of one member (in add order), bit l of word j the cell 64 j + l
        of the flattened domain, the pad bits 0'''
        out = np.empty(self.pitch // 64, dtype=np.uint64)
        self._call('fetch_mask', int(member), self._k(k), self._slot_of(day),
                                 out.ctypes.data_as(C.POINTER(C.c_uint64)))
        return out

    def bounds(self, k, day):
        '''(hi, lo, weights), each [members] uint32 in add order: hi the largest count outside the member's mask
        (0: none), lo the smallest inside it (0xffffffff: the mask is empty)'''
        m = self.members
        hi, lo, w = (np.empty(m, dtype=np.uint32) for _ in range(3))
        u32 = C.POINTER(C.c_uint32)
        self._call('fetch_bounds', self._k(k), self._slot_of(day), hi.ctypes.data_as(u32), lo.ctypes.data_as(u32),
                                   w.ctypes.data_as(u32))
        return hi, lo, w

    def _map(self, k, day, what):
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('map', self._k(k), self._slot_of(day), what, L.p_f64(out))
        return out

    def above(self, k, day):
        '''[N, N] float64 F+: the posterior weight of the members at or above t_k on all of {C >= C(c)}'''
        return self._map(k, day, self.ABOVE)

    def below(self, k, day):
        '''[N, N] float64 F-: the posterior weight of the members below t_k on all of {C <= C(c)}; 1 where no
        member holds anything'''
        return self._map(k, day, self.BELOW)

    def contour(self, k, day):
        '''[N, N] float64 Fc: the posterior weight of the members whose t_k-contour avoids the cell's level pair'''
        return self._map(k, day, self.CONTOUR)

    def region(self, k, day, level=0.95):
        '''[N, N] int8: +1 where F+ >= level (surely reached), -1 where F- >= level (surely not), else 0;
        0.5 < level <= 1'''
        level, = check_excursion_levels([level])
        return ((self.above(k, day) >= level).astype(np.int8) - (self.below(k, day) >= level).astype(np.int8))

    def areas(self, k, day, levels):
        '''[{'level', 'above', 'below', 'band'}, ...] in m^2: the cells x cell_area of {F+ >= level},
        {F- >= level} and the contour's credible band {Fc < level}'''
        levels = check_excursion_levels(levels)
        Fp, Fm, Fc = self.above(k, day), self.below(k, day), self.contour(k, day)
        return [{'level': p, 'above': float(int((Fp >= p).sum())) * self.cell_area,
                 'below': float(int((Fm >= p).sum())) * self.cell_area,
                 'band': float(int((Fc < p).sum())) * self.cell_area} for p in levels]

    def profile(self, enable=None):
        '''HIP-event time of the add, finalize and map launches: (add ms, adds, finalize ms, finalizes, map ms,
        map launches); enable switches it'''
        ms = np.zeros(3, dtype=np.float64)
        n = np.zeros(3, dtype=np.int64)
        self._call('prof', -1 if enable is None else int(bool(enable)), L.p_f64(ms), L.p_i64(n))
        return float(ms[0]), int(n[0]), float(ms[1]), int(n[1]), float(ms[2]), int(n[2])

    def reweighted(self, log_weights):
        '''The ReweightedExcursion of these maps under one log-weight per member in add order (-inf: the member
        drops out; ValueError for NaN, +inf, a wrong length or all -inf) -- OriginMaps.log_weights() per run, a
        trap's log-likelihood per member, or any scenario chosen after the chains have run.  No member is evaluated
        again.  It is closed with these maps, or by its own close().'''
        rw = ReweightedExcursion(self, log_weights)
        self._reweighted = [r for r in getattr(self, '_reweighted', []) if r._h] + [rw]
        return rw

    def close(self):
        for rw in getattr(self, '_reweighted', []):       # they read these masks: first
            rw.close()
        self._reweighted = []
        super().close()


def excursion_member_weights(log_weights, run_lengths):
    '''float64 [members]: w_m = n_m exp(l_m - max l), 0.0 at l_m = -inf -- the definition of
    ReweightedArrival.member_weights; n_m the integer weight a member was added with.  ValueError for NaN, +inf, a
    wrong length or where every log-weight is -inf.'''
    import math
    try:
        lw = [float(v) for v in np.asarray(log_weights, dtype=np.float64).ravel()]
    except (TypeError, ValueError):
        raise ValueError('log_weights must be one number per member, got %r' % (log_weights,))
    n = [int(v) for v in run_lengths]
    if len(lw) != len(n):
        raise ValueError('%d log-weights given, the excursion maps hold %d members' % (len(lw), len(n)))
    if any(math.isnan(v) or v == math.inf for v in lw):
        raise ValueError('the log-weights hold NaN or +inf')
    ref = max(lw) if lw else -math.inf
    if ref == -math.inf:
        raise ValueError('every log-weight is -inf: no member is left with weight')
    return np.array([0.0 if l == -math.inf else k * math.exp(l - ref) for l, k in zip(lw, n)], dtype=np.float64)


class ReweightedExcursion(_Handle):
    '''The excursion functions of an ExcursionMaps under one real weight per member, on the device (ps_wexcur_*,
    csrc/ps_wexcur.hip): from the members' kept masks and w_m = n_m exp(l_m - max l) (excursion_member_weights) the
    weighted count C_w, the members' bounds on it and `above`, `below`, `contour` with the meaning of ExcursionMaps',
    every map a sum over the members in add order divided once by W = sum w_m.  With equal log-weights every map
    holds the bits of the parent's; with members at -inf those of maps fed the other members only.  `weights`
    [members] float64, `total` W (summed in add order) and `ess`, Kish's (sum w)^2 / sum w^2.  The object keeps the
    plane (k, day) it formed last, so the maps of one plane cost one plane build.  It borrows the parent: after a
    further add, merge or reset on the parent every call fails with a ValueError that says so -- the weights no
    longer match the members; take a new `reweighted()`.'''
    _prefix, _noun = 'ps_wexcur', 'reweighted excursion maps'
    _info_types = (C.c_int64, C.c_int64, C.c_double)       # members of the current plane, bytes, its W

    ABOVE, BELOW, CONTOUR, PROB = 0, 1, 2, 3

    def __init__(self, excursion, log_weights):
        if not isinstance(excursion, ExcursionMaps):
            raise ValueError('excursion maps are reweighted over an ExcursionMaps, got %r' % (type(excursion).__name__,))
        self.excursion = excursion
        self._maps()
        M = excursion.members
        lw = np.asarray(log_weights, dtype=np.float64)
        if lw.ndim != 1 or lw.shape[0] != M:
            raise ValueError('%s log-weights given, the excursion maps hold %d members' % (lw.shape, M))
        self._attach(excursion.pm)
        self.thresholds, self.days = excursion.thresholds, excursion.days
        self._create(excursion._h)
        n = np.empty(M, dtype=np.uint32)
        self._call('member_weights', M, n.ctypes.data_as(C.POINTER(C.c_uint32)))
        self.run_lengths = n
        self.log_weights = lw.copy()
        try:
            self.weights = excursion_member_weights(lw, n)
        except ValueError:
            self.close()
            raise
        total = 0.0
        for w in self.weights:
            total = total + float(w)
        self.total = total
        self.ess = float(self.weights.sum()) ** 2 / float((self.weights * self.weights).sum())
        self._plane = None

    def _maps(self):
        if not self.excursion._h:
            raise ValueError('the ExcursionMaps of these reweighted excursion maps are closed')
        return self.excursion

    @property
    def nbytes(self):
        '''the device memory the handle holds now'''
        return self._info()[1]

    def _form(self, k, day):
        '''plane (k, day) as the handle's current plane'''
        E = self._maps()
        if E.members != self.weights.size:
            raise ValueError('the excursion maps hold %d members, these weights are for %d: members were added, merged '
                             'or reset since; take a new reweighted()' % (E.members, self.weights.size))
        key = (E._k(k), E._slot_of(day))
        if self._plane != key:
            self._plane = None
            self._call('plane', key[0], key[1], self.weights.size, L.p_f64(self.weights))
            self._plane = key

    def counts(self, k, day):
        '''[N, N] float64 C_w: the weight of the members at or above t_k on `day`'''
        self._form(k, day)
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('fetch_counts', L.p_f64(out))
        return out

    def bounds(self, k, day):
        '''(hi, lo), each [members] float64 in add order: hi the largest C_w outside the member's mask (0: none), lo
        the smallest inside it (+inf: the mask is empty)'''
        self._form(k, day)
        hi, lo = np.empty(self.weights.size), np.empty(self.weights.size)
        self._call('fetch_bounds', L.p_f64(hi), L.p_f64(lo))
        return hi, lo

    def _map(self, k, day, what):
        self._form(k, day)
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('map', what, L.p_f64(out))
        return out

    def prob(self, k, day):
        '''[N, N] float64: C_w / W, the reweighted probability of >= t_k at the cell'''
        return self._map(k, day, self.PROB)

    def above(self, k, day):
        '''[N, N] float64 F+ under the weights, as ExcursionMaps.above'''
        return self._map(k, day, self.ABOVE)

    def below(self, k, day):
        '''[N, N] float64 F- under the weights, as ExcursionMaps.below'''
        return self._map(k, day, self.BELOW)

    def contour(self, k, day):
        '''[N, N] float64 Fc under the weights, as ExcursionMaps.contour'''
        return self._map(k, day, self.CONTOUR)

    region = ExcursionMaps.region
    areas = ExcursionMaps.areas

    def profile(self, enable=None):
        '''HIP-event time of the count, bounds and map launches: (count ms, launches, bounds ms, launches, map ms,
        launches); enable switches it'''
        ms = np.zeros(3, dtype=np.float64)
        n = np.zeros(3, dtype=np.int64)
        self._call('prof', -1 if enable is None else int(bool(enable)), L.p_f64(ms), L.p_i64(n))
        return float(ms[0]), int(n[0]), float(ms[1]), int(n[1]), float(ms[2]), int(n[2])


MAX_CLUSTERS = 8


def _thousandths(value, name, lo, hi, open_lo=False):
    '''round(1000 * value) for a value that is a multiple of 0.001 (within 1e-9) in [lo, hi] (open_lo: (lo, hi]);
    ValueError otherwise'''
    try:
        x = float(value)
    except (TypeError, ValueError):
        raise ValueError('%s must be a number, got %r' % (name, value))
    e = int(round(1000.0 * x)) if np.isfinite(x) else 0
    if not np.isfinite(x) or abs(x - e / 1000.0) > 1e-9:
        raise ValueError('%s must be a multiple of 0.001, got %r' % (name, value))
    if not (lo < x if open_lo else lo <= x) or not x <= hi:
        raise ValueError('%s must lie in %s%g, %g], got %r' % (name, '(' if open_lo else '[', lo, hi, value))
    return e


def check_clusters(clusters):
    '''the number of scenarios as an int in 1..8; ValueError otherwise'''
    if isinstance(clusters, bool) or not isinstance(clusters, (int, np.integer)) or not 1 <= clusters <= MAX_CLUSTERS:
        raise ValueError('clusters must be an integer in 1..%d, got %r' % (MAX_CLUSTERS, clusters))
    return int(clusters)


def check_representative(arg):
    '''the representative= argument of posterior_predictive -> dict(epsilon, central, clusters, days): True for the
    defaults, or dict(epsilon=0.02, central=0.5, clusters=3, days='all') with any of the keys; epsilon a multiple of
    0.001 in [0, 0.5], central one in (0, 1], clusters in 1..8, days 'all' (the space-time plane) or a non-empty list
    of days >= 0 (one plane each); ValueError otherwise'''
    out = dict(epsilon=0.02, central=0.5, clusters=3, days='all')
    if arg is not True:
        if not isinstance(arg, dict):
            raise ValueError('representative must be True or a dict, got %r' % (arg,))
        unknown = set(arg) - set(out)
        if unknown:
            raise ValueError('representative: unknown keys %r' % (sorted(unknown),))
        out.update(arg)
    _thousandths(out['epsilon'], 'epsilon', 0.0, 0.5)
    _thousandths(out['central'], 'central', 0.0, 1.0, open_lo=True)
    out['epsilon'], out['central'] = float(out['epsilon']), float(out['central'])
    out['clusters'] = check_clusters(out['clusters'])
    if not (isinstance(out['days'], str) and out['days'] == 'all'):
        try:
            days = [int(d) for d in out['days']]
        except (TypeError, ValueError):
            raise ValueError("representative: days must be 'all' or a list of days, got %r" % (out['days'],))
        if not days or min(days) < 0 or len(set(days)) != len(days):
            raise ValueError("representative: days must be 'all' or a non-empty list of distinct days >= 0, got %r"
                             % (out['days'],))
        out['days'] = days
    return out


def _pair_table(I, weights=None):
    '''(I as [M, M] int64, the weights as [M] int64 or None)'''
    I = np.asarray(I).astype(np.int64)
    if I.ndim != 2 or I.shape[0] != I.shape[1] or I.shape[0] < 1:
        raise ValueError('the pair table must be [M, M] with M >= 1, got shape %r' % (I.shape,))
    if weights is None:
        return I, None
    w = np.asarray(weights).astype(np.int64)
    if w.shape != (I.shape[0],) or (w < 1).any():
        raise ValueError('weights must be %d integers >= 1' % I.shape[0])
    return I, w


def inclusion_depth(I, weights, epsilon):
    '''(depth, in, cont), each [M] int64, of the pair table I [M, M] (I_ij = |B_i & B_j|, the diagonal n_i): with
    out_ij = n_i - I_ij member i is eps-included in j where 1000 out_ij <= round(1000 epsilon) n_i (an empty set in
    every set); in_i = the weight of the members i lies in, cont_i of those that lie in i, both with i itself;
    depth = min(in, cont), in [w_i, W].  Integers throughout.'''
    I, w = _pair_table(I, weights)
    e = _thousandths(epsilon, 'epsilon', 0.0, 0.5)
    n = np.diagonal(I)
    inc = 1000 * (n[:, None] - I) <= e * n[:, None]        # [i, j]: i lies in j
    w_in = (inc * w[None, :]).sum(1)
    w_cont = (inc * w[:, None]).sum(0)
    return np.minimum(w_in, w_cont), w_in, w_cont


def median_member(depth):
    '''the member with the largest depth, among equals the smallest index'''
    return int(np.argmax(np.asarray(depth)))


def central_members(depth, weights, central=0.5):
    '''the members of the central set in the order (-depth, index): the shortest prefix whose weight cum satisfies
    1000 cum >= round(1000 central) W'''
    depth = np.asarray(depth).astype(np.int64)
    w = np.asarray(weights).astype(np.int64)
    c = _thousandths(central, 'central', 0.0, 1.0, open_lo=True)
    W = int(w.sum())
    out, cum = [], 0
    for m in sorted(range(len(depth)), key=lambda i: (-int(depth[i]), i)):
        out.append(m)
        cum += int(w[m])
        if 1000 * cum >= c * W:
            break
    return out


def set_distance(I):
    '''[M, M] int64 d_ij = n_i + n_j - 2 I_ij: the cells on which members i and j disagree'''
    I, _w = _pair_table(I)
    n = np.diagonal(I)
    return n[:, None] + n[None, :] - 2 * I


def _pam(D, w, K):
    '''the medoids of deterministic PAM in BUILD order, and their cost'''
    M = len(w)
    big = np.iinfo(np.int64).max
    first = int(np.argmin((w[:, None] * D).sum(0)))
    med = [first]
    near = D[:, first].copy()
    while len(med) < K:                                     # BUILD: the candidate that lowers the cost most
        cost = (w[:, None] * np.minimum(near[:, None], D)).sum(0)
        cost[med] = big
        c = int(np.argmin(cost))
        med.append(c)
        near = np.minimum(near, D[:, c])
    cost = int((w * near).sum())
    while True:                                             # SWAP: the best strict improvement, until there is none
        best = (cost, None, None)
        for p in range(K):
            others = [m for q, m in enumerate(med) if q != p]
            base = D[:, others].min(1) if others else np.full(M, big)
            cand = (w[:, None] * np.minimum(base[:, None], D)).sum(0)
            cand[med] = big
            c = int(np.argmin(cand))
            if int(cand[c]) < best[0]:
                best = (int(cand[c]), p, c)
        if best[1] is None:
            return med, cost
        cost, med[best[1]] = best[0], best[2]


def k_medoids(D, weights, K):
    '''Weighted k-medoids of the members on the integer distances D [M, M] by deterministic PAM (Kaufman &
    Rousseeuw), K in 1..min(8, M): cost(Med) = sum_i w_i min_{m in Med} D[i, m].  BUILD: argmin_m sum_i w_i D[i, m],
    then the candidate that lowers the cost most, among equals the smallest index; SWAP: over every (medoid
    position, other member) the swap with the largest strict improvement, among equals the smallest position, then
    the smallest member, until none improves; a member goes to its nearest medoid, among equals the one with the
    smallest index; clusters by descending weight, then medoid index.  -> dict(medoids [K], assignment [M] (the
    cluster of every member), cluster_weight [K], cost, costs_by_k [K]: the cost PAM reaches with 1..K medoids)'''
    D = np.asarray(D).astype(np.int64)
    if D.ndim != 2 or D.shape[0] != D.shape[1] or D.shape[0] < 1:
        raise ValueError('the distances must be [M, M] with M >= 1, got shape %r' % (D.shape,))
    w = np.asarray(weights).astype(np.int64)
    if w.shape != (D.shape[0],) or (w < 1).any():
        raise ValueError('weights must be %d integers >= 1' % D.shape[0])
    K = check_clusters(K)
    if K > len(w):
        raise ValueError('%d clusters of %d members' % (K, len(w)))
    runs = [_pam(D, w, k) for k in range(1, K + 1)]
    med, cost = runs[-1]
    by_index = sorted(med)
    near = np.argmin(D[:, by_index], axis=1)                # the first minimum: the medoid with the smallest index
    weight = [int(w[near == c].sum()) for c in range(K)]
    order = sorted(range(K), key=lambda c: (-weight[c], by_index[c]))
    rank = np.empty(K, dtype=np.int64)
    rank[order] = np.arange(K)
    return {'medoids': [by_index[c] for c in order], 'assignment': rank[near],
            'cluster_weight': [weight[c] for c in order], 'cost': cost, 'costs_by_k': [c for _m, c in runs]}


class MemberOverlap(_Handle):
    '''The pairwise overlap of the members of an ExcursionMaps, on the device (ps_overlap_*, csrc/ps_overlap.hip):
    per threshold and day the table I[i][j] = |B_i & B_j| of the members' reached sets, and the weighted count
    plane of any selection of members.  The handle borrows the maps and reads them at every call: members added
    later are in the next answer.  Integers throughout; no order changes a bit.'''
    _prefix, _noun = 'ps_overlap', 'member overlap'
    _info_types = (C.c_int64, C.c_int64, C.c_int32)        # members of the last pairs call, bytes, tile
    _prof_pairs = 2

    def __init__(self, excursion):
        if not isinstance(excursion, ExcursionMaps):
            raise ValueError('the member overlap is taken over an ExcursionMaps, got %r' % (type(excursion).__name__,))
        self.excursion = excursion
        self._maps()
        self._attach(excursion.pm)
        self.thresholds, self.days = excursion.thresholds, excursion.days
        self._create(excursion._h)

    def _maps(self):
        if not self.excursion._h:
            raise ValueError('the ExcursionMaps of this member overlap are closed')
        return self.excursion

    @property
    def tile(self):
        '''the member-tile edge of the pair kernel'''
        return self._info()[2]

    @property
    def nbytes(self):
        '''the device memory the handle holds now'''
        return self._info()[1]

    def pairs(self, k, day, window=True):
        '''[M, M] uint32: I[i][j] = the cells where members i and j (in add order) both hold >= t_k on `day`, the
        diagonal each member's own cells.  window: visit only the mask words between the first and the last one in
        which any member holds anything; the table is the same without.'''
        E = self._maps()
        M = E.members
        out = np.empty((M, M), dtype=np.uint32)
        self._call('pairs', E._k(k), E._slot_of(day), M, int(bool(window)), out.ctypes.data_as(C.POINTER(C.c_uint32)))
        return out

    def subset_counts(self, k, day, sel):
        '''[N, N] uint32: sum_m sel[m] [member m holds >= t_k at the cell on `day`]; sel: one integer in
        0..2^32 - 1 per member, their sum below 2^32 - 1'''
        E = self._maps()
        s = np.asarray(sel)
        if s.ndim != 1 or s.shape[0] != E.members or not np.issubdtype(s.dtype, np.integer):
            raise ValueError('the selection must be %d integers, got %r' % (E.members, s.shape))
        if s.size and (s.min() < 0 or int(s.astype(np.int64).sum()) >= 0xffffffff):
            raise ValueError('the selection must be >= 0 and sum to less than 2^32 - 1')
        s = np.ascontiguousarray(s, dtype=np.uint32)
        out = np.empty((self.N, self.N), dtype=np.uint32)
        u32 = C.POINTER(C.c_uint32)
        self._call('subset', E._k(k), E._slot_of(day), s.shape[0], s.ctypes.data_as(u32), out.ctypes.data_as(u32))
        return out

    def profile(self, enable=None):
        '''HIP-event time of the pairs calls and the subset launches: (pairs ms, calls, subset ms, launches);
        enable switches it'''
        return self._profile(enable)


class RepresentativeMembers():
    '''Which members of an ExcursionMaps are typical, on their reached sets {v >= t_k}: the inclusion depth of every
    member (Chaves-de-Plaza et al. 2024), the deepest member, the central set and its band (the contour boxplot of
    Whitaker et al. 2013), and weighted k-medoids scenarios on the area two members disagree on.  `day` is a day of
    the maps, or 'all' for the space-time set (the tables summed over the days).  Holds the maps (not owned), a
    MemberOverlap of its own and the settings; the table of a plane is fetched once and kept on the host, until the
    maps gain members.  Members are numbered in add order, as PredictiveResult.runs.'''

    def __init__(self, excursion, epsilon=0.02, central=0.5, clusters=3):
        checked = check_representative(dict(epsilon=epsilon, central=central, clusters=clusters))
        self.settings = {n: checked[n] for n in ('epsilon', 'central', 'clusters')}
        self.epsilon, self.central_level, self.clusters = (checked[n] for n in ('epsilon', 'central', 'clusters'))
        self.overlap = MemberOverlap(excursion)
        self.excursion = excursion
        self.thresholds, self.days, self.N, self.cell_area = (excursion.thresholds, excursion.days, excursion.N,
                                                              excursion.cell_area)
        self._tables, self._members, self._weights = {}, -1, None

    def close(self):
        self.overlap.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _fresh(self):
        M = self.overlap._maps().members
        if M != self._members:
            self._tables, self._members = {}, M
            self._weights = self.excursion.bounds(0, self.days[0])[2].astype(np.int64) if M else None
        if not M:
            raise ValueError('the excursion maps hold no member')

    @property
    def weights(self):
        '''[members] int64, in add order'''
        self._fresh()
        return self._weights

    def pairs(self, k, day):
        '''the pair table of a plane: [M, M] uint32 of a day, int64 of 'all' (the sum over the days)'''
        self._fresh()
        key = (self.excursion._k(k), day)
        if key not in self._tables:
            if isinstance(day, str) and day == 'all':
                self._tables[key] = sum(self.pairs(k, d).astype(np.int64) for d in self.days)
            else:
                self._tables[key] = self.overlap.pairs(k, day)
        return self._tables[key]

    def depth_counts(self, k, day):
        '''(depth, in, cont) [members] int64 (inclusion_depth)'''
        return inclusion_depth(self.pairs(k, day), self.weights, self.epsilon)

    def depth(self, k, day):
        '''[members] float64: depth / W, in (0, 1]'''
        return self.depth_counts(k, day)[0].astype(np.float64) / float(int(self.weights.sum()))

    def median(self, k, day):
        '''the deepest member'''
        return median_member(self.depth_counts(k, day)[0])

    def central(self, k, day):
        '''the members of the central set, deepest first'''
        return central_members(self.depth_counts(k, day)[0], self.weights, self.central_level)

    def _subset(self, k, day_of_map, members):
        sel = np.zeros(self._members, dtype=np.int64)
        sel[members] = self._weights[members]
        return self.overlap.subset_counts(k, day_of_map, sel), int(sel.sum())

    def band(self, k, day_of_map, plane=None):
        '''[N, N] int8 on `day_of_map`, the central set that of `plane` (default: the day itself): +1 inside every
        central member, 0 inside some (the band), -1 outside all'''
        Cs, Wc = self._subset(k, day_of_map, self.central(k, day_of_map if plane is None else plane))
        return (Cs == Wc).astype(np.int8) - (Cs == 0).astype(np.int8)

    def scenarios(self, k, day, K=None):
        '''k_medoids of the plane with K (default: the setting) clusters, at most the members; besides its keys
        `share` [K], the clusters' weight / W, and `members` [K], every cluster's members'''
        K = min(check_clusters(self.clusters if K is None else K), len(self.weights))
        out = k_medoids(set_distance(self.pairs(k, day)), self.weights, K)
        W = float(int(self.weights.sum()))
        out['share'] = [cw / W for cw in out['cluster_weight']]
        out['members'] = [np.flatnonzero(out['assignment'] == c).tolist() for c in range(K)]
        return out

    def scenario_map(self, k, day_of_map, cluster, plane=None, K=None):
        '''[N, N] float64 on `day_of_map`: the probability of >= t_k given scenario `cluster` of `plane` (default:
        the day itself)'''
        sc = self.scenarios(k, day_of_map if plane is None else plane, K)
        c = _Handle._index(cluster, len(sc['medoids']), 'cluster')
        Cs, Wc = self._subset(k, day_of_map, sc['members'][c])
        return Cs.astype(np.float64) / float(Wc)

    def jaccard(self, k, day):
        '''[M, M] float64 I / (n_i + n_j - I), 1 where both sets are empty; nothing is decided on it'''
        I = self.pairs(k, day).astype(np.int64)
        n = np.diagonal(I)
        union = n[:, None] + n[None, :] - I
        return np.where(union > 0, I / np.maximum(union, 1), 1.0)

    def planes(self, days='all'):
        """the planes of the setting `days` that these maps have: ['all'], or the listed days among the maps'"""
        return ['all'] if isinstance(days, str) else [d for d in days if d in self.days]


def save_representative(outfile, rep, runs=None, chains=None, days='all'):
    '''outfile.npz of one RepresentativeMembers through save_maps, for every threshold k and plane p of `days` ('all',
    or the listed days the maps have): `repr_depth_{k}_{p}`, `repr_in_{k}_{p}`, `repr_cont_{k}_{p}` [members] int64,
    `repr_median_{k}_{p}`, `repr_central_{k}_{p}` (deepest first), `repr_medoids_{k}_{p}`, `repr_assign_{k}_{p}`
    [members], `repr_cluster_weight_{k}_{p}`, `repr_costs_{k}_{p}` (by the number of clusters) and the table itself,
    `repr_pairs_{k}_{p}` (uint32 of a day, int64 of 'all'); `repr_weights`, `repr_thresholds`, `repr_days`; per day
    of the maps that a plane covers dense int8 `{day}_band{k}` (dense because a zero means the band) and the CSR
    triplets `{day}_scen{k}_{c}_*` of scenario c's conditional probability.  runs: [(chain, first row, length)]
    per member and chains: per chain the [rows, parameters] array of the model parameters -> its block for the json:
    the settings and per threshold and plane the median, the central set, the medoids with their shares and the
    costs, every median and medoid with its run (chain, first_row, length, params) where runs are given'''
    w = rep.weights
    extra = {'repr_weights': w, 'repr_thresholds': np.asarray(rep.thresholds, dtype=np.float64),
             'repr_days': np.asarray(rep.days)}
    names = model_names()

    def run_of(m):
        if runs is None:
            return None
        ci, first, length = runs[m]
        block = {'chain': int(ci), 'first_row': int(first), 'length': int(length)}
        if chains is not None:
            block['params'] = {n: float(v) for n, v in zip(names, np.asarray(chains[ci])[first])}
        return block
    planes, day_maps = [], {}
    for k in range(len(rep.thresholds)):
        for p in rep.planes(days):
            tag = '%d_%s' % (k, p)
            depth, w_in, w_cont = rep.depth_counts(k, p)
            med, cen, sc = median_member(depth), rep.central(k, p), rep.scenarios(k, p)
            extra.update({'repr_depth_' + tag: depth, 'repr_in_' + tag: w_in, 'repr_cont_' + tag: w_cont,
                          'repr_median_' + tag: np.int64(med), 'repr_central_' + tag: np.asarray(cen, dtype=np.int64),
                          'repr_pairs_' + tag: rep.pairs(k, p),
                          'repr_medoids_' + tag: np.asarray(sc['medoids'], dtype=np.int64),
                          'repr_assign_' + tag: sc['assignment'],
                          'repr_cluster_weight_' + tag: np.asarray(sc['cluster_weight'], dtype=np.int64),
                          'repr_costs_' + tag: np.asarray(sc['costs_by_k'], dtype=np.int64)})
            for d in (rep.days if p == 'all' else [p]):
                extra['%s_band%d' % (d, k)] = rep.band(k, d, p)
                day_maps.setdefault(d, [])
                day_maps[d] += [('_scen%d_%d' % (k, c), rep.scenario_map(k, d, c, p))
                                for c in range(len(sc['medoids']))]
            planes.append({'threshold': k, 'plane': p, 'median': {'member': med, 'run': run_of(med)},
                           'central': cen, 'costs_by_k': sc['costs_by_k'],
                           'medoids': [{'member': m, 'share': s, 'weight': cw, 'run': run_of(m)}
                                       for m, s, cw in zip(sc['medoids'], sc['share'], sc['cluster_weight'])]})
    save_maps(outfile, [(d, day_maps[d]) for d in rep.days if d in day_maps], extra)
    return {'epsilon': rep.epsilon, 'central': rep.central_level, 'clusters': rep.clusters,
            'days': days if isinstance(days, str) else list(days), 'thresholds': list(rep.thresholds),
            'members': int(len(w)), 'total_weight': int(w.sum()), 'cell_area': rep.cell_area, 'planes': planes}


# ------------------------------------------------------------------ ensemble modes: in what ways do the members differ?
MAX_MODES = 8              # ps_modes: the coefficient rows of one combine
MAX_MODE_DAYS = 8          # ps_modes: the day slots of one handle
MODE_TRANSFORMS = {'raw': 0, 'sqrt': 1}


def check_modes(arg, days):
    '''posterior_predictive's modes= argument, True or dict(days=[...] | 'all', count=4, transform='sqrt' | 'raw'),
    against `days`, the days the fields have (a list, or their number) -> dict(days, count, transform).  days: the
    listed days get a decomposition each; 'all' (the default) is the space-time decomposition over every day.
    ValueError for anything else, a day the fields do not have, a count outside 1..8 and more than 8 days.'''
    if arg is True:
        arg = {}
    if not isinstance(arg, dict):
        raise ValueError("modes must be True or dict(days=[...] | 'all', count=4, transform='sqrt'), got %r" % (arg,))
    unknown = set(arg) - {'days', 'count', 'transform'}
    if unknown:
        raise ValueError('modes: unknown keys %r' % (sorted(unknown),))
    count, transform, want = arg.get('count', 4), arg.get('transform', 'sqrt'), arg.get('days', 'all')
    if isinstance(count, bool) or not isinstance(count, (int, np.integer)) or not 1 <= count <= MAX_MODES:
        raise ValueError('modes: count must be a whole number in 1..%d, got %r' % (MAX_MODES, count))
    if transform not in MODE_TRANSFORMS:
        raise ValueError("modes: transform must be 'sqrt' or 'raw', got %r" % (transform,))
    have = list(range(days)) if isinstance(days, (int, np.integer)) else (None if days is None else list(days))
    if isinstance(want, str):
        if want != 'all':
            raise ValueError("modes: days must be a list of days or 'all', got %r" % (want,))
        if have is not None and len(have) > MAX_MODE_DAYS:
            raise ValueError("modes: 'all' covers %d days, at most %d fit (list the days)" % (len(have), MAX_MODE_DAYS))
    else:
        try:
            want = [int(d) for d in want]
        except (TypeError, ValueError):
            raise ValueError("modes: days must be a list of days or 'all', got %r" % (arg.get('days'),))
        if not want or len(want) > MAX_MODE_DAYS:
            raise ValueError('modes: 1..%d days, got %d' % (MAX_MODE_DAYS, len(want)))
        if any(b <= a for a, b in zip(want, want[1:])):
            raise ValueError('modes: days must be strictly increasing, got %r' % (want,))
        if have is not None and [d for d in want if d not in have]:
            raise ValueError('modes: day %r is not among the days %r' % ([d for d in want if d not in have][0], have))
    return {'days': want, 'count': int(count), 'transform': transform}


def mode_decomposition(G, weights, count):
    '''The weighted principal components of an ensemble from its table G [M, M] of inner products of the centred
    fields and the members' integer weights: B = D^1/2 G D^1/2 / W with D = diag(w), numpy.linalg.eigh, the
    eigenvalues descending, `count` (1..8) eigenpairs (lambda_k, u_k) kept.  The entry of u_k of largest magnitude is
    positive, among equal magnitudes the one of smallest index.  A lambda_k at or below M 2^-52 trace B is absent:
    count shrinks and nothing is divided by it.  -> dict(count, eigenvalues [K], explained [K] = lambda_k / trace B,
    total_variance = trace B, spectrum (every eigenvalue, descending), vectors [M, K], scores [M, K] with
    z_mk = u_mk sqrt(W / w_m) (weighted mean 0, variance 1) and coef [K, M], c_km = sqrt(w_m) u_mk / sqrt(W lambda_k),
    the rows EnsembleModes.combine turns into the unit-norm patterns e_k)'''
    G = np.asarray(G, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    M = len(w)
    if G.shape != (M, M) or M < 1:
        raise ValueError('a table of %r for %d weights' % (G.shape, M))
    if isinstance(count, bool) or not 1 <= int(count) <= MAX_MODES:
        raise ValueError('count must lie in 1..%d, got %r' % (MAX_MODES, count))
    if np.any(w < 1) or np.any(w != np.floor(w)):
        raise ValueError('weights must be whole numbers >= 1')
    W = w.sum()
    r = np.sqrt(w)
    B = r[:, None] * G * r[None, :] / W
    lam, U = np.linalg.eigh(B)
    order = np.argsort(-lam, kind='stable')
    lam, U = lam[order], U[:, order]
    total = float(np.trace(B))
    floor = M * 2.0 ** -52 * total
    K = min(int(count), int(np.sum(lam > floor))) if total > 0 else 0
    lam_k, U = lam[:K], U[:, :K].copy()
    for k in range(K):
        mag = np.abs(U[:, k])
        if U[int(np.argmax(mag == mag.max())), k] < 0:
            U[:, k] = -U[:, k]
    return {'count': K, 'eigenvalues': lam_k, 'explained': lam_k / total if K else lam_k, 'total_variance': total,
            'spectrum': lam, 'vectors': U, 'scores': U * np.sqrt(W / w)[:, None],
            'coef': np.ascontiguousarray((r[:, None] * U / np.sqrt(W * lam_k)[None, :]).T)}


def effective_members(weights):
    '''Kish's effective sample size W^2 / sum w_m^2'''
    w = np.asarray(weights, dtype=np.float64)
    return float(w.sum() ** 2 / (w * w).sum())


def separated(eigenvalues, weights):
    '''North et al.'s (1982) rule of thumb per mode: the sampling error of lambda_k is about lambda_k sqrt(2 / n_eff),
    n_eff = W^2 / sum w_m^2; mode k is separated when its distance to both neighbours among `eigenvalues` (descending;
    the first and the last have one) exceeds it.  A pair that is not separated spans a plane, not two patterns.
    -> [K] bool'''
    lam = np.asarray(eigenvalues, dtype=np.float64)
    err = lam * np.sqrt(2.0 / effective_members(weights))
    out = np.ones(len(lam), dtype=bool)
    for k in range(len(lam)):
        for j in (k - 1, k + 1):
            if 0 <= j < len(lam) and not abs(lam[k] - lam[j]) > err[k]:
                out[k] = False
    return out


def score_drivers(scores, thetas, weights, names):
    '''the weighted correlation of every mode's scores [M, K] with every model parameter of the members' runs, thetas
    [M, P] named `names`; a parameter (or a score) that never moves gets 0 -> dict(names, corr [K, P], strongest:
    per mode the name of the parameter of largest |corr|, None where all are 0)'''
    z = np.asarray(scores, dtype=np.float64)
    th = np.asarray(thetas, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    if z.shape[0] != len(w) or th.shape != (len(w), len(names)):
        raise ValueError('scores %r, parameters %r, %d weights, %d names' % (z.shape, th.shape, len(w), len(names)))
    W = w.sum()
    zc = z - (w[:, None] * z).sum(0) / W
    tc = th - (w[:, None] * th).sum(0) / W
    sz = np.sqrt((w[:, None] * zc * zc).sum(0) / W)
    st = np.sqrt((w[:, None] * tc * tc).sum(0) / W)
    still = st <= 1e-14 * np.maximum(np.abs(th).max(0), 1e-300)      # the chain never moved it
    cov = (w[:, None] * zc).T @ tc / W
    den = sz[:, None] * st[None, :]
    corr = np.where((den > 0) & ~still[None, :], cov / np.where(den > 0, den, 1.0), 0.0)
    strongest = [names[int(np.argmax(np.abs(c)))] if np.any(c != 0) else None for c in corr]
    return {'names': list(names), 'corr': corr, 'strongest': strongest}


class EnsembleModes(_Accumulator):
    '''The members' transformed fields of `pop_model` on the listed model days (strictly increasing, at most 8,
    default all) kept on the device as fp64 -- X = v ('raw') or sqrt(v) ('sqrt', the default: the Hellinger-type
    transform of Legendre & Gallagher 2001 for count-like fields) -- with an integer weight per member, and from
    them the weighted mean plane, the M x M table of inner products of the (centred) fields, a symmetric fp64 product
    on the matrix units, and linear combinations of the (centred) fields.  mean and combine are bit for bit numpy
    loops in add order; the table is symmetric to the bit, the same bits on every call, and within
    2 N^2 2^-53 sqrt(G_ii G_jj) of the exact product.  day 'all' of `table` is the space-time table, the per-day
    tables added in slot order on the host.'''
    _prefix, _noun = 'ps_modes', 'ensemble modes'
    _info_types = (C.c_double, C.c_int64, C.c_int64, C.c_int64)      # weight, members, capacity, bytes
    _prof_pairs = 4

    def __init__(self, pop_model, days=None, transform='sqrt'):
        self._setup(pop_model, None, range(len(pop_model.days)) if days is None else days, transform)

    @classmethod
    def for_projection(cls, source, transform='sqrt'):
        '''The modes of the outputs of `source` (a ReleaseSites or a Projection; at most 8 outputs), the slots its
        outputs in ascending order: `add(weight)` stores the outputs of its last `apply()`.  `days` holds the output
        labels.'''
        self = cls.__new__(cls)
        self._setup(source.pm, source, _output_labels(source), transform)
        return self

    def _setup(self, pop_model, projection, days, transform):
        if transform not in MODE_TRANSFORMS:
            raise ValueError("transform must be 'sqrt' or 'raw', got %r" % (transform,))
        days = check_arrival_days(days)
        if len(days) > MAX_MODE_DAYS:
            raise ValueError('ensemble modes take at most %d days, got %d' % (MAX_MODE_DAYS, len(days)))
        self.transform = transform
        self._attach(pop_model)
        self._set_source(projection, days)
        self.member_nbytes = len(self.days) * self.pitch * 8
        self._create(len(self.days), MODE_TRANSFORMS[transform])

    def reserve(self, n):
        '''room for n members' fields now, so that no add has to grow them'''
        self._call('reserve', int(n))

    def add(self, weight=1):
        '''Store the last evaluation of the model with integer weight >= 1 (one launch on the solver's stream; no host
        synchronisation unless the fields grow).  On a projection or a plan: its last apply, on the handle's stream.'''
        self._add(weight)

    def add_fields(self, fields, weight=1):
        '''Store one member from host arrays [days, N, N] of values >= 0 (fields saved by Run); the transform is
        applied.  ValueError for a shape that does not fit; a negative or non-finite value is refused, nothing stored.'''
        f = np.ascontiguousarray(fields, dtype=np.float64)
        if f.shape != (len(self.days), self.N, self.N):
            raise ValueError('fields of shape %r, the ensemble modes hold %r' % (f.shape, (len(self.days), self.N, self.N)))
        self._call('add_host', L.p_f64(f), self._weight(weight))

    def merge(self, other):
        '''self's members, then other's (same device, domain, days and transform); other is unchanged'''
        if list(other.days) != self.days:
            raise ValueError('ensemble modes over different days')
        self._call('merge', other._h)

    def window(self, on):
        '''on (the default): the table visits only the live window of the mean plane; off: every cell'''
        self._call('set_window', int(bool(on)))

    @property
    def capacity(self):
        '''the members the fields hold room for'''
        return self._info()[2]

    @property
    def nbytes(self):
        '''the device memory the handle holds now'''
        return self._info()[3]

    @property
    def weights(self):
        '''[members] uint32 in add order'''
        out = np.empty(self.members, dtype=np.uint32)
        self._call('weights', len(out), out.ctypes.data_as(C.POINTER(C.c_uint32)))
        return out

    def mean(self, day):
        '''[N, N] float64: the weighted mean of the transformed fields'''
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('mean', self._slot_of(day), L.p_f64(out))
        return out

    def table(self, day, centred=True):
        '''[members, members] float64: G_ij = sum_c A_i(c) A_j(c) with A = X - mean (centred) or X; day 'all': the
        sum over the days in slot order'''
        M = self.members
        if isinstance(day, str) and day == 'all':
            total = np.zeros((M, M), dtype=np.float64)
            for d in self.days:
                total += self.table(d, centred)
            return total
        out = np.empty((M, M), dtype=np.float64)
        self._call('table', self._slot_of(day), int(bool(centred)), M, L.p_f64(out))
        return out

    def combine(self, day, coef, centred=True):
        '''[ncoef, N, N] float64: out_k = sum_m coef[k, m] A_m over the members in add order, coef [ncoef (1..8),
        members]'''
        c = np.ascontiguousarray(coef, dtype=np.float64)
        if c.ndim != 2 or not 1 <= c.shape[0] <= MAX_MODES or c.shape[1] != self.members:
            raise ValueError('coefficients of shape %r for %d members (1..%d rows)' % (c.shape, self.members, MAX_MODES))
        out = np.empty((c.shape[0], self.N, self.N), dtype=np.float64)
        self._call('combine', self._slot_of(day), int(bool(centred)), c.shape[0], L.p_f64(c), L.p_f64(out))
        return out

    def member(self, m, day):
        '''[N, N] float64: the stored transformed field of member m (in add order)'''
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('fetch_member', int(m), self._slot_of(day), L.p_f64(out))
        return out

    def profile(self, enable=None):
        '''HIP-event time of the add, mean, table and combine launches: (add ms, adds, mean ms, means, table ms,
        tables, combine ms, combines); enable switches it'''
        ms = np.zeros(4, dtype=np.float64)
        n = np.zeros(4, dtype=np.int64)
        self._call('prof', -1 if enable is None else int(bool(enable)), L.p_f64(ms), L.p_i64(n))
        return tuple(v for k in range(4) for v in (float(ms[k]), int(n[k])))


class ModesPosterior():
    '''The ensemble modes as posterior_predictive returns them: `modes` (the EnsembleModes, which it owns), `count`,
    `planes` (the decompositions it saves: listed days, or ['all']) and `given`.  A decomposition belongs to a plane
    -- a day of the handle or 'all', the space-time table -- and is cached until members are added; a map belongs to a
    day and, by default, to that day's own decomposition.  `runs` [(chain, first row, length)] per member and
    `chains` (per chain the [rows, parameters] array of the model parameters) are set by the driver; `drivers` and
    `extremes` need them.'''

    def __init__(self, modes, count=4, days='all'):
        self.modes, self.count = modes, int(count)
        self.planes = ['all'] if isinstance(days, str) else [d for d in days if d in modes.days]
        self.given = None
        self.runs = self.chains = None
        self._cache = {}
        self._members = -1

    days = property(lambda self: self.modes.days)
    transform = property(lambda self: self.modes.transform)

    def reserve(self, n):
        self.modes.reserve(n)

    def add(self, weight=1):
        self.modes.add(weight)
        self._members = -1

    def merge(self, other):
        self.modes.merge(other.modes)
        self._members = -1

    def close(self):
        self.modes.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def weights(self):
        return self.modes.weights

    def decomposition(self, plane):
        '''mode_decomposition of the centred table of `plane` (a day or 'all'), cached until members are added.
        Centring leaves M - 1 directions, so at most that many modes are kept: the last eigenvalue of a centred
        table is rounding error of the table's size, which may lie above the floor of mode_decomposition.'''
        if self._members != self.modes.members:
            self._cache, self._members = {}, self.modes.members
        if plane not in self._cache:
            count = max(1, min(self.count, self._members - 1))
            self._cache[plane] = mode_decomposition(self.modes.table(plane, True), self.weights, count)
        return self._cache[plane]

    def eigenvalues(self, day):
        return self.decomposition(day)['eigenvalues']

    def explained(self, day):
        return self.decomposition(day)['explained']

    def separated(self, day):
        '''per kept mode North's rule against its neighbours in the whole spectrum'''
        dec = self.decomposition(day)
        return separated(dec['spectrum'], self.weights)[:dec['count']]

    def scores(self, day):
        '''[members, K]: the standardised scores'''
        return self.decomposition(day)['scores']

    def _mode(self, k, plane):
        dec = self.decomposition(plane)
        return dec, _Handle._index(k, dec['count'], 'mode')

    def unit_patterns(self, day, plane=None):
        '''[K, N, N]: e_k of the decomposition of `plane` (default: the day's own) on `day`, every kept mode from one
        pass over the members'''
        dec = self.decomposition(day if plane is None else plane)
        if not dec['count']:
            return np.zeros((0, self.modes.N, self.modes.N))
        return self.modes.combine(day, dec['coef'], True)

    def unit_pattern(self, k, day, plane=None):
        '''[N, N]: e_k, of unit norm over its plane'''
        dec, k = self._mode(k, day if plane is None else plane)
        return self.modes.combine(day, dec['coef'][k:k + 1], True)[0]

    def pattern(self, k, day, plane=None):
        '''[N, N]: sqrt(lambda_k) e_k, the change of the transformed field per +1 sd of the score'''
        dec, k = self._mode(k, day if plane is None else plane)
        return np.sqrt(dec['eigenvalues'][k]) * self.unit_pattern(k, day, plane)

    def thetas(self):
        '''[members, parameters]: the model parameters of the members' runs'''
        if self.runs is None or self.chains is None:
            raise ValueError('the runs of the members are not known')
        return np.array([np.asarray(self.chains[ci])[first] for ci, first, _l in self.runs], dtype=np.float64)

    def drivers(self, day):
        '''score_drivers of the plane's scores against the model parameters of the members' runs'''
        return score_drivers(self.scores(day), self.thetas(), self.weights, model_names())

    def extremes(self, k, day):
        '''the members with the lowest and the highest score on mode k, each with its score and, where the runs are
        known, its run (chain, first_row, length, params), among equals the smallest index'''
        dec, k = self._mode(k, day)
        z = dec['scores'][:, k]
        out = {}
        for name, m in (('low', int(np.argmin(z))), ('high', int(np.argmax(z)))):
            out[name] = {'member': m, 'score': float(z[m]), 'run': None}
            if self.runs is not None:
                ci, first, length = self.runs[m]
                out[name]['run'] = {'chain': int(ci), 'first_row': int(first), 'length': int(length)}
                if self.chains is not None:
                    out[name]['run']['params'] = {n: float(v) for n, v in
                                                  zip(model_names(), np.asarray(self.chains[ci])[first])}
        return out

    def reconstruct(self, m, day, modes=None, plane=None):
        '''[N, N]: mean + sum over the first `modes` (default all kept) of score x pattern, the transformed field of
        member m as the modes see it'''
        dec = self.decomposition(day if plane is None else plane)
        K = dec['count'] if modes is None else min(int(modes), dec['count'])
        out = self.modes.mean(day)
        if K:
            e = self.modes.combine(day, dec['coef'][:K], True)
            for k in range(K):
                out = out + dec['scores'][m, k] * np.sqrt(dec['eigenvalues'][k]) * e[k]
        return out


def save_modes(outfile, post):
    '''outfile.npz of one ModesPosterior: per plane p of its planes (a day, or 'all') `{p}_eigenvalues`,
    `{p}_explained`, `{p}_separated`, `{p}_scores` [M, K] and, where the runs are known, `{p}_drivers` [K, nparam];
    per day of a plane dense `{day}_mean` and `{day}_mode{k}` (sqrt(lambda_k) e_k; dense because the patterns are
    signed and nowhere sparse); `weights`, `transform`, `days`.  -> its block for the json: the settings, the members,
    n_eff and per plane the explained shares, the separated flags, the strongest driver of each mode and the runs of
    the extremes'''
    w = post.weights
    out = {'weights': w, 'transform': np.asarray(post.transform), 'days': np.asarray(post.days)}
    planes = []
    known = post.runs is not None and post.chains is not None
    for p in post.planes:
        dec = post.decomposition(p)
        K = dec['count']
        sep = post.separated(p)
        out.update({'%s_eigenvalues' % p: dec['eigenvalues'], '%s_explained' % p: dec['explained'],
                    '%s_separated' % p: sep, '%s_scores' % p: dec['scores']})
        drv = post.drivers(p) if known else None
        if drv is not None:
            out['%s_drivers' % p] = drv['corr']
        for d in (post.days if p == 'all' else [p]):
            out['%s_mean' % d] = post.modes.mean(d)
            e = post.unit_patterns(d, p)
            for k in range(K):
                out['%s_mode%d' % (d, k)] = np.sqrt(dec['eigenvalues'][k]) * e[k]
        planes.append({'plane': p, 'count': K, 'total_variance': dec['total_variance'],
                       'explained': [float(v) for v in dec['explained']],
                       'separated': [bool(v) for v in sep],
                       'planes_not_patterns': [k for k in range(K) if not sep[k]],
                       'strongest_driver': None if drv is None else drv['strongest'],
                       'extremes': [post.extremes(k, p) for k in range(K)]})
    os.makedirs(os.path.dirname(os.path.abspath(str(outfile))), exist_ok=True)
    np.savez(str(outfile), **out)
    return {'count': post.count, 'transform': post.transform, 'days': list(post.days),
            'planes_given': 'all' if post.planes == ['all'] else list(post.planes), 'members': int(len(w)),
            'total_weight': int(w.sum()), 'n_eff': effective_members(w), 'planes': planes}


MAX_RANGE_FRACTIONS = 4


def check_range_fractions(fractions):
    '''mass fractions of the core-range maps as a list of floats: 1..4 of them, each a finite number in (0, 1),
    strictly increasing; ValueError otherwise'''
    try:
        fr = [float(p) for p in fractions]
    except (TypeError, ValueError):
        raise ValueError('core-range fractions must be numbers, got %r' % (fractions,))
    if not 1 <= len(fr) <= MAX_RANGE_FRACTIONS:
        raise ValueError('%d core-range fractions; 1..%d are kept' % (len(fr), MAX_RANGE_FRACTIONS))
    if not all(0.0 < p < 1.0 for p in fr):
        raise ValueError('every core-range fraction must lie in (0, 1): %r' % (fr,))
    if any(b <= a for a, b in zip(fr, fr[1:])):
        raise ValueError('core-range fractions must be strictly increasing: %r' % (fr,))
    return fr


def check_core_range(core_range, days=None):
    '''the core_range= argument of posterior_predictive -> (fractions, levels): a list of fractions (1..4, each in
    (0, 1), strictly increasing), or dict(fractions=[...], levels=(0.5, 0.9)), the consensus levels -- the
    posterior probabilities at which the saved consensus range {prob >= level} is cut -- each in (0, 1]; `days`,
    where given, by the rules of check_arrival_days; ValueError otherwise'''
    levels = (0.5, 0.9)
    if isinstance(core_range, dict):
        unknown = set(core_range) - {'fractions', 'levels'}
        if unknown:
            raise ValueError('core_range: unknown keys %r' % (sorted(unknown),))
        if 'fractions' not in core_range:
            raise ValueError('core_range: fractions are needed')
        levels = core_range.get('levels', levels)
        core_range = core_range['fractions']
    try:
        fr = list(core_range)
    except TypeError:
        raise ValueError('core-range fractions must be a list of numbers, got %r' % (core_range,))
    try:
        lv = [float(p) for p in levels]
    except (TypeError, ValueError):
        raise ValueError('core-range consensus levels must be numbers, got %r' % (levels,))
    if not lv or not all(0.0 < p <= 1.0 for p in lv):
        raise ValueError('core-range consensus levels must lie in (0, 1], at least one: %r' % (lv,))
    if days is not None:
        check_arrival_days(days)
    return check_range_fractions(fr), lv


class RangeMaps(_Accumulator):
    '''Where each of `pop_model`'s members holds most of its wasps: for mass fractions p_0 < ... < p_{J-1} (1..4,
    each in (0, 1)) and the model days `days` (strictly increasing, at most 32, default all) the member's own
    highest-density region {v >= lambda_j}, the smallest set of cells that holds the share p_j of the member's
    population on that day -- 0.5 the "core", 0.95 the "range" of the utilisation distribution.  On the device per
    (j, day) the weighted count C of the members whose region holds the cell, and per member the level lambda_j,
    the cells n_j of the region, the integer mass Q and its exponent E (ps_range_*; the statements are those of
    include/parasitoid_hip.h, restated in tests/range_ref.py).  The level is the member's own, so the maps do not
    change with the release number.  Counts are integers: the order of adds and merges changes no bit.'''
    _prefix, _noun, _prof_pairs = 'ps_range', 'core-range maps', 2
    _info_types = (C.c_double, C.c_int64, C.c_int64, C.c_int64)      # weight, members, capacity, bytes

    def __init__(self, pop_model, fractions, days=None):
        self.fractions = check_range_fractions(fractions)
        self._setup(pop_model, None, check_arrival_days(range(len(pop_model.days)) if days is None else days))

    @classmethod
    def for_projection(cls, projection, fractions):
        '''Core-range maps of the outputs of `projection` (a ReleaseSites or a Projection), the slots its outputs
        that carry weight in ascending order: `add(weight)` accumulates the outputs of its last `apply()`.
        `days` holds the output labels -- the plan's output days, or the projection's output indices.'''
        self = cls.__new__(cls)
        self.fractions = check_range_fractions(fractions)
        self._setup(projection.pm, projection, check_arrival_days(_output_labels(projection)))
        return self

    def _setup(self, pop_model, projection, days):
        self._attach(pop_model)
        self._set_source(projection, days)
        self._create(len(self.days), len(self.fractions), L.p_f64(L.f64(self.fractions)))

    def reserve(self, n):
        '''room for n members' rows now, so that no add has to grow them'''
        self._call('reserve', int(n))

    def add(self, weight=1):
        '''Accumulate the last evaluation of the model with integer weight >= 1 (enqueued on the solver's stream;
        no host synchronisation unless the member rows grow).  On a projection or a plan: its last apply, on the
        handle's stream.'''
        self._add(weight)

    def merge(self, other):
        '''self += other (same device, domain, days and fractions); other's members follow self's'''
        if list(other.days) != self.days:
            raise ValueError('core-range maps over different days')
        self._call('merge', other._h)

    @property
    def capacity(self):
        '''the members the rows hold room for'''
        return self._info()[2]

    @property
    def nbytes(self):
        '''the device memory the handle holds now'''
        return self._info()[3]

    def _j(self, j):
        if not 0 <= int(j) < len(self.fractions):
            raise ValueError('fraction %r of %d' % (j, len(self.fractions)))
        return int(j)

    def counts(self, j, day):
        '''[N, N] uint32: the weight of the members whose p_j region on `day` holds the cell'''
        out = np.empty((self.N, self.N), dtype=np.uint32)
        self._call('fetch_counts', self._j(j), self._slot_of(day), out.ctypes.data_as(C.POINTER(C.c_uint32)))
        return out

    def prob(self, j, day):
        '''[N, N] float64: the posterior probability C / W that the cell lies in the member's p_j region'''
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('prob', self._j(j), self._slot_of(day), L.p_f64(out))
        return out

    def range(self, j, day, level=0.5):
        '''[N, N] bool: the consensus region {prob >= level}, 0 < level <= 1'''
        level, = check_levels([level])
        return self.prob(j, day) >= level

    def _members(self, j, day):
        m = self.members
        lam = np.empty(m, dtype=np.float64)
        n, w = np.empty(m, dtype=np.uint32), np.empty(m, dtype=np.uint32)
        u32 = C.POINTER(C.c_uint32)
        self._call('fetch_members', self._j(j), self._slot_of(day), L.p_f64(lam), n.ctypes.data_as(u32),
                                    w.ctypes.data_as(u32))
        return lam, n, w

    @property
    def weights(self):
        '''[members] int64: the members' weights in add order'''
        return self._members(0, self.days[0])[2].astype(np.int64)

    def levels(self, j, day):
        '''[members] float64 in add order: the member's own level lambda_j on `day`, +inf where it holds nothing'''
        return self._members(j, day)[0]

    def cells(self, j, day):
        '''[members] int64 in add order: the cells of the member's p_j region on `day`'''
        return self._members(j, day)[1].astype(np.int64)

    def mass(self, day):
        '''(Q [members] uint64, E [members] int32) in add order: the member's integer mass on `day`, the sum of
        floor(v 2^(36 - E)), and E = floor(log2 max v); both 0 where it holds nothing'''
        m = self.members
        Q, E = np.empty(m, dtype=np.uint64), np.empty(m, dtype=np.int32)
        self._call('fetch_mass', self._slot_of(day), Q.ctypes.data_as(C.POINTER(C.c_uint64)), L.p_i32(E))
        return Q, E

    def area(self, j, day, levels=(0.05, 0.5, 0.95)):
        '''The posterior of the area of the p_j region on `day`: {'day', 'mean', 'quantiles', 'radius_mean',
        'radius_quantiles'}, as one entry of ArrivalMaps.reached_area.  Areas in m^2 (cells x (rad_dist /
        rad_res)^2): the weighted mean and the weighted lower quantiles (weighted_lower_quantile) at `levels`;
        radii sqrt(A / pi) in m.'''
        levels = check_levels(levels)
        _lam, n, w = self._members(j, day)
        return range_area(n, w, self.cell_area, levels, day)

    def profile(self, enable=None):
        '''HIP-event time of the adds and the map launches: (add ms, adds, map ms, map launches); enable
        switches it'''
        return self._profile(enable)



def range_area(cells, weights, cell_area, levels=(0.05, 0.5, 0.95), day=None):
    '''the posterior of a region's area from the members' cell counts and integer weights, as RangeMaps.area
    returns it (no device)'''
    levels = check_levels(levels)
    n = np.asarray(cells).astype(np.int64)
    w = np.asarray(weights).astype(np.int64)
    W = int(w.sum())
    if W == 0:
        raise ValueError('nothing accumulated')
    mean = float(int((n * w).sum())) / float(W) * cell_area
    q = [float(weighted_lower_quantile(n, w, p)) * cell_area for p in levels]
    return {'day': day, 'mean': mean, 'quantiles': q, 'radius_mean': float(np.sqrt(mean / np.pi)),
            'radius_quantiles': [float(np.sqrt(a / np.pi)) for a in q]}


MAX_PATCH_THRESHOLDS = 4
PATCH_WHICH = ('main', 'satellite')


def check_patch_connectivity(connectivity):
    '''4 or 8 as an int; ValueError otherwise'''
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError('patch connectivity must be 4 or 8, got %r' % (connectivity,))
    return int(connectivity)


def check_patches(patches, days=None):
    '''the patches= argument of posterior_predictive -> (thresholds, connectivity, levels): a list of thresholds
    (1..4, finite, > 0, strictly increasing), or dict(thresholds=[...], connectivity=8, levels=(0.05, 0.5, 0.95)),
    the connectivity 4 (default) or 8 and the levels, each in (0, 1], those of the saved quantiles of the patch count
    and of the areas; `days`, where given, by the rules of check_arrival_days; ValueError otherwise'''
    connectivity, levels = 4, (0.05, 0.5, 0.95)
    if isinstance(patches, dict):
        unknown = set(patches) - {'thresholds', 'connectivity', 'levels'}
        if unknown:
            raise ValueError('patches: unknown keys %r' % (sorted(unknown),))
        if 'thresholds' not in patches:
            raise ValueError('patches: thresholds are needed')
        connectivity = patches.get('connectivity', connectivity)
        levels = patches.get('levels', levels)
        patches = patches['thresholds']
    try:
        thr = [float(t) for t in patches]
    except (TypeError, ValueError):
        raise ValueError('patch thresholds must be a list of numbers, got %r' % (patches,))
    if not 1 <= len(thr) <= MAX_PATCH_THRESHOLDS:
        raise ValueError('%d patch thresholds; 1..%d are kept' % (len(thr), MAX_PATCH_THRESHOLDS))
    if not all(np.isfinite(t) and t > 0.0 for t in thr):
        raise ValueError('every patch threshold must be finite and > 0: %r' % (thr,))
    if any(b <= a for a, b in zip(thr, thr[1:])):
        raise ValueError('patch thresholds must be strictly increasing: %r' % (thr,))
    connectivity = check_patch_connectivity(connectivity)
    levels = check_levels(levels)
    if days is not None:
        check_arrival_days(days)
    return thr, connectivity, levels


def patch_number(npatch, weights, levels=(0.05, 0.5, 0.95), day=None):
    '''the posterior of the patch count from the members' counts and integer weights, as PatchMaps.number returns
    it (no device): {'day', 'mean', 'p_fragmented' = P(npatch >= 2), 'p_empty' = P(npatch = 0), 'quantiles'}'''
    levels = check_levels(levels)
    n = np.asarray(npatch).astype(np.int64)
    w = np.asarray(weights).astype(np.int64)
    W = int(w.sum())
    if W == 0:
        raise ValueError('nothing accumulated')
    return {'day': day, 'mean': float(int((n * w).sum())) / float(W),
            'p_fragmented': float(int(w[n >= 2].sum())) / float(W), 'p_empty': float(int(w[n == 0].sum())) / float(W),
            'quantiles': [float(weighted_lower_quantile(n, w, p)) for p in levels]}


def patch_satellite_share(cells, main_cells, weights):
    '''the weighted mean, over the members that hold any cell, of the share of their occupied cells that lies
    outside the main patch; None where no member holds a cell'''
    n = np.asarray(cells).astype(np.int64)
    m = np.asarray(main_cells).astype(np.int64)
    w = np.asarray(weights).astype(np.int64)
    live = n > 0
    if not live.any():
        return None
    share = (n[live] - m[live]) / n[live].astype(np.float64)
    return float((share * w[live]).sum() / float(int(w[live].sum())))


class PatchMaps(_Accumulator):
    '''Whether the area `pop_model`'s members reach is one front or separate foci: for thresholds t_0 < ... <
    t_{K-1} (1..4, finite, > 0) and the model days `days` (strictly increasing, at most 32, default all) the
    patches of each member's set {v >= t_k}, its connected components under `connectivity` 4 or 8 (no wrap at the
    domain edge).  The main patch is the one with the most cells, among equals the one whose smallest linear index
    row * N + col (its label) is smallest -- not the one at the release point.  On the device per (k, day) the
    weighted count of the members whose main patch holds the cell ('main') and of those that hold it in another
    patch ('satellite'), and per member the number of patches, the cells of the set, of the main patch and of the
    largest other patch, and the main patch's label (ps_patch_*; the statements are those of
    include/parasitoid_hip.h, restated in tests/patch_ref.py).  main + satellite is ExcursionMaps.counts.  Every
    number is an integer and the label canonical: the order of adds and merges changes no bit.'''
    _prefix, _noun, _prof_pairs = 'ps_patch', 'patch maps', 2
    _info_types = (C.c_double, C.c_int64, C.c_int64, C.c_int64)      # weight, members, capacity, bytes

    def __init__(self, pop_model, thresholds, days=None, connectivity=4):
        self.thresholds, self.connectivity, _lv = check_patches(dict(thresholds=thresholds, connectivity=connectivity))
        self._setup(pop_model, None, check_arrival_days(range(len(pop_model.days)) if days is None else days))

    @classmethod
    def for_projection(cls, source, thresholds, connectivity=4):
        '''Patch maps of the outputs of `source` (a ReleaseSites or a Projection), the slots its outputs that
        carry weight in ascending order: `add(weight)` accumulates the outputs of its last `apply()`.  `days` holds
        the output labels -- the plan's output days, or the projection's output indices.'''
        self = cls.__new__(cls)
        self.thresholds, self.connectivity, _lv = check_patches(dict(thresholds=thresholds, connectivity=connectivity))
        self._setup(source.pm, source, check_arrival_days(_output_labels(source)))
        return self

    def _setup(self, pop_model, projection, days):
        self._attach(pop_model)
        self._set_source(projection, days)
        self._create(len(self.days), len(self.thresholds), L.p_f64(L.f64(self.thresholds)), self.connectivity)

    def reserve(self, n):
        '''room for n members' rows now, so that no add has to grow them'''
        self._call('reserve', int(n))

    def add(self, weight=1):
        '''Accumulate the last evaluation of the model with integer weight >= 1 (enqueued on the solver's stream;
        no host synchronisation unless the member rows grow).  On a projection or a plan: its last apply, on the
        handle's stream.'''
        self._add(weight)

    def merge(self, other):
        '''self += other (same device, domain, days, thresholds and connectivity); other's members follow self's'''
        if list(other.days) != self.days:
            raise ValueError('patch maps over different days')
        self._call('merge', other._h)

    @property
    def capacity(self):
        '''the members the rows hold room for'''
        return self._info()[2]

    @property
    def nbytes(self):
        '''the device memory the handle holds now'''
        return self._info()[3]

    @staticmethod
    def _which(which):
        if which not in PATCH_WHICH:
            raise ValueError('which must be one of %r, got %r' % (PATCH_WHICH, which))
        return PATCH_WHICH.index(which)

    def counts(self, k, day, which):
        '''[N, N] uint32: the weight of the members whose main patch at t_k on `day` holds the cell ('main'), or
        that hold it in another patch ('satellite')'''
        out = np.empty((self.N, self.N), dtype=np.uint32)
        self._call('fetch_counts', self._k(k), self._slot_of(day), self._which(which),
                   out.ctypes.data_as(C.POINTER(C.c_uint32)))
        return out

    def prob(self, k, day, which):
        '''[N, N] float64: counts / W, the posterior probability of the same'''
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('prob', self._k(k), self._slot_of(day), self._which(which), L.p_f64(out))
        return out

    def _members(self, k, day):
        '''(npatch, cells, main_cells, main_label, sat_cells_max, weights), [members] uint32 each, in add order'''
        out = [np.empty(self.members, dtype=np.uint32) for _ in range(6)]
        self._call('fetch_members', self._k(k), self._slot_of(day),
                   *[a.ctypes.data_as(C.POINTER(C.c_uint32)) for a in out])
        return tuple(out)

    @property
    def weights(self):
        '''[members] int64: the members' weights in add order'''
        return self._members(0, self.days[0])[5].astype(np.int64)

    def patches(self, k, day):
        '''[members] int64 in add order: the number of patches of {v >= t_k} on `day`'''
        return self._members(k, day)[0].astype(np.int64)

    def cells(self, k, day):
        '''[members] int64 in add order: the cells of {v >= t_k} on `day`'''
        return self._members(k, day)[1].astype(np.int64)

    def main_cells(self, k, day):
        '''[members] int64 in add order: the cells of the main patch'''
        return self._members(k, day)[2].astype(np.int64)

    def main_label(self, k, day):
        '''[members] int64 in add order: the main patch's smallest linear index row * N + col, -1 where the set
        is empty'''
        lab = self._members(k, day)[3]
        return np.where(lab == 0xffffffff, -1, lab.astype(np.int64))

    def largest_satellite(self, k, day):
        '''[members] int64 in add order: the cells of the largest patch other than the main one, 0 without one'''
        return self._members(k, day)[4].astype(np.int64)

    def number(self, k, day, levels=(0.05, 0.5, 0.95)):
        '''The posterior of the patch count at t_k on `day`: {'day', 'mean', 'p_fragmented', 'p_empty',
        'quantiles'} (patch_number): the weighted mean, P(npatch >= 2), P(npatch = 0) and the weighted lower
        quantiles (weighted_lower_quantile) at `levels`.'''
        rows = self._members(k, day)
        return patch_number(rows[0], rows[5], levels, day)

    def area(self, k, day, which='main', levels=(0.05, 0.5, 0.95)):
        '''The posterior of the area of the main patch ('main'), of the occupied cells outside it ('satellite') or
        of the whole set ('all') at t_k on `day`, in m^2, as RangeMaps.area (range_area).'''
        if which not in PATCH_WHICH + ('all',):
            raise ValueError('which must be one of %r, got %r' % (PATCH_WHICH + ('all',), which))
        rows = self._members(k, day)
        n, m = rows[1].astype(np.int64), rows[2].astype(np.int64)
        return range_area({'main': m, 'satellite': n - m, 'all': n}[which], rows[5], self.cell_area, levels, day)

    def profile(self, enable=None):
        '''HIP-event time of the adds and the map launches: (add ms, adds, map ms, map launches); enable
        switches it'''
        return self._profile(enable)


def save_patches(outfile, pat, levels=(0.05, 0.5, 0.95)):
    '''outfile.npz of one PatchMaps through save_maps: per day of the maps, under the label `{day}`, the CSR triplets
    `{day}_pmain{k}_*` and `{day}_psat{k}_*` of the probability that the cell lies in the member's main patch, or in
    its set outside it; the members' rows `patch_npatch`, `patch_cells`, `patch_main_cells`, `patch_sat_cells_max`
    (uint32) and `patch_main_label` (int64, -1 where the set is empty) [thresholds, days, members],
    `patch_weights` [members], `patch_thresholds`, `patch_connectivity` and `patch_days` -> its block for the json:
    thresholds, connectivity, days, levels, members, weight, cell area and per threshold and day `p_fragmented`,
    the mean patch count `mean_patches`, its quantiles, `p_empty` and `satellite_share`, the mean share of the
    occupied cells that lies in satellites (null where no member holds a cell)'''
    levels = check_levels(levels)
    nk = len(pat.thresholds)
    maps, number = [], [[] for _ in range(nk)]
    rows = [[pat._members(k, d) for d in pat.days] for k in range(nk)]
    for di, d in enumerate(pat.days):
        day_maps = []
        for k in range(nk):
            day_maps += [('_pmain%d' % k, pat.prob(k, d, 'main')), ('_psat%d' % k, pat.prob(k, d, 'satellite'))]
            r = rows[k][di]
            rec = patch_number(r[0], r[5], levels, d)
            number[k].append({'day': d, 'p_fragmented': rec['p_fragmented'], 'mean_patches': rec['mean'],
                              'quantiles': rec['quantiles'], 'p_empty': rec['p_empty'],
                              'satellite_share': patch_satellite_share(r[1], r[2], r[5])})
        maps.append((d, day_maps))
    extra = {}
    for f, name in enumerate(('npatch', 'cells', 'main_cells', 'main_label', 'sat_cells_max')):
        a = np.array([[x[f] for x in row] for row in rows], dtype=np.uint32)
        extra['patch_' + name] = np.where(a == 0xffffffff, -1, a.astype(np.int64)) if name == 'main_label' else a
    extra.update({'patch_weights': np.asarray(rows[0][0][5], dtype=np.uint32),
                  'patch_thresholds': np.asarray(pat.thresholds, dtype=np.float64),
                  'patch_connectivity': np.asarray(pat.connectivity), 'patch_days': np.asarray(pat.days)})
    save_maps(outfile, maps, extra)
    return {'thresholds': list(pat.thresholds), 'connectivity': pat.connectivity, 'days': list(pat.days),
            'levels': levels, 'members': pat.members, 'total_weight': pat.total_weight, 'cell_area': pat.cell_area,
            'number': number}


MAX_PATHWAY_THRESHOLDS = 4
MAX_PATHWAY_ANCHORS = 32
PATHWAY_WHICH = ('front', 'jump', 'secondary')


def check_pathway_anchors(anchors, N):
    '''anchor cells as a list of (row, col) ints: 1..32 cells on the N x N grid; None: the centre cell, where
    the model releases; ValueError otherwise'''
    if anchors is None:
        return [(N // 2, N // 2)]
    try:
        cells = [(int(r), int(c)) for r, c in anchors]
    except (TypeError, ValueError):
        raise ValueError('pathway anchors must be a list of (row, col) cells, got %r' % (anchors,))
    if not 1 <= len(cells) <= MAX_PATHWAY_ANCHORS:
        raise ValueError('%d pathway anchors; 1..%d are kept' % (len(cells), MAX_PATHWAY_ANCHORS))
    for r, c in cells:
        if not (0 <= r < N and 0 <= c < N):
            raise ValueError('pathway anchor (%d, %d) is off the %d x %d grid' % (r, c, N, N))
    return cells


def check_pathways(pathways, days=None):
    '''the pathways= argument of posterior_predictive -> (thresholds, connectivity, days, levels): a list of
    thresholds (1..4, finite, > 0, strictly increasing), or dict(thresholds=[...], connectivity=8, days=None,
    levels=(0.05, 0.5, 0.95)): the connectivity 4 (default) or 8, the model days of the window by the rules of
    check_arrival_days (None: the `days` given here, the summary's) and the levels, each in (0, 1], of the saved
    quantiles of the foci and of the areas; ValueError otherwise'''
    connectivity, levels, own_days = 4, (0.05, 0.5, 0.95), None
    if isinstance(pathways, dict):
        unknown = set(pathways) - {'thresholds', 'connectivity', 'days', 'levels'}
        if unknown:
            raise ValueError('pathways: unknown keys %r' % (sorted(unknown),))
        if 'thresholds' not in pathways:
            raise ValueError('pathways: thresholds are needed')
        connectivity = pathways.get('connectivity', connectivity)
        levels = pathways.get('levels', levels)
        own_days = pathways.get('days')
        pathways = pathways['thresholds']
    try:
        thr = [float(t) for t in pathways]
    except (TypeError, ValueError):
        raise ValueError('pathway thresholds must be a list of numbers, got %r' % (pathways,))
    if not 1 <= len(thr) <= MAX_PATHWAY_THRESHOLDS:
        raise ValueError('%d pathway thresholds; 1..%d are kept' % (len(thr), MAX_PATHWAY_THRESHOLDS))
    if not all(np.isfinite(t) and t > 0.0 for t in thr):
        raise ValueError('every pathway threshold must be finite and > 0: %r' % (thr,))
    if any(b <= a for a, b in zip(thr, thr[1:])):
        raise ValueError('pathway thresholds must be strictly increasing: %r' % (thr,))
    connectivity = check_patch_connectivity(connectivity)
    levels = check_levels(levels)
    if own_days is not None:
        own_days = check_arrival_days(own_days)
        if days is not None and not set(own_days) <= set(int(d) for d in days):
            raise ValueError('pathway days %r are not among the days %r' % (own_days, list(days)))
    elif days is not None:
        own_days = check_arrival_days(days)
    return thr, connectivity, own_days, levels


def pathway_founded(foci, weights, levels=(0.05, 0.5, 0.95)):
    '''the posterior of the number of foci founded over the window from the members' totals and integer weights,
    as PathwayMaps.founded returns it (no device): {'mean', 'p_any' = P(foci >= 1), 'quantiles'}'''
    levels = check_levels(levels)
    n = np.asarray(foci).astype(np.int64)
    w = np.asarray(weights).astype(np.int64)
    W = int(w.sum())
    if W == 0:
        raise ValueError('nothing accumulated')
    return {'mean': float(int((n * w).sum())) / float(W), 'p_any': float(int(w[n >= 1].sum())) / float(W),
            'quantiles': [float(weighted_lower_quantile(n, w, p)) for p in levels]}


class PathwayMaps(_Accumulator):
    '''How `pop_model`'s members reached each cell: by the advancing front, by a jump, or by the growth of a focus
    a jump founded (stratified dispersal).  For thresholds t_0 < ... < t_{K-1} (1..4, finite, > 0), the model days
    `days` (strictly increasing, at most 32, default all) taken in order, `connectivity` 4 or 8 (no wrap) and the
    anchor cells `anchors` ([(row, col), ...], 1..32, default the centre cell): the patches of {v >= t_k} on each
    day are those of PatchMaps; a patch is `origin` if it holds an anchor or a cell classed front before that day,
    `seeded` if it holds any cell classed before; its cells not classed yet become 'front' if origin, else
    'secondary' if seeded, else 'jump' -- the founding cells of a new focus.  A class is never changed once set.
    On the device the weighted count of the members per class and cell, and per member and day the cells newly
    classed and the foci founded (ps_pathway_*; the statements are those of include/parasitoid_hip.h, restated in
    tests/pathway_ref.py).  front + jump + secondary is ArrivalMaps.counts summed over the days.  Every number is
    an integer and the label canonical: the order of adds and merges changes no bit.'''
    _prefix, _noun, _prof_pairs = 'ps_pathway', 'pathway maps', 1
    _info_types = (C.c_double, C.c_int64, C.c_int64, C.c_int64)      # weight, members, capacity, bytes

    def __init__(self, pop_model, thresholds, days=None, connectivity=4, anchors=None):
        self.thresholds, self.connectivity, _d, _lv = check_pathways(dict(thresholds=thresholds,
                                                                          connectivity=connectivity))
        self._setup(pop_model, None, check_arrival_days(range(len(pop_model.days)) if days is None else days), anchors)

    @classmethod
    def for_projection(cls, release_sites, thresholds, connectivity=4):
        '''Pathway maps of the outputs of a ReleaseSites in ascending output day, the anchors the cells of the
        plan's sites: `add(weight)` accumulates the outputs of its last `apply()`.  `days` holds the plan's output
        days.  A Projection is no source: its outputs are not a sequence of days.'''
        if getattr(release_sites, 'fields_kind', None) != 'sites':
            raise ValueError('pathway maps take a release plan as their source: the outputs of a projection are '
                             'not a sequence of days')
        self = cls.__new__(cls)
        self.thresholds, self.connectivity, _d, _lv = check_pathways(dict(thresholds=thresholds,
                                                                          connectivity=connectivity))
        R = int(release_sites.pm.rad_res)
        anchors = []
        for s in release_sites.sites:
            cell = (R + s['drow'], R + s['dcol'])
            if cell not in anchors:
                anchors.append(cell)
        self._setup(release_sites.pm, release_sites, check_arrival_days(_output_labels(release_sites)), anchors)
        return self

    def _setup(self, pop_model, projection, days, anchors):
        self._attach(pop_model)
        self.anchors = check_pathway_anchors(anchors, self.N)
        self._set_source(projection, days)
        self._create(len(self.days), len(self.thresholds), L.p_f64(L.f64(self.thresholds)), self.connectivity,
                     len(self.anchors), L.p_i32(L.i32([r for r, _c in self.anchors])),
                     L.p_i32(L.i32([c for _r, c in self.anchors])))

    def reserve(self, n):
        '''room for n members' rows now, so that no add has to grow them'''
        self._call('reserve', int(n))

    def add(self, weight=1):
        '''Accumulate the last evaluation of the model with integer weight >= 1 (enqueued on the solver's stream;
        no host synchronisation unless the member rows grow).  On a plan: its last apply, on the handle's stream.'''
        self._add(weight)

    def merge(self, other):
        '''self += other (same device, domain, days, thresholds, connectivity and anchors); other's members follow
        self's'''
        if list(other.days) != self.days:
            raise ValueError('pathway maps over different days')
        self._call('merge', other._h)

    @property
    def capacity(self):
        '''the members the rows hold room for'''
        return self._info()[2]

    @property
    def nbytes(self):
        '''the device memory the handle holds now: counts, parent scratch, flags, states and rows'''
        return self._info()[3]

    @staticmethod
    def _which(which):
        if which not in PATHWAY_WHICH:
            raise ValueError('which must be one of %r, got %r' % (PATHWAY_WHICH, which))
        return PATHWAY_WHICH.index(which)

    def counts(self, k, which):
        '''[N, N] uint32: the weight of the members that reached the cell at t_k within the window by the front
        ('front'), as a founding cell of a new focus ('jump') or by the growth of a focus ('secondary')'''
        out = np.empty((self.N, self.N), dtype=np.uint32)
        self._call('fetch_counts', self._k(k), self._which(which), out.ctypes.data_as(C.POINTER(C.c_uint32)))
        return out

    def prob(self, k, which):
        '''[N, N] float64: counts / W, the posterior probability of the same'''
        return self.counts(k, which).astype(np.float64) / float(self.total_weight)

    def share(self, k, which):
        '''[N, N] float64: counts / (front + jump + secondary), among the members that reached the cell the share
        that did so this way; NaN where nobody reached it'''
        c = [self.counts(k, w).astype(np.float64) for w in PATHWAY_WHICH]
        total = c[0] + c[1] + c[2]
        with np.errstate(invalid='ignore', divide='ignore'):
            return np.where(total > 0, c[self._which(which)] / total, np.nan)

    def _members(self, k, day):
        '''(front, jump, secondary, foci, weights), [members] uint32 each, in add order'''
        out = [np.empty(self.members, dtype=np.uint32) for _ in range(5)]
        self._call('fetch_members', self._k(k), self._slot_of(day),
                   *[a.ctypes.data_as(C.POINTER(C.c_uint32)) for a in out])
        return tuple(out)

    def _window(self, k):
        '''([members, days, 4] int64: the rows of t_k over the window, weights [members] int64)'''
        rows = [self._members(k, d) for d in self.days]
        return (np.array([[r[f] for f in range(4)] for r in rows], dtype=np.int64).transpose(2, 0, 1),
                rows[0][4].astype(np.int64))

    @property
    def weights(self):
        '''[members] int64: the members' weights in add order'''
        return self._members(0, self.days[0])[4].astype(np.int64)

    def new_cells(self, k, day, which):
        '''[members] int64 in add order: the cells newly classed `which` at t_k on `day`'''
        return self._members(k, day)[self._which(which)].astype(np.int64)

    def foci(self, k, day):
        '''[members] int64 in add order: the foci founded at t_k on `day`'''
        return self._members(k, day)[3].astype(np.int64)

    def founded(self, k, levels=(0.05, 0.5, 0.95)):
        '''The posterior of the number of foci founded at t_k over the window: {'mean', 'p_any', 'quantiles'}
        (pathway_founded): the weighted mean, P(foci >= 1) and the weighted lower quantiles at `levels`.'''
        rows, w = self._window(k)
        return pathway_founded(rows[:, :, 3].sum(axis=1), w, levels)

    def area(self, k, which, levels=(0.05, 0.5, 0.95)):
        '''The posterior of the area taken by one pathway at t_k over the window, in m^2, as RangeMaps.area
        (range_area)'''
        rows, w = self._window(k)
        return range_area(rows[:, :, self._which(which)].sum(axis=1), w, self.cell_area, levels)

    def profile(self, enable=None):
        '''HIP-event time of the adds: (add ms, adds); enable switches it'''
        return self._profile(enable)


def pathway_block(thresholds, connectivity, days, anchors, levels, rows, weights, cell_area):
    '''the json block of save_pathways from the members' rows [thresholds, days, 4, members] and weights (no
    device): thresholds, connectivity, days, anchors, levels, members, weight, cell area and per threshold
    `founded` (pathway_founded) and per class `area` (range_area)'''
    levels = check_levels(levels)
    rows = np.asarray(rows).astype(np.int64)
    w = np.asarray(weights).astype(np.int64)
    per = []
    for k in range(len(thresholds)):
        rec = {'founded': pathway_founded(rows[k, :, 3].sum(axis=0), w, levels)}
        for j, which in enumerate(PATHWAY_WHICH):
            rec['area_' + which] = range_area(rows[k, :, j].sum(axis=0), w, cell_area, levels)
        per.append(rec)
    return {'thresholds': [float(t) for t in thresholds], 'connectivity': int(connectivity),
            'days': [int(d) for d in days], 'anchors': [[int(r), int(c)] for r, c in anchors], 'levels': levels,
            'members': int(w.size), 'total_weight': float(int(w.sum())), 'cell_area': float(cell_area),
            'pathways': per}


def pathway_arrays(thresholds, connectivity, days, anchors, rows, weights):
    '''the arrays save_pathways adds to its npz: the members' rows `pathway_front`, `pathway_jump`,
    `pathway_secondary`, `pathway_foci` (uint32) [thresholds, days, members], `pathway_weights` [members],
    `pathway_thresholds`, `pathway_connectivity`, `pathway_days` and `pathway_anchors` [anchors, 2]'''
    rows = np.asarray(rows)
    extra = {'pathway_' + name: rows[:, :, f].astype(np.uint32)
             for f, name in enumerate(PATHWAY_WHICH + ('foci',))}
    extra.update({'pathway_weights': np.asarray(weights, dtype=np.uint32),
                  'pathway_thresholds': np.asarray(thresholds, dtype=np.float64),
                  'pathway_connectivity': np.asarray(int(connectivity)), 'pathway_days': np.asarray(list(days)),
                  'pathway_anchors': np.asarray(anchors, dtype=np.int64).reshape(-1, 2)})
    return extra


def save_pathways(outfile, pw, levels=(0.05, 0.5, 0.95)):
    '''outfile.npz of one PathwayMaps through save_maps: under the label `window` the CSR triplets
    `window_pfront{k}_*`, `window_pjump{k}_*` and `window_psecondary{k}_*` of the probability that the cell was
    reached that way within the window, and the arrays of pathway_arrays -> its block for the json
    (pathway_block)'''
    levels = check_levels(levels)
    nk = len(pw.thresholds)
    rows = np.array([[pw._members(k, d)[:4] for d in pw.days] for k in range(nk)])      # [K, days, 4, members]
    weights = pw.weights
    maps = [('window', [('_p%s%d' % (which, k), pw.prob(k, which)) for k in range(nk) for which in PATHWAY_WHICH])]
    save_maps(outfile, maps, pathway_arrays(pw.thresholds, pw.connectivity, pw.days, pw.anchors, rows, weights))
    return pathway_block(pw.thresholds, pw.connectivity, pw.days, pw.anchors, levels, rows, weights, pw.cell_area)


def check_weights(weights, nin=None, zero_rows=False):
    '''A projection's weight matrix as a float64 [nout, nin] array, by the rules of ps_project_create: 1..32
    outputs, 1..32 inputs (nin if given), every weight finite and >= 0, and no row of all zeros unless
    zero_rows (Projection keeps such rows off the device); ValueError otherwise'''
    try:
        W = np.array(weights, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('projection weights must be a matrix of numbers')
    if W.ndim != 2:
        raise ValueError('projection weights must be a matrix [outputs, inputs], got shape %r' % (W.shape,))
    if not 1 <= W.shape[0] <= MAX_PROJECT_OUT:
        raise ValueError('%d projection outputs; 1..%d are kept' % (W.shape[0], MAX_PROJECT_OUT))
    if not 1 <= W.shape[1] <= MAX_PROJECT_IN:
        raise ValueError('%d projection inputs; 1..%d fit one launch' % (W.shape[1], MAX_PROJECT_IN))
    if nin is not None and W.shape[1] != nin:
        raise ValueError('projection weights have %d columns for %d input days' % (W.shape[1], nin))
    if not np.all(np.isfinite(W)) or not np.all(W >= 0):
        raise ValueError('every projection weight must be finite and >= 0')
    dead = np.flatnonzero(~(W != 0).any(axis=1))
    if dead.size and not zero_rows:
        raise ValueError('projection outputs %s have no non-zero weight' % (dead.tolist(),))
    return np.ascontiguousarray(W)


def emergence_weights(collection_day, in_days, obs_days=None):
    '''[nout, len(in_days)] weights of the emergence projection of Bayes_funcs.popdensity_to_emergence, built
    from Bayes_funcs._projection_matrix: leaves collected on `collection_day` (days post release) carry the
    oviposition of the days [max(collection_day - 25, 0), collection_day), which emerges 19..25 days later.
    obs_days=None: one output per day 0 .. 24 after the collection (the `emerg` matrix before binning);
    else one output per observation day (days post release, strictly increasing, not before the collection;
    nothing emerges after day collection_day + 24), each taking the emergence since the previous one as the
    reference bins it.  An
    output may be all zeros (no listed oviposition day emerges then).  ValueError if an oviposition day that
    carries weight is missing from in_days.'''
    cday = int(collection_day)
    if cday < 1:
        raise ValueError('collection day %r: no oviposition day before it' % (collection_day,))
    horizon = BF.max_incubation_time
    if obs_days is None:
        obs = np.arange(cday, cday + horizon)
    else:
        obs = np.array([int(d) for d in obs_days], dtype=int)
        if obs.size < 1 or obs[0] < cday or np.any(np.diff(obs) <= 0):
            raise ValueError('observation days must be strictly increasing from day %d on: %r' % (cday, obs.tolist()))
    in_days = [int(d) for d in in_days]
    start = max(cday - horizon, 0)
    M = BF._projection_matrix(start, cday, obs)            # [oviposition day - start, output]
    W = np.zeros((len(obs), len(in_days)))
    pos = {d: n for n, d in enumerate(in_days)}
    for n, day in enumerate(range(start, cday)):
        if day in pos:
            W[:, pos[day]] = M[n]
        elif np.any(M[n] != 0):
            raise ValueError('oviposition day %d carries emergence weight and is not among the input days %r'
                             % (day, in_days))
    return W


def exposure_weights(in_days, upto):
    '''[len(upto), len(in_days)] weights of the cumulative exposure (wasp-days) up to each day of `upto`:
    1 where in_days[d] <= upto[e], else 0'''
    d = np.array([int(x) for x in in_days], dtype=int)
    u = np.array([int(x) for x in upto], dtype=int)
    return (d[None, :] <= u[:, None]).astype(np.float64)


class Projection(_FieldSource):
    '''Y_e(c) = sum_d weights[e][d] v_d(c) of `pop_model`'s last evaluation, on the device: v_d the value
    SpreadSummary adds for model day in_days[d] (strictly increasing, at most 32), weights [nout, nin] finite
    and >= 0 (check_weights), at most 32 outputs.  The sum runs in ascending d from +0.0 with the product and
    the sum rounded separately, so a numpy loop reproduces every bit.  An output whose weights are all zero
    is zero throughout: it is kept off the device (`live` lists the others) and reads as zeros.'''
    fields_kind = 'project'      # the accumulators' entry points for these fields: ps_*_add_project
    _prefix, _noun = 'ps_project', 'projection'

    def __init__(self, pop_model, weights, in_days):
        self.in_days = check_in_days(in_days)
        self.weights = check_weights(weights, len(self.in_days), zero_rows=True)
        self.nout = self.weights.shape[0]
        self.live = [int(e) for e in np.flatnonzero((self.weights != 0).any(axis=1))]
        if not self.live:
            raise ValueError('the projection has no non-zero weight')
        self._slot = {e: i for i, e in enumerate(self.live)}
        self._attach(pop_model)
        self.nbytes = len(self.live) * self.pitch * 8       # the output fields
        W = np.ascontiguousarray(self.weights[self.live])
        self._create(len(self.in_days), len(self.live), L.p_f64(W))
        self._set_days(self.in_days)



def emergence_plan(emergence, ndays=None):
    '''posterior_predictive's emergence= argument, dict(collection_day=C, obs_days=None), as (weights,
    in_days, labels): the oviposition days [max(C - 25, 0), C), the labels in days post release (C + j, or the
    observation days).  ValueError for a bad argument, or if the model's ndays days do not reach day C - 1.'''
    if not isinstance(emergence, dict) or 'collection_day' not in emergence \
            or set(emergence) - {'collection_day', 'obs_days'}:
        raise ValueError('emergence must be dict(collection_day=C, obs_days=None), got %r' % (emergence,))
    cday = int(emergence['collection_day'])
    obs = emergence.get('obs_days')
    in_days = list(range(max(cday - BF.max_incubation_time, 0), cday))
    W = check_weights(emergence_weights(cday, in_days, obs), len(in_days), zero_rows=True)
    if not np.any(W != 0):
        raise ValueError('no listed emergence day carries weight')
    if ndays is not None and cday > ndays:
        raise ValueError('the model has %d days; emergence after a collection on day %d needs day %d'
                         % (ndays, cday, cday - 1))
    labels = [cday + j for j in range(W.shape[0])] if obs is None else [int(d) for d in obs]
    return W, in_days, labels


def exposure_plan(exposure, ndays=None):
    '''posterior_predictive's exposure= argument, model days [D1, D2, ...] (strictly increasing, 0..31), as
    (weights, in_days, labels) over the days 0 .. max D.  ValueError for a bad argument, or if the model's
    ndays days do not reach the last one.'''
    try:
        upto = [int(d) for d in exposure]
    except (TypeError, ValueError):
        raise ValueError('exposure must be a list of model days, got %r' % (exposure,))
    if not upto or upto[0] < 0 or any(b <= a for a, b in zip(upto, upto[1:])):
        raise ValueError('exposure days must be model days >= 0, strictly increasing: %r' % (upto,))
    in_days = check_in_days(range(upto[-1] + 1))
    if ndays is not None and upto[-1] >= ndays:
        raise ValueError('the model has %d days; exposure up to day %d needs it' % (ndays, upto[-1]))
    return check_weights(exposure_weights(in_days, upto), len(in_days)), in_days, upto


# ------------------------------------------------------------------ the accumulators fed from one source of fields
# The order in which posterior_predictive feeds one member to the accumulators of one source of fields, per kind of
# source: the model's day fields, a Projection, the ReleaseSites of sites=, after it plan B of compare= and, last,
# the further plans of ranking=.
# 'apply' is the source's own.  The three orders differ for no better reason than the history of the maps.
FEED_ORDER = {
    'days': ('summary', 'origin', 'core_range', 'reweight', 'reweight_histogram', 'reweight_arrival', 'catch', 'neighbourhood', 'proximity', 'information', 'excursion', 'mc_error',
             'sensitivity', 'dependence', 'histogram', 'arrival', 'peak', 'patches', 'pathways', 'weather', 'modes'),
    'projection': ('apply', 'summary', 'reweight', 'reweight_histogram', 'mc_error', 'sensitivity', 'dependence', 'histogram', 'catch',
                   'weather'),
    'sites': ('apply', 'summary', 'reweight', 'reweight_histogram', 'reweight_arrival', 'mc_error', 'sensitivity',
              'dependence', 'histogram', 'arrival', 'peak', 'excursion', 'core_range', 'catch', 'neighbourhood', 'proximity', 'information', 'patches', 'pathways',
              'weather', 'modes'),
    'compare': ('apply', 'contrast', 'reweight_contrast'),
    'ranking': ('apply', 'ranking'),
}


def _add_length(acc, fs, m):
    acc.add(m.length)


def _add_halves(seqs, fs, m):
    '''the run's length, split at the chain's half boundary row, to the chain's two MonteCarloError sequences'''
    for seq, w in zip(seqs, mc_split(m.first, m.length, fs._half)):
        if w:
            seq.add(w)


def _add_reweighted(acc, fs, m):
    if fs._rw_feed is not None:        # the day fields': one gather of all probes; the later sets share the log-weights
        m.lam = fs._rw_feed.log_weights(fs._source, m.first, m.length)
    acc.add(m.lam, m.length)


def _add_catch(acc, fs, m):
    acc.add(m.length, m.lam)
    if acc.mc_error is not None:
        _add_halves(acc.mc_error, fs, m)


# Every accumulator a _FieldSet can hold, and how it takes a member m (theta, first row, length, lam: the run's
# log-weights or None) of the set fs.
FEED = {
    'apply': lambda acc, fs, m: fs._source.apply(),
    'summary': _add_length,
    'histogram': _add_length,
    'arrival': _add_length,
    'sensitivity': lambda acc, fs, m: acc.add(m.theta, m.length),
    'dependence': lambda acc, fs, m: acc.add(m.theta, m.length),
    'peak': _add_length,
    'excursion': _add_length,
    'core_range': _add_length,
    'reweight': _add_reweighted,
    'reweight_histogram': lambda acc, fs, m: acc.add(m.lam, m.length),     # after 'reweight', which sets m.lam
    'reweight_arrival': lambda acc, fs, m: acc.add(m.lam, m.length),
    'catch': _add_catch,
    'neighbourhood': _add_catch,
    'proximity': _add_catch,
    'information': lambda acc, fs, m: acc.add(m.length, m.lam),
    'mc_error': _add_halves,
    'contrast': _add_length,
    'reweight_contrast': lambda acc, fs, m: acc.add(m.lam, m.length),      # m.lam: set by the day set's 'reweight'
    'ranking': _add_length,
    'patches': _add_length,
    'pathways': _add_length,
    'modes': _add_length,
    'origin': _add_length,
    'weather': lambda acc, fs, m: acc.add(),       # one draw of the run's group; the driver closes it with the length
}
ACCUMULATORS = tuple(name for name in FEED if name != 'apply')


def _owned_by(inner, wrap, *args):
    '''wrap(inner, *args), which then owns inner; where that fails inner is closed'''
    try:
        return wrap(inner, *args)
    except BaseException:
        inner.close()
        raise


def _build_mc_error(fs, q):
    if q.mc_b:
        fs.mc_error = []
        for _half in range(2):
            fs.mc_error.append(fs._over(MonteCarloError, (q.mc_b, fs._days, q.thresholds), (q.mc_b, q.thresholds)))
    return fs.mc_error


def _build_reweight(fs, q):
    if q.rw_plan is not None:
        names = q.rw_plan['names']
        fs.reweight = fs._over(ReweightedSummary, (names, fs._days, q.thresholds), (names, q.thresholds))
        if fs._kind == 'days':
            fs._rw_feed = _ReweightFeed(q.rw_plan, fs._chain)
    return fs.reweight


def _reweight_maps(q):
    '''the 'maps' option of the checked reweight=, () where there is none'''
    plan = getattr(q, 'rw_plan', None)
    return plan.get('maps', ()) if plan is not None else ()


def _build_reweight_histogram(fs, q):
    '''the ReweightedHistogram on the edges of the request's quantiles=; None, and nothing built, without
    maps=('quantiles', ...)'''
    if 'quantiles' in _reweight_maps(q):
        names = q.rw_plan['names']
        return fs._over(ReweightedHistogram, (names, fs._days, q.bins, q.edges), (names, q.bins, q.edges))


def _build_reweight_arrival(fs, q):
    '''the ReweightedArrival on the thresholds of the request's arrival=; None, and nothing built, without
    maps=(..., 'arrival')'''
    if 'arrival' in _reweight_maps(q):
        names = q.rw_plan['names']
        return fs._over(ReweightedArrival, (names, q.a_thr, fs._days), (names, q.a_thr))


def _build_reweight_contrast(fs, q):
    '''the ReweightedContrast of plan A against this set's plan B on the request's thresholds; None, and nothing
    built, without maps=(..., 'contrast')'''
    if 'contrast' in _reweight_maps(q):
        return ReweightedContrast(fs._against, fs._source, q.rw_plan['names'], q.thresholds)


def _build_catch(fs, q):
    traps = fs._traps.get('catch')
    if traps:
        cp = _owned_by(fs._over(CatchFields, traps, traps), CatchPosterior, q.ct_plan['levels'], q.mc_b, q.rw_names)
        cp.given = q.ct_plan['given']
        return cp


def _build_neighbourhood(fs, q):
    windows = fs._traps.get('neighbourhood')
    if windows:
        nf = fs._over(NeighbourhoodFields, windows, windows)
        npost = _owned_by(nf, NeighbourhoodPosterior, q.thresholds, q.levels, q.bins, q.edges, q.mc_b, q.rw_names)
        npost.given = q.nb_plan['given']
        return npost


def _build_proximity(fs, q):
    windows = fs._traps.get('proximity')
    if windows:
        plan = q.px_plan
        pf = fs._over(ProximityFields, windows, windows)
        ppost = _owned_by(pf, ProximityPosterior, plan['radii_m'], plan['levels'], plan['ladder'], q.mc_b, q.rw_names)
        ppost.given = plan['given']
        return ppost


def _build_information(fs, q):
    traps = fs._traps.get('information')
    if traps:
        ip = _owned_by(fs._over(InformationFields, traps, traps), InformationPosterior, q.rw_names)
        ip.given = q.in_plan['given']
        return ip


def _build_modes(fs, q):
    plan = q.md_plan
    if plan is not None:
        if fs._kind == 'days':
            days = fs._days if isinstance(plan['days'], str) else plan['days']
            em = EnsembleModes(fs._source, days, plan['transform'])
        else:
            em = EnsembleModes.for_projection(fs._source, plan['transform'])
        mp = _owned_by(em, ModesPosterior, plan['count'], plan['days'])
        mp.given = q.modes
        return mp


def _build_dependence(fs, q):
    '''one DependenceMaps over the pooled edges; where the device has not that much free, a ValueError that names
    the figure'''
    plan = getattr(q, 'dp_plan', None)
    if plan is None:
        return None
    names, edges = plan['params'], q.dp_edges
    try:
        if fs._kind == 'days':
            dm = DependenceMaps(fs._source, names, edges, plan['days'] or fs._days)
        else:
            dm = DependenceMaps.for_projection(fs._source, names, edges)
    except L.HipError as e:
        if e.code != L.PS_ERR_OOM:
            raise
        nbin = max(2, max(len(x) for x in edges) + 1)
        nslot = len(plan['days'] or fs._days) if fs._kind == 'days' else fs._source.nout
        raise ValueError('dependence: %d parameters x %d bins x %d slots need %.3g GB, which do not fit the free '
                         'device memory; days= and a shorter parameter list cut it (%s)'
                         % (len(names), nbin, nslot,
                            ((2 + len(names) * nbin + len(names)) * 8 + 1) * nslot * fs._source_pitch() * 1e-9, e))
    dm.bins_asked = plan['bins']
    return dm


def _build_origin(fs, q):
    '''the OriginMaps of the model's day fields; the models of its later release days are the driver's (fs._late)'''
    if getattr(q, 'or_plan', None) is not None and fs._kind == 'days':
        return OriginMaps(fs._source, q.origin, fs._late)


def _build_weather(fs, q):
    '''the WeatherShare of a weather ensemble (wind= with share); None, and nothing built, without'''
    plan = getattr(q, 'wind_plan', None)
    if plan is not None and plan['share']:
        return fs._over(WeatherShare, (fs._days,), ())


def _reserve_modes(mp, nruns):
    '''room for a chain's runs before its first evaluation; where the device has not that much free, a ValueError
    that names the figure'''
    try:
        mp.reserve(nruns)
    except L.HipError as e:
        if e.code != L.PS_ERR_OOM:
            raise
        em = mp.modes
        raise ValueError('modes: %d members x %d days x %d cells x 8 B = %.3g GB do not fit the free device memory (%s)'
                         % (nruns, len(em.days), em.pitch, nruns * len(em.days) * em.pitch * 8e-9, e))


# How each accumulator is built for the set fs from the checked request q (None or empty: not asked for).  The choice
# between the model's day fields and a source's outputs is _FieldSet._over's.
BUILD = {
    'summary': lambda fs, q: fs._over(SpreadSummary, (q.days, q.thresholds), (q.thresholds,)),
    'histogram': lambda fs, q: q.levels and fs._over(SpreadHistogram, (q.days, q.bins, q.edges), (q.bins, q.edges)),
    'arrival': lambda fs, q: q.a_thr and fs._over(ArrivalMaps, (q.a_thr, fs._days), (q.a_thr,)),
    'sensitivity': lambda fs, q: q.s_names and fs._over(SensitivityMaps, (q.s_names, fs._days), (q.s_names,)),
    'dependence': _build_dependence,
    'peak': lambda fs, q: q.pk_thr is not None and _owned_by(
        fs._over(PeakMaps, (q.pk_thr, fs._days), (q.pk_thr,)), PeakPosterior, q.thresholds, q.pk_levels,
        q.bins if q.levels else None, q.edges if q.levels else None),
    'excursion': lambda fs, q: q.ex_thr and fs._over(ExcursionMaps, (q.ex_thr, fs._days), (q.ex_thr,)),
    'core_range': lambda fs, q: q.cr_frac and fs._over(RangeMaps, (q.cr_frac, fs._days), (q.cr_frac,)),
    'reweight': _build_reweight,
    'reweight_histogram': _build_reweight_histogram,
    'reweight_arrival': _build_reweight_arrival,
    'catch': _build_catch,
    'neighbourhood': _build_neighbourhood,
    'proximity': _build_proximity,
    'information': _build_information,
    'mc_error': _build_mc_error,
    'contrast': lambda fs, q: PlanContrast(fs._against, fs._source, q.thresholds),
    'reweight_contrast': _build_reweight_contrast,
    'ranking': lambda fs, q: PlanRanking([fs._against] + fs._source.plans, q.thresholds, q.rk_plan['names']),
    'patches': lambda fs, q: q.pt_thr and fs._over(PatchMaps, (q.pt_thr, fs._days, q.pt_conn), (q.pt_thr, q.pt_conn)),
    'pathways': lambda fs, q: q.pw_thr and fs._over(PathwayMaps, (q.pw_thr, q.pw_days or fs._days, q.pw_conn),
                                                   (q.pw_thr, q.pw_conn)),
    'modes': _build_modes,
    'origin': _build_origin,
    'weather': _build_weather,
}


class _FieldSet():
    '''The accumulators posterior_predictive feeds from one source of fields -- the model's day fields, a Projection
    or a ReleaseSites -- for one chain: one attribute per name of ACCUMULATORS, None where not asked for (`mc_error`:
    while the chains run the chain's two sequences).  `fed_from` names the source, `build` constructs what the
    request asks for, `feed` adds one member in FEED_ORDER, `merge` takes another chain's set, `close` closes the
    accumulators and `release` the source.'''

    def __init__(self, **accumulators):
        for name in ACCUMULATORS:
            setattr(self, name, accumulators.get(name))
        self.plan = None
        self.representative = None     # the RepresentativeMembers over `excursion`, built once the chains are merged
        self.reweight_excursion = None # {scenario: ReweightedExcursion} over `excursion`, likewise
        self._rw_lam = None            # per member of `excursion` (of `contrast`) the run's log-weights, where those are built
        self._kind = self._name = self._source = self._against = self._days = self._half = self._rw_feed = None
        self._chain = self._late = None
        self._owns = False
        self._traps = {}

    def fed_from(self, kind, source, name=None, owns=True, against=None, **traps):
        '''kind: a key of FEED_ORDER; name: the driver's name of the source (default: the kind); owns: release()
        closes the source; against: plan A of a 'compare' or 'ranking' set; traps: per 'catch' / 'information' / 'neighbourhood' /
        'proximity' the arguments of its fields after the source, None for none'''
        self._kind, self._name, self._source, self._owns = kind, name or kind, source, owns
        self._against, self._traps = against, traps
        return self

    def _source_pitch(self):
        '''the cells of one slot of an accumulator over this set's source, padded as the device pads them'''
        pm = self._source if self._kind == 'days' else self._source.pm
        n = (2 * int(pm.rad_res) + 1) ** 2
        return (n + 63) // 64 * 64

    def _over(self, cls, day_args, out_args):
        '''cls over this set's source: the model's day fields or, for_projection, a source's outputs'''
        if self._kind == 'days':
            return cls(self._source, *day_args)
        return cls.for_projection(self._source, *out_args)

    def build(self, q, chain, nruns):
        '''every accumulator of this kind of source that the request q asks for, for chain `chain` of nruns runs;
        what is built is on the set at once, so that close() finds it whatever fails later'''
        self._chain = chain
        self._half = q.mc_halves[chain][0] if q.mc_b else None
        for name in FEED_ORDER[self._kind]:
            if name == 'apply':
                continue
            acc = BUILD[name](self, q) or None
            setattr(self, name, acc)
            if name == 'summary' and self._kind == 'days':
                self._days = acc.days
            if name in ('excursion', 'core_range', 'patches', 'pathways', 'origin') and acc is not None:
                acc.reserve(nruns)
            if name == 'modes' and acc is not None:
                _reserve_modes(acc, nruns)
        if ('excursion' in _reweight_maps(q) and self.excursion is not None) or self.reweight_contrast is not None:
            self._rw_lam = []
        return self

    def feed(self, m):
        for name in FEED_ORDER[self._kind]:
            acc = getattr(self, name, None)
            if acc is not None or name == 'apply':
                FEED[name](acc, self, m)
        if self._rw_lam is not None:     # the excursion maps (the contrast) have taken the member: its log-weights, in add order
            self._rw_lam.append([float(v) for v in m.lam])

    def merge(self, other):
        for name in ACCUMULATORS:
            mine, theirs = getattr(self, name), getattr(other, name)
            # the Monte Carlo error sequences are pooled (_merge_chains), as are a catch's own, not merged
            if name != 'mc_error' and mine is not None and theirs is not None:
                mine.merge(theirs)
        if self._rw_lam is not None and other._rw_lam is not None:      # as the excursion maps' members
            self._rw_lam.extend(other._rw_lam)

    def close(self):
        if self.representative is not None:    # it reads the excursion maps: first
            self.representative.close()
        for name in ACCUMULATORS:
            acc = getattr(self, name)
            for a in (acc if isinstance(acc, (list, tuple)) else [acc]):
                if a is not None:
                    a.close()

    def release(self):
        '''close the source, where it is this set's: the accumulators hold what they need'''
        if self._owns and self._source is not None:
            self._source.close()
        self._source = self._against = None


def _pool_halves(owners):
    '''the Monte Carlo error sequences of every chain's owner (a _FieldSet or a posterior of its own) pooled in chain order
    into the first's `mc_error` (pool_mc_error, which closes the others)'''
    if owners[0].mc_error is not None:
        pooled = pool_mc_error([o.mc_error for o in owners])
        for o in owners:
            o.mc_error = None
        owners[0].mc_error = pooled


def _merge_chains(sets):
    '''one source's sets, one per chain, merged in chain order into the first, which is returned; the others'
    accumulators are closed.  The sources stay open: a catch reads its source's fields, a contrast both plans'.'''
    first = sets[0]
    _pool_halves(sets)
    for own in ('catch', 'neighbourhood', 'proximity'):
        if getattr(first, own) is not None:
            _pool_halves([getattr(fs, own) for fs in sets])
            # the accumulators hold what they need; an information's fields hold its maps
            getattr(first, own).fields.close()
    for other in sets[1:]:
        first.merge(other)
        other.close()
    return first


class ProjectedMaps(_FieldSet):
    '''The posterior of one projection, as posterior_predictive returns it: `weights` [nout, nin], `in_days`,
    `labels` (one per output), `summary` (SpreadSummary.for_projection) and `histogram`
    (SpreadHistogram.for_projection, None without quantile levels); both take the output index.  Of a release
    plan (`posterior_predictive(sites=...)`): `weights` and `in_days` are None, `labels` are the output days,
    `plan` is ReleaseSites.describe() and `arrival` the ArrivalMaps.for_projection (None without arrival
    thresholds), whose accessors take the output day.  `sensitivity`: the SensitivityMaps.for_projection (None
    unless asked for), which takes the output index.  `dependence`: the DependenceMaps.for_projection (None unless
    asked for), likewise.  `mc_error`: the MonteCarloError.for_projection pooled over
    all chains, with `rhat` (None unless asked for; while the chains run, one chain's two sequences), which takes
    the output index.  `peak`: the PeakPosterior of a release plan's outputs (None unless asked for), whose maps
    take the output day.  `excursion`: the ExcursionMaps.for_projection of a release plan's outputs (None unless
    asked for), whose maps take the output day.  `reweight`: the
    ReweightedSummary.for_projection (None unless asked for), which takes the scenario's name and the output index.
    `reweight_histogram` / `reweight_arrival`: the ReweightedHistogram.for_projection and, of a release plan, the
    ReweightedArrival.for_projection (None unless reweight's maps option asks for them).
    `catch`: the CatchPosterior over the outputs (None unless asked for), whose traps name an output label.
    `neighbourhood`: the NeighbourhoodPosterior over a release plan's outputs (None unless asked for), whose windows
    name an output day.  `proximity`: the ProximityPosterior over a release plan's outputs (None unless asked for),
    likewise.
    `information`: the InformationPosterior over the outputs (None unless asked for), likewise.  `core_range`: the
    RangeMaps.for_projection of a release plan's outputs (None unless asked for), whose maps take the output day.
    `patches`: the PatchMaps.for_projection of a release plan's outputs (None unless asked for), likewise.
    `pathways`: the PathwayMaps.for_projection of a release plan's outputs (None unless asked for), its anchors the
    cells of the plan's sites.
    `representative`: the RepresentativeMembers over a release plan's `excursion` (None unless asked for).
    `merge` and `close` take every accumulator there is (ACCUMULATORS).'''

    def __init__(self, weights, in_days, labels, summary, histogram=None, arrival=None, plan=None,
                 sensitivity=None, mc_error=None, peak=None, excursion=None, reweight=None, catch=None,
                 information=None, core_range=None, patches=None, neighbourhood=None, dependence=None,
                 proximity=None, reweight_histogram=None, reweight_arrival=None):
        super().__init__(summary=summary, histogram=histogram, arrival=arrival, sensitivity=sensitivity,
                         dependence=dependence, reweight_histogram=reweight_histogram,
                         reweight_arrival=reweight_arrival,
                         mc_error=mc_error, peak=peak, excursion=excursion, reweight=reweight, catch=catch,
                         information=information, core_range=core_range, patches=patches,
                         neighbourhood=neighbourhood, proximity=proximity)
        self.weights = weights
        self.in_days = in_days
        self.labels = labels
        self.plan = plan


# ------------------------------------------------------------------ release plans
def check_sites(sites, rad_dist, rad_res):
    '''A release plan as a list of dicts, one per site in the order given: east / north (m from the domain
    centre), amount (multiples of the model's r_number, finite and > 0), lag (whole days >= 0 after the first
    release, the smallest 0), and the cell offset by the package's convention (Data_Import.LocInfo):
    dcol = round(east / res), drow = -round(north / res), res = rad_dist / rad_res.  1..32 sites on at most
    8 different release days, every offset inside the domain (|drow|, |dcol| <= 2 rad_res); ValueError
    otherwise.  rad_res=None skips the cells (no model at hand).'''
    try:
        rows = [tuple(s) for s in sites]
    except TypeError:
        raise ValueError('sites must be a list of (east_m, north_m, amount[, lag_days]), got %r' % (sites,))
    if not 1 <= len(rows) <= MAX_SITES:
        raise ValueError('%d release sites; 1..%d fit one plan' % (len(rows), MAX_SITES))
    out = []
    for k, site in enumerate(rows):
        if len(site) not in (3, 4):
            raise ValueError('site %d: (east_m, north_m, amount[, lag_days]) expected, got %r' % (k, site))
        try:
            east, north, amount = (float(v) for v in site[:3])
            lag = site[3] if len(site) == 4 else 0
            if int(lag) != lag:
                raise ValueError
            lag = int(lag)
        except (TypeError, ValueError):
            raise ValueError('site %d: numbers and a whole number of lag days expected, got %r' % (k, site))
        if not (np.isfinite(east) and np.isfinite(north)):
            raise ValueError('site %d: position %r is not finite' % (k, site[:2]))
        if not (np.isfinite(amount) and amount > 0):
            raise ValueError('site %d: amount %r is not finite and > 0' % (k, site[2]))
        if lag < 0:
            raise ValueError('site %d: lag %d is negative' % (k, lag))
        rec = {'east': east, 'north': north, 'amount': amount, 'lag': lag}
        if rad_res is not None:
            res = float(rad_dist) / int(rad_res)
            rec['dcol'] = int(np.around(east / res))
            rec['drow'] = -int(np.around(north / res))
            if max(abs(rec['drow']), abs(rec['dcol'])) > 2 * int(rad_res):
                raise ValueError('site %d: offset (%d, %d) cells lies beyond the %d x %d domain'
                                 % (k, rec['drow'], rec['dcol'], 2 * int(rad_res) + 1, 2 * int(rad_res) + 1))
        out.append(rec)
    lags = sorted({r['lag'] for r in out})
    if lags[0] != 0:
        raise ValueError('the first release defines day 0: the smallest lag must be 0, got %d' % lags[0])
    if len(lags) > MAX_SITE_GROUPS:
        raise ValueError('%d different release days; at most %d fit one plan' % (len(lags), MAX_SITE_GROUPS))
    return out


def site_groups(sites):
    '''[(lag, [site index, ...]), ...] of a checked plan: ascending lag, the sites of a lag in the order given'''
    return [(lag, [k for k, s in enumerate(sites) if s['lag'] == lag]) for lag in sorted({s['lag'] for s in sites})]


def check_site_days(days, ndays=None):
    '''a plan's output days as a list of ints: 1..32 model days >= 0 counted from the first release, strictly
    increasing, within the model's ndays days if given; ValueError otherwise'''
    try:
        d = [int(x) for x in days]
    except (TypeError, ValueError):
        raise ValueError('release-plan days must be model days, got %r' % (days,))
    if not 1 <= len(d) <= MAX_SITE_OUT:
        raise ValueError('%d release-plan output days; 1..%d fit one plan' % (len(d), MAX_SITE_OUT))
    if d[0] < 0 or any(b <= a for a, b in zip(d, d[1:])):
        raise ValueError('release-plan days must be model days >= 0, strictly increasing: %r' % (d,))
    if ndays is not None and d[-1] >= ndays:
        raise ValueError('the model has %d days; the release plan asks for day %d' % (ndays, d[-1]))
    return d


def site_slots(lags, days):
    '''per lag the model day of that release's own model behind every output day: D - lag, None (PS_REC_NONE)
    while D < lag -- the group is not released yet.  ValueError for a lag after the last output day.'''
    for lag in lags:
        if lag > days[-1]:
            raise ValueError('a release %d days after the first lies beyond the last output day %d' % (lag, days[-1]))
    return [[D - lag if D >= lag else None for D in days] for lag in lags]


def check_lagged(pop_model, lags, lagged):
    '''the models of the later release days, {lag: PopModel} for every non-zero lag: each runs over
    pop_model.days[lag:] with the same domain, r_number, prob_model and device; ValueError otherwise'''
    lagged = dict(lagged or {})
    for lag in lags:
        if lag == 0:
            continue
        if lag >= len(pop_model.days):
            raise ValueError('a release %d days after the first lies beyond the model\'s %d days'
                             % (lag, len(pop_model.days)))
        if lag not in lagged:
            raise ValueError('no model for the release %d days after the first (lagged[%d])' % (lag, lag))
        m = lagged[lag]
        if list(m.days) != list(pop_model.days[lag:]):
            raise ValueError('lagged[%d] runs over the days %r, not over the base model\'s days[%d:] = %r'
                             % (lag, list(m.days), lag, list(pop_model.days[lag:])))
        for name in ('rad_dist', 'rad_res', 'r_number', 'prob_model', 'device'):
            if getattr(m, name) != getattr(pop_model, name):
                raise ValueError('lagged[%d].%s = %r, the base model has %r'
                                 % (lag, name, getattr(m, name), getattr(pop_model, name)))
    return {lag: lagged[lag] for lag in lags if lag != 0}


def lagged_models(pop_model, lags, wind_data=None):
    '''{lag: PopModel} for every non-zero lag: a model over pop_model.days[lag:] -- the release that starts
    `lag` days later sees the later days' wind -- with the base model's settings.  wind_data: the dict the
    base model was built from (default: the one it kept).'''
    from .pop_model import PopModel
    wd = pop_model.wind_data if wind_data is None else wind_data
    out = {}
    for lag in sorted({int(x) for x in lags} - {0}):
        if not 0 < lag < len(pop_model.days):
            raise ValueError('a release %d days after the first lies beyond the model\'s %d days'
                             % (lag, len(pop_model.days)))
        out[lag] = PopModel(wd, pop_model.days[lag:], domain_info=(pop_model.rad_dist, pop_model.rad_res),
                            r_number=pop_model.r_number, r_start=pop_model.r_start, mode=pop_model.mode,
                            device=pop_model.device, max_solvers=pop_model._max_solvers,
                            prob_model=pop_model.prob_model)
    return out


def sites_plan(arg, pop_model=None):
    '''posterior_predictive's sites= argument, dict(sites=[(east_m, north_m, amount[, lag_days]), ...],
    days=None), as (sites, days, lags): the checked sites (check_sites), the output days (check_site_days, None:
    all the model's days) and the release days.  With a model at hand the cells, and the days and lags against
    the model's days, are checked too.  ValueError for a bad plan.'''
    if not isinstance(arg, dict) or 'sites' not in arg or set(arg) - {'sites', 'days'}:
        raise ValueError('sites must be dict(sites=[(east_m, north_m, amount[, lag_days]), ...], days=None), got %r'
                         % (arg,))
    have = pop_model is not None
    sites = check_sites(arg['sites'], pop_model.rad_dist if have else None, pop_model.rad_res if have else None)
    lags = [lag for lag, _k in site_groups(sites)]
    ndays = len(pop_model.days) if have else None
    if have and lags[-1] >= ndays:
        raise ValueError('a release %d days after the first lies beyond the model\'s %d days' % (lags[-1], ndays))
    days = arg.get('days')
    if days is None and have:
        days = range(ndays)
    if days is not None:
        days = check_site_days(days, ndays)
        site_slots(lags, days)
    return sites, days, lags


class ReleaseSites(_FieldSource):
    '''The field of a whole release plan, member by member, on the device: Y_e = sum over the sites of
    amount * (the field of that site's release on output day days[e], translated to the site).  sites:
    [(east_m, north_m, amount[, lag_days=0]), ...] (check_sites); days: output model days counted from the first
    release (check_site_days, default all); lagged: {lag: PopModel} for every non-zero lag (check_lagged,
    lagged_models).  One wind station and a homogeneous landscape make the translation exact; what left the
    single-release domain is lost, so near its own far edge a far-off-centre site gives a lower bound; values
    are thresholded (1e-8) per site before the sum.  Groups run in ascending lag and sites in the order
    given, acc = acc + amount * v with the product and the sum rounded separately: a numpy loop reproduces
    every bit.  Every output carries weight (`live`), so SpreadSummary.for_projection,
    SpreadHistogram.for_projection and ArrivalMaps.for_projection accept a plan.'''
    fields_kind = 'sites'        # the accumulators' entry points for these fields: ps_*_add_sites
    _prefix, _info_n = 'ps_sites', 5
    _owned = ()                  # the lagged models with_lagged_models built: closed with the plan

    def __init__(self, pop_model, sites, days=None, lagged=None):
        self.sites = check_sites(sites, pop_model.rad_dist, pop_model.rad_res)
        self.days = check_site_days(range(len(pop_model.days)) if days is None else days, len(pop_model.days))
        self.groups = site_groups(self.sites)
        self.lags = [lag for lag, _k in self.groups]
        self.slots = site_slots(self.lags, self.days)
        self.lagged = check_lagged(pop_model, self.lags, lagged)
        self.nout = len(self.days)
        self.live = list(range(self.nout))
        self._attach(pop_model)
        self.nbytes = self.nout * self.pitch * 8            # the output fields
        order = [k for _lag, ks in self.groups for k in ks]
        nsite = L.i32([len(ks) for _lag, ks in self.groups])
        drow = L.i32([self.sites[k]['drow'] for k in order])
        dcol = L.i32([self.sites[k]['dcol'] for k in order])
        amount = L.f64([self.sites[k]['amount'] for k in order])
        self._create(self.nout, len(self.groups), L.p_i32(nsite), L.p_i32(drow), L.p_i32(dcol), L.p_f64(amount))

    @classmethod
    def with_lagged_models(cls, pop_model, sites, days=None, wind_data=None):
        '''the plan with the models of its later release days built here (lagged_models); `close()` closes
        them too'''
        lags = [lag for lag, _k in site_groups(check_sites(sites, pop_model.rad_dist, pop_model.rad_res))]
        check_site_days(range(len(pop_model.days)) if days is None else days, len(pop_model.days))
        made = lagged_models(pop_model, lags, wind_data)
        try:
            self = cls(pop_model, sites, days, made)
        except Exception:
            for m in made.values():
                m.close()
            raise
        self._owned = list(made.values())
        return self

    def models(self):
        '''[(lag, model), ...] in group order'''
        return [(lag, self.pm if lag == 0 else self.lagged[lag]) for lag in self.lags]

    def evaluate_lagged(self, *model_args):
        '''evaluate the model of every later release day over the days the outputs need, enqueued only'''
        for lag, m in self.models():
            if lag:
                m.evaluate(*model_args, ndays=self.days[-1] - lag + 1, want_stats=False)

    def evaluate(self, *model_args):
        '''evaluate the base model over all its days and every later release's model over the days the
        outputs need, enqueued only (want_stats=False), then apply()'''
        self.pm.evaluate(*model_args, want_stats=False)
        self.evaluate_lagged(*model_args)
        self.apply()

    def apply(self):
        '''Superpose the last evaluations of the plan's models, group by group in ascending lag (each
        enqueued on its solver's stream; no host synchronisation); the outputs of the previous apply are
        overwritten.'''
        for call in self._calls():                             # every model checked before the first launch
            self._call('apply', *call)

    def _calls(self):
        '''the arguments of ps_sites_apply behind the handle, group by group, from each model's last evaluation'''
        calls = []
        for g, (lag, m) in enumerate(self.models()):
            md = self.slots[g]
            _check_evaluated(m, [d for d in md if d is not None], 'release plan (lag %d)' % lag)
            days = [0 if d is None else d for d in md]
            kind, idx, delta = _day_slots(days)
            kind[np.array([d is None for d in md], dtype=bool)] = L.REC_NONE
            stat, post = _day_scales(m, days)
            calls.append((m.solver._h, g, self.nout, L.p_i32(kind), L.p_i32(idx), L.p_f64(stat), L.p_f64(post),
                          L.p_i32(delta), NEGVAL))                 # the pointers keep their arrays alive
        return calls

    def describe(self):
        '''the plan for a result file: sites in metres and cells, release days, output days'''
        return {'sites': [dict(s) for s in self.sites], 'lags': list(self.lags), 'days': list(self.days)}

    def close(self):
        super().close()
        for m in self._owned:
            m.close()
        self._owned = []


# ------------------------------------------------------------------ paired contrast of two plans
MAX_CONTRAST_THRESHOLDS = 4


def check_contrast_thresholds(thresholds):
    '''a contrast's thresholds as a list of floats: 0..4 of them, each finite and > 0, strictly increasing;
    ValueError otherwise'''
    try:
        thr = [float(t) for t in thresholds]
    except (TypeError, ValueError):
        raise ValueError('contrast thresholds must be numbers, got %r' % (thresholds,))
    if len(thr) > MAX_CONTRAST_THRESHOLDS:
        raise ValueError('%d contrast thresholds; at most %d are kept' % (len(thr), MAX_CONTRAST_THRESHOLDS))
    if not all(np.isfinite(t) and t > 0 for t in thr):
        raise ValueError('every contrast threshold must be finite and > 0: %r' % (thr,))
    if any(b <= a for a, b in zip(thr, thr[1:])):
        raise ValueError('contrast thresholds must be strictly increasing: %r' % (thr,))
    return thr


def coverage_difference(cells_a, cells_b, weights, cell_area, levels=(0.05, 0.5, 0.95)):
    '''Per output the posterior of the difference of the areas two plans cover, from the paired per-member cell
    counts cells_a, cells_b [members, nout] and the members' integer weights: [{'mean', 'quantiles',
    'p_a_larger', 'p_b_larger'}, ...].  Areas in m^2 (cells x cell_area), signed A - B: the weighted mean (from
    integers, as ArrivalMaps.reached_area), the weighted lower quantiles (weighted_lower_quantile) at `levels`,
    and the weight of the members with a > b (b > a) over W.  ValueError at W = 0.'''
    levels = check_levels(levels)
    a = np.asarray(cells_a, dtype=np.int64)
    b = np.asarray(cells_b, dtype=np.int64)
    w = np.asarray(weights, dtype=np.int64).ravel()
    if a.ndim != 2 or a.shape != b.shape or a.shape[0] != w.size:
        raise ValueError('cell counts %r and %r with %d weights' % (a.shape, b.shape, w.size))
    if w.size and w.min() < 0:
        raise ValueError('weights must be >= 0')
    W = int(w.sum())
    if W == 0:
        raise ValueError('nothing accumulated')
    out = []
    for s in range(a.shape[1]):
        d = a[:, s] - b[:, s]
        out.append({'mean': float(int((d * w).sum())) / float(W) * float(cell_area),
                    'quantiles': [float(weighted_lower_quantile(d, w, p)) * float(cell_area) for p in levels],
                    'p_a_larger': float(int(w[d > 0].sum())) / float(W),
                    'p_b_larger': float(int(w[d < 0].sum())) / float(W)})
    return out


def contrast_plan(arg, sites_arg, pop_model=None):
    '''posterior_predictive's compare= argument, dict(sites=[(east_m, north_m, amount[, lag_days]), ...]): plan B,
    compared with the plan A of the sites= argument `sites_arg` on A's output days, as (sites, days, lags) of B
    (sites_plan).  ValueError for a bad plan, for a compare= without sites=, or for output days of its own.'''
    if not isinstance(arg, dict) or 'sites' not in arg or set(arg) - {'sites'}:
        raise ValueError('compare must be dict(sites=[(east_m, north_m, amount[, lag_days]), ...]), got %r' % (arg,))
    if sites_arg is None:
        raise ValueError('compare= names plan B and needs plan A: give sites= too')
    a_sites, a_days, _lags = sites_plan(sites_arg, pop_model)
    return sites_plan(dict(sites=arg['sites'], days=a_days), pop_model)


def _check_paired(a, b):
    '''what a paired accumulator asks of its two sources: two ReleaseSites or two Projection, not the same one, on
    the same device and domain with the same outputs (of two ReleaseSites also the same output days)'''
    if a is b:
        raise ValueError('a plan is compared with another one, not with itself')
    if type(a) is not type(b) or not isinstance(a, (ReleaseSites, Projection)):
        raise ValueError('two ReleaseSites or two Projection expected, got %s and %s'
                         % (type(a).__name__, type(b).__name__))
    if a.pm.device != b.pm.device:
        raise ValueError('the plans\' models are on devices %r and %r' % (a.pm.device, b.pm.device))
    for name in ('device', 'N', 'nout', 'live') + (('days',) if isinstance(a, ReleaseSites) else ()):
        if getattr(a, name) != getattr(b, name):
            raise ValueError('the plans differ in %s: %r and %r' % (name, getattr(a, name), getattr(b, name)))


class PlanContrast(_Accumulator):
    '''The posterior of the difference of two plans, member by member, on the device: `a` and `b` are two
    ReleaseSites or two Projection on the same device and domain with the same outputs (nout, live; of two
    ReleaseSites also the same output days -- outputs are paired by index and labelled by A's days; of two
    Projection the caller sees to it that output e means the same in both).
    After both were applied to one member, `add(weight)` accumulates per output and cell d = a - b (one rounded
    subtraction): its weighted mean and M2 by SpreadSummary's step, the weight of the members with d > 0 and
    with d < 0, per threshold t_k (0..4, finite, > 0, strictly increasing) the weight of those with
    a >= t_k > b (gain) and b >= t_k > a (loss), and per member the cells either plan covers at t_k on every
    output -- the pairing the two plans' own maps have lost.  The accessors take the output index; outputs
    kept off the device read as zeros.  Counts are integers: the order of adds and merges changes no bit.'''

    _prefix = 'ps_contrast'

    def __init__(self, a, b, thresholds=()):
        _check_paired(a, b)
        self.thresholds = check_contrast_thresholds(thresholds)
        self.a, self.b = a, b
        self._attach(a.pm)
        self.device, self.nout, self.live = a.device, a.nout, list(a.live)
        self.labels = list(getattr(a, 'days', range(a.nout)))
        self._slot = {e: i for i, e in enumerate(self.live)}
        self.nbytes = len(self.live) * self.pitch * (16 + 4 * (2 + 2 * len(self.thresholds)))   # moments and counts
        thr = L.f64(self.thresholds if self.thresholds else [0.0])
        self._create(len(self.live), len(self.thresholds), L.p_f64(thr))

    def add(self, weight=1):
        '''Accumulate the last apply of both plans with integer weight >= 1 (on the handle's stream behind both;
        no host synchronisation)'''
        self._from_fields('add', self.a, self.b._h, self._weight(weight))

    def merge(self, other):
        '''self += other (same device, domain, outputs and thresholds); other's members follow self's'''
        if other.live != self.live or other.nout != self.nout or list(other.labels) != self.labels:
            raise ValueError('contrasts over different outputs')
        self._call('merge', other._h)

    def _fetch(self, e, what):
        e = self._e(e)
        if e not in self._slot:
            return np.zeros((self.N, self.N), dtype=np.float64)
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('fetch', self._slot[e], int(what), L.p_f64(out))
        return out

    def mean(self, e):
        '''[N, N] float64: the posterior mean of A - B on output e'''
        return self._fetch(e, 0)

    def variance(self, e):
        return self._fetch(e, 1)

    def sd(self, e):
        return np.sqrt(self.variance(e))

    def prob_positive(self, e):
        '''P(A > B) per cell'''
        return self._fetch(e, 2)

    def prob_negative(self, e):
        '''P(A < B) per cell'''
        return self._fetch(e, 3)

    def gain(self, e, k):
        '''P(A >= thresholds[k] > B) per cell: plan A reaches the threshold where plan B does not'''
        return self._fetch(e, 4 + 2 * self._k(k))

    def loss(self, e, k):
        '''P(B >= thresholds[k] > A) per cell'''
        return self._fetch(e, 5 + 2 * self._k(k))

    def counts(self, e, which):
        '''[N, N] uint32: the raw count plane (0 d > 0, 1 d < 0, 2 + 2k gain_k, 3 + 2k loss_k) of output e'''
        e = self._e(e)
        if not 0 <= int(which) < 2 + 2 * len(self.thresholds):
            raise ValueError('count plane %r of %d' % (which, 2 + 2 * len(self.thresholds)))
        if e not in self._slot:
            return np.zeros((self.N, self.N), dtype=np.uint32)
        out = np.empty((self.N, self.N), dtype=np.uint32)
        self._call('fetch_counts', self._slot[e], int(which), out.ctypes.data_as(C.POINTER(C.c_uint32)))
        return out

    def _coverage(self):
        m = self.members
        cells = np.zeros((m, 2, len(self.thresholds), len(self.live)), dtype=np.uint32)
        w = np.zeros(m, dtype=np.uint32)
        u32 = C.POINTER(C.c_uint32)
        self._call('fetch_coverage', 0, m, cells.ctypes.data_as(u32), w.ctypes.data_as(u32))
        return cells, w

    @property
    def weights(self):
        '''[members] int64: the members' weights in add order'''
        return self._coverage()[1].astype(np.int64)

    def coverage(self, k):
        '''(cells_a [members, nout] int64, cells_b, weights [members] int64): per member in add order the number
        of cells where plan A (plan B) is >= thresholds[k] on every output'''
        k = self._k(k)
        cells, w = self._coverage()
        out = np.zeros((2, cells.shape[0], self.nout), dtype=np.int64)
        out[:, :, self.live] = cells[:, :, k, :].transpose(1, 0, 2)
        return out[0], out[1], w.astype(np.int64)

    def coverage_difference(self, k, levels=(0.05, 0.5, 0.95)):
        '''Per output the posterior of the covered area of A minus that of B at thresholds[k]
        (coverage_difference of the paired rows), each entry with its output `label`'''
        ca, cb, w = self.coverage(k)
        out = coverage_difference(ca, cb, w, self.cell_area, levels)
        for label, rec in zip(self.labels, out):
            rec['label'] = label
        return out

    def profile(self, enable=None):
        '''HIP-event time of the add launches: (total ms, adds); enable switches it'''
        return self._profile(enable)


# ------------------------------------------------------------------ ranking of several named plans
MIN_RANKED_PLANS = 2
MAX_RANKED_PLANS = 8       # ps_rank: the plans of one handle, plan A of sites= among them


def coverage_ranking(cells, weights, cell_area, levels=(0.05, 0.5, 0.95)):
    '''Per output the posterior of the areas P plans cover and of their order, from the joint per-member cell
    counts cells [members, P, nout] and the members' integer weights: [{'plans': [{'mean', 'quantiles', 'p_most',
    'mean_rank', 'mean_shortfall'}, ... one per plan], 'p_tied'}, ... one per output].  Areas in m^2 (cells x
    cell_area).  mean: the weighted mean area (from integer sums with one division, as ArrivalMaps.reached_area);
    quantiles: its weighted lower quantiles (weighted_lower_quantile) at `levels`; p_most: the weight of the
    members in which the plan covers strictly the most, over W; mean_rank: the weighted mean mid-rank, 1 the
    largest area, tied plans sharing the average of their ranks; mean_shortfall: the weighted mean of (the
    member's largest count - the plan's) x cell_area; p_tied: the weight of the members whose largest area is
    shared, over W.  Everything is computed from integers.  ValueError at W = 0.'''
    levels = check_levels(levels)
    c = np.asarray(cells, dtype=np.int64)
    w = np.asarray(weights, dtype=np.int64).ravel()
    if c.ndim != 3 or c.shape[1] < 1 or c.shape[0] != w.size:
        raise ValueError('cell counts %r with %d weights' % (c.shape, w.size))
    if w.size and w.min() < 0:
        raise ValueError('weights must be >= 0')
    W = int(w.sum())
    if W == 0:
        raise ValueError('nothing accumulated')
    area = float(cell_area)
    out = []
    for s in range(c.shape[2]):
        x = c[:, :, s]                                       # [members, P]
        top = x.max(axis=1)
        ntop = (x == top[:, None]).sum(axis=1)
        plans = []
        for j in range(x.shape[1]):
            xj = x[:, j]
            rank2 = 2 * (x > xj[:, None]).sum(axis=1) + (x == xj[:, None]).sum(axis=1) + 1     # twice the mid-rank
            plans.append({'mean': float(int((xj * w).sum())) / float(W) * area,
                          'quantiles': [float(weighted_lower_quantile(xj, w, p)) * area for p in levels],
                          'p_most': float(int(w[(xj == top) & (ntop == 1)].sum())) / float(W),
                          'mean_rank': float(int((rank2 * w).sum())) / float(2 * W),
                          'mean_shortfall': float(int(((top - xj) * w).sum())) / float(W) * area})
        out.append({'plans': plans, 'p_tied': float(int(w[ntop > 1].sum())) / float(W)})
    return out


def ranking_plan(arg, sites_arg, pop_model=None):
    '''posterior_predictive's ranking= argument, dict(plans=[dict(sites=[(east_m, north_m, amount[, lag_days]),
    ...]), ...], names=None, levels=(0.05, 0.5, 0.95)) or the bare list of plans: 1..7 further plans, ranked with
    the plan A of the sites= argument `sites_arg` (plan 0) on A's output days -> dict(plans=[(sites, days, lags),
    ...] of the further plans (sites_plan), names=[...] of all plans, A's first (default 'plan0', 'plan1', ...),
    levels=[...]).  ValueError, in this order, for: an argument of another shape; a ranking= without sites=; fewer
    than 1 or more than 7 plans; a plan that is no dict(sites=[...]) -- output days of its own among that; bad
    names (not one string per plan, A included, or a name twice); bad levels; a bad plan A; a bad further plan
    (its number in the message).'''
    shape = ('ranking must be dict(plans=[dict(sites=[(east_m, north_m, amount[, lag_days]), ...]), ...], names=None, '
             'levels=(0.05, 0.5, 0.95)) or the list of plans, got %r' % (arg,))
    if isinstance(arg, (list, tuple)):
        arg = dict(plans=list(arg))
    if not isinstance(arg, dict) or 'plans' not in arg or set(arg) - {'plans', 'names', 'levels'} \
            or not isinstance(arg['plans'], (list, tuple)):
        raise ValueError(shape)
    if sites_arg is None:
        raise ValueError('ranking= names further plans and needs plan A: give sites= too')
    plans = list(arg['plans'])
    if not 1 <= len(plans) <= MAX_RANKED_PLANS - 1:
        raise ValueError('%d further plans; 1..%d are ranked with plan A' % (len(plans), MAX_RANKED_PLANS - 1))
    for j, p in enumerate(plans):
        if not isinstance(p, dict) or 'sites' not in p or set(p) - {'sites'}:
            raise ValueError('ranking: plan %d must be dict(sites=[(east_m, north_m, amount[, lag_days]), ...]) -- '
                             'every plan is ranked on plan A\'s output days -- got %r' % (j + 1, p))
    names = arg.get('names')
    if names is None:
        names = ['plan%d' % j for j in range(len(plans) + 1)]
    else:
        if isinstance(names, str) or not isinstance(names, (list, tuple)) or len(names) != len(plans) + 1 \
                or not all(isinstance(n, str) and n for n in names):
            raise ValueError('ranking: names must be %d non-empty strings, plan A\'s first, got %r'
                             % (len(plans) + 1, names))
        names = list(names)
        if len(set(names)) != len(names):
            raise ValueError('ranking: plan names listed twice: %r' % (names,))
    levels = check_levels(arg.get('levels', (0.05, 0.5, 0.95)))
    _a_sites, a_days, _lags = sites_plan(sites_arg, pop_model)
    checked = []
    for j, p in enumerate(plans):
        try:
            checked.append(sites_plan(dict(sites=p['sites'], days=a_days), pop_model))
        except ValueError as e:
            raise ValueError('ranking: plan %d: %s' % (j + 1, e))
    return dict(plans=checked, names=names, levels=list(levels))


class _RankedPlans():
    '''the further plans of a ranking as one source of the driver: apply() applies each in order, close() closes
    them'''

    def __init__(self):
        self.plans = []

    def apply(self):
        for p in self.plans:
            p.apply()

    def describe(self):
        return [p.describe() for p in self.plans]

    def close(self):
        for p in self.plans:
            p.close()


class PlanRanking(_Accumulator):
    '''The posterior of the order of several named plans, member by member, on the device: `plans` are 2..8
    different ReleaseSites or 2..8 different Projection on the same device and domain with the same outputs (nout,
    live; of ReleaseSites also the same output days -- outputs are paired by index and labelled by the first
    plan's days; of Projection the caller sees to it that output e means the same in all).  After all were
    applied to one member, `add(weight)` accumulates per output and cell, with a_j the value of plan j and
    m = max_j a_j: the weight of the members in which plan j alone holds m (`prob_best`; a tie, the zeros of most
    of the domain among them, counts for nobody: `prob_undecided`), the weighted mean and M2 of the regret
    r_j = m - a_j (one rounded subtraction) by SpreadSummary's step, per threshold t_k (0..4, finite, > 0, strictly
    increasing) the weight of those in which plan j alone reaches t_k (`sole`), some plan does (`any`) and every
    plan does (`all`), and per member the cells every plan covers at t_k on every output (`coverage`,
    `coverage_ranking`) -- joint statements over the plans inside one member, which no set of pairwise contrasts
    holds.  The accessors take the output index and the plan's index; outputs kept off the device read as zeros.
    Counts are integers: the order of adds and merges changes no bit.  The plans are the ones the caller names:
    nothing is searched, proposed or recommended.'''

    _prefix = 'ps_rank'

    def __init__(self, plans, thresholds=(), names=None):
        plans = list(plans)
        if not MIN_RANKED_PLANS <= len(plans) <= MAX_RANKED_PLANS:
            raise ValueError('%d plans; %d..%d are ranked' % (len(plans), MIN_RANKED_PLANS, MAX_RANKED_PLANS))
        a = plans[0]
        if any(type(p) is not type(a) for p in plans) or not isinstance(a, (ReleaseSites, Projection)):
            raise ValueError('ReleaseSites only or Projection only expected, got %s'
                             % ', '.join(type(p).__name__ for p in plans))
        for j, p in enumerate(plans):
            if any(p is o for o in plans[:j]):
                raise ValueError('plan %d is listed twice: a plan is ranked with others, not with itself' % j)
            if p.pm.device != a.pm.device:
                raise ValueError('the plans\' models are on devices %r and %r' % (a.pm.device, p.pm.device))
            for name in ('device', 'N', 'nout', 'live') + (('days',) if isinstance(a, ReleaseSites) else ()):
                if getattr(p, name) != getattr(a, name):
                    raise ValueError('plans 0 and %d differ in %s: %r and %r'
                                     % (j, name, getattr(a, name), getattr(p, name)))
        self.thresholds = check_contrast_thresholds(thresholds)
        if names is None:
            names = ['plan%d' % j for j in range(len(plans))]
        names = [str(n) for n in names]
        if len(names) != len(plans) or len(set(names)) != len(names):
            raise ValueError('%d different names expected, one per plan, got %r' % (len(plans), names))
        self.plans, self.names, self.nplan = plans, names, len(plans)
        self._attach(a.pm)
        self.device, self.nout, self.live = a.device, a.nout, list(a.live)
        self.labels = list(getattr(a, 'days', range(a.nout)))
        self._slot = {e: i for i, e in enumerate(self.live)}
        self.nplanes = self.nplan + len(self.thresholds) * (self.nplan + 2)
        self.nbytes = len(self.live) * self.pitch * (16 * self.nplan + 4 * self.nplanes)    # moments and counts
        thr = L.f64(self.thresholds if self.thresholds else [0.0])
        self._create(self.nplan, len(self.live), len(self.thresholds), L.p_f64(thr))

    def add(self, weight=1):
        '''Accumulate the last apply of every plan with integer weight >= 1 (on the handle's stream behind all of
        them; no host synchronisation)'''
        handles = (L._VP * self.nplan)(*[p._h.value for p in self.plans])
        self._call('add_' + self.plans[0].fields_kind, handles, self.nplan, self._weight(weight))

    def merge(self, other):
        '''self += other (same device, domain, number of plans, outputs and thresholds); other's members follow
        self's'''
        if other.live != self.live or other.nout != self.nout or list(other.labels) != self.labels \
                or other.nplan != self.nplan:
            raise ValueError('rankings over different outputs or numbers of plans')
        self._call('merge', other._h)

    def _j(self, j):
        return self._index(j, self.nplan, 'plan')

    def _fetch(self, e, j, what):
        e, j = self._e(e), self._j(j)
        if e not in self._slot:
            return np.zeros((self.N, self.N), dtype=np.float64)
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('fetch', self._slot[e], j, int(what), L.p_f64(out))
        return out

    def regret(self, e, j):
        '''[N, N] float64: the posterior mean of max_i a_i - a_j on output e -- what choosing plan j gives away
        at a cell against the best of the named plans there'''
        return self._fetch(e, j, 0)

    def regret_variance(self, e, j):
        return self._fetch(e, j, 1)

    def regret_sd(self, e, j):
        return np.sqrt(self.regret_variance(e, j))

    def prob_best(self, e, j):
        '''P(plan j alone holds the largest value) per cell'''
        return self._fetch(e, j, 2)

    def counts(self, e, which):
        '''[N, N] uint32: the raw count plane of output e -- j: best_j; P + k (P + 2) + j: sole_kj, then any_k and
        all_k'''
        e = self._e(e)
        which = self._index(which, self.nplanes, 'count plane')
        if e not in self._slot:
            return np.zeros((self.N, self.N), dtype=np.uint32)
        out = np.empty((self.N, self.N), dtype=np.uint32)
        self._call('fetch_counts', self._slot[e], which, out.ctypes.data_as(C.POINTER(C.c_uint32)))
        return out

    def _share(self, e, which):
        return self.counts(e, which).astype(np.float64) / float(self.total_weight)

    def prob_undecided(self, e):
        '''1 - sum_j best_j / W per cell: the share of the members in which no plan alone is best -- ties, and
        the cells no plan reaches'''
        e = self._e(e)
        best = np.zeros((self.N, self.N), dtype=np.int64)
        for j in range(self.nplan):
            best += self.counts(e, j)
        return 1.0 - best.astype(np.float64) / float(self.total_weight)

    def leader(self, e):
        '''[N, N] int8: the plan with the largest P(best) per cell, among equals the smallest index, -1 where every
        P(best) is 0.  A summary of the posterior in the sense of OriginMaps.mode(), not a recommendation: it says
        which of the named plans is most often alone on top at a cell, nothing about which plan to choose.'''
        e = self._e(e)
        best = np.stack([self.counts(e, j) for j in range(self.nplan)])
        out = np.argmax(best, axis=0).astype(np.int8)
        out[best.max(axis=0) == 0] = -1
        return out

    def _plane(self, k, j):
        return self.nplan + self._k(k) * (self.nplan + 2) + j

    def sole(self, e, k, j):
        '''P(plan j reaches thresholds[k] and no other plan does) per cell: reached only if plan j is chosen'''
        return self._share(e, self._plane(k, self._j(j)))

    def any(self, e, k):
        '''P(some plan reaches thresholds[k]) per cell'''
        return self._share(e, self._plane(k, self.nplan))

    def all(self, e, k):
        '''P(every plan reaches thresholds[k]) per cell: reached whichever plan is chosen'''
        return self._share(e, self._plane(k, self.nplan + 1))

    def _coverage(self):
        m = self.members
        cells = np.zeros((m, self.nplan, len(self.thresholds), len(self.live)), dtype=np.uint32)
        w = np.zeros(m, dtype=np.uint32)
        u32 = C.POINTER(C.c_uint32)
        self._call('fetch_coverage', 0, m, cells.ctypes.data_as(u32), w.ctypes.data_as(u32))
        return cells, w

    @property
    def weights(self):
        '''[members] int64: the members' weights in add order'''
        return self._coverage()[1].astype(np.int64)

    def coverage(self, k):
        '''(cells [members, P, nout] int64, weights [members] int64): per member in add order the number of cells
        where each plan is >= thresholds[k] on every output'''
        k = self._k(k)
        cells, w = self._coverage()
        out = np.zeros((cells.shape[0], self.nplan, self.nout), dtype=np.int64)
        out[:, :, self.live] = cells[:, :, k, :]
        return out, w.astype(np.int64)

    def coverage_ranking(self, k, levels=(0.05, 0.5, 0.95)):
        '''Per output the posterior of the plans' covered areas and of their order at thresholds[k]
        (coverage_ranking of the joint rows), each entry with its output `label` and each plan's with its `name`'''
        cells, w = self.coverage(k)
        out = coverage_ranking(cells, w, self.cell_area, levels)
        for label, rec in zip(self.labels, out):
            rec['label'] = label
            for name, p in zip(self.names, rec['plans']):
                p['name'] = name
        return out

    def profile(self, enable=None):
        '''HIP-event time of the add launches: (total ms, adds); enable switches it'''
        return self._profile(enable)


# ------------------------------------------------------------------ sensitivity
MAX_SENS_PARAMS = 16       # ps_sens: the scalars of one handle


def check_sens_params(params):
    '''posterior_predictive's sensitivity= argument as a list of names from mcmc.MODEL_BLOCK: None or True
    is all of them, in their order; else 1..16 different names; ValueError otherwise'''
    known = [m[0] for m in mcmc.MODEL_BLOCK]
    if params is None or params is True:
        return known
    if isinstance(params, str):
        params = [params]
    try:
        names = [str(n) for n in params]
    except TypeError:
        raise ValueError('sensitivity parameters must be a list of names, got %r' % (params,))
    bad = [n for n in names if n not in known]
    if bad:
        raise ValueError('unknown sensitivity parameters %r; the model parameters are %r' % (bad, known))
    if not 1 <= len(names) <= MAX_SENS_PARAMS:
        raise ValueError('%d sensitivity parameters; 1..%d fit one handle' % (len(names), MAX_SENS_PARAMS))
    if len(set(names)) != len(names):
        raise ValueError('sensitivity parameters listed twice: %r' % (names,))
    return names


class ParamMoments():
    '''Weighted running mean, co-moment matrix and total weight of the scalars `names` (1..16) of the members,
    on the host: the scalar side of ps_sens, whose adds take the vector `update` returns.  The first member sets
    the mean to its scalars exactly, so a scalar that never changes has deviation, variance and co-moments
    exactly 0.'''

    def __init__(self, names):
        self.names = [str(n) for n in names]
        if not 1 <= len(self.names) <= MAX_SENS_PARAMS:
            raise ValueError('%d scalars; 1..%d fit one handle' % (len(self.names), MAX_SENS_PARAMS))
        self.reset()

    def reset(self):
        n = len(self.names)
        self.W = 0
        self.members = 0
        self.m = np.zeros(n)
        self.C = np.zeros((n, n))

    def _state(self):
        return self.W, self.members, self.m.copy(), self.C.copy()

    def _restore(self, state):
        self.W, self.members, self.m, self.C = state

    def update(self, theta, w=1):
        '''One member with integer weight w >= 1 -> e = theta - (the weighted mean after this member), the
        vector its device add needs: Wn = W + w, d = theta - m, m' = m + d w / Wn, e = theta - m',
        C += outer(w d, e).'''
        t = np.array(theta, dtype=np.float64).ravel()
        if t.size != len(self.names):
            raise ValueError('%d scalars given, the moments hold %d' % (t.size, len(self.names)))
        if not np.all(np.isfinite(t)):
            raise ValueError('every scalar must be finite: %r' % (t.tolist(),))
        if int(w) != w or int(w) < 1:
            raise ValueError('weight must be a positive integer')
        w = int(w)
        if self.W + w >= 2 ** 32:
            raise ValueError('total weight %d would reach 2^32' % (self.W + w))
        if self.W == 0:
            m1 = t.copy()
        else:
            d = t - self.m
            m1 = self.m + d * float(w) / float(self.W + w)
        e = t - m1
        if self.W:
            self.C = self.C + np.outer(float(w) * d, e)
        self.m = m1
        self.W += w
        self.members += 1
        return e

    def merge(self, other):
        '''self += other (Chan et al.) -> dtheta = other's means minus self's before the merge, the vector the
        device merge needs'''
        if other.names != self.names:
            raise ValueError('moments of different scalars: %r and %r' % (self.names, other.names))
        if self.W + other.W >= 2 ** 32:
            raise ValueError('total weight %d would reach 2^32' % (self.W + other.W))
        if other.W == 0:
            return np.zeros(len(self.names))
        d = other.m - self.m
        if self.W == 0:
            self.m, self.C = other.m.copy(), other.C.copy()
        else:
            Wa, Wb = float(self.W), float(other.W)
            self.C = self.C + other.C + np.outer(d, d) * (Wa * Wb / (Wa + Wb))
            self.m = self.m + d * (Wb / (Wa + Wb))
        self.W += other.W
        self.members += other.members
        return d

    def mean(self):
        return self.m.copy()

    def cov(self):
        '''the weighted covariance matrix C / W (symmetrised)'''
        if self.W == 0:
            raise ValueError('nothing accumulated')
        return 0.5 * (self.C + self.C.T) / float(self.W)

    def constant(self):
        '''mask of the scalars whose variance is 0'''
        return np.diag(self.C) == 0.0

    def inv_sd(self):
        '''1 / sd per scalar, 0 for a constant one'''
        var = np.diag(self.cov())
        out = np.zeros(len(self.names))
        live = ~self.constant()
        out[live] = 1.0 / np.sqrt(var[live])
        return out

    def corr(self):
        '''the correlation matrix of the scalars; rows and columns of constant ones are 0'''
        isd = self.inv_sd()
        return self.cov() * isd[:, None] * isd[None, :]

    def factor(self):
        '''(F, rank, eigenvalues): F [n, rank] with F F' the pseudo-inverse of the covariance of the
        non-constant scalars (rows of constant ones are 0); the eigenvalues of that covariance in descending
        order, of which those below 1e-12 times the largest -- eigenvalues[rank:] -- are dropped, never
        regularised.'''
        n = len(self.names)
        live = np.flatnonzero(~self.constant())
        if live.size == 0:
            return np.zeros((n, 0)), 0, np.zeros(0)
        lam, V = np.linalg.eigh(self.cov()[np.ix_(live, live)])
        lam, V = lam[::-1], V[:, ::-1]
        rank = int(np.count_nonzero(lam >= 1e-12 * lam[0])) if lam[0] > 0 else 0
        F = np.zeros((n, rank))
        F[live] = V[:, :rank] / np.sqrt(lam[:rank])
        return F, rank, lam


def finalize_factor(moments):
    '''(F, rank, eigenvalues, isd) of ParamMoments for ps_sens_finalize, F and isd contiguous float64.
    ValueError when nothing varies or members < rank + 2: a regression through that few members fits exactly
    and would report explained == 1 everywhere.'''
    if moments.W == 0:
        raise ValueError('nothing accumulated')
    F, rank, lam = moments.factor()
    if rank < 1:
        raise ValueError('no sensitivity parameter varies over the %d members' % moments.members)
    if moments.members < rank + 2:
        raise ValueError('%d members for %d independent parameters: a linear fit through fewer than rank + 2 '
                         'members is exact and explains everything' % (moments.members, rank))
    return L.f64(F), rank, lam, L.f64(moments.inv_sd())


class SensitivityMaps(_Accumulator):
    '''Which parameter drives the posterior spread where: per cell of `pop_model`'s days the weighted
    covariance between the value SpreadSummary adds and each of `params` (names from mcmc.MODEL_BLOCK, default
    all 15) over the members added, on the device (ps_sens_*, csrc/ps_sens.hip), next to the mean and the
    variance (the same bits as a SpreadSummary fed alongside).  `add(theta, weight)` takes the member's full
    model block and picks the columns.  After `finalize()`: `explained(day)`, the share of the cell's
    posterior variance that a linear dependence on the parameters explains -- a linear, global,
    posterior-weighted measure, not a Sobol index, and 1 by construction when members <= rank + 1, which
    `finalize` therefore refuses -- and `dominant(day)`, the parameter with the largest |correlation|.'''

    _prefix, _noun = 'ps_sens', 'sensitivity maps'

    def __init__(self, pop_model, params=None, days=None):
        self._setup(pop_model, params, _model_days(pop_model, days), None)

    @classmethod
    def for_projection(cls, projection, params=None):
        '''Sensitivity maps of the outputs of `projection` (a Projection or a ReleaseSites), one slot per
        output: `add(theta, weight)` accumulates the outputs of its last `apply()`, and the accessors take the
        output index where the day-based maps take a day.'''
        self = cls.__new__(cls)
        self._setup(projection.pm, params, list(range(projection.nout)), projection)
        return self

    def _setup(self, pop_model, params, days, projection):
        self.params = check_sens_params(params)
        known = [m[0] for m in mcmc.MODEL_BLOCK]
        self._cols = [known.index(n) for n in self.params]
        self._nblock = len(known)
        self.moments = ParamMoments(self.params)
        self._attach(pop_model)
        self._set_source(projection, days, projection and projection.live)
        self.nbytes = len(self._slot) * self.pitch * ((len(self.params) + 3) * 8 + 1)
        self.rank = None
        self.eigenvalues = None
        self._create(len(self._slot), len(self.params))

    def add(self, theta, weight=1):
        '''Accumulate the last evaluation of the model (on a projection or a plan: its last apply), whose
        model block is `theta`, with integer weight >= 1; enqueued, no host synchronisation.'''
        t = np.array(theta, dtype=np.float64).ravel()
        if t.size != self._nblock:
            raise ValueError('theta has %d entries, the model block %d' % (t.size, self._nblock))
        state = self.moments._state()
        e = L.f64(self.moments.update(t[self._cols], weight))          # refuses a weight below 1
        try:
            self._read('add', self._proj, e.size, L.p_f64(e), int(weight))
        except Exception:
            self.moments._restore(state)       # a refused add is added nowhere
            raise
        self.rank = None

    def merge(self, other):
        '''self += other (same device, domain, days and parameters)'''
        if list(other.days) != self.days or other._slot != self._slot or other.params != self.params:
            raise ValueError('sensitivity maps over different days or parameters')
        state = self.moments._state()
        dtheta = L.f64(self.moments.merge(other.moments))
        try:
            self._call('merge', other._h, dtheta.size, L.p_f64(dtheta))
        except Exception:
            self.moments._restore(state)
            raise
        self.rank = None

    def reset(self):
        super().reset()
        self.moments.reset()
        self.rank = None

    def finalize(self):
        '''Compute `explained` and `dominant` from the members so far -> (rank, dropped eigenvalues).
        ValueError when nothing varies or members < rank + 2: a regression through that few members fits
        exactly and would report explained == 1 everywhere; the correlation maps stay available.'''
        F, rank, lam, isd = finalize_factor(self.moments)
        self._call('finalize', len(self.params), rank, L.p_f64(F), L.p_f64(isd))
        self.rank, self.eigenvalues = rank, lam
        self.F, self.isd = F, isd
        return rank, lam[rank:]

    def _fetch(self, day, what):
        slot = self._slot_of(day)
        if slot is None:                                          # an output without weight
            return np.full((self.N, self.N), -1.0 if what == 3 else 0.0)
        return self.fetch_slot(slot, what)

    def fetch_slot(self, slot, what):
        '''raw access by slot index (0 mean, 1 variance, 2 explained, 3 dominant, 16 + i covariance)'''
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('fetch', int(slot), int(what), L.p_f64(out))
        return out

    def _i(self, name):
        if name not in self.params:
            raise ValueError('parameter %r is not among %r' % (name, self.params))
        return self.params.index(name)

    def mean(self, day):
        return self._fetch(day, 0)

    def variance(self, day):
        return self._fetch(day, 1)

    def covariance(self, day, name):
        '''posterior covariance of the cell's value with parameter `name`'''
        return self._fetch(day, 16 + self._i(name))

    def correlation(self, day, name):
        '''covariance / sqrt(variance of the cell x variance of the parameter), 0 where either is 0'''
        i = self._i(name)
        cov, var = self._fetch(day, 16 + i), self.variance(day)
        vt = self.moments.cov()[i, i] if not self.moments.constant()[i] else 0.0
        den = np.sqrt(var * vt)
        out = np.zeros_like(cov)
        np.divide(cov, den, out=out, where=den > 0)
        return out

    def explained(self, day):
        '''share of the cell's posterior variance explained by a linear dependence on the parameters'''
        return self._fetch(day, 2)

    def dominant(self, day):
        '''int8 index into `params` of the parameter with the largest |correlation|, -1 where nothing varies'''
        return self._fetch(day, 3).astype(np.int8)

    def describe(self):
        '''the parameter block of a result file'''
        mo = self.moments
        out = {'params': list(self.params), 'members': int(mo.members), 'total_weight': int(mo.W)}
        if mo.W:
            _F, rank, lam = mo.factor()
            out.update({'mean': mo.mean().tolist(), 'sd': np.sqrt(np.diag(mo.cov())).tolist(),
                        'correlation': mo.corr().tolist(), 'rank': rank,
                        'dropped_eigenvalues': lam[rank:].tolist()})
        return out

    def profile(self, enable=None):
        '''HIP-event time of the accumulate launches: (total ms, launches); enable switches it'''
        return self._profile(enable)



# ------------------------------------------------------------------ dependence
MAX_DEP_BINS = 16          # ps_depend: the bins of one scalar
DEFAULT_DEP_BINS = 8


def dependence_edges(values, weights, bins):
    '''The interior cut points of one parameter for DependenceMaps: `values` per member, `weights` their positive
    integer weights (run lengths), `bins` 2..16 -> a strictly increasing float64 array of at most bins - 1 edges;
    a member's bin is np.searchsorted(edges, value, side='right').  The bins have as nearly equal weight as the
    distinct values allow, decided in integers: cut j = 1 .. bins - 1 goes behind the distinct value whose
    cumulative weight c minimises |c bins - j total| (the lower one on a tie), and lies at the midpoint between
    that value and the next distinct one -- equal values always share a bin and no value sits on an edge.  Cuts
    that fall together are one: a parameter with fewer distinct values than bins uses fewer bins, a constant
    one a single bin (no edge).'''
    if int(bins) != bins or not 2 <= int(bins) <= MAX_DEP_BINS:
        raise ValueError('dependence bins must be an integer in 2..%d, got %r' % (MAX_DEP_BINS, bins))
    v = np.array(values, dtype=np.float64).ravel()
    w = np.asarray(weights).ravel()
    if v.size == 0 or v.size != w.size:
        raise ValueError('%d values and %d weights' % (v.size, w.size))
    if not np.all(np.isfinite(v)):
        raise ValueError('every value must be finite')
    if np.any(w != np.floor(w)) or np.any(w < 1):
        raise ValueError('weights must be positive integers')
    u, inv = np.unique(v, return_inverse=True)
    cw = np.cumsum(np.bincount(inv.ravel(), weights=w.astype(np.float64)).astype(np.int64))
    total, nb = int(cw[-1]), int(bins)
    edges = []
    last = -1
    for j in range(1, nb):
        if u.size < 2:
            break
        i = int(np.argmin(np.abs(cw[:-1] * nb - j * total)))      # the first of equals: the lower value
        if i == last:
            continue
        last = i
        mid = u[i] + 0.5 * (u[i + 1] - u[i])
        edges.append(mid if mid > u[i] else u[i + 1])             # neighbouring doubles: the upper one goes right
    return np.array(edges, dtype=np.float64)


def check_dependence(arg):
    '''posterior_predictive's dependence= argument -> dict(params=[names], bins=B, days=None | [model days]):
    True (all 15 model parameters, 8 bins), a list of names from mcmc.MODEL_BLOCK (check_sens_params), or
    dict(params=..., bins=8, days=...) with bins in 2..16 and days a strictly increasing list of model days
    (default: the summary's); ValueError otherwise'''
    if isinstance(arg, dict):
        unknown = sorted(set(arg) - {'params', 'bins', 'days'})
        if unknown:
            raise ValueError('dependence: unknown keys %r (params, bins, days)' % (unknown,))
        params, bins, days = arg.get('params'), arg.get('bins', DEFAULT_DEP_BINS), arg.get('days')
    else:
        params, bins, days = arg, DEFAULT_DEP_BINS, None
    if params is False or (params is not None and params is not True and not isinstance(params, (str, list, tuple))):
        raise ValueError('dependence parameters must be True or a list of names, got %r' % (params,))
    names = check_sens_params(params)
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 2 <= int(bins) <= MAX_DEP_BINS:
        raise ValueError('dependence bins must be an integer in 2..%d, got %r' % (MAX_DEP_BINS, bins))
    if days is not None:
        try:
            days = [int(d) for d in days]
        except (TypeError, ValueError):
            raise ValueError('dependence days must be a list of model days, got %r' % (days,))
        if not days or days[0] < 0 or any(b <= a for a, b in zip(days, days[1:])):
            raise ValueError('dependence days must be model days >= 0, strictly increasing: %r' % (days,))
    return {'params': names, 'bins': int(bins), 'days': days}


def adjusted_ratio(eta2, members, bins_used):
    '''max(0, 1 - (1 - eta2)(members - 1) / (members - bins_used)): the epsilon^2 adjustment of a correlation
    ratio over `bins_used` non-empty bins of `members` members'''
    n, k = int(members), int(bins_used)
    if n <= k:
        raise ValueError('%d members in %d bins: nothing is left to adjust with' % (n, k))
    return np.maximum(0.0, 1.0 - (1.0 - np.asarray(eta2, dtype=np.float64)) * ((n - 1) / (n - k)))


def finalize_bin_weights(params, bin_weights, members):
    '''Wb [nparam, nbin] contiguous float64 for ps_depend_finalize from the integer bin weights of `members`
    members.  ValueError when nothing is accumulated or, for any parameter, members < 2 x (its non-empty bins):
    bins of single members reproduce every member and give eta^2 = 1 by construction -- the argument of
    finalize_factor's members < rank + 2.'''
    if int(members) < 1:
        raise ValueError('nothing accumulated')
    for n, row in zip(params, np.asarray(bin_weights)):
        used = int(np.count_nonzero(row))
        if members < 2 * used:
            raise ValueError('%d members in %d bins of %r: with fewer than two members per bin on average '
                             'the bin means reproduce the members and eta^2 is 1 by construction'
                             % (members, used, n))
    return L.f64(bin_weights)


class DependenceMaps(_Accumulator):
    '''On which parameter a cell depends, linearly or not: per cell of `pop_model`'s days and per parameter of
    `params` (names from mcmc.MODEL_BLOCK) the correlation ratio eta^2 = Var_b(E[v | parameter in bin b]) / Var(v)
    of the value SpreadSummary adds, over the members added, on the device (ps_depend_*, csrc/ps_depend.hip),
    next to the mean and the variance (the same bits as a SpreadSummary fed alongside).  `edges`: per parameter
    the interior cut points (dependence_edges), at most 15 each.  `add(theta, weight)` takes the member's full
    model block and bins the columns.  After `finalize()`: `ratio(day, name)`, `dominant(day)`, `adjusted`,
    `excess`.  eta^2 is the given-data estimator of the first-order variance-based index (Plischke 2010): a
    statement about one parameter at a time, like SensitivityMaps.correlation; where the parameters are
    correlated, as in a posterior, it credits a parameter with what its correlates do.  It holds no interaction
    or total-effect index, and a parameter without any influence shows `floor(name)` on average, not 0.'''

    _prefix, _noun = 'ps_depend', 'dependence maps'

    def __init__(self, pop_model, params, edges, days=None):
        self._setup(pop_model, params, edges, _model_days(pop_model, days), None)

    @classmethod
    def for_projection(cls, projection, params, edges):
        '''Dependence maps of the outputs of `projection` (a Projection or a ReleaseSites), one slot per output:
        `add(theta, weight)` accumulates the outputs of its last `apply()`, and the accessors take the output
        index where the day-based maps take a day.'''
        self = cls.__new__(cls)
        self._setup(projection.pm, params, edges, list(range(projection.nout)), projection)
        return self

    def _setup(self, pop_model, params, edges, days, projection):
        self.params = check_sens_params(params)
        known = [m[0] for m in mcmc.MODEL_BLOCK]
        self._cols = [known.index(n) for n in self.params]
        self._nblock = len(known)
        if isinstance(edges, dict):
            edges = [edges[n] for n in self.params]
        self.edges = [np.array(e, dtype=np.float64).ravel() for e in edges]
        if len(self.edges) != len(self.params):
            raise ValueError('%d lists of edges for %d parameters' % (len(self.edges), len(self.params)))
        for n, e in zip(self.params, self.edges):
            if e.size > MAX_DEP_BINS - 1 or not np.all(np.isfinite(e)) or np.any(np.diff(e) <= 0):
                raise ValueError('the edges of %r must be finite, strictly increasing and at most %d: %r'
                                 % (n, MAX_DEP_BINS - 1, e.tolist()))
        self.nbin = max(2, max(e.size for e in self.edges) + 1)
        self.bins_asked = self.nbin
        self._attach(pop_model)
        self._set_source(projection, days, projection and projection.live)
        self.nbytes = len(self._slot) * self.pitch * ((2 + len(self.params) * self.nbin + len(self.params)) * 8 + 1)
        self._zero()
        self._create(len(self._slot), len(self.params), self.nbin)

    def _zero(self):
        self.bin_weights = np.zeros((len(self.params), self.nbin), dtype=np.int64)
        self._members = 0
        self.finalized = False

    def bins_of(self, theta):
        '''the bin of every listed parameter of the model block `theta` -> int32 [nparam]'''
        t = np.array(theta, dtype=np.float64).ravel()
        if t.size != self._nblock:
            raise ValueError('theta has %d entries, the model block %d' % (t.size, self._nblock))
        if not np.all(np.isfinite(t[self._cols])):
            raise ValueError('every listed parameter must be finite: %r' % (t[self._cols].tolist(),))
        return L.i32([np.searchsorted(e, t[c], side='right') for e, c in zip(self.edges, self._cols)])

    def add(self, theta, weight=1):
        '''Accumulate the last evaluation of the model (on a projection or a plan: its last apply), whose
        model block is `theta`, with integer weight >= 1; enqueued, no host synchronisation.'''
        b = self.bins_of(theta)
        w = self._weight(weight)
        state = (self.bin_weights.copy(), self._members)
        self.bin_weights[np.arange(b.size), b] += w
        self._members += 1
        try:
            self._read('add', self._proj, b.size, L.p_i32(b), w)
        except Exception:
            self.bin_weights, self._members = state       # a refused add is added nowhere
            raise
        self.finalized = False

    def merge(self, other):
        '''self += other (same device, domain, days, parameters and edges)'''
        if (list(other.days) != self.days or other._slot != self._slot or other.params != self.params
                or len(other.edges) != len(self.edges)
                or not all(np.array_equal(a, b) for a, b in zip(self.edges, other.edges))):
            raise ValueError('dependence maps over different days, parameters or edges')
        self._call('merge', other._h)
        self.bin_weights = self.bin_weights + other.bin_weights
        self._members += other._members
        self.finalized = False

    def reset(self):
        super().reset()
        self._zero()

    def bins_used(self, name):
        '''the bins of parameter `name` that hold a member'''
        return int(np.count_nonzero(self.bin_weights[self._i(name)]))

    def finalize(self):
        '''Compute the ratios and `dominant` from the members so far.  ValueError when nothing is accumulated or,
        for any listed parameter, members < 2 x (its non-empty bins): bins of single members reproduce every
        member and give eta^2 = 1 by construction.'''
        Wb = finalize_bin_weights(self.params, self.bin_weights, self._members)
        self._call('finalize', len(self.params), self.nbin, L.p_f64(Wb))
        self.finalized = True

    def _fetch(self, day, what):
        slot = self._slot_of(day)
        if slot is None:                                          # an output without weight
            return np.full((self.N, self.N), -1.0 if what == 2 else 0.0)
        return self.fetch_slot(slot, what)

    def fetch_slot(self, slot, what):
        '''raw access by slot index (0 mean, 1 variance, 2 dominant, 3 M2, 16 + p eta^2, 256 + 16 p + b the sum
        of w v over the members of bin b of parameter p)'''
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('fetch', int(slot), int(what), L.p_f64(out))
        return out

    def _i(self, name):
        if name not in self.params:
            raise ValueError('parameter %r is not among %r' % (name, self.params))
        return self.params.index(name)

    def mean(self, day):
        return self._fetch(day, 0)

    def variance(self, day):
        return self._fetch(day, 1)

    def bin_sum(self, day, name, b):
        '''the sum of w v over the members whose parameter `name` fell in bin b'''
        return self._fetch(day, 256 + 16 * self._i(name) + self._index(b, self.nbin, 'bin'))

    def ratio(self, day, name):
        '''eta^2 of the cell on parameter `name`: the share of the cell's posterior variance that lies between
        the bin means, in [0, 1], 0 where the cell does not vary'''
        return self._fetch(day, 16 + self._i(name))

    def dominant(self, day):
        '''int8 index into `params` of the parameter with the largest eta^2, -1 where nothing varies'''
        return self._fetch(day, 2).astype(np.int8)

    def floor(self, name):
        '''(bins used - 1) / (members - 1): what eta^2 of a parameter without any influence shows on average'''
        if self._members < 2:
            raise ValueError('the floor needs two members')
        return (self.bins_used(name) - 1) / (self._members - 1)

    def adjusted(self, day, name):
        '''max(0, 1 - (1 - eta^2)(members - 1) / (members - bins used)), the classical epsilon^2 adjustment of
        eta^2 for its floor.  It assumes independent, equally weighted members, which the runs of a chain are
        not: a guide to what is above the floor, not an interval.'''
        return adjusted_ratio(self.ratio(day, name), self._members, self.bins_used(name))

    def excess(self, day, name, sensitivity):
        '''max(0, adjusted - r^2), r the correlation of `sensitivity` (a SensitivityMaps over the same members)
        with the same parameter: the share that only a non-linear dependence explains.  The binned eta^2 is not
        >= r^2 in general -- a bin loses the trend inside it -- hence the clip at 0.'''
        r = sensitivity.correlation(day, name)
        return np.maximum(0.0, self.adjusted(day, name) - r * r)

    def describe(self):
        '''the parameter block of a result file'''
        n = self._members
        return {'params': list(self.params), 'bins': int(self.bins_asked),
                'bins_used': [self.bins_used(p) for p in self.params],
                'edges': [e.tolist() for e in self.edges],
                'bin_weights': [[int(x) for x in row[:e.size + 1]] for row, e in zip(self.bin_weights, self.edges)],
                'members': int(n), 'total_weight': int(self.bin_weights[0].sum()),
                'floor': [self.floor(p) if n >= 2 else None for p in self.params]}

    def profile(self, enable=None):
        '''HIP-event time of the accumulate launches: (total ms, launches); enable switches it'''
        return self._profile(enable)


def pooled_dependence_edges(prepared, names, bins):
    '''the edges of every parameter of `names` over the runs of all chains (prepared: per chain (rows, runs, model
    columns, ...) as _check_request loads them), shared by every chain's DependenceMaps'''
    known = [m[0] for m in mcmc.MODEL_BLOCK]
    thetas = np.array([rows[first, mcols] for rows, rl, mcols, *_rest in prepared for first, _n in rl])
    lengths = np.array([n for _rows, rl, *_rest in prepared for _first, n in rl], dtype=np.int64)
    if not lengths.size:
        raise ValueError('dependence: the chains hold no rows')
    return [dependence_edges(thetas[:, known.index(n)], lengths, bins) for n in names]



# ------------------------------------------------------------------ Monte Carlo error
MAX_MC_THRESHOLDS = 4
MAX_MC_SEQUENCES = 16      # ps_mcerr_rhat: the sequences of one launch's plane pointers
MAX_MC_WEIGHT = 2 ** 32 - 1


def check_mc_thresholds(thresholds):
    '''0..4 thresholds, finite and strictly increasing -> [float]'''
    thr = [float(t) for t in thresholds]
    if len(thr) > MAX_MC_THRESHOLDS:
        raise ValueError('at most %d thresholds, got %d' % (MAX_MC_THRESHOLDS, len(thr)))
    if not all(np.isfinite(t) for t in thr) or any(b <= a for a, b in zip(thr, thr[1:])):
        raise ValueError('thresholds must be finite and strictly increasing, got %r' % (thr,))
    return thr


def mc_batch_plan(rows_per_chain, batches):
    '''How posterior_predictive cuts its chains for the Monte Carlo error: rows_per_chain, the kept rows of
    every chain; batches, the batches a chain of the shortest length gives (even and >= 4, so that either half
    has at least two) -> (b, [(half, rows), ...]): the batch weight b = min(rows_per_chain) // batches, one for
    all chains, and per chain the row `half` = rows // 2 at which its second sequence starts -- rows [0, half)
    feed the first, [half, rows) the second.  ValueError where a chain has fewer than `batches` rows.'''
    rows = [int(n) for n in rows_per_chain]
    if int(batches) != batches or batches < 4 or batches % 2:
        raise ValueError('batches must be an even integer >= 4, got %r' % (batches,))
    if not rows:
        raise ValueError('no chains')
    b = min(rows) // int(batches)
    if b < 1:
        raise ValueError('a chain of %d rows is shorter than %d batches' % (min(rows), batches))
    if max(rows) > MAX_MC_WEIGHT:
        raise ValueError('a chain of %d rows is past the weight 2^32 - 1 of one sequence' % max(rows))
    return b, [(n // 2, n) for n in rows]


def mc_split(first, length, half):
    '''the weight of the run of rows [first, first + length) before and from the row `half` on'''
    head = max(0, min(first + length, half) - first)
    return head, length - head


def mc_error_plan(mc_error):
    '''the mc_error= argument of posterior_predictive -> the batches per chain: True -> 20, dict(batches=B)'''
    if mc_error is True:
        return 20
    if not isinstance(mc_error, dict) or set(mc_error) - {'batches'}:
        raise ValueError('mc_error must be True or dict(batches=B), got %r' % (mc_error,))
    batches = mc_error.get('batches', 20)
    mc_batch_plan([batches], batches)
    return int(batches)


class MonteCarloError(_Handle):
    '''Batch means of one sequence of members -- a chain, or half of one -- on the device (ps_mcerr_*,
    csrc/ps_mcerr.hip): how far the posterior mean and the exceedance probabilities of `SpreadSummary` are from
    what a longer chain would give.  The sequence is cut into batches of exactly `batch_weight` rows of weight;
    `add(weight)` takes the value `SpreadSummary.add` takes and splits the weight at the batch boundaries.
    `finish()` discards the open batch, so the maps are those of the used rows n = b B alone.  days, thresholds
    (0..4, finite, strictly increasing) as SpreadSummary; the accessors take a model day, of `for_projection`
    the output index.  `rhat`: {day: split R-hat map} where posterior_predictive pooled the sequences, else None.'''

    rhat = None
    _prefix, _noun, _prof_pairs = 'ps_mcerr', 'Monte Carlo error', 2
    _info_types = (C.c_int64,) * 6     # batches, batch weight, used, open and discarded weight, members

    def __init__(self, pop_model, batch_weight, days=None, thresholds=()):
        self._setup(pop_model, batch_weight, _model_days(pop_model, days), thresholds, None)

    @classmethod
    def for_projection(cls, projection, batch_weight, thresholds=()):
        '''The batch means of the outputs of `projection` (a Projection or a ReleaseSites), one slot per output
        that carries weight: `add(weight)` takes the outputs of its last `apply()`.'''
        self = cls.__new__(cls)
        self._setup(projection.pm, batch_weight, list(range(projection.nout)), thresholds, projection)
        return self

    def _setup(self, pop_model, batch_weight, days, thresholds, projection):
        self.thresholds = check_mc_thresholds(thresholds)
        b = int(batch_weight)
        if b != batch_weight or not 1 <= b <= MAX_MC_WEIGHT:
            raise ValueError('batch_weight must be an integer in 1 .. 2^32 - 1, got %r' % (batch_weight,))
        self._attach(pop_model)
        self._set_source(projection, days, projection and projection.live)
        n = len(self._slot)
        self.nbytes = n * self.pitch * (40 + 16 * len(self.thresholds))     # five fp64 planes, counts per threshold
        thr = L.f64(self.thresholds if self.thresholds else [0.0])
        self._create(n, len(self.thresholds), L.p_f64(thr), b)

    def add(self, weight=1):
        '''Accumulate the last evaluation of the model (of a projection: its last apply) with integer weight
        >= 1, split at the batch boundaries; a batch that fills up is closed.  No host synchronisation.'''
        self._read('add', self._proj, self._weight(weight))

    def finish(self):
        '''discard the open batch (its weight goes to `discarded_weight`)'''
        self._call('finish')

    def merge(self, other):
        '''self += other: the closed batches of both pooled (same device, domain, days, thresholds and batch
        weight; both finished)'''
        if list(other.days) != self.days or other._slot != self._slot:
            raise ValueError('sequences over different days')
        self._call('merge', other._h)

    def reset(self):
        self._call('reset')
        self.rhat = None

    @property
    def batches(self):
        return self._info()[0]

    @property
    def batch_weight(self):
        return self._info()[1]

    @property
    def used_weight(self):
        return self._info()[2]

    @property
    def open_weight(self):
        return self._info()[3]

    @property
    def discarded_weight(self):
        return self._info()[4]

    @property
    def members(self):
        return self._info()[5]

    def _slot_of(self, day):
        '''the slot of a day, None for an output without weight'''
        return super()._slot_of(day, 'sequence')

    def plane(self, day, what):
        '''[N, N] float64: a raw plane (0 gmean, 1 gM2, 2 wM2)'''
        slot = self._slot_of(day)
        if slot is None:
            return np.zeros((self.N, self.N), dtype=np.float64)
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('fetch', slot, int(what), L.p_f64(out))
        return out

    def counts(self, day, k):
        '''(s1 [N, N] uint32, s2 [N, N] uint64): over the closed batches the sum of the weight with value >=
        thresholds[k] and the sum of its squares'''
        if not 0 <= int(k) < len(self.thresholds):
            raise ValueError('threshold %r of %d' % (k, len(self.thresholds)))
        slot = self._slot_of(day)
        s1 = np.zeros((self.N, self.N), dtype=np.uint32)
        s2 = np.zeros((self.N, self.N), dtype=np.uint64)
        if slot is not None:
            self._call('fetch_counts', slot, int(k), s1.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       s2.ctypes.data_as(C.POINTER(C.c_uint64)))
        return s1, s2

    def mean(self, day):
        '''The mean over the used rows n = b B.  It differs from `SpreadSummary.mean` only by the discarded
        remainder -- the rows of the open batch `finish()` dropped.'''
        return self.plane(day, 0)

    def mcse(self, day):
        '''the Monte Carlo standard error of `mean`: sqrt(gM2 / (B - 1) / B), the batch means' standard error'''
        B = float(self.batches)
        return np.sqrt(self.plane(day, 1) / (B - 1.0) / B)

    def variance(self, day):
        '''(wM2 + b gM2) / n: the variance over the used rows'''
        _B, b, n = self._info()[:3]
        return (self.plane(day, 2) + float(b) * self.plane(day, 1)) / float(n)

    def ess(self, day):
        '''The effective sample size n variance / (b gM2 / (B - 1)); 0 where gM2 == 0.  Not capped at n:
        antithetic chains exceed it.'''
        B, b, n = self._info()[:3]
        g = self.plane(day, 1)
        num = float(n) * ((self.plane(day, 2) + float(b) * g) / float(n))
        out = np.zeros_like(g)
        np.divide(num, float(b) * (g / (B - 1.0)), out=out, where=g != 0.0)
        return out

    def prob(self, day, k):
        '''P(value >= thresholds[k]) over the used rows: s1 / n'''
        return self.counts(day, k)[0] / float(self.used_weight)

    def _batch_count_variance(self, day, k):
        '''(s1, B s2 - s1^2 in exact integer arithmetic (B s2 <= n^2 < 2^64) as float64)'''
        s1, s2 = self.counts(day, k)
        q = s1.astype(np.uint64)
        return s1, (np.uint64(self.batches) * s2 - q * q).astype(np.float64)

    def prob_mcse(self, day, k):
        '''the Monte Carlo standard error of `prob`: sqrt((B s2 - s1^2) / (B (B - 1)) / b^2 / B)'''
        B, b = float(self.batches), float(self.batch_weight)
        return np.sqrt(self._batch_count_variance(day, k)[1] / (B * (B - 1.0)) / (b * b) / B)

    def prob_ess(self, day, k):
        '''the effective sample size of `prob`: n p (1 - p) / (b var), var the batch proportions' sample
        variance; 0 where that is 0'''
        B, b, n = [float(x) for x in self._info()[:3]]
        s1, num = self._batch_count_variance(day, k)
        p = s1 / n
        out = np.zeros(p.shape)
        np.divide(n * (p * (1.0 - p)), b * (num / (B * (B - 1.0)) / (b * b)), out=out, where=num != 0.0)
        return out

    def profile(self, enable=None):
        '''HIP-event time of the add launches, one per piece, and of the close launches: (add ms, add launches,
        close ms, close launches); enable switches it'''
        return self._profile(enable)



def split_rhat(sequences, day):
    '''[N, N] float64: the split R-hat of 2..16 finished MonteCarloError sequences (same days and batch weight,
    each with >= 2 batches, which may differ in number) at a day, on the device (ps_mcerr_rhat); 0 where
    every sequence is constant'''
    seqs = list(sequences)
    if not 2 <= len(seqs) <= MAX_MC_SEQUENCES:
        raise ValueError('2..%d sequences, got %d' % (MAX_MC_SEQUENCES, len(seqs)))
    s0 = seqs[0]
    if any(list(s.days) != s0.days or s._slot != s0._slot for s in seqs[1:]):
        raise ValueError('sequences over different days')
    slot = s0._slot_of(day)
    out = np.zeros((s0.N, s0.N), dtype=np.float64)
    if slot is not None:
        hs = (L._VP * len(seqs))(*[s._h.value for s in seqs])
        L.check(s0._lib.ps_mcerr_rhat(hs, len(seqs), slot, L.p_f64(out)))
    return out


def pool_mc_error(pairs):
    '''pairs: per chain its two sequences.  Finishes them all, takes the split R-hat maps of all of them
    together (None where there are more than 16, or one has fewer than 2 batches -- failed members), then merges
    them in chain order into the first, which is returned with `rhat` set; the others are closed.'''
    seqs = [s for pair in pairs for s in pair]
    for s in seqs:
        s.finish()
    first = seqs[0]
    rhat = None
    if len(seqs) <= MAX_MC_SEQUENCES and all(s.batches >= 2 for s in seqs):
        rhat = {d: split_rhat(seqs, d) for d in first.days}
    for s in seqs[1:]:
        first.merge(s)
        s.close()
    first.rhat = rhat
    return first


# ------------------------------------------------------------------ weather ensembles
WIND_KEYS = ('draws', 'block', 'seed', 'pool', 'sequences', 'share', 'pool_kernels')
WEATHER_PLANES = {'imean': 0, 'iM2': 1, 'omean': 2, 'oM2': 3, 'wS': 4, 'vw': 5, 'vp': 6, 'share': 7}
WEATHER_PARTS = {'weather': 5, 'parameter': 6}


def _whole(value, name, least):
    '''an integer >= least that is no bool -> int'''
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or value < least:
        raise ValueError('wind: %s must be an integer >= %d, got %r' % (name, least, value))
    return int(value)


def wind_sequences(pool, ndays, draws, block=3, seed=0):
    '''[draws, ndays] int: day keys resampled from `pool` -- the sorted distinct day keys of a wind record, at
    least 2 -- by the circular moving-block bootstrap (Politis & Romano 1992).  A draw is made of blocks of `block`
    consecutive pool entries, the successor of the last pool day being the first; the block starts come from
    numpy.random.Generator(PCG64(seed)).integers(0, len(pool)); the last block is cut to length.  block=1 gives
    independent days.  The days keep the order and the repeats of one recorded season: no weather is generated.'''
    keys = [int(d) for d in pool]
    if len(keys) < 2 or any(b <= a for a, b in zip(keys, keys[1:])):
        raise ValueError('wind: the pool must be at least 2 sorted distinct day keys, got %r' % (list(pool),))
    ndays, draws, block = _whole(ndays, 'ndays', 1), _whole(draws, 'draws', 1), _whole(block, 'block', 1)
    rng = np.random.Generator(np.random.PCG64(_whole(seed, 'seed', 0)))
    nblock = -(-ndays // block)
    starts = rng.integers(0, len(keys), size=(draws, nblock))
    pos = (starts[:, :, None] + np.arange(block)[None, None, :]) % len(keys)
    return np.asarray(keys, dtype=np.int64)[pos.reshape(draws, nblock * block)[:, :ndays]]


def check_wind(arg, pop_model):
    '''wind=dict(draws=8, block=3, seed=0, pool=None, sequences=None, share=True, pool_kernels=True) of
    posterior_predictive against the model -> the plan: the same keys, `pool` the sorted distinct day keys drawn
    from (default every day of the model's wind record), `sequences` [K, len(pop_model.days)] the day keys as
    evaluated -- the user's rows where given, which replace the draws, else wind_sequences -- and `used`, the sorted
    distinct days among them.  ValueError on a bad key, length, count or type, and on fewer than 2 sequences
    while `share` is true (a variance within a group needs two draws).'''
    if not isinstance(arg, dict) or set(arg) - set(WIND_KEYS):
        raise ValueError('wind must be dict(%s), got %r' % (', '.join(WIND_KEYS), arg))
    record = sorted(int(d) for d in pop_model.wind_data.keys())
    ndays = len(pop_model.days)
    plan = dict(draws=_whole(arg.get('draws', 8), 'draws', 1), block=_whole(arg.get('block', 3), 'block', 1),
                seed=_whole(arg.get('seed', 0), 'seed', 0))
    for flag in ('share', 'pool_kernels'):
        if not isinstance(arg.get(flag, True), (bool, np.bool_)):
            raise ValueError('wind: %s must be True or False, got %r' % (flag, arg[flag]))
        plan[flag] = bool(arg.get(flag, True))

    def keys_of(values, what):
        try:
            keys = [_whole(d, 'a day key of ' + what, min(record)) for d in values]
        except TypeError:
            raise ValueError('wind: %s must be a list of day keys, got %r' % (what, values))
        off = [d for d in keys if d not in record]
        if off:
            raise ValueError('wind: day %r of %s is not in the wind record %r' % (off[0], what, record))
        return keys
    pool = record if arg.get('pool') is None else sorted(set(keys_of(arg['pool'], 'the pool')))
    if len(pool) < 2:
        raise ValueError('wind: the pool needs at least 2 distinct days, got %r' % (pool,))
    plan['pool'] = pool
    if arg.get('sequences') is None:
        seqs = wind_sequences(pool, ndays, plan['draws'], plan['block'], plan['seed'])
    else:
        try:
            rows = [list(r) for r in arg['sequences']]
        except TypeError:
            raise ValueError('wind: sequences must be rows of day keys, got %r' % (arg['sequences'],))
        if not rows:
            raise ValueError('wind: sequences is empty')
        for r in rows:
            if len(r) != ndays:
                raise ValueError('wind: a sequence has %d days, the model %d' % (len(r), ndays))
        seqs = np.asarray([keys_of(r, 'a sequence') for r in rows], dtype=np.int64)
        plan['draws'] = len(rows)
    if plan['share'] and len(seqs) < 2:
        raise ValueError('wind: the weather share needs at least 2 sequences per run, got %d (share=False runs one)'
                         % len(seqs))
    plan['sequences'] = seqs
    plan['used'] = sorted(set(int(d) for d in seqs.ravel()))
    return plan


class WeatherShare(_Accumulator):
    '''How much of a cell's posterior spread is weather and how much is parameters, on the device (ps_nested_*,
    csrc/ps_nested.hip).  The members come in groups: `add()` takes the model's last evaluation (of a projection:
    its last apply) as one more draw of the open group -- one parameter vector under one more wind sequence --
    and `close_group(weight)` closes the group with the run's weight; at least 2 draws per group and 2 groups.
    `variance(day, 'weather')` is the variance over the wind at fixed parameters, the weighted mean of the groups'
    own sample variances; `variance(day, 'parameter')` the variance of the group means less what their k_g draws
    of weather leave in them, the one-way random-effects estimate with the package's / W convention, clipped at 0;
    `share(day)` the weather's part of their sum.  days as SpreadSummary; of `for_projection` the output index.'''
    _prefix, _noun, _prof_pairs = 'ps_nested', 'weather share', 2
    _info_types = (C.c_double, C.c_int64, C.c_int64, C.c_int64, C.c_double)   # W, members, groups, open draws, sum w/k

    def __init__(self, pop_model, days=None):
        self._setup(pop_model, _model_days(pop_model, days), None)

    @classmethod
    def for_projection(cls, projection):
        '''The split of the outputs of `projection` (a Projection or a ReleaseSites), one slot per output that
        carries weight: `add()` takes the outputs of its last `apply()`.'''
        self = cls.__new__(cls)
        self._setup(projection.pm, list(range(projection.nout)), projection)
        return self

    def _setup(self, pop_model, days, projection):
        self._attach(pop_model)
        self._set_source(projection, days, projection and projection.live)
        self.nbytes = len(self._slot) * self.pitch * 64        # eight fp64 planes
        self._final = False
        self._create(len(self._slot))

    def add(self):
        '''one more draw of the open group, weight 1; no host synchronisation'''
        self._read('add', self._proj)
        self._final = False

    def close_group(self, weight=1):
        '''the open group (>= 2 draws) becomes a closed group of integer weight >= 1'''
        self._call('close', self._weight(weight))
        self._final = False

    def merge(self, other):
        '''self += other (same device, domain and days; no open group on either side)'''
        if list(other.days) != self.days or other._slot != self._slot:
            raise ValueError('weather shares over different days')
        self._call('merge', other._h)
        self._final = False

    def reset(self):
        self._call('reset')
        self._final = False

    @property
    def groups(self):
        return self._info()[2]

    @property
    def open_draws(self):
        return self._info()[3]

    def plane(self, day, what):
        '''[N, N] float64: a raw plane by name (WEATHER_PLANES); 'vw', 'vp' and 'share' are finalized first'''
        code = WEATHER_PLANES[what] if what in WEATHER_PLANES else self._index(what, 8, 'plane')
        slot = self._slot_of(day)
        if slot is None:
            return np.zeros((self.N, self.N), dtype=np.float64)
        if code >= 5 and not self._final:
            self._call('finalize')
            self._final = True
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('fetch', slot, code, L.p_f64(out))
        return out

    def mean(self, day):
        '''the weighted mean of the groups' means'''
        return self.plane(day, 'omean')

    def variance(self, day, part='total'):
        '''part: 'weather' | 'parameter' | 'total', the sum of the two'''
        if part == 'total':
            return self.plane(day, 'vp') + self.plane(day, 'vw')
        if part not in WEATHER_PARTS:
            raise ValueError("part must be 'weather', 'parameter' or 'total', got %r" % (part,))
        return self.plane(day, WEATHER_PARTS[part])

    def share(self, day):
        '''weather / total; 0 where the total is 0'''
        return self.plane(day, 'share')

    def profile(self, enable=None):
        '''HIP-event time of the add and of the close launches: (add ms, add launches, close ms, close launches)'''
        return self._profile(enable)


def weather_block(ws, keys, labels, prefix, mean_of, maps):
    '''The json block of one WeatherShare -- groups, members, total weight and per day the mean-weighted share
    sum(share mean) / sum(mean), mean_of(key) the summary's mean map -- its maps appended to `maps` as save_maps
    takes them: per day `{prefix}{label}` with `_vw`, `_vp` and `_share`.'''
    shares = {}
    for key, label in zip(keys, labels):
        share, mean = ws.share(key), mean_of(key)
        maps.append(('%s%s' % (prefix, label), [('_vw', ws.variance(key, 'weather')),
                                                ('_vp', ws.variance(key, 'parameter')), ('_share', share)]))
        total = float(mean.sum())
        shares[str(label)] = float((share * mean).sum() / total) if total > 0 else 0.0
    return {'groups': ws.groups, 'members': ws.members, 'total_weight': ws.total_weight, 'weather_share': shares}


# ------------------------------------------------------------------ reweighting for new observations
MAX_REWEIGHT_SCENARIOS = 4
MAX_REWEIGHT_SLOTS = 32    # ps_wsum: the slots of one launch's descriptors
PROBE_KINDS = ('count', 'none', 'found')
DEFAULT_MIN_ESS = 50.0
REWEIGHT_MAPS = ('quantiles', 'arrival', 'contrast', 'excursion')      # the 'maps' option of reweight=: what else is reweighted


def check_scenarios(scenarios):
    '''the scenario names of a ReweightedSummary as a list of strings: 1..4 distinct names; ValueError otherwise'''
    if isinstance(scenarios, str):
        raise ValueError('scenarios must be a list of names, got %r' % (scenarios,))
    try:
        names = [str(n) for n in scenarios]
    except TypeError:
        raise ValueError('scenarios must be a list of names, got %r' % (scenarios,))
    if not 1 <= len(names) <= MAX_REWEIGHT_SCENARIOS:
        raise ValueError('%d reweighting scenarios; 1..%d fit one handle' % (len(names), MAX_REWEIGHT_SCENARIOS))
    if len(set(names)) != len(names):
        raise ValueError('duplicate scenario names in %r' % (names,))
    return names


def check_probes(probes, rad_dist, rad_res, ndays=None):
    '''Probe observations as a list of dicts, one per probe in the order given.  A probe is
    (east_m, north_m, day, kind, rate[, n]): the position in metres from the domain centre, resolved to a cell as
    check_sites resolves a site (col = rad_res + round(east / res), row = rad_res - round(north / res),
    res = rad_dist / rad_res; the cell has to lie inside the domain), a model day (a whole number >= 0, below
    ndays if given), the kind -- 'count' (n wasps found, a whole number >= 0), 'none' (looked, nothing found) or
    'found' (at least one found) -- and rate, finite and > 0: the expected number found per wasp in the cell.
    rad_res=None skips the cells (no model at hand).  ValueError otherwise.'''
    try:
        rows = [tuple(p) for p in probes]
    except TypeError:
        raise ValueError('probes must be a list of (east_m, north_m, day, kind, rate[, n]), got %r' % (probes,))
    if not rows:
        raise ValueError('a probe scenario needs at least one probe')
    out = []
    for k, p in enumerate(rows):
        if len(p) not in (5, 6):
            raise ValueError('probe %d: (east_m, north_m, day, kind, rate[, n]) expected, got %r' % (k, p))
        kind = p[3]
        if kind not in PROBE_KINDS:
            raise ValueError('probe %d: kind %r is not one of %r' % (k, kind, PROBE_KINDS))
        try:
            east, north, rate = float(p[0]), float(p[1]), float(p[4])
            if int(p[2]) != p[2]:
                raise ValueError
            day = int(p[2])
        except (TypeError, ValueError):
            raise ValueError('probe %d: numbers and a whole model day expected, got %r' % (k, p))
        if not (np.isfinite(east) and np.isfinite(north)):
            raise ValueError('probe %d: position %r is not finite' % (k, p[:2]))
        if day < 0 or (ndays is not None and day >= ndays):
            raise ValueError('probe %d: day %d is not a model day%s' % (k, day, '' if ndays is None else
                                                                       ' (0..%d)' % (ndays - 1)))
        if not (np.isfinite(rate) and rate > 0):
            raise ValueError('probe %d: rate %r is not finite and > 0' % (k, p[4]))
        n = None
        if kind == 'count':
            if len(p) != 6:
                raise ValueError("probe %d: a 'count' probe needs the number found" % k)
            try:
                if int(p[5]) != p[5] or int(p[5]) < 0:
                    raise ValueError
                n = int(p[5])
            except (TypeError, ValueError):
                raise ValueError('probe %d: the number found must be a whole number >= 0, got %r' % (k, p[5]))
        elif len(p) == 6 and p[5] is not None:
            raise ValueError('probe %d: a %r probe takes no number found' % (k, kind))
        rec = {'east': east, 'north': north, 'day': day, 'kind': kind, 'rate': rate, 'n': n}
        if rad_res is not None:
            res = float(rad_dist) / int(rad_res)
            rec['col'] = int(rad_res) + int(np.around(east / res))
            rec['row'] = int(rad_res) - int(np.around(north / res))
            if not (0 <= rec['row'] <= 2 * int(rad_res) and 0 <= rec['col'] <= 2 * int(rad_res)):
                raise ValueError('probe %d: cell (%d, %d) lies outside the %d x %d domain'
                                 % (k, rec['row'], rec['col'], 2 * int(rad_res) + 1, 2 * int(rad_res) + 1))
        out.append(rec)
    return out


def probe_loglik(kind, rate, v, n=None):
    '''log-likelihood of one probe where the member holds the density v (what PopModel.gather_days returns at the
    probe's cell and day), mu = rate * v, by the math module:
    'count': n log(mu) - mu - lgamma(n + 1), at mu = 0: 0 if n == 0 else -inf;  'none': -mu;
    'found': log(1 - exp(-mu)), at mu = 0: -inf -- as log(-expm1(-mu)) up to mu = log 2 and as log1p(-exp(-mu))
    above it, where 1 - exp(-mu) is close to 1 and the first form would lose the digits of a small result'''
    import math
    mu = float(rate) * float(v)
    if kind == 'none':
        return -mu
    if kind == 'found':
        if mu == 0.0:
            return -math.inf
        return math.log(-math.expm1(-mu)) if mu <= math.log(2.0) else math.log1p(-math.exp(-mu))
    if kind == 'count':
        if mu == 0.0:
            return 0.0 if n == 0 else -math.inf
        return n * math.log(mu) - mu - math.lgamma(n + 1)
    raise ValueError('kind %r is not one of %r' % (kind, PROBE_KINDS))


def probes_loglik(probes, values):
    '''the sum of probe_loglik over checked probes and their values, in list order, from 0.0'''
    lam = 0.0
    for p, v in zip(probes, values):
        lam = lam + probe_loglik(p['kind'], p['rate'], v, p['n'])
    return lam


def run_log_weight(row_log_weights):
    '''the log-weight of a run of rows sharing one member: mx + log(sum(exp(l - mx)) / n), mx their maximum (the
    log of the rows' mean weight); -inf if every row is -inf; equal rows give their value exactly'''
    import math
    ls = [float(v) for v in row_log_weights]
    mx = max(ls)
    if mx == -math.inf:
        return -math.inf
    s = 0.0
    for v in ls:
        s = s + math.exp(v - mx)
    return mx + math.log(s / len(ls))


def reweight_diagnostics(row_log_weights):
    '''what a scenario's weights did to the sample, from the log-weight of every row (of the members that
    evaluated): rows; skipped_rows, those whose weight is 0 next to the largest; ess, the Kish effective sample
    size (sum e)^2 / sum e^2; max_share, the largest row's share of the total; log_mean_weight =
    logsumexp - log(rows), for a probe scenario the log predictive density of the new observations.  With every
    row at -inf: ess 0, max_share nan, log_mean_weight -inf.'''
    l = np.asarray(row_log_weights, dtype=np.float64).ravel()
    rows = int(l.size)
    mx = l.max() if rows else -np.inf
    if not np.isfinite(mx):
        return {'rows': rows, 'skipped_rows': rows, 'ess': 0.0, 'max_share': float('nan'),
                'log_mean_weight': float('-inf')}
    e = np.exp(l - mx)
    s1, s2 = float(e.sum()), float((e * e).sum())
    return {'rows': rows, 'skipped_rows': int((e == 0.0).sum()), 'ess': s1 * s1 / s2, 'max_share': float(e.max()) / s1,
            'log_mean_weight': float(mx + np.log(s1) - np.log(rows))}


def check_reweight_maps(maps):
    '''the 'maps' option of reweight=: a subset of REWEIGHT_MAPS ('quantiles', 'arrival', 'contrast', 'excursion') as a tuple in that order,
    () for None; ValueError otherwise'''
    if maps is None:
        return ()
    if isinstance(maps, str):
        raise ValueError("reweight: maps takes a list of names out of %r, got %r" % (REWEIGHT_MAPS, maps))
    try:
        asked = [str(m) for m in maps]
    except TypeError:
        raise ValueError("reweight: maps takes a list of names out of %r, got %r" % (REWEIGHT_MAPS, maps))
    bad = [m for m in asked if m not in REWEIGHT_MAPS]
    if bad or len(set(asked)) != len(asked):
        raise ValueError('reweight: maps %r is not a subset of %r' % (asked, REWEIGHT_MAPS))
    return tuple(m for m in REWEIGHT_MAPS if m in asked)


def check_reweight(reweight, rad_dist=None, rad_res=None, ndays=None):
    '''the reweight= argument of posterior_predictive -> dict(names, kinds, probes, given, log_weights, min_ess):
    {name: dict(probes=[...]) or dict(log_weights=[one 1-D array per chain]), ...} with 1..4 names, and
    optionally 'options': dict(min_ess=50, maps=('quantiles', 'arrival')); with maps the plan also carries `maps`
    (check_reweight_maps).  Per scenario `kinds` is 'probes' or 'log_weights', `probes` the
    checked probes (check_probes) or None, `given` the probes as given, `log_weights` the float64 arrays or None
    (every entry finite or -inf).  ValueError otherwise.'''
    if not isinstance(reweight, dict):
        raise ValueError('reweight must be a dict {name: dict(probes=[...]) or dict(log_weights=[...])}, got %r'
                         % (reweight,))
    specs = dict(reweight)
    options = specs.pop('options', None) or {}
    if not isinstance(options, dict) or set(options) - {'min_ess', 'maps'}:
        raise ValueError("reweight: 'options' takes dict(min_ess=..., maps=...), got %r" % (options,))
    min_ess = float(options.get('min_ess', DEFAULT_MIN_ESS))
    if not (np.isfinite(min_ess) and min_ess >= 0):
        raise ValueError('reweight: min_ess %r is not finite and >= 0' % (options.get('min_ess'),))
    maps = check_reweight_maps(options.get('maps'))
    names = check_scenarios(list(specs))
    out = {'names': names, 'kinds': [], 'probes': [], 'given': [], 'log_weights': [], 'min_ess': min_ess}
    if maps:                          # without the option the plan is what it was
        out['maps'] = maps
    for name in names:
        spec = specs[name]
        if not isinstance(spec, dict) or len(set(spec) & {'probes', 'log_weights'}) != 1 \
                or set(spec) - {'probes', 'log_weights'}:
            raise ValueError('reweight[%r] must be dict(probes=[...]) or dict(log_weights=[...]), got %r'
                             % (name, spec))
        if 'probes' in spec:
            try:
                checked = check_probes(spec['probes'], rad_dist, rad_res, ndays)
            except ValueError as e:
                raise ValueError('reweight[%r]: %s' % (name, e))
            out['kinds'].append('probes')
            out['probes'].append(checked)
            out['given'].append([list(p) for p in spec['probes']])
            out['log_weights'].append(None)
        else:
            try:
                arrs = [np.array(a, dtype=np.float64) for a in spec['log_weights']]
            except (TypeError, ValueError):
                raise ValueError('reweight[%r]: log_weights must be a list of one 1-D array per chain' % name)
            for c, a in enumerate(arrs):
                if a.ndim != 1:
                    raise ValueError('reweight[%r]: the log-weights of chain %d are not 1-D' % (name, c))
                if np.isnan(a).any() or (a == np.inf).any():
                    raise ValueError('reweight[%r]: the log-weights of chain %d hold NaN or +inf' % (name, c))
            out['kinds'].append('log_weights')
            out['probes'].append(None)
            out['given'].append(None)
            out['log_weights'].append(arrs)
    return out


def check_reweight_rows(plan, chain_rows):
    '''the row log-weights of a checked reweight= against the chains' rows after burn and thin; ValueError on a
    wrong number of chains or rows'''
    for name, arrs in zip(plan['names'], plan['log_weights']):
        if arrs is None:
            continue
        if len(arrs) != len(chain_rows):
            raise ValueError('reweight[%r]: log-weights for %d chains, %d chains given' % (name, len(arrs),
                                                                                           len(chain_rows)))
        for c, (a, n) in enumerate(zip(arrs, chain_rows)):
            if a.size != n:
                raise ValueError('reweight[%r]: %d log-weights for chain %d, which has %d rows after burn and thin'
                                 % (name, a.size, c, n))


def reweight_scale(scenarios, refs, log_weights, weight=1):
    '''(r, omega, ref) per scenario for a member with these log-weights (one per name of `scenarios`, or a dict by
    name) and run length `weight`, `refs` the largest log-weight of every scenario so far -- the rule every
    reweighted accumulator shares (ReweightedSummary, ReweightedHistogram, ReweightedArrival):
    lambda = -inf: omega 0;  an empty scenario: ref = lambda, r 1, omega = weight;  lambda > ref:
    r = exp(ref - lambda), ref = lambda, omega = weight;  else r 1, omega = weight * exp(lambda - ref), which
    may underflow to 0 (the member is then skipped).  ValueError for NaN, +inf or a wrong number.'''
    import math
    if isinstance(log_weights, dict):
        if set(log_weights) != set(scenarios):
            raise ValueError('log-weights for %r, the scenarios are %r' % (sorted(log_weights), scenarios))
        log_weights = [log_weights[n] for n in scenarios]
    try:
        lam = [float(v) for v in log_weights]
    except TypeError:
        raise ValueError('log_weights must be one number per scenario, got %r' % (log_weights,))
    if len(lam) != len(scenarios):
        raise ValueError('%d log-weights given, the handle has %d scenarios' % (len(lam), len(scenarios)))
    w = float(weight)
    if not (math.isfinite(w) and w > 0):
        raise ValueError('weight must be finite and > 0')
    r, om, ref = [], [], []
    for lj, rj in zip(lam, refs):
        if math.isnan(lj) or lj == math.inf:
            raise ValueError('log-weight %r is NaN or +inf' % (lj,))
        if lj == -math.inf:
            r.append(1.0), om.append(0.0), ref.append(rj)
        elif rj == -math.inf:
            r.append(1.0), om.append(w), ref.append(lj)
        elif lj > rj:
            r.append(math.exp(rj - lj)), om.append(w), ref.append(lj)
        else:
            r.append(1.0), om.append(w * math.exp(lj - rj)), ref.append(rj)
    return r, om, ref


def reweight_merge_scale(ref_a, ref_b):
    '''(ra, rb, ref) per scenario that bring two reweighted accumulators to the larger of their references:
    L = max(ref_a, ref_b), ra = exp(ref_a - L), rb = exp(ref_b - L); 1 where both are empty'''
    import math
    ra, rb, ref = [], [], []
    for a, b in zip(ref_a, ref_b):
        top = max(a, b)
        ref.append(top)
        ra.append(1.0 if top == -math.inf else math.exp(a - top))
        rb.append(1.0 if top == -math.inf else math.exp(b - top))
    return ra, rb, ref


class ReweightedSummary(_Handle):
    '''The maps of a SpreadSummary under up to 4 reweighting scenarios at once, on the device (ps_wsum_*,
    csrc/ps_wsum.hip): member m counts with the real weight weight_m exp(lambda_m), lambda_m the log-weight the
    caller gives per scenario -- the log-likelihood of new observations under the member (probes_loglik), or any
    other per-member log-weight.  scenarios: 1..4 distinct names; days, thresholds as SpreadSummary (at most 32
    days; thresholds finite, > 0, strictly increasing).  The class keeps the log scale: per scenario `ref`, the
    largest log-weight so far (-inf while the scenario is empty), so that the device only sees weights
    <= weight_m however many orders of magnitude the likelihoods span.  A scenario whose log-weights are all 0
    holds the bits of a SpreadSummary fed alongside.  Importance reweighting degrades as the new data disagree with
    the posterior: watch reweight_diagnostics' ess.'''

    _prefix, _noun = 'ps_wsum', 'reweighted summary'

    def __init__(self, pop_model, scenarios, days=None, thresholds=()):
        self._setup(pop_model, scenarios, _model_days(pop_model, days), thresholds, None)

    @classmethod
    def for_projection(cls, source, scenarios, thresholds=()):
        '''Reweighted maps of the outputs of `source` (a Projection, a ReleaseSites or a PeakMaps), one slot per
        output: `add(log_weights, weight)` accumulates the outputs of its last `apply()`, and the accessors take
        the output index where the day-based maps take a day.'''
        self = cls.__new__(cls)
        nout = getattr(source, 'nout', 1)
        self._setup(source.pm, scenarios, list(range(nout)), thresholds, source)
        return self

    def _setup(self, pop_model, scenarios, days, thresholds, projection):
        import math
        self.scenarios = check_scenarios(scenarios)
        self.thresholds = check_peak_thresholds(thresholds)
        self._set_source(projection, days, projection and getattr(projection, 'live', days))
        n = len(self._slot)
        if not 1 <= n <= MAX_REWEIGHT_SLOTS:
            raise ValueError('%d slots; 1..%d fit one handle' % (n, MAX_REWEIGHT_SLOTS))
        self._attach(pop_model)
        self.ref = [-math.inf] * len(self.scenarios)
        self.nbytes = len(self.scenarios) * (2 + len(self.thresholds)) * 8 * n * self.pitch
        thr = L.f64(self.thresholds if self.thresholds else [0.0])
        self._create(len(self.scenarios), n, len(self.thresholds), L.p_f64(thr))

    def _j(self, name):
        if name not in self.scenarios:
            raise ValueError('scenario %r is not one of %r' % (name, self.scenarios))
        return self.scenarios.index(name)

    def scale(self, log_weights, weight=1):
        '''(r, omega, ref) per scenario that add() would pass for these log-weights, without adding (reweight_scale)'''
        return reweight_scale(self.scenarios, self.ref, log_weights, weight)

    def add(self, log_weights, weight=1):
        '''Accumulate the last evaluation of the model (on a projection, a plan or a peak: its last apply) with
        weight `weight` (the run length) times exp(log_weights[j]) in scenario j; enqueued, no host
        synchronisation.  A refused add changes nothing.'''
        r, om, ref = self.scale(log_weights, weight)
        self._read('add', self._proj, len(self.scenarios), L.p_f64(L.f64(r)), L.p_f64(L.f64(om)))
        # a member whose weight underflowed is skipped and moves no reference
        self.ref = [b if o > 0.0 else a for a, b, o in zip(self.ref, ref, om)]

    def merge(self, other):
        '''self += other (same device, domain, scenarios, days and thresholds), both brought to the larger of the
        two references per scenario: L = max(ref_a, ref_b), ra = exp(ref_a - L), rb = exp(ref_b - L)'''
        import math
        if list(other.days) != self.days or other._slot != self._slot or other.scenarios != self.scenarios:
            raise ValueError('reweighted summaries over different days or scenarios')
        ra, rb, ref = [], [], []
        for a, b in zip(self.ref, other.ref):
            top = max(a, b)
            ref.append(top)
            ra.append(1.0 if top == -math.inf else math.exp(a - top))
            rb.append(1.0 if top == -math.inf else math.exp(b - top))
        self._call('merge', other._h, L.p_f64(L.f64(ra)), L.p_f64(L.f64(rb)))
        self.ref = ref

    def reset(self):
        import math
        self._call('reset')
        self.ref = [-math.inf] * len(self.scenarios)

    def _info(self):
        n = len(self.scenarios)
        w, m, s = np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        self._call('info', L.p_f64(w), L.p_i64(m), L.p_i64(s))
        return w, m, s

    def total_weight(self, name):
        '''W of the scenario on its own scale exp(ref)'''
        return float(self._info()[0][self._j(name)])

    def log_total_weight(self, name):
        '''ref + log W: the log of the scenario's total weight (-inf while it is empty)'''
        import math
        j = self._j(name)
        W = float(self._info()[0][j])
        return -math.inf if W == 0.0 else self.ref[j] + math.log(W)

    def members(self, name):
        return int(self._info()[1][self._j(name)])

    def skipped(self, name):
        return int(self._info()[2][self._j(name)])

    def _fetch(self, name, day, what):
        j = self._j(name)
        slot = self._slot_of(day)
        if slot is None:                                          # an output without weight
            return np.zeros((self.N, self.N), dtype=np.float64)
        return self.fetch_slot(j, slot, what)

    def fetch_slot(self, scen, slot, what):
        '''raw access by scenario and slot index (0 mean, 1 variance, 2 + k exceedance)'''
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('fetch', int(scen), int(slot), int(what), L.p_f64(out))
        return out

    def mean(self, name, day):
        return self._fetch(name, day, 0)

    def variance(self, name, day):
        return self._fetch(name, day, 1)

    def sd(self, name, day):
        return np.sqrt(self.variance(name, day))

    def exceedance(self, name, day, k):
        '''P(population >= thresholds[k]) per cell under the scenario'''
        if not 0 <= k < len(self.thresholds):
            raise ValueError('threshold %r of %d' % (k, len(self.thresholds)))
        return self._fetch(name, day, 2 + k)

    def profile(self, enable=None):
        '''HIP-event time of the add launches: (total ms, launches); enable switches it'''
        return self._profile(enable)



class _ReweightedCounts(_Handle):
    '''What ReweightedHistogram and ReweightedArrival share: the scenarios, the log scale of ReweightedSummary
    (reweight_scale, reweight_merge_scale; per scenario `ref`, the largest log-weight so far), the add, the merge
    and the host-side counters.  Fed alongside a ReweightedSummary with the same log-weights they report the same
    ref, W, members and skipped, bit for bit.'''
    _prof_pairs = 3

    def _scenarios(self, scenarios):
        import math
        self.scenarios = check_scenarios(scenarios)
        self.ref = [-math.inf] * len(self.scenarios)

    def _slots(self):
        n = len(self._slot)
        if not 1 <= n <= MAX_REWEIGHT_SLOTS:
            raise ValueError('%d slots; 1..%d fit one handle' % (n, MAX_REWEIGHT_SLOTS))
        return n

    def _j(self, name):
        if name not in self.scenarios:
            raise ValueError('scenario %r is not one of %r' % (name, self.scenarios))
        return self.scenarios.index(name)

    def scale(self, log_weights, weight=1):
        '''(r, omega, ref) per scenario that add() would pass for these log-weights, without adding (reweight_scale)'''
        return reweight_scale(self.scenarios, self.ref, log_weights, weight)

    def add(self, log_weights, weight=1):
        '''Accumulate the last evaluation of the model (on a projection or a plan: its last apply) with weight `weight`
        (the run length) times exp(log_weights[j]) in scenario j; enqueued, no host synchronisation.  A refused add
        changes nothing.'''
        r, om, ref = self.scale(log_weights, weight)
        self._read('add', self._proj, len(self.scenarios), L.p_f64(L.f64(r)), L.p_f64(L.f64(om)))
        # a member whose weight underflowed is skipped and moves no reference
        self.ref = [b if o > 0.0 else a for a, b, o in zip(self.ref, ref, om)]
        return r, om

    def _check_merge(self, other):
        if list(other.days) != self.days or other._slot != self._slot or other.scenarios != self.scenarios:
            raise ValueError('%ss over different days or scenarios' % self._noun)

    def merge(self, other):
        '''self += other (same device, domain, scenarios and days), both brought to the larger of the two references
        per scenario (reweight_merge_scale); other is unchanged'''
        self._check_merge(other)
        ra, rb, ref = reweight_merge_scale(self.ref, other.ref)
        self._call('merge', other._h, L.p_f64(L.f64(ra)), L.p_f64(L.f64(rb)))
        self.ref = ref

    def reset(self):
        import math
        self._call('reset')
        self.ref = [-math.inf] * len(self.scenarios)

    def _info(self):
        n = len(self.scenarios)
        w, m, s = np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        self._call('info', L.p_f64(w), L.p_i64(m), L.p_i64(s))
        return w, m, s

    def total_weight(self, name):
        '''W of the scenario on its own scale exp(ref)'''
        return float(self._info()[0][self._j(name)])

    def log_total_weight(self, name):
        '''ref + log W: the log of the scenario's total weight (-inf while it is empty)'''
        import math
        j = self._j(name)
        W = float(self._info()[0][j])
        return -math.inf if W == 0.0 else self.ref[j] + math.log(W)

    def members(self, name):
        return int(self._info()[1][self._j(name)])

    def skipped(self, name):
        return int(self._info()[2][self._j(name)])

    def profile(self, enable=None):
        '''HIP-event time of the add, read and rescale launches: (add ms, adds, read ms, reads, rescale ms, rescales);
        enable switches it'''
        return self._profile(enable)


class ReweightedHistogram(_ReweightedCounts):
    '''The histograms of a SpreadHistogram under up to 4 reweighting scenarios at once, on the device (ps_whist_*,
    csrc/ps_whist.hip): member m counts with the real weight weight_m exp(lambda_m) in the bin of its value, by the
    log scale of ReweightedSummary.  scenarios: 1..4 distinct names; days (at most 32), bins and edges as
    SpreadHistogram.  From them the reweighted quantile (median, credible band) of every cell and the exceedance at
    any edge, chosen after the run.  A scenario whose log-weights are all 0 holds the counts of a SpreadHistogram fed
    alongside, and its quantiles and exceedances are that one's bit for bit.  With real weights these are
    floating-point sums: the same calls give the same bits, another order of adds or merges moves a plane within
    the rounding of its sums.'''
    _prefix, _noun = 'ps_whist', 'reweighted histogram'

    def __init__(self, pop_model, scenarios, days=None, bins=DEFAULT_BINS, edges=None):
        self._setup(pop_model, scenarios, _model_days(pop_model, days), bins, edges, None)

    @classmethod
    def for_projection(cls, source, scenarios, bins=DEFAULT_BINS, edges=None):
        '''Reweighted histograms of the outputs of `source` (a Projection or a ReleaseSites), one slot per output:
        `add(log_weights, weight)` accumulates the outputs of its last `apply()`, and the accessors take the output
        index where the day-based histograms take a day.'''
        self = cls.__new__(cls)
        self._setup(source.pm, scenarios, list(range(source.nout)), bins, edges, source)
        return self

    def _setup(self, pop_model, scenarios, days, bins, edges, projection):
        self._edges = bin_edges(bins, edges)
        self.bins = None if edges is not None else tuple(float(b) for b in bins)
        self._scenarios(scenarios)
        self._set_source(projection, days, projection and projection.live)
        n = self._slots()
        self._attach(pop_model)
        J, nedge = len(self.scenarios), self._edges.size
        self.nbytes = J * n * nedge * self.pitch * 8 + n * self.pitch * 4       # the planes + the range words
        try:
            self._create(J, n, nedge, L.p_f64(self._edges))
        except L.HipError as e:
            if e.code != L.PS_ERR_OOM:
                raise
            raise ValueError('reweighted histogram: %d scenarios x %d slots x %d edges x %d cells x 8 B = %.3g GB do '
                             'not fit the free device memory; fewer days, scenarios or bins per decade cut it (%s)'
                             % (J, n, nedge, self.pitch, self.nbytes * 1e-9, e))

    @property
    def edges(self):
        return self._edges.copy()

    def _level(self, p):
        if not 0.0 < float(p) <= 1.0:
            raise ValueError('quantile level %r is not in (0, 1]' % (p,))
        return float(p)

    def _quantile(self, name, day, p):
        '''(value, lower, upper, bin) maps of one scenario and day'''
        j, s, p = self._j(name), self._slot_of(day), self._level(p)
        shape = (self.N, self.N)
        if s is None:                    # an output without weight: every member's value is 0, bin 0 = [0, e_0)
            return np.zeros(shape), np.zeros(shape), np.full(shape, self._edges[0]), np.zeros(shape, dtype=np.int32)
        v, lo, hi = np.empty(shape), np.empty(shape), np.empty(shape)
        b = np.empty(shape, dtype=np.int32)
        self._call('quantile', j, s, p, L.p_f64(v), L.p_f64(lo), L.p_f64(hi), L.p_i32(b))
        return v, lo, hi, b

    def quantile(self, name, day, p):
        '''(value, lower, upper): N x N maps of the scenario's weighted lower quantile at level p -- the point value,
        log-interpolated inside its bin, and the bin [lower, upper) that holds it, as SpreadHistogram's'''
        return self._quantile(name, day, p)[:3]

    def quantile_bin(self, name, day, p):
        '''N x N int32: b*, the smallest bin whose cumulated weight reaches p W'''
        return self._quantile(name, day, p)[3]

    def exceed(self, name, day, k):
        '''P(population >= edges[k]) per cell under the scenario, at any edge'''
        j, k, s = self._j(name), self._index(k, self._edges.size, 'edge'), self._slot_of(day)
        out = np.zeros((self.N, self.N), dtype=np.float64)
        if s is not None:
            self._call('exceed', j, s, k, L.p_f64(out))
        return out

    def plane(self, name, day, b):
        '''N x N float64: the raw weight of bin b (1 .. B + 1) on the scenario's own scale exp(ref)'''
        j, s = self._j(name), self._slot_of(day)
        if not 1 <= int(b) <= self._edges.size:
            raise ValueError('bin %r of 1..%d' % (b, self._edges.size))
        out = np.zeros((self.N, self.N), dtype=np.float64)
        if s is not None:
            self._call('fetch', j, s, int(b), L.p_f64(out))
        return out


class ReweightedArrival(_ReweightedCounts):
    '''The arrival counts of an ArrivalMaps under up to 4 reweighting scenarios at once, on the device (ps_warr_*,
    csrc/ps_warr.hip): when do they reach each cell, given the new observations?  scenarios: 1..4 distinct names;
    thresholds and days as ArrivalMaps.  A scenario whose log-weights are all 0 holds the counts of an ArrivalMaps
    fed alongside, and its probabilities and quantile days are that one's bit for bit.  The class keeps per scenario
    the (log-weight, run length) of every member in add order, for the reached-area curve, which needs no device
    work of its own (`reached_area`).  Floating-point sums as ReweightedHistogram's.'''
    _prefix, _noun = 'ps_warr', 'reweighted arrival maps'

    def __init__(self, pop_model, scenarios, thresholds, days=None):
        self._setup(pop_model, scenarios, thresholds, None,
                    check_arrival_days(range(len(pop_model.days)) if days is None else days))

    @classmethod
    def for_projection(cls, source, scenarios, thresholds):
        '''Reweighted arrival maps of the outputs of `source` (a ReleaseSites or a Projection), the slots its outputs
        that carry weight in ascending order; `days` holds the output labels, as ArrivalMaps.for_projection's.'''
        self = cls.__new__(cls)
        self._setup(source.pm, scenarios, thresholds, source, check_arrival_days(_output_labels(source)))
        return self

    def _setup(self, pop_model, scenarios, thresholds, projection, days):
        self.thresholds = check_arrival_thresholds(thresholds)
        self._scenarios(scenarios)
        self._set_source(projection, days)
        n = self._slots()
        self._attach(pop_model)
        self._member_lw = [[] for _ in self.scenarios]
        self.nbytes = len(self.scenarios) * len(self.thresholds) * n * self.pitch * 8      # the planes
        self._create(len(self.scenarios), n, len(self.thresholds), L.p_f64(L.f64(self.thresholds)))

    def add(self, log_weights, weight=1):
        scaled = super().add(log_weights, weight)      # a refused add raises here and records nothing
        lam = [log_weights[n] for n in self.scenarios] if isinstance(log_weights, dict) else list(log_weights)
        for rows, lj in zip(self._member_lw, lam):
            rows.append((float(lj), float(weight)))
        return scaled

    add.__doc__ = _ReweightedCounts.add.__doc__

    def merge(self, other):
        '''self += other as ReweightedHistogram.merge; other's members follow self's'''
        super().merge(other)
        for rows, more in zip(self._member_lw, other._member_lw):
            rows.extend(more)

    def reset(self):
        super().reset()
        self._member_lw = [[] for _ in self.scenarios]

    def member_log_weights(self, name):
        '''[(log-weight, run length), ...] of every member of the scenario, in add order (the skipped ones too)'''
        return list(self._member_lw[self._j(name)])

    def plane(self, name, k, day):
        '''N x N float64: the raw weight of the members whose arrival day at t_k is `day`, on the scale exp(ref)'''
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('fetch', self._j(name), self._k(k), self._slot_of(day), L.p_f64(out))
        return out

    def prob_by(self, name, k, day):
        '''[N, N] float64: P(arrived at t_k by `day`) under the scenario = min(C / W, 1), C the weight of the
        arrivals up to `day`'''
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('prob', self._j(name), self._k(k), self._slot_of(day), L.p_f64(out))
        return out

    def quantile(self, name, k, p):
        '''[N, N] int32 map of model days: the first day whose C reaches p W under the scenario, -1 where even the
        last day falls short'''
        if not 0.0 < float(p) <= 1.0:
            raise ValueError('quantile level %r is not in (0, 1]' % (p,))
        slot = np.empty((self.N, self.N), dtype=np.int32)
        self._call('quantile', self._j(name), self._k(k), float(p), L.p_i32(slot))
        day = np.append(np.asarray(self.days, dtype=np.int32), np.int32(-1))
        return day[slot]          # slot -1 picks the appended -1

    def member_weights(self, name):
        '''float64 [members]: n exp(lambda - ref) of every member of the scenario in add order, 0 at lambda = -inf'''
        import math
        j = self._j(name)
        ref = self.ref[j]
        return np.array([0.0 if l == -math.inf else n * math.exp(l - ref) for l, n in self._member_lw[j]],
                        dtype=np.float64)

    def reached_area(self, name, k, arrival_maps, levels=(0.05, 0.5, 0.95)):
        '''The reached-area curve of ArrivalMaps.reached_area under the scenario: the members' reached-cell rows of
        `arrival_maps` (the ArrivalMaps fed alongside, same add order) weighted by n exp(lambda - ref) with
        weighted_lower_quantile.  ValueError where the rows and the members of this handle differ in number.'''
        levels = check_levels(levels)
        w = self.member_weights(name)
        cells, _w = arrival_maps.reached(self._k(k))
        if cells.shape[0] != w.size:
            raise ValueError('%d reached-cell rows, the reweighted arrival maps hold %d members' % (cells.shape[0], w.size))
        if list(arrival_maps.days) != list(self.days):
            raise ValueError('arrival maps over different days')
        W = float(w.sum())
        if not W > 0.0:
            raise ValueError('nothing accumulated')
        out = []
        for s, d in enumerate(self.days):
            n = cells[:, s]
            mean = float((n * w).sum()) / W * self.cell_area
            q = [float(weighted_lower_quantile(n, w, p)) * self.cell_area for p in levels]
            out.append({'day': d, 'mean': mean, 'quantiles': q, 'radius_mean': float(np.sqrt(mean / np.pi)),
                        'radius_quantiles': [float(np.sqrt(a / np.pi)) for a in q]})
        return out


def reweighted_coverage_difference(cells_a, cells_b, weights, log_weights, cell_area, levels=(0.05, 0.5, 0.95)):
    '''coverage_difference for members of real weight omega_m = w_m exp(lambda_m - max lambda), the maximum over the
    members with w > 0 and a finite lambda: per output {'mean', 'quantiles', 'p_a_larger', 'p_b_larger'} of the
    signed area A - B in m^2 from the paired per-member cell counts cells_a, cells_b [members, nout], the members'
    integer weights and their log-weights (finite or -inf).  The mean is sum omega d / sum omega, both sums by
    math.fsum; a lower quantile is the smallest distinct d whose cumulative omega (over the sorted distinct d, each
    prefix by math.fsum) is >= p sum omega; p_a_larger (p_b_larger) is the share of sum omega with d > 0 (d < 0).
    With every lambda = 0 these are coverage_difference's numbers exactly.  ValueError when every member is at
    -inf or without weight.'''
    import math
    levels = check_levels(levels)
    a = np.asarray(cells_a, dtype=np.int64)
    b = np.asarray(cells_b, dtype=np.int64)
    w = np.asarray(weights, dtype=np.int64).ravel()
    lam = np.asarray(log_weights, dtype=np.float64).ravel()
    if a.ndim != 2 or a.shape != b.shape or a.shape[0] != w.size or lam.size != w.size:
        raise ValueError('cell counts %r and %r with %d weights and %d log-weights' % (a.shape, b.shape, w.size, lam.size))
    if w.size and w.min() < 0:
        raise ValueError('weights must be >= 0')
    if np.isnan(lam).any() or (lam == np.inf).any():
        raise ValueError('log-weights hold NaN or +inf')
    alive = (w > 0) & np.isfinite(lam)
    if not alive.any():
        raise ValueError('nothing accumulated: every member is at -inf or without weight')
    top = float(lam[alive].max())
    om = [float(wm) * math.exp(float(lm) - top) if ok else 0.0 for wm, lm, ok in zip(w, lam, alive)]
    W = math.fsum(om)
    out = []
    for s in range(a.shape[1]):
        d = a[:, s] - b[:, s]
        by_d = {}
        for dm, o in zip(d.tolist(), om):
            by_d.setdefault(dm, []).append(o)
        distinct = sorted(by_d)
        seen, cum = [], []
        for v in distinct:
            seen.extend(by_d[v])
            cum.append(math.fsum(seen))
        q = []
        for p in levels:
            at = next((i for i, c in enumerate(cum) if c >= float(p) * W), len(distinct) - 1)
            q.append(float(distinct[at]) * float(cell_area))
        out.append({'mean': math.fsum(o * float(dm) for dm, o in zip(d.tolist(), om)) / W * float(cell_area),
                    'quantiles': q,
                    'p_a_larger': math.fsum(o for dm, o in zip(d.tolist(), om) if dm > 0) / W,
                    'p_b_larger': math.fsum(o for dm, o in zip(d.tolist(), om) if dm < 0) / W})
    return out


class ReweightedContrast(_Handle):
    '''The maps of a PlanContrast under up to 4 reweighting scenarios at once, on the device (ps_wcontrast_*,
    csrc/ps_wcontrast.hip): is plan A still better than plan B, now that the traps found this?  `a` and `b` as
    PlanContrast takes them (two ReleaseSites or two Projection, same device, domain and outputs), scenarios and
    the log scale as ReweightedSummary (per scenario `ref`, the largest log-weight so far), thresholds as
    PlanContrast (0..4, finite, > 0, strictly increasing).  After both plans were applied to one member,
    `add(log_weights, weight)` accumulates per output and cell d = a - b with the real weight
    weight exp(log_weights[j]) in scenario j: its weighted mean and M2, the weight of the members with d > 0 and
    with d < 0 and per threshold of those with a >= t_k > b (gain) and b >= t_k > a (loss).  The accessors take the
    scenario's name and the output index; outputs kept off the device read as zeros.  A scenario whose log-weights
    are all 0 holds the bits of a PlanContrast fed alongside.  The per-member coverage rows are that
    PlanContrast's: reweighted_coverage_difference takes them with the members' log-weights.  The ranking of
    several plans, Pareto smoothing, the Monte Carlo error or sensitivity of these maps and any search for a plan
    are not computed.'''

    _prefix, _noun = 'ps_wcontrast', 'reweighted contrast'

    def __init__(self, a, b, scenarios, thresholds=()):
        import math
        _check_paired(a, b)
        self.scenarios = check_scenarios(scenarios)
        self.thresholds = check_contrast_thresholds(thresholds)
        self.a, self.b = a, b
        self._attach(a.pm)
        self.device, self.nout, self.live = a.device, a.nout, list(a.live)
        self.labels = list(getattr(a, 'days', range(a.nout)))
        self._slot = {e: i for i, e in enumerate(self.live)}
        n = len(self.live)
        if not 1 <= n <= MAX_REWEIGHT_SLOTS:
            raise ValueError('%d slots; 1..%d fit one handle' % (n, MAX_REWEIGHT_SLOTS))
        self.ref = [-math.inf] * len(self.scenarios)
        self.nbytes = len(self.scenarios) * (4 + 2 * len(self.thresholds)) * 8 * n * self.pitch
        thr = L.f64(self.thresholds if self.thresholds else [0.0])
        self._create(len(self.scenarios), n, len(self.thresholds), L.p_f64(thr))

    def _j(self, name):
        if name not in self.scenarios:
            raise ValueError('scenario %r is not one of %r' % (name, self.scenarios))
        return self.scenarios.index(name)

    def scale(self, log_weights, weight=1):
        '''(r, omega, ref) per scenario that add() would pass for these log-weights, without adding (reweight_scale)'''
        return reweight_scale(self.scenarios, self.ref, log_weights, weight)

    def add(self, log_weights, weight=1):
        '''Accumulate the last apply of both plans with weight `weight` (the run length) times exp(log_weights[j])
        in scenario j (on the handle's stream behind both; no host synchronisation).  A refused add changes
        nothing.'''
        r, om, ref = self.scale(log_weights, weight)
        self._from_fields('add', self.a, self.b._h, len(self.scenarios), L.p_f64(L.f64(r)), L.p_f64(L.f64(om)))
        # a member whose weight underflowed is skipped and moves no reference
        self.ref = [b if o > 0.0 else a for a, b, o in zip(self.ref, ref, om)]

    def merge(self, other):
        '''self += other (same device, domain, scenarios, outputs and thresholds), both brought to the larger of the
        two references per scenario (reweight_merge_scale); other is unchanged'''
        if other.live != self.live or other.nout != self.nout or list(other.labels) != self.labels \
                or other.scenarios != self.scenarios:
            raise ValueError('reweighted contrasts over different outputs or scenarios')
        ra, rb, ref = reweight_merge_scale(self.ref, other.ref)
        self._call('merge', other._h, L.p_f64(L.f64(ra)), L.p_f64(L.f64(rb)))
        self.ref = ref

    def reset(self):
        import math
        self._call('reset')
        self.ref = [-math.inf] * len(self.scenarios)

    def _info(self):
        n = len(self.scenarios)
        w, m, s = np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        self._call('info', L.p_f64(w), L.p_i64(m), L.p_i64(s))
        return w, m, s

    def total_weight(self, name):
        '''W of the scenario on its own scale exp(ref)'''
        return float(self._info()[0][self._j(name)])

    def log_total_weight(self, name):
        '''ref + log W: the log of the scenario's total weight (-inf while it is empty)'''
        import math
        j = self._j(name)
        W = float(self._info()[0][j])
        return -math.inf if W == 0.0 else self.ref[j] + math.log(W)

    def members(self, name):
        return int(self._info()[1][self._j(name)])

    def skipped(self, name):
        return int(self._info()[2][self._j(name)])

    def fetch_slot(self, scen, slot, what):
        '''raw access by scenario and slot index (0 mean, 1 variance, 2 P(d > 0), 3 P(d < 0), 4 + 2k gain, 5 + 2k loss)'''
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('fetch', int(scen), int(slot), int(what), L.p_f64(out))
        return out

    def _fetch(self, name, e, what):
        j = self._j(name)
        e = self._e(e)
        if e not in self._slot:                                   # an output without weight
            return np.zeros((self.N, self.N), dtype=np.float64)
        return self.fetch_slot(j, self._slot[e], what)

    def mean(self, name, e):
        '''[N, N] float64: the mean of A - B on output e under the scenario'''
        return self._fetch(name, e, 0)

    def variance(self, name, e):
        return self._fetch(name, e, 1)

    def sd(self, name, e):
        return np.sqrt(self.variance(name, e))

    def prob_positive(self, name, e):
        '''P(A > B) per cell under the scenario'''
        return self._fetch(name, e, 2)

    def prob_negative(self, name, e):
        '''P(A < B) per cell under the scenario'''
        return self._fetch(name, e, 3)

    def gain(self, name, e, k):
        '''P(A >= thresholds[k] > B) per cell under the scenario'''
        return self._fetch(name, e, 4 + 2 * self._k(k))

    def loss(self, name, e, k):
        '''P(B >= thresholds[k] > A) per cell under the scenario'''
        return self._fetch(name, e, 5 + 2 * self._k(k))

    def profile(self, enable=None):
        '''HIP-event time of the add launches: (total ms, launches); enable switches it'''
        return self._profile(enable)


class _ReweightFeed():
    '''one chain's side of posterior_predictive(reweight=): the log-weights of every run, by one device gather of
    all probes of all scenarios, and the row log-weights the diagnostics are taken from'''

    def __init__(self, plan, chain):
        self.plan = plan
        self.chain = chain
        self.rows = [[] for _ in plan['names']]        # per scenario the log-weight of every evaluated row
        flat = [p for ps in plan['probes'] if ps is not None for p in ps]
        self.days = sorted({p['day'] for p in flat})
        self.prow = L.i32([p['row'] for p in flat])
        self.pcol = L.i32([p['col'] for p in flat])
        self.pday = [self.days.index(p['day']) for p in flat]

    def log_weights(self, pm, first, length):
        lam = []
        vals = None
        if self.pday:
            got = pm.gather_days(self.days, self.prow, self.pcol)
            vals = [float(got[d, k]) for k, d in enumerate(self.pday)]
        at = 0
        for j, kind in enumerate(self.plan['kinds']):
            if kind == 'probes':
                ps = self.plan['probes'][j]
                lj = probes_loglik(ps, vals[at:at + len(ps)])
                at += len(ps)
                self.rows[j].extend([lj] * length)
            else:
                l = self.plan['log_weights'][j][self.chain][first:first + length]
                lj = run_log_weight(l)
                self.rows[j].extend(float(v) for v in l)
            lam.append(lj)
        return lam


# ------------------------------------------------------------------ catch probability: what a trap would find
MAX_CATCH_IN = 32          # ps_catch: the input records of one launch's descriptors
MAX_CATCH_OUT = 32
MAX_CATCH_COUNT = 16       # the largest count n of P(N >= n) the kernel's series is stated for


def check_traps(traps, what='day'):
    '''traps [(key, rate[, n=1]), ...] as [(key, rate, n), ...]: 1..32 traps, the key (a model day, or the output
    label of a projection or plan) a whole number >= 0, rate finite and > 0, n a whole number in 1..16;
    ValueError otherwise'''
    import math
    try:
        rows = [tuple(t) for t in traps]
    except TypeError:
        raise ValueError('traps must be a list of (%s, rate[, n]), got %r' % (what, traps))
    if not 1 <= len(rows) <= MAX_CATCH_OUT:
        raise ValueError('%d traps; 1..%d fit one handle' % (len(rows), MAX_CATCH_OUT))
    out = []
    for t in rows:
        if len(t) not in (2, 3):
            raise ValueError('a trap is (%s, rate[, n]), got %r' % (what, t))
        try:
            key, rate, n = float(t[0]), float(t[1]), float(t[2]) if len(t) == 3 else 1.0
        except (TypeError, ValueError):
            raise ValueError('a trap is (%s, rate[, n]) of numbers, got %r' % (what, t))
        if not (math.isfinite(key) and key == int(key) and key >= 0):
            raise ValueError('trap %r: the %s must be a whole number >= 0' % (t, what))
        if not (math.isfinite(rate) and rate > 0):
            raise ValueError('trap %r: the rate must be finite and > 0' % (t,))
        if not (math.isfinite(n) and n == int(n) and 1 <= n <= MAX_CATCH_COUNT):
            raise ValueError('trap %r: the count must be a whole number in 1..%d' % (t, MAX_CATCH_COUNT))
        out.append((int(key), rate, int(n)))
    return out


def check_catch_levels(levels):
    '''the levels of a catch summary's `sure` maps as a list: 0..4 probabilities in (0, 1], strictly increasing'''
    try:
        lv = [float(p) for p in levels]
    except TypeError:
        raise ValueError('catch levels must be a list of probabilities, got %r' % (levels,))
    if len(lv) > 4 or any(not 0.0 < p <= 1.0 for p in lv) or any(b <= a for a, b in zip(lv, lv[1:])):
        raise ValueError('catch levels must be at most 4 probabilities in (0, 1], strictly increasing: %r' % (lv,))
    return lv


def check_catch(catch, ndays=None, emergence=None, evaluate=None):
    '''posterior_predictive's catch= argument, dict(traps=[(day, rate[, n]), ...], levels=(0.5, 0.95),
    emergence=[(obs_day, rate[, n]), ...]) -> dict(traps, levels, emergence, given): the checked traps
    (check_traps) over model days < ndays, at most 32 distinct ones; the levels (check_catch_levels); the traps
    over the outputs of the emergence projection, whose key is one of its labels that carries weight -- they
    need posterior_predictive's emergence= argument, passed here -- or None; and the argument as given for the
    json.  evaluate: posterior_predictive's evaluate=, which has no device fields.  ValueError otherwise.'''
    if not isinstance(catch, dict) or 'traps' not in catch or set(catch) - {'traps', 'levels', 'emergence'}:
        raise ValueError('catch must be dict(traps=[(day, rate[, n]), ...], levels=(0.5, 0.95), emergence=None), '
                         'got %r' % (catch,))
    if evaluate is not None:
        raise ValueError('catch= needs the device: not with evaluate=')
    traps = check_traps(catch['traps'])
    for t in traps:
        if ndays is not None and t[0] >= ndays:
            raise ValueError('trap %r: the model has %d days' % (t, ndays))
    if len({t[0] for t in traps}) > MAX_CATCH_IN:
        raise ValueError('the traps name more than %d days' % MAX_CATCH_IN)
    levels = check_catch_levels(catch.get('levels', (0.5, 0.95)))
    em = None
    if catch.get('emergence') is not None:
        if emergence is None:
            raise ValueError('catch[\'emergence\'] needs the emergence= projection')
        em = check_traps(catch['emergence'], 'emergence day')
        W, _in_days, labels = emergence_plan(emergence)
        for t in em:
            if t[0] not in labels or not np.any(W[labels.index(t[0])] != 0):
                raise ValueError('trap %r: %d is not an emergence day that carries weight (%r)' % (t, t[0], labels))
    given = {k: [list(t) for t in v] if k != 'levels' else list(v) for k, v in catch.items() if v is not None}
    return {'traps': traps, 'levels': levels, 'emergence': em, 'given': given}


def parse_traps(text):
    '''the command line's 'KEY,RATE[,N];...' as [(key, rate[, n]), ...] (format_traps is its inverse); the
    values are checked by check_traps, here only the shape'''
    out = []
    for part in str(text).split(';'):
        if not part.strip():
            continue
        f = [x.strip() for x in part.split(',')]
        if len(f) not in (2, 3):
            raise ValueError('a trap is KEY,RATE[,N], got %r' % (part,))
        try:
            out.append((int(f[0]), float(f[1])) + ((int(f[2]),) if len(f) == 3 else ()))
        except ValueError:
            raise ValueError('a trap is KEY,RATE[,N] with whole KEY and N, got %r' % (part,))
    return out


def format_traps(traps):
    return ';'.join(','.join(repr(x) for x in t) for t in traps)


def required_rate(traps, means, day, n, level):
    '''Per cell the smallest listed rate among the traps (key, rate, n) with this (day, n) whose mean catch
    probability means[e] is >= level, NaN where none reaches it: a step function over the ladder of rates the
    user listed, not a search.  Traps of another day or count are ignored; of two traps with the same rate
    either may answer.  ValueError where no trap has this (day, n).'''
    rungs = sorted(((t[1], e) for e, t in enumerate(traps) if t[0] == int(day) and t[2] == int(n)), reverse=True)
    if not rungs:
        raise ValueError('no trap with day %r and count %r' % (day, n))
    out = None
    for rate, e in rungs:                       # descending: the smallest rate that suffices is written last
        m = np.asarray(means[e], dtype=np.float64)
        if out is None:
            out = np.full(m.shape, np.nan)
        out = np.where(m >= level, rate, out)
    return out


class CatchFields(_FieldSource):
    '''Y_e(c) = P(Poisson(rate_e v(c)) >= n_e) of `pop_model`'s last evaluation, on the device (ps_catch_*,
    csrc/ps_catch.hip): what a trap of effort rate_e on model day day_e would find at every cell, under the
    package's own observation model (mcmc.loglik_parts).  traps: [(day, rate[, n=1]), ...] (check_traps), v the
    value SpreadSummary adds for that day; days: the model days the handle reads, default the traps' own (at
    most 32).  `for_projection` reads the outputs of a Projection or a ReleaseSites instead.  The statements of
    the evaluation are fixed in include/parasitoid_hip.h (tests/catch_ref.py restates them): Y is exactly 0
    where v is 0 and lies in [0, 1] elsewhere; P(N = 0) is 1 - Y of an n = 1 trap.  The handle holds
    len(traps) x pitch x 8 B.  SpreadSummary.for_projection, MonteCarloError.for_projection and
    ReweightedSummary.for_projection accept it.'''
    fields_kind = 'catch'        # the accumulators' entry points for these fields: ps_*_add_catch
    _prefix, _noun = 'ps_catch', 'catch fields'
    _items, _item, _check, _max_in = 'traps', 'trap', staticmethod(check_traps), MAX_CATCH_IN

    def __init__(self, pop_model, traps, days=None):
        self._from_days(pop_model, traps, days)

    @classmethod
    def for_projection(cls, source, traps, labels=None):
        '''The catch fields of the outputs of `source` (a Projection or a ReleaseSites): a trap's first entry is
        the source's output label (labels: one per output, default a ReleaseSites' output days, else the output
        indices); `apply()` reads the outputs of the source's last apply.  An output without weight is
        refused.'''
        return cls._over(source, traps, labels)

    def _setup(self, pop_model, inputs, nin):
        self._attach(pop_model)
        self.nout = len(self.traps)
        self.live = list(range(self.nout))
        self.rates = [t[1] for t in self.traps]
        self.counts = [t[2] for t in self.traps]
        self.nbytes = self.nout * self.pitch * 8                 # the output fields
        self._create(int(nin), self.nout, L.p_i32(L.i32(inputs)), L.p_f64(L.f64(self.rates)),
                     L.p_i32(L.i32(self.counts)))



class CatchPosterior():
    '''The posterior of catch fields, as posterior_predictive returns it: `fields` (the CatchFields; closed once
    the chains have run), `traps` [(key, rate, n)], `levels` and `summary`, the
    SpreadSummary.for_projection(fields, levels), which takes the trap's index; `mc_error`: the
    MonteCarloError.for_projection (while the chains run, one chain's two sequences) and `reweight`: the
    ReweightedSummary.for_projection, both None unless asked for; `given`: the driver's catch= argument.'''

    def __init__(self, fields, levels=(0.5, 0.95), mc_batch=None, scenarios=None):
        self.fields = fields
        self.traps = list(fields.traps)
        self.levels = check_catch_levels(levels)
        self.mc_error = None
        self.reweight = None
        self.given = None
        self.summary = SpreadSummary.for_projection(fields, self.levels)
        if mc_batch:
            self.mc_error = [MonteCarloError.for_projection(fields, mc_batch, self.levels) for _half in range(2)]
        if scenarios:
            self.reweight = ReweightedSummary.for_projection(fields, scenarios, self.levels)

    def add(self, weight=1, log_weights=None):
        '''apply the fields to the last evaluation (or the source's last apply) and add them to the summary and,
        with the run's log-weights, to the reweighted summary; the Monte Carlo error sequences are the caller's
        to feed (the run is split between them)'''
        self.fields.apply()
        self.summary.add(weight)
        if self.reweight is not None:
            self.reweight.add(log_weights, weight)

    def merge(self, other):
        if other.traps != self.traps or other.levels != self.levels:
            raise ValueError('catch posteriors over different traps or levels')
        self.summary.merge(other.summary)
        if self.reweight is not None:
            self.reweight.merge(other.reweight)

    def _e(self, e):
        if not 0 <= int(e) < len(self.traps):
            raise ValueError('trap %r of %d' % (e, len(self.traps)))
        return int(e)

    def prob(self, e):
        '''the posterior mean of the catch probability of trap e'''
        return self.summary.mean(self._e(e))

    def sd(self, e):
        '''the posterior sd of the catch probability of trap e (a variance that rounding left below 0 reads as 0)'''
        return np.sqrt(np.maximum(self.summary.variance(self._e(e)), 0.0))

    def sure(self, e, k):
        '''the posterior probability that the member's catch probability of trap e is >= levels[k]'''
        return self.summary.exceedance(self._e(e), k)

    def required_rate(self, day, n=1, level=0.95):
        '''per cell the smallest listed rate of the traps with this (day, n) whose prob() is >= level, NaN where
        none reaches it (required_rate)'''
        use = [e for e, t in enumerate(self.traps) if t[0] == int(day) and t[2] == int(n)]
        means = {e: self.prob(e) for e in use}
        return required_rate(self.traps, means, day, n, level)

    def close(self):
        self.fields.close()
        self.summary.close()
        if self.reweight is not None:
            self.reweight.close()
        if self.mc_error is not None:
            for s in (self.mc_error if isinstance(self.mc_error, (list, tuple)) else [self.mc_error]):
                s.close()


def save_catch(outfile, catch, cell_area=None):
    '''outfile.npz of one CatchPosterior through save_maps: per trap e under the label `c{e}` the CSR triplets
    `c{e}_*` of the posterior mean catch probability, `c{e}_sd_*` and `c{e}_sure{k}_*`; `days` (the traps' days
    or output labels), `rates`, `counts` and `levels` -> its block for
    the json: the traps, levels, members, weight and per trap the largest mean probability and, with a cell
    area, the m^2 where it is >= each level'''
    maps, outs = [], []
    for e, t in enumerate(catch.traps):
        mean = catch.prob(e)
        day_maps = [('', mean), ('_sd', catch.sd(e))]
        day_maps += [('_sure%d' % k, catch.sure(e, k)) for k in range(len(catch.levels))]
        maps.append(('c%d' % e, day_maps))
        outs.append({'trap': list(t), 'max_prob': float(mean.max()),
                     'area': [None if cell_area is None else float((mean >= p).sum() * cell_area)
                              for p in catch.levels]})
    extra = {'days': np.array([t[0] for t in catch.traps], dtype=np.int32),      # in place of save_maps' labels
             'rates': np.array([t[1] for t in catch.traps], dtype=np.float64),
             'counts': np.array([t[2] for t in catch.traps], dtype=np.int32),
             'levels': np.array(catch.levels, dtype=np.float64)}
    save_maps(outfile, maps, extra)
    return {'traps': [list(t) for t in catch.traps], 'levels': list(catch.levels),
            'members': catch.summary.members, 'total_weight': catch.summary.total_weight, 'outputs': outs}


# ------------------------------------------------------------------ neighbourhood maxima: t wasps within r of a cell?
MAX_NBHD_IN = 32           # ps_nbhd: the input records of one launch's descriptors
MAX_NBHD_OUT = 32
MAX_NBHD_HALF = 32         # PS_NBHD_MAX_HALF: the largest half-width of a disc in cells


def check_windows(windows, what='day'):
    '''windows [(key, radius_m), ...] as [(key, radius_m), ...]: 1..32 windows, the key (a model day, or the output
    label of a projection or plan) a whole number >= 0, the radius finite and >= 0; ValueError otherwise'''
    import math
    try:
        rows = [tuple(t) for t in windows]
    except TypeError:
        raise ValueError('windows must be a list of (%s, radius_m), got %r' % (what, windows))
    if not 1 <= len(rows) <= MAX_NBHD_OUT:
        raise ValueError('%d windows; 1..%d fit one handle' % (len(rows), MAX_NBHD_OUT))
    out = []
    for t in rows:
        if len(t) != 2:
            raise ValueError('a window is (%s, radius_m), got %r' % (what, t))
        try:
            key, radius = float(t[0]), float(t[1])
        except (TypeError, ValueError):
            raise ValueError('a window is (%s, radius_m) of numbers, got %r' % (what, t))
        if not (math.isfinite(key) and key == int(key) and key >= 0):
            raise ValueError('window %r: the %s must be a whole number >= 0' % (t, what))
        if not (math.isfinite(radius) and radius >= 0):
            raise ValueError('window %r: the radius must be finite and >= 0' % (t,))
        out.append((int(key), radius))
    return out


def parse_windows(text):
    '''the command line's 'KEY,RADIUS_M;...' as [(key, radius_m), ...]; the values are checked by check_windows,
    here only the shape'''
    out = []
    for part in str(text).split(';'):
        if not part.strip():
            continue
        f = [x.strip() for x in part.split(',')]
        if len(f) != 2:
            raise ValueError('a window is KEY,RADIUS_M, got %r' % (part,))
        try:
            out.append((int(f[0]), float(f[1])))
        except ValueError:
            raise ValueError('a window is KEY,RADIUS_M with a whole KEY, got %r' % (part,))
    return out


def window_cells(radius_m, cell_m):
    '''(r2, H, ncells) of a disc of radius_m on a grid of cell_m: rho = radius_m / cell_m, r2 = floor(rho^2 + 1e-9)
    -- the 1e-9 keeps a radius of exactly k cells at r2 = k^2 where the quotient rounds below k --, H =
    floor(sqrt(r2)) the half-width and ncells the cells (dy, dx) with dy^2 + dx^2 <= r2.  ValueError where
    H > 32, the largest half-width ps_nbhd stages.'''
    import math
    rho = float(radius_m) / float(cell_m)
    if not (math.isfinite(rho) and rho >= 0):
        raise ValueError('radius %r m on cells of %r m' % (radius_m, cell_m))
    if rho >= MAX_NBHD_HALF + 2:      # far out: the square below need not fit an int
        r2 = None
    else:
        r2 = int(math.floor(rho * rho + 1e-9))
    H = None if r2 is None else math.isqrt(r2)
    if H is None or H > MAX_NBHD_HALF:
        raise ValueError('a radius of %g m is %.4g cells of %g m: at most a half-width of %d cells, radii below %g m '
                         'on this grid' % (radius_m, rho, cell_m, MAX_NBHD_HALF, (MAX_NBHD_HALF + 1) * float(cell_m)))
    ncells = sum(2 * math.isqrt(r2 - dy * dy) + 1 for dy in range(-H, H + 1))
    return r2, H, ncells


def check_neighbourhood(neighbourhood, ndays=None, cell_m=None, evaluate=None):
    '''posterior_predictive's neighbourhood= argument, [(day, radius_m), ...] or dict(windows=[...]) ->
    dict(windows, given): the checked windows (check_windows) over model days < ndays, at most 32 distinct ones,
    every radius within the largest disc of a grid of cell_m (window_cells; None: no model at hand), and the
    argument as given for the json.  evaluate: posterior_predictive's evaluate=, which has no device fields.
    ValueError otherwise.'''
    arg = neighbourhood
    if isinstance(arg, dict):
        if 'windows' not in arg or set(arg) - {'windows'}:
            raise ValueError('neighbourhood must be [(day, radius_m), ...] or dict(windows=[...]), got %r' % (arg,))
        arg = arg['windows']
    if evaluate is not None:
        raise ValueError('neighbourhood= needs the device: not with evaluate=')
    windows = check_windows(arg)
    for t in windows:
        if ndays is not None and t[0] >= ndays:
            raise ValueError('window %r: the model has %d days' % (t, ndays))
        if cell_m is not None:
            window_cells(t[1], cell_m)
    if len({t[0] for t in windows}) > MAX_NBHD_IN:
        raise ValueError('the windows name more than %d days' % MAX_NBHD_IN)
    return {'windows': windows, 'given': [list(t) for t in windows]}


class NeighbourhoodFields(_FieldSource):
    '''Z_e(y, x) = max of v over the cells of the domain within radius_e of (y, x), of `pop_model`'s last
    evaluation, on the device (ps_nbhd_*, csrc/ps_nbhd.hip): per member the largest density a search within
    radius_e metres of the cell would meet on model day day_e.  windows: [(day, radius_m), ...] (check_windows),
    v the value SpreadSummary adds for that day; the disc holds the cells with dy^2 + dx^2 <= r2, r2 =
    floor((radius_m / cell_m)^2 + 1e-9) (window_cells; at most a half-width of 32 cells); days: the model days
    the handle reads, default the windows' own (at most 32).  `for_projection` reads the outputs of a Projection
    or a ReleaseSites instead.  Cells outside the domain do not exist; a radius of 0 returns v; the maximum is
    exact, so the fields equal tests/nbhd_ref.py's bit for bit.  The handle holds len(windows) x pitch x 8 B and
    one int32 flag per input and tile of 32 x 64 cells (`nbytes`); `set_skip(False)` stages every tile, which
    changes no output.  SpreadSummary.for_projection, SpreadHistogram.for_projection,
    MonteCarloError.for_projection and ReweightedSummary.for_projection accept it.'''
    fields_kind = 'nbhd'         # the accumulators' entry points for these fields: ps_*_add_nbhd
    _prefix, _noun = 'ps_nbhd', 'neighbourhood fields'
    _items, _item, _check, _max_in = 'windows', 'window', staticmethod(check_windows), MAX_NBHD_IN

    def __init__(self, pop_model, windows, days=None):
        self._from_days(pop_model, windows, days)

    @classmethod
    def for_projection(cls, source, windows, labels=None):
        '''The neighbourhood fields of the outputs of `source` (a Projection or a ReleaseSites): a window's first
        entry is the source's output label (labels: one per output, default a ReleaseSites' output days, else the
        output indices); `apply()` reads the outputs of the source's last apply.  An output without weight is
        refused.'''
        return cls._over(source, windows, labels)

    def _setup(self, pop_model, inputs, nin):
        self._attach(pop_model)
        self.nout = len(self.windows)
        self.live = list(range(self.nout))
        self.radii_m = [t[1] for t in self.windows]
        cell_m = float(pop_model.rad_dist) / int(pop_model.rad_res)
        cells = [window_cells(r, cell_m) for r in self.radii_m]
        self.r2 = [c[0] for c in cells]
        self.half = [c[1] for c in cells]
        self.cells = [c[2] for c in cells]
        tiles = ((self.N + 31) // 32) * ((self.N + 63) // 64)
        self.nbytes = self.nout * self.pitch * 8 + int(nin) * tiles * 4      # the output fields and the tile flags
        self._create(int(nin), self.nout, L.p_i32(L.i32(inputs)), L.p_i32(L.i32(self.r2)))

    def set_skip(self, on=True):
        '''the empty-tile pre-pass of the next applies: on (the default) or off; the outputs are the same'''
        self._call('set_skip', int(bool(on)))

    def profile(self, enable=None):
        '''HIP-event time of the applies, pre-pass included: (total ms, applies); enable switches it'''
        return self._profile(enable)


class NeighbourhoodPosterior():
    '''The posterior of neighbourhood fields, as posterior_predictive returns it: `fields` (the
    NeighbourhoodFields; closed once the chains have run), `windows` [(key, radius_m)], `thresholds` and `summary`,
    the SpreadSummary.for_projection(fields, thresholds), which takes the window's index; `histogram`: the
    SpreadHistogram.for_projection, None without quantile `levels`; `mc_error`: the MonteCarloError.for_projection
    (while the chains run, one chain's two sequences) and `reweight`: the ReweightedSummary.for_projection, both
    None unless asked for; `given`: the driver's neighbourhood= argument.'''

    def __init__(self, fields, thresholds=(), levels=None, bins=DEFAULT_BINS, edges=None, mc_batch=None,
                 scenarios=None):
        self.fields = fields
        self.windows = list(fields.windows)
        self.radii_m, self.r2, self.cells = list(fields.radii_m), list(fields.r2), list(fields.cells)
        self.thresholds = [float(t) for t in thresholds]
        self.levels = list(levels) if levels else None
        self.histogram = self.mc_error = self.reweight = self.given = None
        self.summary = SpreadSummary.for_projection(fields, self.thresholds)
        try:
            if self.levels:
                self.histogram = SpreadHistogram.for_projection(fields, bins, edges)
            if mc_batch:
                self.mc_error = [MonteCarloError.for_projection(fields, mc_batch, self.thresholds)
                                 for _half in range(2)]
            if scenarios:
                self.reweight = ReweightedSummary.for_projection(fields, scenarios, self.thresholds)
        except BaseException:
            self.fields = None           # the caller's (_owned_by) to close
            self.close()
            raise

    def add(self, weight=1, log_weights=None):
        '''apply the fields to the last evaluation (or the source's last apply) and add them to the summary, the
        histogram and, with the run's log-weights, to the reweighted summary; the Monte Carlo error sequences are
        the caller's to feed (the run is split between them)'''
        self.fields.apply()
        self.summary.add(weight)
        if self.histogram is not None:
            self.histogram.add(weight)
        if self.reweight is not None:
            self.reweight.add(log_weights, weight)

    def merge(self, other):
        if other.windows != self.windows or other.thresholds != self.thresholds:
            raise ValueError('neighbourhood posteriors over different windows or thresholds')
        self.summary.merge(other.summary)
        if self.histogram is not None:
            self.histogram.merge(other.histogram)
        if self.reweight is not None:
            self.reweight.merge(other.reweight)

    def _e(self, e):
        if not 0 <= int(e) < len(self.windows):
            raise ValueError('window %r of %d' % (e, len(self.windows)))
        return int(e)

    def maximum(self, e):
        '''the posterior mean of the largest value within the radius of window e'''
        return self.summary.mean(self._e(e))

    def sd(self, e):
        '''its posterior sd (a variance that rounding left below 0 reads as 0)'''
        return np.sqrt(np.maximum(self.summary.variance(self._e(e)), 0.0))

    def prob(self, e, k):
        '''the posterior probability of at least thresholds[k] somewhere within the radius of window e'''
        return self.summary.exceedance(self._e(e), k)

    def quantile(self, e, p):
        '''the weighted lower quantile at level p of the neighbourhood maximum of window e (SpreadHistogram)'''
        if self.histogram is None:
            raise ValueError('no quantile levels were asked for: there is no histogram')
        return self.histogram.quantile(self._e(e), p)

    def close(self):
        accs = [self.fields, self.summary, self.histogram, self.reweight]
        accs += list(self.mc_error) if isinstance(self.mc_error, (list, tuple)) else [self.mc_error]
        for a in accs:
            if a is not None:
                a.close()


def save_neighbourhood(outfile, post, cell_area=None):
    '''outfile.npz of one NeighbourhoodPosterior through save_maps: per window e under the label `n{e}` the CSR
    triplets `n{e}_*` of the posterior mean of the neighbourhood maximum, `n{e}_sd_*`, `n{e}_pexc{k}_*` (the
    probability of at least thresholds[k] within the radius) and, with levels, `n{e}_q{tag}_*`; `days` (the
    windows' days or output labels), `radii_m`, `r2`, `cells` and `thresholds` -> its block for the json: the
    windows, members, weight and per window and threshold, with a cell area, the m^2 where that probability is
    >= 0.5'''
    maps, outs = [], []
    nk = len(post.thresholds)
    for e, t in enumerate(post.windows):
        probs = [post.prob(e, k) for k in range(nk)]
        day_maps = [('', post.maximum(e)), ('_sd', post.sd(e))]
        day_maps += [('_pexc%d' % k, probs[k]) for k in range(nk)]
        day_maps += [('_' + quantile_tag(p), post.quantile(e, p)) for p in (post.levels or ())]
        maps.append(('n%d' % e, day_maps))
        outs.append({'window': list(t), 'r2': post.r2[e], 'cells': post.cells[e],
                     'area': [None if cell_area is None else float((pr >= 0.5).sum() * cell_area) for pr in probs]})
    extra = {'days': np.array([t[0] for t in post.windows], dtype=np.int32),     # in place of save_maps' labels
             'radii_m': np.array(post.radii_m, dtype=np.float64), 'r2': np.array(post.r2, dtype=np.int32),
             'cells': np.array(post.cells, dtype=np.int32),
             'thresholds': np.array(post.thresholds, dtype=np.float64)}
    save_maps(outfile, maps, extra)
    return {'windows': [list(t) for t in post.windows], 'thresholds': list(post.thresholds),
            'levels': list(post.levels or ()), 'members': post.summary.members,
            'total_weight': post.summary.total_weight, 'outputs': outs}


# ------------------------------------------------------------------ proximity: how far is the nearest ground with t?
MAX_PROX_IN = 32           # ps_prox: the input records of one launch's descriptors
MAX_PROX_OUT = 32
MAX_PROX_RADII = 3         # the summary keeps four thresholds; the fourth is far_m (the empty share)
PROX_SIDES = ('to', 'in')


def check_prox_windows(windows, what='day'):
    '''windows [(key, t[, 'to' | 'in']), ...] as [(key, t, side), ...]: 1..32 windows, the key (a model day, or the
    output label of a projection or plan) a whole number >= 0, t finite and > 0, the side 'to' (the distance to
    the ground with at least t, the default) or 'in' (the depth inside it); ValueError otherwise'''
    import math
    try:
        rows = [tuple(t) for t in windows]
    except TypeError:
        raise ValueError("windows must be a list of (%s, t[, 'to' | 'in']), got %r" % (what, windows))
    if not 1 <= len(rows) <= MAX_PROX_OUT:
        raise ValueError('%d windows; 1..%d fit one handle' % (len(rows), MAX_PROX_OUT))
    out = []
    for t in rows:
        if len(t) not in (2, 3):
            raise ValueError("a window is (%s, t[, 'to' | 'in']), got %r" % (what, t))
        try:
            key, thr = float(t[0]), float(t[1])
        except (TypeError, ValueError):
            raise ValueError("a window is (%s, t[, 'to' | 'in']) with numbers first, got %r" % (what, t))
        side = t[2] if len(t) == 3 else 'to'
        if not (math.isfinite(key) and key == int(key) and key >= 0):
            raise ValueError('window %r: the %s must be a whole number >= 0' % (t, what))
        if not (math.isfinite(thr) and thr > 0):
            raise ValueError('window %r: t must be finite and > 0' % (t,))
        if side not in PROX_SIDES:
            raise ValueError("window %r: the side is 'to' or 'in'" % (t,))
        out.append((int(key), thr, side))
    return out


def parse_prox_windows(text):
    '''the command line's 'DAY,T[,in];...' as [(day, t[, side]), ...]; the values are checked by check_prox_windows,
    here only the shape'''
    out = []
    for part in str(text).split(';'):
        if not part.strip():
            continue
        f = [x.strip() for x in part.split(',')]
        if len(f) not in (2, 3):
            raise ValueError('a window is DAY,T[,in], got %r' % (part,))
        try:
            out.append((int(f[0]), float(f[1])) + tuple(f[2:]))
        except ValueError:
            raise ValueError('a window is DAY,T[,in] with a whole DAY, got %r' % (part,))
    return out


def check_ascending(values, what, limit=None):
    '''values as a list of floats, every one finite and > 0, strictly increasing, at most `limit` of them;
    ValueError otherwise'''
    import math
    try:
        out = [float(v) for v in values]
    except (TypeError, ValueError):
        raise ValueError('%s must be a list of numbers, got %r' % (what, values))
    if limit is not None and len(out) > limit:
        raise ValueError('%d %s; at most %d' % (len(out), what, limit))
    if any(not (math.isfinite(v) and v > 0) for v in out):
        raise ValueError('%s must be finite and > 0: %r' % (what, out))
    if any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError('%s must be strictly increasing: %r' % (what, out))
    return out


def prox_far(N, cell_m):
    '''(far2, far_m) of a domain of N cells a side: far2 = 2 (N - 1)^2 + 1, one more than any squared distance
    the domain holds, and its field value sqrt(far2) * cell_m as the device rounds it'''
    far2 = 2 * (int(N) - 1) ** 2 + 1
    return far2, float(np.sqrt(np.float64(far2)) * np.float64(cell_m))


def default_ladder(cell_m, far_m):
    '''cell_m * 2^(j / 4), j = 0, 1, .. up to the first entry above far_m: a quarter octave per rung, about 45
    rungs at R = 400'''
    out, j = [], 0
    while True:
        out.append(float(cell_m) * 2.0 ** (j / 4.0))
        if out[-1] > far_m:
            return out
        j += 1


def check_proximity(proximity, ndays=None, cell_m=None, evaluate=None):
    '''posterior_predictive's proximity= argument, [(day, t[, 'to' | 'in']), ...] or dict(windows=[...],
    radii_m=[...], levels=(...), ladder=[...]) -> dict(windows, radii_m, levels, ladder, given): the checked windows
    (check_prox_windows) over model days < ndays, at most 32 distinct ones; at most 3 radii_m, finite, > 0 and
    strictly increasing (the summary's fourth threshold is far_m); quantile levels in (0, 1] or None; a ladder of
    radii, finite, > 0 and strictly increasing (2..1024), or None for default_ladder; and the argument as given for
    the json.  evaluate: posterior_predictive's evaluate=, which has no device fields.  cell_m is accepted for the
    symmetry with check_neighbourhood: no radius is too large.  ValueError otherwise.'''
    arg, radii, levels, ladder = proximity, (), None, None
    if isinstance(arg, dict):
        if 'windows' not in arg or set(arg) - {'windows', 'radii_m', 'levels', 'ladder'}:
            raise ValueError("proximity must be [(day, t[, 'to' | 'in']), ...] or dict(windows=[...], radii_m=[...], "
                             'levels=(...), ladder=[...]), got %r' % (arg,))
        radii, levels, ladder = arg.get('radii_m') or (), arg.get('levels'), arg.get('ladder')
        arg = arg['windows']
    if evaluate is not None:
        raise ValueError('proximity= needs the device: not with evaluate=')
    windows = check_prox_windows(arg)
    for t in windows:
        if ndays is not None and t[0] >= ndays:
            raise ValueError('window %r: the model has %d days' % (t, ndays))
    if len({t[0] for t in windows}) > MAX_PROX_IN:
        raise ValueError('the windows name more than %d days' % MAX_PROX_IN)
    radii = check_ascending(radii, 'radii_m', MAX_PROX_RADII)
    levels = (check_levels(levels) if levels is not None else []) or None
    if ladder is not None:
        ladder = check_ascending(ladder, 'ladder entries')
        bin_edges(edges=ladder)
    return {'windows': windows, 'radii_m': radii, 'levels': levels, 'ladder': ladder,
            'given': {'windows': [list(t) for t in windows], 'radii_m': radii, 'levels': levels, 'ladder': ladder}}


class ProximityFields(_FieldSource):
    '''Z_e(y, x) = the distance in metres from (y, x) to the nearest cell of the set S_e = {v >= t_e} of
    `pop_model`'s last evaluation, on the device (ps_prox_*, csrc/ps_prox.hip): per member how far from each cell
    the nearest ground lies that holds at least t_e on model day day_e.  windows: [(day, t[, 'to' | 'in']), ...]
    (check_prox_windows), v the value SpreadSummary adds for that day; 'in' measures to the complement of S_e within
    the domain instead: the depth of a reached cell inside the reached ground.  days: the model days the handle
    reads, default the windows' own (at most 32).  `for_projection` reads the outputs of a Projection or a
    ReleaseSites instead.  The squared distance in cells is an exact integer (`d2`), far2 = 2 (N - 1)^2 + 1 where
    the set searched for is empty, and Z = sqrt(d2) * cell_m (`field`; `far_m` at far2): both equal
    tests/prox_ref.py's bit for bit.  Nothing wraps and the domain's edge is not unreached ground.  N <= 32767.  The
    handle holds len(windows) x pitch x 14.125 B (`nbytes`: the metres, d2, the row distances and the set's words);
    `set_strip(w)` narrows the column pass's strip for testing, which changes no output.
    SpreadSummary.for_projection, SpreadHistogram.for_projection, MonteCarloError.for_projection and
    ReweightedSummary.for_projection accept it.'''
    fields_kind = 'prox'         # the accumulators' entry points for these fields: ps_*_add_prox
    _prefix, _noun, _prof_pairs = 'ps_prox', 'proximity fields', 2
    _items, _item, _check, _max_in = 'windows', 'window', staticmethod(check_prox_windows), MAX_PROX_IN

    def __init__(self, pop_model, windows, days=None):
        self._from_days(pop_model, windows, days)

    @classmethod
    def for_projection(cls, source, windows, labels=None):
        '''The proximity fields of the outputs of `source` (a Projection or a ReleaseSites): a window's first entry
        is the source's output label (labels: one per output, default a ReleaseSites' output days, else the output
        indices); `apply()` reads the outputs of the source's last apply.  An output without weight is refused.'''
        return cls._over(source, windows, labels)

    def _setup(self, pop_model, inputs, nin):
        self._attach(pop_model)
        self.nout = len(self.windows)
        self.live = list(range(self.nout))
        self.thresholds = [t[1] for t in self.windows]
        self.sides = [t[2] for t in self.windows]
        self.cell_m = float(pop_model.rad_dist) / int(pop_model.rad_res)
        self.far2, self.far_m = prox_far(self.N, self.cell_m)
        self.nbytes = self.nout * self.pitch * 14 + self.nout * self.pitch // 8
        self._create(int(nin), self.nout, L.p_i32(L.i32(inputs)), L.p_f64(L.f64(self.thresholds)),
                     L.p_i32(L.i32([PROX_SIDES.index(s) for s in self.sides])), self.cell_m)

    def set_strip(self, width=0):
        '''testing: the columns of one workgroup's strip in the next applies, a power of two up to the default; 0:
        the default; the outputs are the same'''
        self._call('set_strip', int(width))

    def _counter(self, k):
        out = [C.c_int(), C.c_int(), C.c_int(), C.c_int64(), C.c_int()]
        self._call('info', *[C.byref(v) for v in out])
        return out[k].value

    @property
    def applies(self):
        return self._counter(3)

    @property
    def strip(self):
        '''the columns of one workgroup's strip in the column pass'''
        return self._counter(4)

    def d2(self, e):
        '''[N, N] uint32: the squared distance of output e in cells, far2 where the set searched for is empty'''
        out = np.empty((self.N, self.N), dtype=np.uint32)
        self._call('fetch_d2', self._e(e), out.ctypes.data_as(C.POINTER(C.c_uint32)))
        return out

    def profile(self, enable=None):
        '''HIP-event time of the applies: (ms of the set and the row pass, applies, ms of the column pass,
        applies); enable switches it'''
        return self._profile(enable)


def ladder_radius(edges, exceed, level):
    '''Per cell the smallest edge r with P(d < r) = 1 - exceed(r) >= level, NaN where none reaches it: a step
    function over the ladder, read off the exact exceedance at the edges as required_rate reads the ladder of
    rates.  exceed(r) -> the N x N map P(d >= r).'''
    out = None
    for r in sorted((float(x) for x in edges), reverse=True):   # descending: the smallest that suffices is written last
        near = 1.0 - np.asarray(exceed(r), dtype=np.float64)
        if out is None:
            out = np.full(near.shape, np.nan)
        out = np.where(near >= level, r, out)
    return out


class ProximityPosterior():
    '''The posterior of proximity fields, as posterior_predictive returns it: `fields` (the ProximityFields; closed
    once the chains have run), `windows` [(key, t, side)], `radii_m` (at most 3) and `summary`, the
    SpreadSummary.for_projection(fields, radii_m + [far_m]), which takes the window's index; `histogram`: the
    SpreadHistogram.for_projection on the `ladder` of radii (default_ladder unless given), None without quantile
    `levels`; `mc_error`: the MonteCarloError.for_projection (while the chains run, one chain's two sequences) and
    `reweight`: the ReweightedSummary.for_projection, both None unless asked for; `given`: the driver's proximity=
    argument.  A member whose set is empty enters every cell at `far_m`, one step beyond the domain's diagonal:
    `mean` and `sd` include those members at far_m, and `empty_share` is their share of the weight.'''

    def __init__(self, fields, radii_m=(), levels=None, ladder=None, mc_batch=None, scenarios=None):
        self.fields = fields
        self.windows = list(fields.windows)
        self.far_m, self.far2, self.cell_m = fields.far_m, fields.far2, fields.cell_m
        self.radii_m = check_ascending(radii_m, 'radii_m', MAX_PROX_RADII)
        self.thresholds = self.radii_m + [self.far_m]
        self.levels = list(levels) if levels else None
        self.ladder = None
        self.histogram = self.mc_error = self.reweight = self.given = None
        self.summary = SpreadSummary.for_projection(fields, self.thresholds)
        try:
            if self.levels:
                self.ladder = (default_ladder(self.cell_m, self.far_m) if ladder is None
                               else check_ascending(ladder, 'ladder entries'))
                self.histogram = SpreadHistogram.for_projection(fields, edges=self.ladder)
            if mc_batch:
                self.mc_error = [MonteCarloError.for_projection(fields, mc_batch, self.thresholds)
                                 for _half in range(2)]
            if scenarios:
                self.reweight = ReweightedSummary.for_projection(fields, scenarios, self.thresholds)
        except BaseException:
            self.fields = None           # the caller's (_owned_by) to close
            self.close()
            raise

    def add(self, weight=1, log_weights=None):
        '''apply the fields to the last evaluation (or the source's last apply) and add them to the summary, the
        histogram and, with the run's log-weights, to the reweighted summary; the Monte Carlo error sequences are
        the caller's to feed (the run is split between them)'''
        self.fields.apply()
        self.summary.add(weight)
        if self.histogram is not None:
            self.histogram.add(weight)
        if self.reweight is not None:
            self.reweight.add(log_weights, weight)

    def merge(self, other):
        if other.windows != self.windows or other.thresholds != self.thresholds or other.ladder != self.ladder:
            raise ValueError('proximity posteriors over different windows, radii or ladders')
        self.summary.merge(other.summary)
        if self.histogram is not None:
            self.histogram.merge(other.histogram)
        if self.reweight is not None:
            self.reweight.merge(other.reweight)

    def _e(self, e):
        if not 0 <= int(e) < len(self.windows):
            raise ValueError('window %r of %d' % (e, len(self.windows)))
        return int(e)

    def _k(self, k):
        if not 0 <= int(k) < len(self.radii_m):
            raise ValueError('radius %r of %d' % (k, len(self.radii_m)))
        return int(k)

    def mean(self, e):
        '''the posterior mean of the distance of window e in metres, the members without such ground at far_m'''
        return self.summary.mean(self._e(e))

    def sd(self, e):
        '''its posterior sd (a variance that rounding left below 0 reads as 0)'''
        return np.sqrt(np.maximum(self.summary.variance(self._e(e)), 0.0))

    def beyond(self, e, k):
        '''P(d >= radii_m[k]): the posterior probability that no such ground lies within radii_m[k] of the cell'''
        return self.summary.exceedance(self._e(e), self._k(k))

    def nearer(self, e, k):
        '''P(d < radii_m[k]) = 1 - beyond'''
        return 1.0 - self.beyond(e, k)

    def empty_share(self, e):
        '''the share of the weight of the members whose set was empty: the summary's exceedance at far_m, the same
        at every cell'''
        return float(self.summary.exceedance(self._e(e), len(self.radii_m))[0, 0])

    def quantile(self, e, p):
        '''the weighted lower quantile at level p of the distance of window e (SpreadHistogram, on the ladder)'''
        if self.histogram is None:
            raise ValueError('no quantile levels were asked for: there is no histogram')
        return self.histogram.quantile(self._e(e), p)

    def radius(self, e, level):
        '''per cell the smallest ladder radius r with P(d < r) >= level, NaN where none reaches it
        (ladder_radius over the histogram's exact exceedance at its edges).  The last rung of the default ladder
        lies beyond far_m: a cell that reads it has no such ground within the domain at that level.'''
        if self.histogram is None:
            raise ValueError('no quantile levels were asked for: there is no histogram')
        if not 0.0 < float(level) <= 1.0:
            raise ValueError('level %r is not in (0, 1]' % (level,))
        e = self._e(e)
        return ladder_radius(self.histogram.edges, lambda r: self.histogram.exceedance(e, r), float(level))

    def close(self):
        accs = [self.fields, self.summary, self.histogram, self.reweight]
        accs += list(self.mc_error) if isinstance(self.mc_error, (list, tuple)) else [self.mc_error]
        for a in accs:
            if a is not None:
                a.close()


def save_proximity(outfile, post, cell_area=None):
    '''outfile.npz of one ProximityPosterior through save_maps: per window e under the label `x{e}` the CSR
    triplets `x{e}_*` of the posterior mean of the distance in metres, `x{e}_sd_*`, `x{e}_pnear{k}_*` (the
    probability of such ground within radii_m[k]) and, with levels, `x{e}_q{tag}_*`; `days` (the windows' days or
    output labels), `thresholds`, `sides`, `radii_m`, `ladder`, `far_m` and `empty_share` -> its block for the
    json: the windows, members, weight and per window the empty share and, with a cell area, per radius the m^2
    where that probability is >= 0.5'''
    maps, outs = [], []
    nk = len(post.radii_m)
    shares = [post.empty_share(e) for e in range(len(post.windows))]
    for e, t in enumerate(post.windows):
        near = [post.nearer(e, k) for k in range(nk)]
        day_maps = [('', post.mean(e)), ('_sd', post.sd(e))]
        day_maps += [('_pnear%d' % k, near[k]) for k in range(nk)]
        day_maps += [('_' + quantile_tag(p), post.quantile(e, p)) for p in (post.levels or ())]
        maps.append(('x%d' % e, day_maps))
        outs.append({'window': list(t), 'empty_share': shares[e],
                     'area': [None if cell_area is None else float((pr >= 0.5).sum() * cell_area) for pr in near]})
    extra = {'days': np.array([t[0] for t in post.windows], dtype=np.int32),     # in place of save_maps' labels
             'thresholds': np.array([t[1] for t in post.windows], dtype=np.float64),
             'sides': np.array([t[2] for t in post.windows]),
             'radii_m': np.array(post.radii_m, dtype=np.float64),
             'ladder': np.array(post.ladder or (), dtype=np.float64),
             'far_m': np.float64(post.far_m), 'empty_share': np.array(shares, dtype=np.float64)}
    save_maps(outfile, maps, extra)
    return {'windows': [list(t) for t in post.windows], 'radii_m': list(post.radii_m),
            'levels': list(post.levels or ()), 'far_m': post.far_m, 'members': post.summary.members,
            'total_weight': post.summary.total_weight, 'outputs': outs}


# ------------------------------------------------------------------ trap information: what a catch would teach
MAX_GAIN_IN = 32           # ps_gain: the input records of one launch's descriptors
MAX_GAIN_PLANES = 32       # the planes of all traps of one handle: the slots of one accumulator
MAX_GAIN_YMAX = 15         # the largest count a trap resolves: the classes 0 .. ymax and ">= ymax + 1"


def check_info_traps(traps, what='day'):
    '''traps [(key, rate[, ymax=0]), ...] as [(key, rate, ymax), ...]: at least one trap, the key (a model day, or
    the output label of a projection or plan) a whole number >= 0, rate finite and > 0, ymax a whole number in
    0..15, and at most 32 planes in all, ymax + 3 per trap; ValueError otherwise'''
    import math
    try:
        rows = [tuple(t) for t in traps]
    except TypeError:
        raise ValueError('traps must be a list of (%s, rate[, ymax]), got %r' % (what, traps))
    if not rows:
        raise ValueError('no traps; at least one is needed')
    out = []
    for t in rows:
        if len(t) not in (2, 3):
            raise ValueError('a trap is (%s, rate[, ymax]), got %r' % (what, t))
        try:
            key, rate, ymax = float(t[0]), float(t[1]), float(t[2]) if len(t) == 3 else 0.0
        except (TypeError, ValueError):
            raise ValueError('a trap is (%s, rate[, ymax]) of numbers, got %r' % (what, t))
        if not (math.isfinite(key) and key == int(key) and key >= 0):
            raise ValueError('trap %r: the %s must be a whole number >= 0' % (t, what))
        if not (math.isfinite(rate) and rate > 0):
            raise ValueError('trap %r: the rate must be finite and > 0' % (t,))
        if not (math.isfinite(ymax) and ymax == int(ymax) and 0 <= ymax <= MAX_GAIN_YMAX):
            raise ValueError('trap %r: ymax must be a whole number in 0..%d' % (t, MAX_GAIN_YMAX))
        out.append((int(key), rate, int(ymax)))
    planes = sum(t[2] + 3 for t in out)
    if planes > MAX_GAIN_PLANES:
        raise ValueError('the traps own %d planes (ymax + 3 each); at most %d fit one handle'
                         % (planes, MAX_GAIN_PLANES))
    return out


def check_information(information, ndays=None, evaluate=None):
    '''posterior_predictive's information= argument, dict(traps=[(day, rate[, ymax]), ...]) -> dict(traps, given):
    the checked traps (check_info_traps) over model days < ndays and the argument as given for the json.
    evaluate: posterior_predictive's evaluate=, which has no device fields.  ValueError otherwise.'''
    if not isinstance(information, dict) or set(information) != {'traps'}:
        raise ValueError('information must be dict(traps=[(day, rate[, ymax]), ...]), got %r' % (information,))
    if evaluate is not None:
        raise ValueError('information= needs the device: not with evaluate=')
    traps = check_info_traps(information['traps'])
    for t in traps:
        if ndays is not None and t[0] >= ndays:
            raise ValueError('trap %r: the model has %d days' % (t, ndays))
    if len({t[0] for t in traps}) > MAX_GAIN_IN:
        raise ValueError('the traps name more than %d days' % MAX_GAIN_IN)
    return {'traps': traps, 'given': {'traps': [list(t) for t in information['traps']]}}


def weight_entropy(weights):
    '''-sum (w / W) log (w / W) of the member weights, in nats: the most any map of the ensemble can tell about
    which member is true, so no information map can exceed it'''
    w = np.asarray([x for x in weights if x > 0], dtype=np.float64)
    if w.size == 0:
        return 0.0
    q = w / w.sum()
    return float(-(q * np.log(q)).sum())


class InformationFields(_FieldSource):
    '''One member's whole count distribution at every cell for traps the user describes, on the device
    (ps_gain_*, csrc/ps_gain.hip): trap e = (day, rate[, ymax=0]) observes Poisson(rate v) as the classes 0, 1,
    .., ymax and ">= ymax + 1" (ymax = 0: found / none), v the value SpreadSummary adds for that day, under the
    package's own observation model (mcmc.loglik_parts).  Trap e owns ymax + 3 planes: 'd0' = 1 - P(0), 'p1' ..
    'p{ymax}', 'tail' = P(>= ymax + 1) and 'h', the entropy of the class distribution in nats; every plane is
    exactly 0 where v is 0.  At most 32 planes in all.  days: the model days the handle reads, default the traps'
    own.  `for_projection` reads the outputs of a Projection or a ReleaseSites instead.  The statements are fixed
    in include/parasitoid_hip.h (tests/gain_ref.py restates them).  SpreadSummary.for_projection and
    ReweightedSummary.for_projection accept it, one slot per plane; InformationPosterior turns their means into
    the information maps.'''
    fields_kind = 'gain'         # the accumulators' entry points for these fields: ps_*_add_gain
    _prefix, _noun, _info_n = 'ps_gain', 'information fields', 5
    _items, _item, _check, _max_in = 'traps', 'trap', staticmethod(check_info_traps), MAX_GAIN_IN

    def __init__(self, pop_model, traps, days=None):
        self._from_days(pop_model, traps, days)

    @classmethod
    def for_projection(cls, source, traps, labels=None):
        '''The information fields of the outputs of `source` (a Projection or a ReleaseSites): a trap's first
        entry is the source's output label (labels: one per output, default a ReleaseSites' output days, else the
        output indices); `apply()` reads the outputs of the source's last apply.  An output without weight is
        refused.'''
        return cls._over(source, traps, labels)

    def _setup(self, pop_model, inputs, nin):
        self._attach(pop_model)
        self.ntrap = len(self.traps)
        self.rates = [t[1] for t in self.traps]
        self.ymax = [t[2] for t in self.traps]
        self.base = [sum(y + 3 for y in self.ymax[:e]) for e in range(self.ntrap)]
        self.nout = sum(y + 3 for y in self.ymax)           # the planes: the slots of an accumulator over them
        self.live = list(range(self.nout))
        self.nbytes = (self.nout + 3 * self.ntrap) * self.pitch * 8      # the planes and three maps per trap
        self._create(int(nin), self.ntrap, L.p_i32(L.i32(inputs)), L.p_f64(L.f64(self.rates)),
                     L.p_i32(L.i32(self.ymax)))

    field = property()     # none: a trap's planes go by name (`plane`), and `_e` is a trap's index

    def _e(self, e):
        return self._index(e, self.ntrap, 'trap')

    def plane_names(self, e):
        '''the names of trap e's planes: 'd0', 'p1' .. 'p{ymax}', 'tail' and 'h', in this order'''
        return ['d0'] + ['p%d' % y for y in range(1, self.ymax[self._e(e)] + 1)] + ['tail', 'h']

    def plane_index(self, e, name):
        '''the handle's plane (an accumulator's slot) of trap e's plane `name`'''
        names = self.plane_names(e)
        if name not in names:
            raise ValueError('plane %r of trap %d is not one of %r' % (name, e, names))
        return self.base[int(e)] + names.index(name)

    def plane(self, e, name):
        '''[N, N] float64: plane `name` ('d0', 'p1' .., 'tail', 'h') of trap e of the last apply'''
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('fetch', self.plane_index(e, name), L.p_f64(out))
        return out

    def finish(self, accumulator, scenario=None):
        '''the information maps of every trap from the mean planes of `accumulator`, a
        SpreadSummary.for_projection(self) or, with the scenario's name, a ReweightedSummary.for_projection(self);
        on the device, no host synchronisation; `result` fetches them'''
        if scenario is None:
            self._call('finish_summary', accumulator._h)
        else:
            self._call('finish_wsum', accumulator._h, accumulator._j(scenario))

    def result(self, e, what):
        '''[N, N] float64 of the last finish: what 'gain' (the mutual information in nats), 'entropy' (of the
        posterior predictive class distribution) or 'conditional' (the mean entropy of the members')'''
        names = ('gain', 'entropy', 'conditional')
        if what not in names:
            raise ValueError('%r is not one of %r' % (what, names))
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('fetch_result', self._e(e), names.index(what), L.p_f64(out))
        return out



class InformationPosterior():
    '''The information maps of described traps, as posterior_predictive returns them: `fields` (the
    InformationFields, which also holds the finished maps), `traps` [(key, rate, ymax)], `summary`, the
    SpreadSummary.for_projection(fields) without thresholds, whose slots are the fields' planes; `reweight`: the
    ReweightedSummary.for_projection, None unless asked for; `weights`: the weight of every member added, in
    order, and `cap`, their entropy (weight_entropy): no finite ensemble can show a larger gain, and near it the
    gain is an upper-biased estimate bounded by the ensemble, not by the trap; `given`: the driver's
    information= argument.  The gain is in nats and a lower bound of the uncoarsened count's information.'''

    def __init__(self, fields, scenarios=None):
        self.fields = fields
        self.traps = list(fields.traps)
        self.reweight = None
        self.given = None
        self.weights = []
        self.summary = SpreadSummary.for_projection(fields)
        if scenarios:
            self.reweight = ReweightedSummary.for_projection(fields, scenarios)
        self._finished = ()            # the source of the fields' finished maps: (scenario,), () for none

    def add(self, weight=1, log_weights=None):
        '''apply the fields to the last evaluation (or the source's last apply) and add the planes to the summary
        and, with the run's log-weights, to the reweighted summary'''
        self.fields.apply()
        self.summary.add(weight)
        if self.reweight is not None:
            self.reweight.add(log_weights, weight)
        self.weights.append(int(weight))
        self._finished = ()

    def merge(self, other):
        if other.traps != self.traps:
            raise ValueError('information posteriors over different traps')
        self.summary.merge(other.summary)
        if self.reweight is not None:
            self.reweight.merge(other.reweight)
        self.weights.extend(other.weights)
        self._finished = ()

    @property
    def cap(self):
        return weight_entropy(self.weights)

    def pmf(self, e, y):
        '''the posterior predictive probability that trap e's count is y (y = ymax + 1: at least that)'''
        f = self.fields
        ymax = f.ymax[f._e(e)]
        if not (y == int(y) and 0 <= y <= ymax + 1):
            raise ValueError('class %r of trap %d is not in 0..%d' % (y, e, ymax + 1))
        m = self.summary.mean(f.base[int(e)] + int(y))
        return 1.0 - m if int(y) == 0 else m

    def _result(self, e, what, scenario=None):
        if scenario is not None and self.reweight is None:
            raise ValueError('no reweighted maps: scenario %r needs reweight=' % (scenario,))
        if self._finished != (scenario,):
            self.fields.finish(self.summary if scenario is None else self.reweight, scenario)
            self._finished = (scenario,)
        return self.fields.result(e, what)

    def gain(self, e, scenario=None):
        '''the mutual information in nats between trap e's count and the identity of the member, per cell: the
        expected Kullback-Leibler divergence from this posterior to the reweighted one after the reading; with a
        scenario's name from the reweighted means -- after that scenario's observations'''
        return self._result(e, 'gain', scenario)

    def entropy(self, e):
        '''the entropy of the posterior predictive class distribution of trap e'''
        return self._result(e, 'entropy')

    def conditional(self, e):
        '''the posterior mean of the entropy of the member's own class distribution, H(count | member)'''
        return self._result(e, 'conditional')

    def close(self):
        self.fields.close()
        self.summary.close()
        if self.reweight is not None:
            self.reweight.close()


def save_information(outfile, info, cell_area=None):
    '''outfile.npz of one InformationPosterior through save_maps: per trap e under the label `i{e}` the CSR
    triplets `i{e}_gain_*`, `i{e}_entropy_*`, `i{e}_d0_*` (1 - P(count = 0), the deficit, so that the triplets stay
    sparse) and `i{e}_p{y}_*` for y = 1 .. ymax + 1 (the last: at least that); `days` (the traps' days or output
    labels), `rates`, `ymax` -> its block for the json: the traps, members, weight, `cap` and per trap the largest
    gain and, with a cell area, the m^2 where the gain reaches half of it'''
    maps, outs = [], []
    for e, t in enumerate(info.traps):
        g = info.gain(e)
        trap_maps = [('_gain', g), ('_entropy', info.entropy(e)), ('_d0', 1.0 - info.pmf(e, 0))]
        trap_maps += [('_p%d' % y, info.pmf(e, y)) for y in range(1, t[2] + 2)]
        maps.append(('i%d' % e, trap_maps))
        top = float(g.max())
        outs.append({'trap': list(t), 'max_gain': top,
                     'half_area': None if cell_area is None or not top > 0
                     else float((g >= 0.5 * top).sum() * cell_area)})
    extra = {'days': np.array([t[0] for t in info.traps], dtype=np.int32),
             'rates': np.array([t[1] for t in info.traps], dtype=np.float64),
             'ymax': np.array([t[2] for t in info.traps], dtype=np.int32)}
    save_maps(outfile, maps, extra)
    return {'traps': [list(t) for t in info.traps], 'members': info.summary.members,
            'total_weight': info.summary.total_weight, 'cap': info.cap, 'units': 'nats', 'outputs': outs}


def warn_information(info, what='information'):
    '''a UserWarning where a trap's largest gain exceeds cap / 2: the map is then bounded by the ensemble, not by
    the trap -> the largest gain per trap'''
    import warnings
    cap = info.cap
    tops = [float(info.gain(e).max()) for e in range(len(info.traps))]
    for e, top in enumerate(tops):
        if top > 0.5 * cap:
            warnings.warn('%s: the largest gain of trap %r, %.3g nats, exceeds half the ensemble\'s cap of %.3g nats '
                          '(%d members): the map is bounded by the ensemble, not by the trap'
                          % (what, info.traps[e], top, cap, len(info.weights)), UserWarning, stacklevel=3)
    return tops


# ------------------------------------------------------------------ origin maps: where did these wasps come from?
MAX_ORIGIN_FINDINGS = 64   # ps_origin: the findings, their distinct days, the hypotheses and their distinct lags
MAX_ORIGIN_DAYS = 32
MAX_ORIGIN_HYPOTHESES = 8
MAX_ORIGIN_LAGS = 4
ORIGIN_KIND_CODE = {'count': 0, 'none': 1, 'found': 2}


def parse_origin(text):
    '''"east,north,day,kind,rate[,n];..." -> [(east_m, north_m, day, kind, rate[, n]), ...]; ValueError if malformed'''
    out = []
    for item in str(text).split(';'):
        parts = [s.strip() for s in item.split(',')]
        if not item.strip():
            continue
        if len(parts) not in (5, 6):
            raise ValueError('finding %r is not east,north,day,kind,rate[,n]' % item)
        try:
            row = (float(parts[0]), float(parts[1]), int(parts[2]), parts[3], float(parts[4]))
            if len(parts) == 6:
                row = row + (int(parts[5]),)
        except ValueError:
            raise ValueError('finding %r is not east,north,day,kind,rate[,n]' % item)
        out.append(row)
    if not out:
        raise ValueError('no finding in %r' % (text,))
    return out


def parse_origin_known(text):
    '''"east,north,amount[,lag];..." -> [(east_m, north_m, amount[, lag_days]), ...], or 'sites' for the word itself;
    ValueError if malformed'''
    if str(text).strip() == 'sites':
        return 'sites'
    out = []
    for item in str(text).split(';'):
        if not item.strip():
            continue
        parts = [x.strip() for x in item.split(',')]
        try:
            if len(parts) not in (3, 4):
                raise ValueError
            row = (float(parts[0]), float(parts[1]), float(parts[2])) + ((int(parts[3]),) if len(parts) == 4 else ())
        except ValueError:
            raise ValueError('known release %r is not east,north,amount[,lag]' % item)
        out.append(row)
    if not out:
        raise ValueError('no known release in %r' % (text,))
    return out


def origin_request(findings, amounts='', lags='', levels='', prior='', rad_dist=None, rad_res=None, known='',
                   sites=None):
    '''the origin= argument from the command line's strings: findings 'east,north,day,kind,rate[,n];...', amounts
    '0.1,1,10', lags '0,2', levels '0.5,0.95', prior the path of an .npy plane, known 'east,north,amount[,lag];...'
    or 'sites' (the release sites of the run's own plan, `sites`); empty strings leave the defaults.
    Checked (check_origin) before it is returned; ValueError otherwise.'''
    def numbers(text, kind, what):
        try:
            return [kind(x) for x in str(text).split(',') if x.strip()]
        except ValueError:
            raise ValueError('%s %r is not a list of numbers' % (what, text))
    arg = {'findings': parse_origin(findings)}
    if amounts:
        arg['amounts'] = numbers(amounts, float, 'amounts')
    if lags:
        arg['lags'] = numbers(lags, int, 'lags')
    if levels:
        arg['levels'] = numbers(levels, float, 'levels')
    if prior:
        arg['prior'] = np.load(prior)
    if known:
        arg['known'] = parse_origin_known(known)
    check_origin(arg, rad_dist, rad_res, sites=sites)
    return arg


MAX_ORIGIN_KNOWN_LAGS = 4


def check_origin_known(known, rad_dist, rad_res, ndays=None, sites=None):
    '''The known= key of origin=: releases that are facts, not hypotheses -- [(east_m, north_m, amount[, lag_days]),
    ...] as check_sites takes them (1..32, amount > 0 in multiples of the release number, the smallest lag 0), on at
    most 4 distinct lags, each below ndays; or 'sites': the sites of the run's own plan, `sites` (the driver's).  A
    known release after the last finding is allowed: it contributes 0.  -> the checked sites.  ValueError with the
    offender named.'''
    if isinstance(known, str):
        if known != 'sites':
            raise ValueError("origin: known must be a list of (east_m, north_m, amount[, lag_days]) or 'sites', got %r"
                             % (known,))
        if sites is None:
            raise ValueError("origin: known='sites' takes the sites of the run's own sites= plan, and there is none")
        known = sites
    try:
        out = check_sites(known, rad_dist, rad_res)
    except ValueError as e:
        raise ValueError('origin: known: %s' % str(e).replace('site ', 'known release '))
    lags = sorted({r['lag'] for r in out})
    if len(lags) > MAX_ORIGIN_KNOWN_LAGS:
        raise ValueError('origin: known: %d different lags %r; at most %d fit one handle'
                         % (len(lags), lags, MAX_ORIGIN_KNOWN_LAGS))
    for k, r in enumerate(out):
        if ndays is not None and r['lag'] >= ndays:
            raise ValueError('origin: known release %d: a release %d days after the first lies beyond the model\'s %d days'
                             % (k, r['lag'], ndays))
    return out


def check_origin(arg, rad_dist, rad_res, ndays=None, sites=None):
    '''The origin= argument as a plan.  arg: a list of findings, probes in the format of check_probes,
    (east_m, north_m, day, kind, rate[, n]), or dict(findings=[...], amounts=[0.1, 1, 10], lags=[0, 2],
    hypotheses=None, prior=None, levels=(0.5, 0.95)).  A hypothesis is (amount, lag): amount finite and > 0 in
    multiples of the model's release number, lag a whole number of days >= 0 after the model's first day; amounts x
    lags in that order is the default product, an explicit `hypotheses` list overrides it, [(1.0, 0)] where neither
    is given.  1..64 findings on at most 32 distinct days, 1..8 distinct hypotheses with at most 4 distinct lags,
    every lag below ndays and no later than the last finding (a release after every finding explains none).
    prior: an N x N float64 log-prior plane, finite or -inf (a cell that cannot be the origin), not all -inf.
    levels in (0, 1].  known: releases that are facts (check_origin_known; `sites`: the run's own release sites, for
    known='sites'): every finding also catches their wasps, and the hypotheses are those of a second source.
    -> dict(findings, given, days, slots, hypotheses, lags, groups, prior, levels, known, known_given, known_lags,
    known_groups, model_lags); model_lags: the lags a model is needed for -- the hypotheses' and the known lags up to
    the last finding's day.  ValueError with the offender named.  rad_res=None skips the cells and the prior's shape.'''
    keys = {'findings', 'amounts', 'lags', 'hypotheses', 'prior', 'levels', 'known'}
    if isinstance(arg, dict):
        if 'findings' not in arg or set(arg) - keys:
            raise ValueError('origin must be a list of findings or dict(findings=[...], amounts=, lags=, hypotheses=, '
                             'prior=, levels=, known=), got keys %r' % (sorted(arg),))
        spec = dict(arg)
    else:
        spec = {'findings': arg}
    try:
        findings = check_probes(spec['findings'], rad_dist, rad_res, ndays)
    except ValueError as e:
        raise ValueError('origin: %s' % str(e).replace('probe', 'finding'))
    if len(findings) > MAX_ORIGIN_FINDINGS:
        raise ValueError('origin: %d findings; 1..%d fit one handle' % (len(findings), MAX_ORIGIN_FINDINGS))
    days = sorted({f['day'] for f in findings})
    if len(days) > MAX_ORIGIN_DAYS:
        raise ValueError('origin: findings on %d different days; at most %d fit one handle' % (len(days), MAX_ORIGIN_DAYS))
    hyp = spec.get('hypotheses')
    if hyp is None:
        amounts = [1.0] if spec.get('amounts') is None else list(spec['amounts'])
        lags = [0] if spec.get('lags') is None else list(spec['lags'])
        hyp = [(a, g) for a in amounts for g in lags]
    elif spec.get('amounts') is not None or spec.get('lags') is not None:
        raise ValueError('origin: give hypotheses, or amounts and lags, not both')
    try:
        hyp = [tuple(h) for h in hyp]
    except TypeError:
        raise ValueError('origin: hypotheses must be a list of (amount, lag_days), got %r' % (hyp,))
    if not 1 <= len(hyp) <= MAX_ORIGIN_HYPOTHESES:
        raise ValueError('origin: %d hypotheses; 1..%d fit one handle' % (len(hyp), MAX_ORIGIN_HYPOTHESES))
    out = []
    for k, h in enumerate(hyp):
        try:
            if len(h) != 2:
                raise ValueError
            amount = float(h[0])
            if int(h[1]) != h[1]:
                raise ValueError
            lag = int(h[1])
        except (TypeError, ValueError):
            raise ValueError('origin: hypothesis %d: (amount, whole lag days) expected, got %r' % (k, h))
        if not (np.isfinite(amount) and amount > 0):
            raise ValueError('origin: hypothesis %d: amount %r is not finite and > 0' % (k, h[0]))
        if lag < 0:
            raise ValueError('origin: hypothesis %d: lag %d is negative' % (k, lag))
        if ndays is not None and lag >= ndays:
            raise ValueError('origin: hypothesis %d: a release %d days after the first lies beyond the model\'s %d days'
                             % (k, lag, ndays))
        if lag > days[-1]:
            raise ValueError('origin: hypothesis %d: a release on day %d comes after the last finding (day %d) and '
                             'explains none' % (k, lag, days[-1]))
        if (amount, lag) in out:
            raise ValueError('origin: hypothesis %d repeats (%g, %d)' % (k, amount, lag))
        out.append((amount, lag))
    lags = sorted({g for _a, g in out})
    if len(lags) > MAX_ORIGIN_LAGS:
        raise ValueError('origin: %d different lags; at most %d fit one handle' % (len(lags), MAX_ORIGIN_LAGS))
    prior = spec.get('prior')
    if prior is not None:
        try:
            prior = np.ascontiguousarray(prior, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError('origin: the prior must be an N x N array of log-prior values')
        if rad_res is not None and prior.shape != (2 * int(rad_res) + 1,) * 2:
            raise ValueError('origin: the prior has shape %r, the domain is %d x %d'
                             % (prior.shape, 2 * int(rad_res) + 1, 2 * int(rad_res) + 1))
        if np.isnan(prior).any() or (prior == np.inf).any():
            raise ValueError('origin: the prior holds NaN or +inf (finite or -inf expected)')
        if not np.isfinite(prior).any():
            raise ValueError('origin: the prior excludes every cell')
    try:
        levels = check_levels(spec.get('levels', (0.5, 0.95)))
    except (TypeError, ValueError) as e:
        raise ValueError('origin: %s' % e)
    if not levels:
        raise ValueError('origin: at least one level expected')
    known, known_given, known_lags = None, None, []
    if spec.get('known') is not None:
        known = check_origin_known(spec['known'], rad_dist, rad_res, ndays, sites)
        known_given = [[r['east'], r['north'], r['amount'], r['lag']] for r in known]
        known_lags = sorted({r['lag'] for r in known})
    return {'findings': findings, 'given': [list(p) for p in spec['findings']], 'days': days,
            'slots': [days.index(f['day']) for f in findings], 'hypotheses': out, 'lags': lags,
            'groups': [lags.index(g) for _a, g in out], 'prior': prior, 'levels': levels,
            'known': known, 'known_given': known_given, 'known_lags': known_lags,
            'known_groups': [known_lags.index(r['lag']) for r in known or ()],
            'model_lags': sorted(set(lags) | {g for g in known_lags if g <= days[-1]})}


def origin_log_evidence(A, S, W):
    '''E = A + log S - log W per cell from the fetched planes; -inf where A is (no member makes the cell possible)'''
    A, S = np.asarray(A, dtype=np.float64), np.asarray(S, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        E = A + np.log(S) - np.log(float(W))
    return np.where(A == -np.inf, -np.inf, E)


def origin_posterior(E, log_prior=None):
    '''[H, N, N] posterior mass of (hypothesis, origin cell) from E [H, N, N]: proportional to pi(s) exp E_h(s) with
    equal hypothesis priors, normalised over every cell and hypothesis; summed in a fixed order.  ValueError where
    no cell of any hypothesis is possible.'''
    E = np.asarray(E, dtype=np.float64)
    x = E if log_prior is None else E + np.asarray(log_prior, dtype=np.float64)[None]
    x = np.where(np.isnan(x), -np.inf, x)               # -inf evidence under a -inf prior
    mx = x.max()
    if mx == -np.inf:
        raise ValueError('no candidate cell explains the findings under any hypothesis')
    p = np.exp(x - mx)
    return p / p.sum()


def origin_region(mass, level):
    '''int8 [N, N]: the smallest set of cells holding `level` of the mass of `mass` [N, N] -- cells in descending
    mass, ties by the smaller linear index, until the running sum reaches level x the total'''
    level, = check_levels([level])
    m = np.asarray(mass, dtype=np.float64)
    flat = m.ravel()
    order = np.lexsort((np.arange(flat.size), -flat))
    cs = np.cumsum(flat[order])
    k = int(np.searchsorted(cs, level * cs[-1], side='left')) + 1
    out = np.zeros(flat.size, dtype=np.int8)
    out[order[:min(k, flat.size)]] = 1
    return out.reshape(m.shape)


def origin_hypothesis_masses(P, hypotheses):
    '''the posterior mass per (amount, lag) and its marginals per amount and per lag, from P [H, N, N]'''
    mass = [float(P[h].sum()) for h in range(len(hypotheses))]
    amounts = sorted({a for a, _g in hypotheses})
    lags = sorted({g for _a, g in hypotheses})
    return {'hypotheses': [{'amount': a, 'lag': g, 'mass': m} for (a, g), m in zip(hypotheses, mass)],
            'amounts': [{'amount': a, 'mass': sum(m for (b, _g), m in zip(hypotheses, mass) if b == a)} for a in amounts],
            'lags': [{'lag': g, 'mass': sum(m for (_a, k), m in zip(hypotheses, mass) if k == g)} for g in lags]}


def origin_log_prior_mass(log_prior, ncell):
    '''log of the prior's total mass: log(ncell) for the default of zeros, else the logsumexp of the plane'''
    if log_prior is None:
        return float(np.log(float(ncell)))
    lp = np.asarray(log_prior, dtype=np.float64)
    return float(lp.max() + np.log(np.exp(lp - lp.max()).sum()))


def origin_member_log_evidence(rows, log_prior_mass=0.0):
    '''[members] float64: log of the member's marginal likelihood of the findings with the origin and the
    hypothesis integrated out, from its rows [members, H, 2]: logsumexp over h of (mx + log sum) - log H - the log of
    the prior's total mass (origin_log_prior_mass); -inf where no cell of any hypothesis is possible'''
    rows = np.asarray(rows, dtype=np.float64)
    rows = rows.reshape(-1, rows.shape[-2], 2)
    with np.errstate(divide='ignore', invalid='ignore'):
        lm = np.where(rows[..., 0] == -np.inf, -np.inf, rows[..., 0] + np.log(rows[..., 1]))
        mx = lm.max(axis=1) if lm.shape[0] else np.zeros(0)
        out = mx + np.log(np.exp(lm - mx[:, None]).sum(axis=1)) - np.log(lm.shape[1]) - log_prior_mass
    return np.where(mx == -np.inf, -np.inf, out)


def _check_prior_second(prior):
    try:
        p = float(prior)
    except (TypeError, ValueError):
        raise ValueError('the prior probability of a second source must be a number in [0, 1], got %r' % (prior,))
    if not 0.0 <= p <= 1.0:
        raise ValueError('the prior probability of a second source must lie in [0, 1], got %r' % (prior,))
    return p


def origin_log_mean_exp(values, weights):
    '''log(sum_m w_m exp(x_m) / sum_m w_m), summed in member order; -inf where every x is'''
    x, w = np.asarray(values, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    mx = x.max() if x.size else -np.inf
    if mx == -np.inf:
        return float('-inf')
    return float(mx + np.log((w * np.exp(x - mx)).sum()) - np.log(w.sum()))


def origin_log_evidence_second(E, log_prior=None):
    '''log of the prior-weighted mean over cells and hypotheses of exp E_h(s), from E [H, N, N]: the prior pi
    normalised to 1 (zeros: the uniform prior), the hypotheses equally likely; -inf where no cell is possible'''
    E = np.asarray(E, dtype=np.float64)
    x = E if log_prior is None else E + np.asarray(log_prior, dtype=np.float64)[None]
    x = np.where(np.isnan(x), -np.inf, x)
    mx = x.max()
    if mx == -np.inf:
        return float('-inf')
    return float(mx + np.log(np.exp(x - mx).sum()) - np.log(E.shape[0])
                 - origin_log_prior_mass(log_prior, E.shape[1] * E.shape[2]))


def origin_second_source(log_evidence_second, log_evidence_null, prior=0.5, ess_second=None, ess_null=None):
    '''the summary of "second source or the known releases alone?" from the two log evidences: the log Bayes
    factor second : alone (nan where both are -inf) and the posterior probability of a second source at `prior`'''
    a, b = float(log_evidence_second), float(log_evidence_null)
    if a == -np.inf and b == -np.inf:
        lbf, prob = float('nan'), float('nan')
    else:
        lbf = a - b
        with np.errstate(divide='ignore', over='ignore'):
            lo = lbf + np.log(prior) - np.log1p(-prior)          # the posterior log-odds
            prob = float(1.0 / (1.0 + np.exp(-lo)))
    return {'log_bayes_factor': lbf, 'probability': prob, 'prior': float(prior), 'log_evidence_second': a,
            'log_evidence_null': b, 'ess_second': ess_second, 'ess_null': ess_null}


class OriginMaps(_Accumulator):
    '''Where, when and in what number did the wasps in these traps start?  For findings in the format of the
    reweighting probes and up to 8 hypotheses (amount, lag) the likelihood of every candidate origin cell at once,
    member by member on the device (ps_origin_*, csrc/ps_origin.hip; the statements are those of
    include/parasitoid_hip.h, restated in tests/origin_ref.py): one wind station and a homogeneous landscape make the
    field of a release elsewhere the centre release translated, the chain is linear in the released number, and a
    later release day is a model of its own (`lagged`, as ReleaseSites).  Per hypothesis and cell the handle keeps the
    streaming log-sum-exp pair (A, S) of the members' log-likelihoods, per member and hypothesis the evidence with the
    origin integrated out.  The accumulator is floating point, unlike the integer maps: another order of adds or
    merges moves the evidence within the bound of DESIGN 7y; the same calls give the same bits.  Everything below
    `log_evidence` is numpy on fetched planes; `pairs` lists the (amount, lag) of every hypothesis in the order of the
    planes.  It is inference about the past: it recommends nothing.  There is no
    `for_projection`: an unknown origin of a release plan or of a projection over days is not defined.'''
    _prefix, _noun, _prof_pairs = 'ps_origin', 'origin maps', 3
    _info_types = (C.c_double, C.c_int64, C.c_int64, C.c_int64)      # weight, members, capacity, bytes
    _owned = ()

    def __init__(self, pop_model, origin, lagged=None):
        self.plan = check_origin(origin, pop_model.rad_dist, pop_model.rad_res, len(pop_model.days))
        self.findings, self.pairs = self.plan['findings'], self.plan['hypotheses']
        self.days, self.lags, self.levels = self.plan['days'], self.plan['lags'], self.plan['levels']
        self.log_prior = self.plan['prior']
        self.known, self.known_lags = self.plan['known'], self.plan['known_lags']
        self.model_lags = self.plan['model_lags']
        self.lagged = check_lagged(pop_model, self.model_lags, lagged)
        self.slots = site_slots(self.lags, self.days)
        # a known release after the last finding reads no day: every slot None, it contributes 0
        self.known_slots = [[D - lag if D >= lag else None for D in self.days] for lag in self.known_lags]
        self._attach(pop_model)
        f = self.findings
        prior = None if self.log_prior is None else L.p_f64(self.log_prior)
        self._create(len(f), L.p_i32(L.i32([p['row'] for p in f])), L.p_i32(L.i32([p['col'] for p in f])),
                     L.p_i32(L.i32(self.plan['slots'])), L.p_i32(L.i32([ORIGIN_KIND_CODE[p['kind']] for p in f])),
                     L.p_f64(L.f64([p['rate'] for p in f])), L.p_f64(L.f64([p['n'] or 0 for p in f])), len(self.days),
                     len(self.pairs), L.p_f64(L.f64([a for a, _g in self.pairs])),
                     L.p_i32(L.i32(self.plan['groups'])), len(self.lags), prior)
        if self.known:
            try:
                self._call('set_known', len(self.known), L.p_i32(L.i32([k['drow'] for k in self.known])),
                           L.p_i32(L.i32([k['dcol'] for k in self.known])),
                           L.p_f64(L.f64([k['amount'] for k in self.known])),
                           L.p_i32(L.i32(self.plan['known_groups'])), len(self.known_lags))
            except Exception:
                self.close()
                raise

    @classmethod
    def with_lagged_models(cls, pop_model, origin, wind_data=None):
        '''the maps with the models of the later release days built here (lagged_models); `close()` closes them'''
        plan = check_origin(origin, pop_model.rad_dist, pop_model.rad_res, len(pop_model.days))
        made = lagged_models(pop_model, plan['model_lags'], wind_data)
        try:
            self = cls(pop_model, origin, made)
        except Exception:
            for m in made.values():
                m.close()
            raise
        self._owned = list(made.values())
        return self

    def models(self):
        '''[(lag, model), ...] in group order'''
        return [(lag, self.pm if lag == 0 else self.lagged[lag]) for lag in self.lags]

    def evaluate_lagged(self, *model_args):
        '''evaluate the model of every later release day over the days the findings need, enqueued only'''
        for lag, m in sorted(self.lagged.items()):
            m.evaluate(*model_args, ndays=self.days[-1] - lag + 1, want_stats=False)

    def _model(self, lag):
        '''the model of a release `lag` days after the first; a known lag after the last finding reads no record and
        takes the base model'''
        return self.pm if lag == 0 or lag not in self.lagged else self.lagged[lag]

    def _group_call(self, g, lag, md, what):
        m = self._model(lag)
        _check_evaluated(m, [d for d in md if d is not None], 'origin maps (%s %d)' % (what, lag))
        days = [0 if d is None else d for d in md]
        kind, idx, delta = _day_slots(days)
        kind[np.array([d is None for d in md], dtype=bool)] = L.REC_NONE
        stat, post = _day_scales(m, days)
        return (m.solver._h, g, len(days), L.p_i32(kind), L.p_i32(idx), L.p_f64(stat), L.p_f64(post), L.p_i32(delta),
                NEGVAL)

    def _calls(self, w):
        '''[(operation, arguments), ...] of one member: the backgrounds of the known groups, then the adds'''
        calls = [('background', self._group_call(g, lag, self.known_slots[g], 'known lag'))
                 for g, lag in enumerate(self.known_lags)]
        calls += [('add', self._group_call(g, lag, self.slots[g], 'lag') + (w,)) for g, lag in enumerate(self.lags)]
        return calls

    def reserve(self, n):
        '''room for n members' rows now, so that no add has to grow them'''
        self._call('reserve', int(n))

    def add(self, weight=1):
        '''Accumulate the last evaluation of the model -- and of every lagged model (`evaluate_lagged`) -- with
        integer weight >= 1: one launch pair per lag, each on its solver's stream, no host synchronisation unless
        the member rows grow.  Every model is checked before the first launch.  With known releases the background
        calls of the known lags come first, one small launch each.'''
        for op, call in self._calls(self._weight(weight)):
            self._call(op, *call)

    def merge(self, other):
        '''self += other (same device, domain, findings, hypotheses and prior); other's members follow self's'''
        self._call('merge', other._h)

    @property
    def capacity(self):
        return self._info()[2]

    @property
    def nbytes(self):
        '''the device memory the handle holds now'''
        return self._info()[3]

    def profile(self, enable=None):
        '''HIP-event time per kernel class: (add ms, adds, row-reduction ms, reductions, merge ms, merges)'''
        return self._profile(enable)

    def _h_index(self, h):
        return self._index(h, len(self.pairs), 'hypothesis')

    def plane(self, what, h):
        '''[N, N] float64 as the device holds it: what 'A', 'S' or 'l' (the last member's log-likelihood)'''
        out = np.empty((self.N, self.N), dtype=np.float64)
        self._call('fetch', {'A': 0, 'S': 1, 'l': 2}[what], self._h_index(h), L.p_f64(out))
        return out

    def member_rows(self):
        '''(rows [members, H, 2] float64, weights [members] int64) in add order: per member and hypothesis
        (mx, sum) over the cells of l + log prior'''
        m = self.members
        rows, w = np.empty((m, len(self.pairs), 2), dtype=np.float64), np.empty(m, dtype=np.uint32)
        self._call('members', m, L.p_f64(rows), w.ctypes.data_as(C.POINTER(C.c_uint32)))
        return rows, w.astype(np.int64)

    # ---------------------------------------------------------------- numpy on fetched planes, deterministic
    def log_evidence(self, h):
        '''[N, N]: E_h = A + log S - log W, the log of the members' mean likelihood of the findings for an origin at
        each cell; -inf where no member makes the cell possible'''
        return origin_log_evidence(self.plane('A', h), self.plane('S', h), self.total_weight)

    def _posterior(self):
        E = np.stack([self.log_evidence(h) for h in range(len(self.pairs))])
        return origin_posterior(E, self.log_prior)

    def posterior(self, h=None):
        '''[N, N]: the posterior mass of the origin, normalised over all cells and hypotheses with the prior pi and
        equal hypothesis priors; h=None: the marginal over the hypotheses, else the share of hypothesis h'''
        P = self._posterior()
        return P.sum(axis=0) if h is None else P[self._h_index(h)]

    def hypotheses(self):
        '''posterior mass per (amount, lag) and its marginals per amount and per lag'''
        return origin_hypothesis_masses(self._posterior(), self.pairs)

    def region(self, level):
        '''int8 [N, N]: the smallest set of cells holding `level` of the marginal posterior; ties by linear index'''
        return origin_region(self.posterior(), level)

    def area(self, level):
        '''the area of region(level) in m^2'''
        return float(self.region(level).sum()) * self.cell_area

    def _metres(self, row, col):
        res = float(self.pm.rad_dist) / int(self.pm.rad_res)
        R = int(self.pm.rad_res)
        return (col - R) * res, (R - row) * res

    def mode(self):
        '''the most probable (hypothesis, cell): a summary of the posterior, not a recommendation.  A UserWarning
        where it sits on the outermost rung of an amounts ladder of three or more: the ladder may be too short.'''
        import warnings
        P = self._posterior()
        h, row, col = (int(v) for v in np.unravel_index(int(np.argmax(P)), P.shape))
        east, north = self._metres(row, col)
        amounts = sorted({a for a, _g in self.pairs})
        if len(amounts) >= 3 and self.pairs[h][0] in (amounts[0], amounts[-1]):
            warnings.warn('origin: the mode sits on the outermost amount %g of the ladder %r: the founding number may '
                          'lie beyond it' % (self.pairs[h][0], amounts), UserWarning, stacklevel=2)
        return {'row': row, 'col': col, 'east': east, 'north': north, 'hypothesis': h,
                'amount': self.pairs[h][0], 'lag': self.pairs[h][1], 'mass': float(P[h, row, col]),
                'cell_mass': float(P[:, row, col].sum())}

    def _cell(self, east_m, north_m):
        p, = check_probes([(east_m, north_m, 0, 'none', 1.0)], self.pm.rad_dist, self.pm.rad_res)
        return p['row'], p['col']

    def at(self, east_m, north_m):
        '''the marginal posterior mass at the cell that holds (east_m, north_m)'''
        row, col = self._cell(east_m, north_m)
        return float(self.posterior()[row, col])

    def log_bayes_factor(self, a, b):
        '''log of (evidence for an origin at a) / (evidence for an origin at b), a and b (east_m, north_m), the
        hypotheses averaged with equal priors and the cell prior left out: "our site or theirs?"'''
        E = np.stack([self.log_evidence(h) for h in range(len(self.pairs))])
        out = []
        for east, north in (a, b):
            row, col = self._cell(east, north)
            x = E[:, row, col]
            mx = x.max()
            out.append(-np.inf if mx == -np.inf else float(mx + np.log(np.exp(x - mx).sum())))
        if out[0] == -np.inf and out[1] == -np.inf:
            return float('nan')
        return out[0] - out[1]

    def member_log_evidence(self):
        '''[members]: log of each member's marginal likelihood of the findings, origin and hypothesis integrated out
        (origin_member_log_evidence)'''
        return origin_member_log_evidence(self.member_rows()[0], origin_log_prior_mass(self.log_prior, self.N * self.N))

    def log_weights(self, prior_second=None):
        '''the members' log-evidence in chain-row form, one entry per row of the chain (a member of weight w is w
        equal rows): what posterior_predictive(reweight={name: dict(log_weights=[...])}) takes per chain, to update
        every forward map for the findings under an unknown origin.  With known releases that is conditional on a
        second source existing; prior_second, a probability in [0, 1], gives per row the mixture of both
        explanations instead: log(p exp(second) + (1 - p) exp(l0)).'''
        rows, w = self.member_rows()
        lw = np.repeat(origin_member_log_evidence(rows, origin_log_prior_mass(self.log_prior, self.N * self.N)), w)
        if prior_second is None:
            return lw
        p = _check_prior_second(prior_second)
        l0 = np.repeat(self.null_rows(), w)
        with np.errstate(divide='ignore'):
            return np.logaddexp(np.log(p) + lw, np.log1p(-p) + l0)

    # ---------------------------------------------------------------- known releases: is there a second source?
    def _need_known(self, what):
        if not getattr(self, 'known', None):
            raise ValueError('%s: these origin maps have no known releases (origin=dict(known=[...]))' % what)

    def background(self):
        '''(bg [findings] in the order given, l0): the last member's background -- what the known releases alone put
        into every trap, in the units of mu -- and its null row'''
        self._need_known('background')
        bg, l0 = np.empty(len(self.findings), dtype=np.float64), C.c_double()
        self._call('fetch_background', L.p_f64(bg), C.byref(l0))
        return bg, float(l0.value)

    def null_rows(self):
        '''[members] float64 in add order: l0, each member's log-likelihood of the findings under the known releases
        alone'''
        self._need_known('null_rows')
        out = np.empty(self.members, dtype=np.float64)
        self._call('null_rows', self.members, L.p_f64(out))
        return out

    def log_evidence_null(self):
        '''log of the weighted mean over the members of exp(l0): the evidence for "the known releases alone"'''
        self._need_known('log_evidence_null')
        return origin_log_mean_exp(self.null_rows(), self.member_rows()[1])

    def log_evidence_second(self):
        '''log of the prior-weighted mean over cells and hypotheses of exp E_h(s): the evidence for "a second source
        somewhere", the prior pi normalised and the hypotheses equally likely'''
        self._need_known('log_evidence_second')
        E = np.stack([self.log_evidence(h) for h in range(len(self.pairs))])
        return origin_log_evidence_second(E, self.log_prior)

    def second_source(self, prior=0.5):
        '''Do the findings need a second source, or do the known releases explain them?  -> dict(log_bayes_factor:
        second source : known releases alone, probability: the posterior probability of a second source at the prior
        probability `prior`, prior, log_evidence_second, log_evidence_null, ess_second, ess_null: the Kish effective
        sample of the chain's rows behind either evidence).  A summary; it recommends nothing.'''
        self._need_known('second_source')
        p = _check_prior_second(prior)
        w = self.member_rows()[1]
        second, null = self.log_evidence_second(), self.log_evidence_null()
        return origin_second_source(second, null, p, reweight_diagnostics(self.log_weights())['ess'],
                                    reweight_diagnostics(np.repeat(self.null_rows(), w))['ess'])

    def diagnostics(self, min_ess=DEFAULT_MIN_ESS):
        '''reweight_diagnostics of the rows' contributions to the total evidence (Kish ESS, the largest share); a
        UserWarning below min_ess: an inversion that hangs on a few members of the chain needs saying'''
        import warnings
        d = reweight_diagnostics(self.log_weights())
        if d['ess'] < min_ess:
            warnings.warn('origin: the evidence rests on an effective sample of %.1f rows of %d (largest share %.2f); '
                          'below %g the posterior of the origin is that of a few members'
                          % (d['ess'], d['rows'], d['max_share'], min_ess), UserWarning, stacklevel=2)
        return d

    def describe(self):
        '''the request for a result file'''
        out = {'findings': self.plan['given'], 'hypotheses': [list(h) for h in self.pairs],
               'levels': list(self.levels), 'prior': self.log_prior is not None}
        if getattr(self, 'known', None):
            out['known'] = self.plan['known_given']
        return out

    def close(self):
        super().close()
        for m in self._owned:
            m.close()
        self._owned = []


def origin_block(om):
    '''the json block of an OriginMaps: request, hypothesis masses, mode, areas and diagnostics'''
    import warnings
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        block = dict(om.describe(), members=int(om.members), total_weight=float(om.total_weight),
                     diagnostics=om.diagnostics())
        try:
            block.update(masses=om.hypotheses(), mode=om.mode(), areas={level_tag(p): om.area(p) for p in om.levels})
        except ValueError as e:        # no member makes any cell possible: said in the block, the files are still written
            block.update(masses=None, mode=None, areas=None, impossible=str(e))
        if getattr(om, 'known', None):     # second source or the known releases alone: a summary, no recommendation
            block['second_source'] = om.second_source()
    block['warnings'] = [str(w.message) for w in caught]
    for w in caught:
        warnings.warn(w.message, w.category, stacklevel=2)
    return block


def save_origin(outfile, om):
    '''PREFIX_origin.npz: E_h per hypothesis (log_evidence_h<h>), the marginal posterior, the regions at the
    request's levels (region_<tag>), the member rows and weights, the hypotheses -- with known releases also `known`,
    `null_rows` and `background_last`, and a `second_source` entry in the block; -> (path, json block).  Where no
    member makes any cell possible the posterior is all zero, the regions are empty and the block says so
    (`impossible`).'''
    arrays = {'log_evidence_h%d' % h: om.log_evidence(h) for h in range(len(om.pairs))}
    try:
        arrays['posterior'] = om.posterior()
        for p in om.levels:
            arrays['region_' + level_tag(p)] = om.region(p)
    except ValueError:                 # no candidate cell explains the findings: zero mass, empty regions
        arrays['posterior'] = np.zeros((om.N, om.N), dtype=np.float64)
        for p in om.levels:
            arrays['region_' + level_tag(p)] = np.zeros((om.N, om.N), dtype=np.int8)
    rows, w = om.member_rows()
    arrays.update(member_rows=rows, member_weights=w, hypotheses=np.array(om.pairs, dtype=np.float64))
    if getattr(om, 'known', None):         # [K, 4] east, north, amount, lag; l0 per member; the last member's bg
        arrays.update(known=np.array(om.plan['known_given'], dtype=np.float64), null_rows=om.null_rows(),
                      background_last=om.background()[0])
    path = outfile + '_origin.npz'
    np.savez_compressed(path, **arrays)
    return path, origin_block(om)


# ------------------------------------------------------------------ traces
def model_names():
    return [m[0] for m in mcmc.MODEL_BLOCK]


def nuisance_names():
    return [m[0] for m in mcmc.NUISANCE]


def load_chain(chain):
    '''(trace, names, source) of one `Sampler.save` file or (trace, names) pair'''
    if isinstance(chain, (str, os.PathLike)):
        fname = str(chain)
        f = np.load(fname if fname.endswith('.npz') else fname + '.npz', allow_pickle=False)
        return np.asarray(f['trace'], dtype=np.float64), [str(n) for n in f['names']], fname
    trace, names = chain
    return np.asarray(trace, dtype=np.float64), [str(n) for n in names], None


def _columns(names, want):
    '''column index of every name of `want`; the ValueError of Sampler.resume when one is missing'''
    pos = {n: i for i, n in enumerate(names)}
    if any(n not in pos for n in want):
        raise ValueError('the chain file was written for a different model')
    return [pos[n] for n in want]


def runs(trace, model_cols, burn=0, thin=1):
    '''burn / thin one chain, then split it into runs of identical model-block rows ->
    (rows [n, ncol], [(first_row, length), ...])'''
    if burn < 0 or thin < 1:
        raise ValueError('burn must be >= 0 and thin >= 1')
    rows = trace[burn::thin]
    out = []
    i = 0
    theta = rows[:, model_cols]
    while i < len(rows):
        j = i + 1
        while j < len(rows) and np.array_equal(theta[j], theta[i]):
            j += 1
        out.append((i, j - i))
        i = j
    return rows, out


# ------------------------------------------------------------------ observation model
def observation_rates(expected, locinfo, nuis, sent_obs_probs):
    '''Poisson rates of the reference's observation model (Bayes_Run.py:344-433), as mcmc.loglik_parts
    uses them: release grids xi * emergence * effort * em_obs_prob, sentinel fields
    xi * emergence * sent_obs_prob[field], grid counts grid_obs_prob * samples * density.
    -> (list of release arrays, list of sentinel arrays, grid array)'''
    rel, sen, grid = expected
    xi, em_p, grid_p = (float(v) for v in nuis)
    c = mcmc.observation_cache(locinfo)
    r_rel = [xi * np.asarray(e, dtype=np.float64) * (c['effort'][ii] * em_p)[:, None] for ii, e in enumerate(rel)]
    sp = np.asarray(sent_obs_probs, dtype=np.float64)[:, None]
    r_sen = [xi * np.asarray(e, dtype=np.float64) * sp for e in sen]
    r_grid = grid_p * c['samples'] * np.asarray(grid, dtype=np.float64)
    return r_rel, r_sen, r_grid


def _flat(arrs):
    arrs = [np.asarray(a, dtype=np.float64).ravel() for a in arrs]
    return np.concatenate(arrs) if arrs else np.zeros(0)


def observation_predictive(rates, locinfo, seed=0):
    '''rates: one observation_rates result per trace row.  Replicated counts drawn with
    default_rng(seed) -> per group (release, sentinel, grid): mean rate, 5/50/95 % quantiles of
    the replicated counts per observation, P(total replicated >= total observed).'''
    c = mcmc.observation_cache(locinfo)
    observed = {'release': _flat(c['rel']), 'sentinel': _flat(c['sen']), 'grid': _flat([c['grid']])}
    rng = np.random.default_rng(seed)
    out = {}
    for g, gi in (('release', 0), ('sentinel', 1), ('grid', 2)):
        lam = np.array([_flat(r[gi] if gi < 2 else [r[2]]) for r in rates]).reshape(len(rates), -1)
        rep = rng.poisson(lam) if lam.size else np.zeros(lam.shape)
        obs = observed[g]
        out[g] = {'mean_rate': lam.mean(0) if len(rates) else np.zeros(obs.size),
                  'q05': np.quantile(rep, 0.05, axis=0) if len(rates) else np.zeros(obs.size),
                  'q50': np.quantile(rep, 0.50, axis=0) if len(rates) else np.zeros(obs.size),
                  'q95': np.quantile(rep, 0.95, axis=0) if len(rates) else np.zeros(obs.size),
                  'observed': obs,
                  'p_total': float(np.mean(rep.sum(1) >= obs.sum())) if len(rates) else float('nan')}
    return out


# ------------------------------------------------------------------ result files
def save_maps(outfile, maps, extra=None, signed=False):
    '''outfile.npz in the layout of Run.save_result (Run.py:490-516 of the reference), which
    Plot_Result.main reads.  maps: [(day label, [(suffix, N x N array), ...]), ...] -> per day and
    suffix the CSR triplet `{label}{suffix}_data/_ind/_indptr` of the array thresholded at 1e-8,
    and `days` = the labels; extra: {key: array} written as given (a `days` of its own replaces the labels).  signed: keep the entries with
    |value| >= 1e-8, for maps that take either sign.  The directory is created if needed.'''
    from scipy import sparse
    out = dict(extra or {})
    labels = []
    for label, day_maps in maps:
        labels.append(label)
        for suffix, m in day_maps:
            csr = sparse.csr_matrix(np.where((np.abs(m) if signed else m) >= NEGVAL, m, 0.0))
            out['%s%s_data' % (label, suffix)] = csr.data
            out['%s%s_ind' % (label, suffix)] = csr.indices
            out['%s%s_indptr' % (label, suffix)] = csr.indptr
    out.setdefault('days', np.array(labels))
    d = os.path.dirname(str(outfile))
    if d and not os.path.exists(d):
        os.makedirs(d)
    np.savez(str(outfile), **out)


def params_dict(params):
    '''the run parameters of a result file: None, a dict or a Run.Params-like object'''
    if params is None:
        return {}
    if isinstance(params, dict):
        return dict(params)
    pdict = dict(params.__dict__)
    pdict.pop('maps_key', None)
    return pdict


def save_sensitivity(outfile, sens, keys, labels):
    '''outfile.npz of one SensitivityMaps through save_maps (keys: its days or output indices, labels: theirs in
    the file), finalized here if it can be -> its block for the json (SensitivityMaps.describe, `finalized` and,
    where finalize refused, `reason`)'''
    block = sens.describe()
    try:
        if sens.rank is None:
            sens.finalize()
        block['finalized'] = True
    except ValueError as e:
        block['finalized'] = False
        block['reason'] = str(e)
    maps, extra = [], {}
    for k, label in zip(keys, labels):
        day_maps = [('_corr_%s' % n, sens.correlation(k, n)) for n in sens.params]
        if block['finalized']:
            day_maps.append(('_r2', sens.explained(k)))
            extra['%s_dom' % label] = sens.dominant(k)
        maps.append((label, day_maps))
    save_maps(outfile, maps, extra, signed=True)
    return block


def save_dependence(outfile, dep, keys, labels, sensitivity=None):
    '''outfile.npz of one DependenceMaps through save_maps (keys: its days or output indices, labels: theirs in the
    file), finalized here if it can be: per label `{label}_eta2_{name}` as CSR triplets, dense int8 `{label}_dom`
    and, with a SensitivityMaps over the same members that lists the name, `{label}_excess_{name}` -> its block for
    the json (DependenceMaps.describe, `finalized` and, where finalize refused, `reason`; no ratio maps are written
    then)'''
    block = dep.describe()
    try:
        if not dep.finalized:
            dep.finalize()
        block['finalized'] = True
    except ValueError as e:
        block['finalized'] = False
        block['reason'] = str(e)
    maps, extra = [], {}
    shared = [n for n in dep.params if sensitivity is not None and n in sensitivity.params]
    for k, label in zip(keys, labels):
        if not block['finalized']:
            break
        day_maps = [('_eta2_%s' % n, dep.ratio(k, n)) for n in dep.params]
        day_maps += [('_excess_%s' % n, dep.excess(k, n, sensitivity)) for n in shared]
        extra['%s_dom' % label] = dep.dominant(k)
        maps.append((label, day_maps))
    save_maps(outfile, maps, dict(extra, days=np.array(labels)))
    return block


def save_reweight(outfile, rw, keys, labels):
    '''outfile.npz of one ReweightedSummary through save_maps (keys: its days or output indices, labels: theirs in
    the file): per scenario index j and label the CSR triplets `s{j}_{label}_*` of the reweighted mean,
    `s{j}_{label}_sd_*` and `s{j}_{label}_pexc{k}_*`; `scenarios` the names, `labels` the labels'''
    maps = []
    for j, name in enumerate(rw.scenarios):
        for k, label in zip(keys, labels):
            day_maps = [('', rw.mean(name, k)), ('_sd', rw.sd(name, k))]
            day_maps += [('_pexc%d' % t, rw.exceedance(name, k, t)) for t in range(len(rw.thresholds))]
            maps.append(('s%d_%s' % (j, label), day_maps))
    save_maps(outfile, maps, {'scenarios': np.array(rw.scenarios), 'labels': np.array(labels)})


def save_reweight_quantiles(outfile, rh, keys, labels, levels):
    '''outfile.npz of one ReweightedHistogram through save_maps (keys: its days or output indices, labels: theirs in
    the file): per scenario index j, label and level the CSR triplets `s{j}_{label}_q{tag}_*` of the reweighted
    quantile point map (quantile_tag), as the main file's `{label}_q{tag}_*`; `scenarios`, `labels`, `levels` and
    the edge table `edges`'''
    maps = []
    for j, name in enumerate(rh.scenarios):
        for k, label in zip(keys, labels):
            maps.append(('s%d_%s' % (j, label), [('_' + quantile_tag(p), rh.quantile(name, k, p)[0]) for p in levels]))
    save_maps(outfile, maps, {'scenarios': np.array(rh.scenarios), 'labels': np.array(labels),
                              'levels': np.array(levels, dtype=np.float64), 'edges': rh.edges})


def save_reweight_arrival(outfile, ra, keys, labels, levels):
    '''outfile.npz of one ReweightedArrival through save_maps (keys: its days, labels: theirs in the file): per
    scenario index j, label and threshold k the CSR triplets `s{j}_{label}_parr{k}_*` (P(arrived at t_k by that day)
    under the scenario) and per level the dense int16 model-day map `s{j}_arrival{k}_q{tag}` (-1: not within the
    window), as the main file's `{label}_parr{k}_*` and `arrival{k}_q{tag}`; `scenarios`, `labels`, `thresholds`'''
    maps, extra = [], {'scenarios': np.array(ra.scenarios), 'labels': np.array(labels),
                       'thresholds': np.array(ra.thresholds, dtype=np.float64)}
    nk = len(ra.thresholds)
    for j, name in enumerate(ra.scenarios):
        for d, label in zip(keys, labels):
            maps.append(('s%d_%s' % (j, label), [('_parr%d' % k, ra.prob_by(name, k, d)) for k in range(nk)]))
        for k in range(nk):
            for p in levels:
                extra['s%d_arrival%d_%s' % (j, k, quantile_tag(p))] = ra.quantile(name, k, p).astype(np.int16)
    save_maps(outfile, maps, extra)


def save_peak(outfile, peak, quantiles=()):
    '''outfile.npz of one PeakPosterior through save_maps: under the label `peak` the CSR triplets `peak_*` of the
    posterior mean of the peak value, `peak_sd_*`, `peak_pexc{k}_*` (P(peak >= t_k)) and, with a histogram,
    `peak_q{tag}_*` at the levels `quantiles`; per threshold k under the label `days{k}` the triplet
    `days{k}_mean_*` of the posterior mean duration; dense int16 `peakday_q{tag}` model-day maps (-1: too few
    members ever hold anything there) and `days{k}_q{tag}` duration maps at the peak's own levels (dense because
    the CSR writer drops day 0); the count planes `peakday_counts` [days, N, N] and `days{k}_counts`
    [days + 1, N, N] (n = 0 first; uint16 where the total weight fits, else uint32), `peak_thresholds` and
    `peak_days` -> its block for the json'''
    P, S, H = peak.maps, peak.summary, peak.histogram
    nk = len(P.thresholds)
    W = int(P.total_weight)
    ctype = np.uint16 if W <= 0xffff else np.uint32
    day_maps = [('', S.mean(0)), ('_sd', S.sd(0))]
    day_maps += [('_pexc%d' % k, S.exceedance(0, k)) for k in range(len(S.thresholds))]
    if H is not None:
        day_maps += [('_' + quantile_tag(p), H.quantile(0, p)) for p in quantiles]
    maps = [('peak', day_maps)]
    extra = {'peak_thresholds': np.asarray(P.thresholds, dtype=np.float64), 'peak_days': np.asarray(P.days),
             'peakday_counts': np.stack([P.day_counts(d) for d in P.days]).astype(ctype)}
    for p in peak.levels:
        extra['peakday_%s' % quantile_tag(p)] = P.day_quantile(p).astype(np.int16)
    longest = []
    for k in range(nk):
        mean = P.duration_mean(k)
        longest.append(float(mean.max()))
        maps.append(('days%d' % k, [('_mean', mean)]))
        for p in peak.levels:
            extra['days%d_%s' % (k, quantile_tag(p))] = P.duration_quantile(k, p).astype(np.int16)
        extra['days%d_counts' % k] = np.stack([P.duration_counts(k, n)
                                               for n in range(len(P.days) + 1)]).astype(ctype)
    save_maps(outfile, maps, extra)
    return {'thresholds': list(P.thresholds), 'days': list(P.days), 'levels': list(peak.levels),
            'consecutive': bool(P.consecutive), 'members': P.members, 'total_weight': P.total_weight,
            'summary_thresholds': list(S.thresholds), 'max_mean_duration': longest}


def save_excursion(outfile, exc, levels=(0.9, 0.95)):
    '''outfile.npz of one ExcursionMaps through save_maps: per day of the maps, under the label `{day}`, the CSR
    triplets `{day}_above{k}_*`, `{day}_below{k}_*` and `{day}_contour{k}_*` of the three functions; dense int8
    `{day}_region{k}_{tag}` per level (+1 surely reached, -1 surely not, 0 neither; dense because the CSR writer
    cannot keep a zero that means something; level_tag: l90, l95); the count planes `excur_counts`
    [thresholds, days, N, N] (uint16 where the total weight fits, else uint32), the bounds `excur_hi` / `excur_lo`
    [thresholds, days, members] uint32, `excur_weights` [members], `excur_thresholds` and `excur_days` -> its
    block for the json: thresholds, days, levels, members, weight, cell area and per threshold and day the areas
    of ExcursionMaps.areas'''
    levels = check_excursion_levels(levels)
    nk = len(exc.thresholds)
    W = int(exc.total_weight)
    ctype = np.uint16 if W <= 0xffff else np.uint32
    maps, extra, areas = [], {}, []
    for d in exc.days:
        day_maps = []
        for k in range(nk):
            Fp, Fm, Fc = exc.above(k, d), exc.below(k, d), exc.contour(k, d)
            day_maps += [('_above%d' % k, Fp), ('_below%d' % k, Fm), ('_contour%d' % k, Fc)]
            for p in levels:
                extra['%s_region%d_%s' % (d, k, level_tag(p))] = (Fp >= p).astype(np.int8) - (Fm >= p).astype(np.int8)
        maps.append((d, day_maps))
    for k in range(nk):
        areas.append([{'day': d, 'levels': exc.areas(k, d, levels)} for d in exc.days])
    extra['excur_counts'] = np.array([[exc.counts(k, d) for d in exc.days] for k in range(nk)]).astype(ctype)
    b = [[exc.bounds(k, d) for d in exc.days] for k in range(nk)]
    extra['excur_hi'] = np.array([[x[0] for x in row] for row in b], dtype=np.uint32)
    extra['excur_lo'] = np.array([[x[1] for x in row] for row in b], dtype=np.uint32)
    extra['excur_weights'] = np.asarray(b[0][0][2], dtype=np.uint32)
    extra['excur_thresholds'] = np.asarray(exc.thresholds, dtype=np.float64)
    extra['excur_days'] = np.asarray(exc.days)
    save_maps(outfile, maps, extra)
    return {'thresholds': list(exc.thresholds), 'days': list(exc.days), 'levels': levels, 'members': exc.members,
            'total_weight': exc.total_weight, 'cell_area': exc.cell_area, 'areas': areas}


def save_reweight_contrast(outfile, rc, contrast=None, levels=(0.05, 0.5, 0.95)):
    '''outfile.npz of one ReweightedContrast through save_maps(signed=True): per scenario index j and output label
    the signed CSR triplets `s{j}_{label}_*` of the reweighted mean of A - B, `s{j}_{label}_sd_*`,
    `s{j}_{label}_ppos_*` / `_pneg_*` and per threshold `s{j}_{label}_pgain{k}_*` / `_ploss{k}_*`, as the contrast's
    own file; `scenarios` the names, `labels` the labels.  -> the json block: per scenario the thresholds, the total
    log-weight, members and skipped and, with the PlanContrast fed alongside and the members' log-weights
    (rc.member_log_weights, [members][scenarios] in its add order), per threshold the
    reweighted_coverage_difference of its paired rows'''
    nk = len(rc.thresholds)
    maps = []
    for j, name in enumerate(rc.scenarios):
        for e, label in enumerate(rc.labels):
            out_maps = [('', rc.mean(name, e)), ('_sd', rc.sd(name, e)), ('_ppos', rc.prob_positive(name, e)),
                        ('_pneg', rc.prob_negative(name, e))]
            for k in range(nk):
                out_maps += [('_pgain%d' % k, rc.gain(name, e, k)), ('_ploss%d' % k, rc.loss(name, e, k))]
            maps.append(('s%d_%s' % (j, label), out_maps))
    save_maps(outfile, maps, {'scenarios': np.array(rc.scenarios), 'labels': np.array(rc.labels)}, signed=True)
    block = {}
    lam = getattr(rc, 'member_log_weights', None)
    for j, name in enumerate(rc.scenarios):
        rec = {'thresholds': list(rc.thresholds), 'log_total_weight': rc.log_total_weight(name),
               'members': rc.members(name), 'skipped': rc.skipped(name)}
        if contrast is not None and lam is not None:
            rec['levels'] = list(levels)
            rec['coverage_difference'] = []
            for k in range(nk):
                ca, cb, w = contrast.coverage(k)
                rows = reweighted_coverage_difference(ca, cb, w, [m[j] for m in lam], contrast.cell_area, levels)
                for label, row in zip(contrast.labels, rows):
                    row['label'] = label
                rec['coverage_difference'].append(rows)
        block[name] = rec
    return block


def save_reweight_excursion(outfile, rx, levels=(0.9, 0.95)):
    '''outfile.npz of the ReweightedExcursion of every scenario ({name: ReweightedExcursion} over one ExcursionMaps)
    through save_maps: per scenario index j and day of the maps, under the label `{day}_s{j}`, the CSR triplets
    `{day}_s{j}_above{k}_*`, `{day}_s{j}_below{k}_*` and `{day}_s{j}_contour{k}_*`; dense int8
    `{day}_s{j}_region{k}_{tag}` per level, as save_excursion's; `wexcur_counts` [scenarios, thresholds, days, N, N],
    `wexcur_hi` / `wexcur_lo` [scenarios, thresholds, days, members] and `wexcur_weights` [scenarios, members], all
    float64; `wexcur_scenarios` the names, `wexcur_thresholds`, `wexcur_days` and `days` -> its block for the json:
    scenarios, thresholds, days, levels, cell area and per scenario members, total weight, ess and per threshold and
    day the areas of ReweightedExcursion.areas'''
    levels = check_excursion_levels(levels)
    names = list(rx)
    first = rx[names[0]]
    nk = len(first.thresholds)
    maps, extra, block = [], {}, {}
    for j, name in enumerate(names):
        R = rx[name]
        areas = [[] for _ in range(nk)]
        cnt, hi, lo = [], [], []
        for k in range(nk):       # plane by plane: one plane build serves its maps, counts and bounds
            cnt.append([]), hi.append([]), lo.append([])
            for d in R.days:
                Fp, Fm, Fc = R.above(k, d), R.below(k, d), R.contour(k, d)
                maps.append(('%s_s%d' % (d, j), [('_above%d' % k, Fp), ('_below%d' % k, Fm), ('_contour%d' % k, Fc)]))
                for p in levels:
                    extra['%s_s%d_region%d_%s' % (d, j, k, level_tag(p))] = \
                        (Fp >= p).astype(np.int8) - (Fm >= p).astype(np.int8)
                areas[k].append({'day': d, 'levels': [
                    {'level': p, 'above': float(int((Fp >= p).sum())) * R.cell_area,
                     'below': float(int((Fm >= p).sum())) * R.cell_area,
                     'band': float(int((Fc < p).sum())) * R.cell_area} for p in levels]})
                cnt[k].append(R.counts(k, d))
                b = R.bounds(k, d)
                hi[k].append(b[0]), lo[k].append(b[1])
        extra.setdefault('wexcur_counts', []).append(cnt)
        extra.setdefault('wexcur_hi', []).append(hi)
        extra.setdefault('wexcur_lo', []).append(lo)
        extra.setdefault('wexcur_weights', []).append(R.weights)
        block[name] = {'members': int(R.weights.size), 'total_weight': R.total, 'ess': R.ess, 'areas': areas}
    for key in ('wexcur_counts', 'wexcur_hi', 'wexcur_lo', 'wexcur_weights'):
        extra[key] = np.array(extra[key], dtype=np.float64)
    extra['wexcur_scenarios'] = np.array(names)
    extra['wexcur_thresholds'] = np.asarray(first.thresholds, dtype=np.float64)
    extra['wexcur_days'] = extra['days'] = np.asarray(first.days)
    save_maps(outfile, maps, extra)
    return {'scenarios': names, 'thresholds': list(first.thresholds), 'days': list(first.days), 'levels': levels,
            'cell_area': first.cell_area, 'scenario': block}


def save_range(outfile, rng, levels=(0.5, 0.9)):
    '''outfile.npz of one RangeMaps through save_maps: per day of the maps, under the label `{day}`, the CSR
    triplets `{day}_prange{j}_*` of the probability that the cell lies in the member's p_j region; the count planes
    `range_counts` [fractions, days, N, N] (uint16 where the total weight fits, else uint32), the members' rows
    `range_lambda` (fp64) and `range_cells` (uint32) [fractions, days, members], `range_Q` (uint64) and `range_E`
    (int32) [days, members], `range_weights` [members], `range_fractions` and `range_days` -> its block for the
    json: fractions, days, levels, members, weight, cell area and per fraction and day the mean and quantiles of
    the region's area (RangeMaps.area at 0.05, 0.5, 0.95) and the m^2 of the consensus region {prob >= level} at
    each level'''
    levels = check_levels(levels)
    nj = len(rng.fractions)
    W = int(rng.total_weight)
    ctype = np.uint16 if W <= 0xffff else np.uint32
    q_levels = [0.05, 0.5, 0.95]
    maps, areas = [], [[] for _ in range(nj)]
    for d in rng.days:
        day_maps = []
        for j in range(nj):
            P = rng.prob(j, d)
            day_maps.append(('_prange%d' % j, P))
            rec = rng.area(j, d, q_levels)
            rec['consensus'] = [{'level': p, 'area': float(int((P >= p).sum())) * rng.cell_area} for p in levels]
            areas[j].append(rec)
        maps.append((d, day_maps))
    rows = [[rng._members(j, d) for d in rng.days] for j in range(nj)]
    mass = [rng.mass(d) for d in rng.days]
    extra = {'range_counts': np.array([[rng.counts(j, d) for d in rng.days] for j in range(nj)]).astype(ctype),
             'range_lambda': np.array([[x[0] for x in row] for row in rows], dtype=np.float64),
             'range_cells': np.array([[x[1] for x in row] for row in rows], dtype=np.uint32),
             'range_Q': np.array([x[0] for x in mass], dtype=np.uint64),
             'range_E': np.array([x[1] for x in mass], dtype=np.int32),
             'range_weights': np.asarray(rows[0][0][2], dtype=np.uint32),
             'range_fractions': np.asarray(rng.fractions, dtype=np.float64), 'range_days': np.asarray(rng.days)}
    save_maps(outfile, maps, extra)
    return {'fractions': list(rng.fractions), 'days': list(rng.days), 'levels': levels, 'area_levels': q_levels,
            'members': rng.members, 'total_weight': rng.total_weight, 'cell_area': rng.cell_area, 'areas': areas}


def mc_error_block(mc, keys, labels, prefix, maps):
    '''the maps of one pooled MonteCarloError appended to `maps` for save_maps (keys: its days or output
    indices, labels: theirs in the file behind `prefix`) -> its block for the json'''
    nk = len(mc.thresholds)
    outputs = []
    for key, label in zip(keys, labels):
        ess = mc.ess(key)
        rhat = None if mc.rhat is None else mc.rhat[key]
        day_maps = [('_mcse', mc.mcse(key)), ('_ess', ess)]
        if rhat is not None:
            day_maps.append(('_rhat', rhat))
        day_maps += [('_pmcse%d' % k, mc.prob_mcse(key, k)) for k in range(nk)]
        maps.append(('%s%s' % (prefix, label), day_maps))
        live = mc.counts(key, 0)[0] > 0 if nk else mc.mean(key) > 0
        rec = {'label': label, 'cells': int(live.sum()), 'ess_min': None, 'ess_median': None, 'rhat_max': None}
        if live.any():
            rec['ess_min'] = float(ess[live].min())
            rec['ess_median'] = float(np.median(ess[live]))
            if rhat is not None:
                rec['rhat_max'] = float(rhat[live].max())
        outputs.append(rec)
    return {'thresholds': list(mc.thresholds), 'batches_pooled': mc.batches, 'used_weight': mc.used_weight,
            'discarded_weight': mc.discarded_weight, 'members': mc.members, 'outputs': outputs}


# ------------------------------------------------------------------ driver
class PredictiveResult():
    '''What posterior_predictive returns: `summary` (a SpreadSummary, None without a device),
    `rows` (trace rows after burn / thin), `evaluations`, `failed`, `seconds`, `runs`
    ([(chain, first_row, weight)] of every evaluated run), `observations` (observation_predictive
    or None) and `provenance`; with quantile levels `histogram` (a SpreadHistogram, None without a
    device) and `quantiles` (the levels), else both None; with arrival thresholds `arrival` (ArrivalMaps,
    None without a device) and `arrival_levels`, else both None; `emergence` / `exposure`: ProjectedMaps of the
    emergence and cumulative-exposure projections, None where not asked for; `sites`: ProjectedMaps of the
    release plan (with `plan` and, with arrival thresholds, `arrival`), None where not asked for;
    `sensitivity`: SensitivityMaps over the summary's days, None where not asked for (the projections and the
    plan then carry one of their own); `contrast`: the PlanContrast of the release plan against the plan of
    compare= and `compare_plan` that plan (ReleaseSites.describe()), both None where not asked for; `ranking`: the
    PlanRanking of the release plan and the further plans of ranking=, `ranking_plans` all of them, plan A's first
    (ReleaseSites.describe()), and `ranking_levels` the levels of its saved area quantiles, all None where not
    asked for; `weather`: the WeatherShare over the summary's days of a weather ensemble (wind= with share; the
    projections and the plan carry one of their own) and `wind` its plan as evaluated (pool, block, seed, the
    sequences, host seconds of the kernel batches and the draws), both None without wind=; `mc_error`:
    the MonteCarloError over the summary's days, all chains' half sequences pooled in chain order, its `rhat`
    their split R-hat maps, and `mc_plan` = dict(batches, batch_weight, sequences), both None where not asked for
    (the projections and the plan then carry an `mc_error` of their own); `peak`: the PeakPosterior over the
    summary's days, None where not asked for (the plan then carries a `peak` of its own); `excursion`: the
    ExcursionMaps over the summary's days and `excursion_levels` the credible levels of its saved regions, both
    None where not asked for (the plan then carries an `excursion` of its own); `reweight`: the ReweightedSummary
    over the summary's days and thresholds, and `reweight_info` = dict(names, probes -- as given, None for a
    scenario of row log-weights --, min_ess, diagnostics: {name: reweight_diagnostics + members, skipped,
    log_total_weight}), both None where not asked for (the projections and the plan then carry a `reweight` of
    their own); `reweight_histogram` / `reweight_arrival`: the ReweightedHistogram and the ReweightedArrival over
    the summary's days, on the edges of quantiles= and the thresholds of arrival=, None unless reweight's
    options['maps'] names 'quantiles' / 'arrival' (the projections then carry a `reweight_histogram`, the plan both);
    `reweight_excursion`: {scenario: ReweightedExcursion} over `excursion`, None unless the maps name 'excursion' (the
    plan then carries one over its own excursion maps); `reweight_contrast`: the ReweightedContrast of the release
    plan against the plan of compare=, None unless the maps name 'contrast';
    `catch`: the CatchPosterior of the traps over the model's day fields, None where not asked for
    (the emergence projection and the plan then carry a `catch` of their own where asked for); `information`: the
    InformationPosterior of the described traps over the model's day fields, None where not asked for (the plan then
    carries an `information` of its own); `core_range`: the RangeMaps over the summary's days and
    `core_range_levels` the consensus levels of its saved regions, both None where not asked for (the plan then
    carries a `core_range` of its own); `patches`: the PatchMaps over the summary's days and `patch_levels` the
    levels of its saved quantiles, both None where not asked for (the plan then carries a `patches` of its own);
    `pathways`: the PathwayMaps over the summary's days (or the days asked for) and `pathway_levels` the levels of
    its saved quantiles, both None where not asked for (the plan then carries a `pathways` of its own);
    `representative`: the RepresentativeMembers over `excursion`, `representative_days` the planes of its saved
    outputs ('all' or a list of days) and `representative_chains` per chain the model parameters of its rows, all
    None where not asked for (the plan then carries a `representative` of its own); `neighbourhood`: the
    NeighbourhoodPosterior of the windows over the model's day fields, None where not asked for (the plan then
    carries a `neighbourhood` of its own over the windows on its output days); `modes`: the ModesPosterior over the
    listed days of the model's day fields, None where not asked for (the plan then carries a `modes` of its own);
    `dependence`: the DependenceMaps over the summary's days (or the days asked for), None where not asked for (the
    projections and the plan then carry one of their own); `proximity`: the ProximityPosterior of the windows over
    the model's day fields, None where not asked for (the plan then carries a `proximity` of its own over the
    windows on its output days); `origin`: the OriginMaps of the findings over the model's day records, None where
    not asked for.'''

    def __init__(self, summary, rows, evaluations, failed, seconds, runs, observations, provenance, days,
                 histogram=None, quantiles=None, arrival=None, arrival_levels=None, emergence=None, exposure=None,
                 sites=None, sensitivity=None, contrast=None, compare_plan=None, mc_error=None, mc_plan=None,
                 peak=None, excursion=None, excursion_levels=None, reweight=None, reweight_info=None, catch=None,
                 information=None, core_range=None, core_range_levels=None, patches=None, patch_levels=None,
                 representative=None, representative_days=None, representative_chains=None, neighbourhood=None,
                 modes=None, dependence=None, pathways=None, pathway_levels=None, proximity=None, origin=None,
                 reweight_histogram=None, reweight_arrival=None, ranking=None, ranking_plans=None,
                 ranking_levels=None, weather=None, wind=None, reweight_excursion=None, reweight_contrast=None):
        self.reweight_contrast = reweight_contrast
        self.reweight_excursion = reweight_excursion
        self.weather = weather
        self.wind = wind
        self.ranking = ranking
        self.ranking_plans = ranking_plans
        self.ranking_levels = ranking_levels
        self.reweight_histogram = reweight_histogram
        self.reweight_arrival = reweight_arrival
        self.origin = origin
        self.proximity = proximity
        self.pathways = pathways
        self.pathway_levels = pathway_levels
        self.dependence = dependence
        self.modes = modes
        self.neighbourhood = neighbourhood
        self.representative = representative
        self.representative_days = representative_days
        self.representative_chains = representative_chains
        self.patches = patches
        self.patch_levels = patch_levels
        self.catch = catch
        self.information = information
        self.core_range = core_range
        self.core_range_levels = core_range_levels
        self.peak = peak
        self.excursion = excursion
        self.excursion_levels = excursion_levels
        self.reweight = reweight
        self.reweight_info = reweight_info
        self.summary = summary
        self.mc_error = mc_error
        self.mc_plan = mc_plan
        self.contrast = contrast
        self.compare_plan = compare_plan
        self.sensitivity = sensitivity
        self.emergence = emergence
        self.exposure = exposure
        self.sites = sites
        self.histogram = histogram
        self.quantiles = quantiles
        self.arrival = arrival
        self.arrival_levels = arrival_levels
        self.rows = rows
        self.evaluations = evaluations
        self.failed = failed
        self.seconds = seconds
        self.runs = runs
        self.observations = observations
        self.provenance = provenance
        self.days = days

    def save(self, outfile, params=None):
        '''outfile.npz in the layout of Run.save_result (Run.py:490-516 of the reference), which
        Plot_Result.main reads: per day `{day}_data/_ind/_indptr` of the posterior mean thresholded at
        1e-8, `days`; besides `{day}_sd_*` and `{day}_pexc{k}_*` CSR triplets, and with a histogram
        `{day}_q{tag}_*` of the quantile point maps (quantile_tag: q5, q50, q95, q2p5).  With arrival maps
        `{day}_parr{k}_*` (P(arrived at t_k by that day)), dense int16 `arrival{k}_{tag}` model-day maps
        (-1: not within the window; dense because the CSR writer drops day 0), `arrival{k}_cells` [members,
        days] and `arrival_weights`.  outfile.json: the params, the thresholds, the chain provenance, with a
        histogram the quantile levels and the edge definition, with arrival maps their thresholds, levels,
        days, cell area and per threshold and day the reached area.  The projections go into files of their own,
        outfile_emergence.npz / outfile_exposure.npz in the same layout (`days` of the main file are model days):
        per output `{label}_*` of the mean, `{label}_sd_*`, `{label}_pexc{k}_*`, `{label}_q{tag}_*`, the label
        the emergence day in days post release, or the exposure's model day; their weights, input days and
        labels under `predictive.emergence` / `predictive.exposure` of the json.  A release plan goes into
        outfile_sites.npz in that layout too, the label the output day; with arrival maps also `{label}_parr{k}_*`,
        the dense `arrival{k}_{tag}`, `arrival{k}_cells` and `arrival_weights` of the plan, as in the main file;
        under `predictive.sites` of the json the plan (sites in metres and cells, lags, days), the thresholds,
        the levels and with arrival maps their thresholds, levels, cell area and the reached area per threshold.
        Sensitivity maps go into outfile_sens.npz (those of a projection or a plan into outfile_NAME_sens.npz):
        per day `{day}_corr_{name}_*` signed CSR triplets (|value| >= 1e-8) of the correlation with every
        parameter and, once finalized, `{day}_r2_*` of the explained share and dense int8 `{day}_dom` (index
        into the parameters, -1: nothing varies; dense because the CSR writer drops index 0); under
        `predictive.sensitivity` (`predictive.NAME.sensitivity`) of the json the parameter names, their
        posterior means, sds and correlation matrix, rank and dropped eigenvalues, members and weight, and
        where finalize refused -- too few members -- the reason, the correlations alone being saved.
        Dependence maps go into outfile_depend.npz (save_dependence; those of a projection or a plan into
        outfile_NAME_depend.npz): per day `{day}_eta2_{name}_*` CSR triplets of the correlation ratio, dense int8
        `{day}_dom` and, with sensitivity maps over the same names, `{day}_excess_{name}_*`; their block --
        parameters, bins asked and used, edges, bin weights, members, weight and floors -- under
        `predictive.dependence` (`predictive.NAME.dependence`), and where finalize refused the reason, no ratio
        map being saved.
        A contrast of two plans goes into outfile_contrast.npz: per output day `{label}_*` signed CSR triplets
        (|value| >= 1e-8) of the mean of A - B, `{label}_sd_*`, `{label}_ppos_*` / `{label}_pneg_*` (P(A > B),
        P(A < B)), `{label}_pgain{k}_*` / `{label}_ploss{k}_*`, and `coverage{k}_a` / `coverage{k}_b` [members,
        outputs] with `contrast_weights`; under `predictive.contrast` of the json plan B, the thresholds, labels,
        members, weight, cell area, levels and per threshold the coverage difference.
        A ranking of several plans goes into outfile_ranking.npz: per output day and plan j `{label}_pbest{j}_*`
        (P(plan j alone is best)), `{label}_regret{j}_*`, `{label}_regret_sd{j}_*` and per threshold
        `{label}_psole{k}_{j}_*`; per output day and threshold `{label}_pany{k}_*` / `{label}_pall{k}_*`; dense int8
        `{label}_leader` (PlanRanking.leader: -1 where no plan is ever alone on top; dense because the CSR writer
        drops index 0), `coverage{k}` [members, plans, outputs] and `ranking_weights`; under `predictive.ranking`
        of the json the plans, names, thresholds, labels, members, weight, cell area, levels and per threshold
        the coverage ranking.
        The Monte Carlo error goes into outfile_mcerr.npz: per day `{label}_mcse_*` (the standard error of the
        posterior mean), `{label}_ess_*`, `{label}_rhat_*` (where there are R-hat maps) and per threshold
        `{label}_pmcse{k}_*` (the standard error of the exceedance probability); those of a projection or a plan
        in the same file under the labels `NAME_{label}`; under `predictive.mc_error` of the json the batches
        per chain, the batch weight, the sequences, the used and the discarded weight and per output `ess_min`,
        `ess_median` and `rhat_max` over the cells whose threshold-0 count is > 0 (without thresholds: whose mean
        is > 0), null where there are none; `predictive.mc_error.NAME` the same for a projection or a plan.
        Peak maps go into outfile_peak.npz (save_peak; those of a release plan into outfile_sites_peak.npz), their
        block under `predictive.peak` (`predictive.sites.peak`) of the json.
        Reweighted quantile and arrival maps (reweight's maps option) go into outfile_reweight_quantiles.npz
        (save_reweight_quantiles: `s{j}_{label}_q{tag}_*`) and outfile_reweight_arrival.npz (save_reweight_arrival:
        `s{j}_{label}_parr{k}_*`, dense `s{j}_arrival{k}_q{tag}`), those of a projection or a plan into
        outfile_NAME_reweight_quantiles.npz / outfile_NAME_reweight_arrival.npz; reweighted excursion regions into
        outfile_reweight_excur.npz and outfile_sites_reweight_excur.npz (save_reweight_excursion), their block under
        `predictive.reweight.excursion` (`predictive.sites.reweight.excursion`); a reweighted contrast into
        outfile_reweight_contrast.npz (save_reweight_contrast: `s{j}_{label}_*` as the contrast's own file), its
        block -- per scenario the thresholds, the total log-weight and per threshold the reweighted coverage
        difference -- under `predictive.reweight.contrast`; `predictive.reweight` of the json
        then carries `maps` and, with arrival maps, per scenario the reached-area curve `reached_area`
        (`predictive.sites.reweight.reached_area` for a plan).
        Excursion maps go into outfile_excur.npz (save_excursion; those of a release plan into
        outfile_sites_excur.npz), their block under `predictive.excursion` (`predictive.sites.excursion`).
        Catch-probability maps go into outfile_catch.npz (save_catch; those of the emergence projection and of a
        release plan into outfile_NAME_catch.npz), their block under `predictive.catch` (`predictive.NAME.catch`),
        with the traps as given; their reweighted maps into outfile_catch_reweight.npz (save_reweight) and their
        Monte Carlo error into outfile_mcerr.npz under the labels `catch_c{e}`.
        Information maps go into outfile_information.npz (save_information; those of a release plan into
        outfile_sites_information.npz), their block under `predictive.information` (`predictive.sites.information`),
        with the traps as given.
        Core-range maps go into outfile_range.npz (save_range; those of a release plan into
        outfile_sites_range.npz), their block under `predictive.core_range` (`predictive.sites.core_range`).
        Patch maps go into outfile_patch.npz (save_patches; those of a release plan into outfile_sites_patch.npz),
        their block under `predictive.patches` (`predictive.sites.patches`).
        Pathway maps go into outfile_pathway.npz (save_pathways; those of a release plan into
        outfile_sites_pathway.npz), their block under `predictive.pathways` (`predictive.sites.pathways`).
        Representative members go into outfile_repr.npz (save_representative; those of a release plan into
        outfile_sites_repr.npz), their block under `predictive.representative` (`predictive.sites.representative`).
        Ensemble modes go into outfile_modes.npz (save_modes; those of a release plan into outfile_sites_modes.npz),
        their block under `predictive.modes` (`predictive.sites.modes`).
        A weather ensemble's split goes into outfile_weather.npz: per day `{label}_vw_*`, `{label}_vp_*` and
        `{label}_share_*` (the variance over the wind, the parameters' and the weather's share), those of a
        projection or a plan under the labels `NAME_{label}`; under `predictive.wind` of the json the pool, block,
        seed and sequences as evaluated, the groups, the members and per day the mean-weighted share
        sum(share mean) / sum(mean) (`predictive.wind.NAME` for a projection or a plan).
        -> (npz path, json path)'''
        s = self.summary
        if s is None:
            raise ValueError('no spread summary to save (evaluate= runs without a device)')
        h = self.histogram
        levels = list(self.quantiles or ()) if h is not None else []
        A = self.arrival
        a_levels = list(self.arrival_levels or ()) if A is not None else []
        maps = []
        for d in s.days:
            label = s.pm.days[d] if d < len(s.pm.days) else d
            day_maps = [('', s.mean(d)), ('_sd', s.sd(d))]
            day_maps += [('_pexc%d' % k, s.exceedance(d, k)) for k in range(len(s.thresholds))]
            day_maps += [('_' + quantile_tag(p), h.quantile(d, p)) for p in levels]
            if A is not None:
                day_maps += [('_parr%d' % k, A.prob_by(k, d)) for k in range(len(A.thresholds))]
            maps.append((label, day_maps))
        extra = {}
        if A is not None:
            for k in range(len(A.thresholds)):
                for p in a_levels:
                    extra['arrival%d_%s' % (k, quantile_tag(p))] = A.quantile(k, p).astype(np.int16)
                cells, w = A.reached(k)
                extra['arrival%d_cells' % k] = cells
            extra['arrival_weights'] = w
        save_maps(outfile, maps, extra)
        pdict = params_dict(params)
        meta = dict(pdict)
        meta['predictive'] = {'thresholds': s.thresholds, 'total_weight': s.total_weight, 'members': s.members,
                              'rows': self.rows, 'evaluations': self.evaluations, 'failed': self.failed,
                              'chains': self.provenance}
        if h is not None:
            meta['predictive']['quantiles'] = {'levels': levels, 'bins': None if h.bins is None else list(h.bins),
                                               'edges': None if h.bins is not None else [float(e) for e in h.edges],
                                               'nedge': int(h.edges.size)}
        if A is not None:
            meta['predictive']['arrival'] = {'thresholds': list(A.thresholds), 'levels': a_levels,
                                             'days': list(A.days), 'cell_area': A.cell_area,
                                             'reached_area': [A.reached_area(k, a_levels)
                                                              for k in range(len(A.thresholds))]}
        if self.sensitivity is not None:
            labels = [s.pm.days[d] if d < len(s.pm.days) else d for d in s.days]
            meta['predictive']['sensitivity'] = save_sensitivity('%s_sens' % outfile, self.sensitivity, s.days, labels)
        if self.dependence is not None:
            dm = self.dependence
            labels = [s.pm.days[d] if d < len(s.pm.days) else d for d in dm.days]
            meta['predictive']['dependence'] = save_dependence('%s_depend' % outfile, dm, dm.days, labels,
                                                               self.sensitivity)
        for name, pr in (('emergence', self.emergence), ('exposure', self.exposure), ('sites', self.sites)):
            if pr is None:
                continue
            ps, ph, pa = pr.summary, pr.histogram, pr.arrival
            p_levels = list(self.quantiles or ()) if ph is not None else []
            pa_levels = list(self.arrival_levels or ()) if pa is not None else []
            pmaps = []
            for e, label in enumerate(pr.labels):
                out_maps = [('', ps.mean(e)), ('_sd', ps.sd(e))]
                out_maps += [('_pexc%d' % k, ps.exceedance(e, k)) for k in range(len(ps.thresholds))]
                out_maps += [('_' + quantile_tag(p), ph.quantile(e, p)) for p in p_levels]
                if pa is not None:
                    out_maps += [('_parr%d' % k, pa.prob_by(k, label)) for k in range(len(pa.thresholds))]
                pmaps.append((label, out_maps))
            pextra = {}
            if pa is not None:
                for k in range(len(pa.thresholds)):
                    for p in pa_levels:
                        pextra['arrival%d_%s' % (k, quantile_tag(p))] = pa.quantile(k, p).astype(np.int16)
                    cells, w = pa.reached(k)
                    pextra['arrival%d_cells' % k] = cells
                pextra['arrival_weights'] = w
            save_maps('%s_%s' % (outfile, name), pmaps, pextra)
            if pr.plan is None:
                meta['predictive'][name] = {'weights': np.asarray(pr.weights).tolist(), 'in_days': list(pr.in_days)}
            else:
                meta['predictive'][name] = dict(pr.plan)
            meta['predictive'][name].update({'labels': list(pr.labels), 'thresholds': list(ps.thresholds),
                                             'levels': p_levels})
            if pa is not None:
                meta['predictive'][name]['arrival'] = {
                    'thresholds': list(pa.thresholds), 'levels': pa_levels, 'cell_area': pa.cell_area,
                    'reached_area': [pa.reached_area(k, pa_levels) for k in range(len(pa.thresholds))]}
            if pr.sensitivity is not None:
                meta['predictive'][name]['sensitivity'] = save_sensitivity(
                    '%s_%s_sens' % (outfile, name), pr.sensitivity, list(range(len(pr.labels))), pr.labels)
            if pr.dependence is not None:
                meta['predictive'][name]['dependence'] = save_dependence(
                    '%s_%s_depend' % (outfile, name), pr.dependence, list(range(len(pr.labels))), pr.labels,
                    pr.sensitivity)
            if pr.peak is not None:
                meta['predictive'][name]['peak'] = save_peak('%s_%s_peak' % (outfile, name), pr.peak,
                                                             list(self.quantiles or ()))
            if pr.excursion is not None:
                meta['predictive'][name]['excursion'] = save_excursion('%s_%s_excur' % (outfile, name), pr.excursion,
                                                                       self.excursion_levels)
            if pr.core_range is not None:
                meta['predictive'][name]['core_range'] = save_range('%s_%s_range' % (outfile, name), pr.core_range,
                                                                    self.core_range_levels)
            if pr.patches is not None:
                meta['predictive'][name]['patches'] = save_patches('%s_%s_patch' % (outfile, name), pr.patches,
                                                                   self.patch_levels)
            if pr.pathways is not None:
                meta['predictive'][name]['pathways'] = save_pathways('%s_%s_pathway' % (outfile, name), pr.pathways,
                                                                     self.pathway_levels)
        for name, rp in (('', self.representative),
                         ('sites_', None if self.sites is None else self.sites.representative)):
            if rp is not None:
                block = save_representative('%s_%srepr' % (outfile, name), rp, self.runs, self.representative_chains,
                                            self.representative_days)
                (meta['predictive'][name[:-1]] if name else meta['predictive'])['representative'] = block
        for name, mp in (('', self.modes), ('sites_', None if self.sites is None else self.sites.modes)):
            if mp is not None:
                block = save_modes('%s_%smodes' % (outfile, name), mp)
                block['given'] = mp.given
                (meta['predictive'][name[:-1]] if name else meta['predictive'])['modes'] = block
        if self.pathways is not None:
            meta['predictive']['pathways'] = save_pathways('%s_pathway' % outfile, self.pathways, self.pathway_levels)
        if self.patches is not None:
            meta['predictive']['patches'] = save_patches('%s_patch' % outfile, self.patches, self.patch_levels)
        if self.core_range is not None:
            meta['predictive']['core_range'] = save_range('%s_range' % outfile, self.core_range,
                                                          self.core_range_levels)
        if self.excursion is not None:
            meta['predictive']['excursion'] = save_excursion('%s_excur' % outfile, self.excursion,
                                                             self.excursion_levels)
        if self.peak is not None:
            meta['predictive']['peak'] = save_peak('%s_peak' % outfile, self.peak, list(self.quantiles or ()))
        X = self.contrast
        if X is not None:
            x_levels = list(self.arrival_levels or (0.05, 0.5, 0.95))
            nk = len(X.thresholds)
            xmaps = []
            for e, label in enumerate(X.labels):
                out_maps = [('', X.mean(e)), ('_sd', X.sd(e)), ('_ppos', X.prob_positive(e)),
                            ('_pneg', X.prob_negative(e))]
                for k in range(nk):
                    out_maps += [('_pgain%d' % k, X.gain(e, k)), ('_ploss%d' % k, X.loss(e, k))]
                xmaps.append((label, out_maps))
            xextra = {'contrast_weights': X.weights}
            for k in range(nk):
                xextra['coverage%d_a' % k], xextra['coverage%d_b' % k], _w = X.coverage(k)
            save_maps('%s_contrast' % outfile, xmaps, xextra, signed=True)
            meta['predictive']['contrast'] = {
                'plan_b': self.compare_plan, 'thresholds': list(X.thresholds), 'labels': list(X.labels),
                'members': X.members, 'total_weight': X.total_weight, 'cell_area': X.cell_area, 'levels': x_levels,
                'coverage_difference': [X.coverage_difference(k, x_levels) for k in range(nk)]}
        K = self.ranking
        if K is not None:
            k_levels = list(self.ranking_levels or (0.05, 0.5, 0.95))
            nk = len(K.thresholds)
            kmaps = []
            kextra = {'ranking_weights': K.weights}
            for e, label in enumerate(K.labels):
                out_maps = []
                for j in range(K.nplan):
                    out_maps += [('_pbest%d' % j, K.prob_best(e, j)), ('_regret%d' % j, K.regret(e, j)),
                                 ('_regret_sd%d' % j, K.regret_sd(e, j))]
                    out_maps += [('_psole%d_%d' % (k, j), K.sole(e, k, j)) for k in range(nk)]
                for k in range(nk):
                    out_maps += [('_pany%d' % k, K.any(e, k)), ('_pall%d' % k, K.all(e, k))]
                kmaps.append((label, out_maps))
                kextra['%s_leader' % label] = K.leader(e)
            for k in range(nk):
                kextra['coverage%d' % k] = K.coverage(k)[0]
            save_maps('%s_ranking' % outfile, kmaps, kextra)
            meta['predictive']['ranking'] = {
                'plans': self.ranking_plans, 'names': list(K.names), 'thresholds': list(K.thresholds),
                'labels': list(K.labels), 'members': K.members, 'total_weight': K.total_weight,
                'cell_area': K.cell_area, 'levels': k_levels,
                'coverage_ranking': [K.coverage_ranking(k, k_levels) for k in range(nk)]}
        R = self.reweight
        if R is not None:
            labels = [s.pm.days[d] if d < len(s.pm.days) else d for d in s.days]
            save_reweight('%s_reweight' % outfile, R, s.days, labels)
            meta['predictive']['reweight'] = dict(self.reweight_info or {})
            meta['predictive']['reweight'].update({'days': list(s.days), 'labels': labels,
                                                   'thresholds': list(R.thresholds)})
            for name, pr in (('emergence', self.emergence), ('exposure', self.exposure), ('sites', self.sites)):
                if pr is not None and pr.reweight is not None:
                    save_reweight('%s_%s_reweight' % (outfile, name), pr.reweight, list(range(len(pr.labels))),
                                  pr.labels)
            # the maps option: outfile_reweight_quantiles.npz / outfile_reweight_arrival.npz, those of a projection
            # or a plan outfile_NAME_reweight_*.npz; per scenario the reached-area curve into the json
            for name, fs, keys, flabels in [('', self, s.days, labels)] + [
                    (n + '_', pr, list(range(len(pr.labels))), pr.labels) for n, pr in (
                        ('emergence', self.emergence), ('exposure', self.exposure), ('sites', self.sites))
                    if pr is not None]:
                rh, ra = fs.reweight_histogram, fs.reweight_arrival
                if rh is not None:
                    save_reweight_quantiles('%s_%sreweight_quantiles' % (outfile, name), rh, keys, flabels,
                                            list(self.quantiles or ()))
                if ra is not None:
                    ra_levels = list(self.arrival_levels or ())
                    save_reweight_arrival('%s_%sreweight_arrival' % (outfile, name), ra, ra.days,
                                          flabels if not name else ra.days, ra_levels)     # a plan's days are its labels
                    block = meta['predictive']['reweight'] if not name else \
                        meta['predictive'][name[:-1]].setdefault('reweight', {})
                    block['reached_area'] = {n: [ra.reached_area(n, k, fs.arrival, ra_levels)
                                                 for k in range(len(ra.thresholds))] for n in ra.scenarios}
            # maps=('excursion',): outfile_reweight_excur.npz, the plan's outfile_sites_reweight_excur.npz
            for name, fs in (('', self), ('sites_', self.sites)):
                rx = getattr(fs, 'reweight_excursion', None)
                if rx:
                    block = save_reweight_excursion('%s_%sreweight_excur' % (outfile, name), rx,
                                                    self.excursion_levels)
                    (meta['predictive']['reweight'] if not name else
                     meta['predictive'][name[:-1]].setdefault('reweight', {}))['excursion'] = block
            # maps=('contrast',): outfile_reweight_contrast.npz, per scenario the coverage difference into the json
            if self.reweight_contrast is not None:
                meta['predictive']['reweight']['contrast'] = save_reweight_contrast(
                    '%s_reweight_contrast' % outfile, self.reweight_contrast, self.contrast,
                    list(self.arrival_levels or (0.05, 0.5, 0.95)))
        area = getattr(self, 'cell_area', None)
        for name, cp in [('', self.catch)] + [(n + '_', pr.catch) for n, pr in (
                ('emergence', self.emergence), ('sites', self.sites)) if pr is not None]:
            if cp is None:
                continue
            block = save_catch('%s_%scatch' % (outfile, name), cp, area)
            block['given'] = cp.given
            keys, labels = list(range(len(cp.traps))), ['c%d' % e for e in range(len(cp.traps))]
            if cp.reweight is not None:
                save_reweight('%s_%scatch_reweight' % (outfile, name), cp.reweight, keys, labels)
            (meta['predictive'][name[:-1]] if name else meta['predictive'])['catch'] = block
        for name, nb in (('', self.neighbourhood),
                         ('sites_', None if self.sites is None else self.sites.neighbourhood)):
            if nb is None:
                continue
            block = save_neighbourhood('%s_%snbhd' % (outfile, name), nb, area)
            block['given'] = nb.given
            if nb.reweight is not None:
                save_reweight('%s_%snbhd_reweight' % (outfile, name), nb.reweight, list(range(len(nb.windows))),
                              ['n%d' % e for e in range(len(nb.windows))])
            (meta['predictive'][name[:-1]] if name else meta['predictive'])['neighbourhood'] = block
        for name, px in (('', self.proximity),
                         ('sites_', None if self.sites is None else self.sites.proximity)):
            if px is None:
                continue
            block = save_proximity('%s_%sprox' % (outfile, name), px, area)
            block['given'] = px.given
            if px.reweight is not None:
                save_reweight('%s_%sprox_reweight' % (outfile, name), px.reweight, list(range(len(px.windows))),
                              ['x%d' % e for e in range(len(px.windows))])
            (meta['predictive'][name[:-1]] if name else meta['predictive'])['proximity'] = block
        for name, ip in (('', self.information),
                         ('sites_', None if self.sites is None else self.sites.information)):
            if ip is None:
                continue
            block = save_information('%s_%sinformation' % (outfile, name), ip, area)
            block['given'] = ip.given
            (meta['predictive'][name[:-1]] if name else meta['predictive'])['information'] = block
        if self.origin is not None:       # outfile_origin.npz (save_origin), the block under predictive.origin
            _path, meta['predictive']['origin'] = save_origin(str(outfile), self.origin)
        if self.mc_error is not None:
            mmaps = []
            labels = [s.pm.days[d] if d < len(s.pm.days) else d for d in s.days]
            block = dict(self.mc_plan or {})
            block.update(mc_error_block(self.mc_error, s.days, labels, '', mmaps))
            for name, pr in (('emergence', self.emergence), ('exposure', self.exposure), ('sites', self.sites)):
                if pr is not None and pr.mc_error is not None:
                    block[name] = mc_error_block(pr.mc_error, list(range(len(pr.labels))), pr.labels, name + '_',
                                                 mmaps)
            for name, cp in (('catch', self.catch),
                             ('emergence_catch', None if self.emergence is None else self.emergence.catch),
                             ('sites_catch', None if self.sites is None else self.sites.catch)):
                if cp is not None and cp.mc_error is not None:
                    block[name] = mc_error_block(cp.mc_error, list(range(len(cp.traps))),
                                                 ['c%d' % e for e in range(len(cp.traps))], name + '_', mmaps)
            for name, nb in (('neighbourhood', self.neighbourhood),
                             ('sites_neighbourhood', None if self.sites is None else self.sites.neighbourhood)):
                if nb is not None and nb.mc_error is not None:
                    block[name] = mc_error_block(nb.mc_error, list(range(len(nb.windows))),
                                                 ['n%d' % e for e in range(len(nb.windows))], name + '_', mmaps)
            for name, px in (('proximity', self.proximity),
                             ('sites_proximity', None if self.sites is None else self.sites.proximity)):
                if px is not None and px.mc_error is not None:
                    block[name] = mc_error_block(px.mc_error, list(range(len(px.windows))),
                                                 ['x%d' % e for e in range(len(px.windows))], name + '_', mmaps)
            save_maps('%s_mcerr' % outfile, mmaps)
            meta['predictive']['mc_error'] = block
        if self.wind is not None:
            w = self.wind
            block = {'pool': list(w['pool']), 'block': w['block'], 'seed': w['seed'], 'share': w['share'],
                     'pool_kernels': w['pool_kernels'], 'sequences': np.asarray(w['sequences']).tolist()}
            if self.weather is not None:
                wmaps = []
                labels = [s.pm.days[d] if d < len(s.pm.days) else d for d in s.days]
                block.update(weather_block(self.weather, s.days, labels, '', s.mean, wmaps))
                for name, pr in (('emergence', self.emergence), ('exposure', self.exposure), ('sites', self.sites)):
                    if pr is not None and pr.weather is not None:
                        block[name] = weather_block(pr.weather, list(range(len(pr.labels))), pr.labels, name + '_',
                                                    pr.summary.mean, wmaps)
                save_maps('%s_weather' % outfile, wmaps)
            meta['predictive']['wind'] = block
        with open(str(outfile) + '.json', 'w') as fobj:
            json.dump(meta, fobj, default=str)
        return str(outfile) + '.npz', str(outfile) + '.json'


def _evaluate_wind_run(pm, theta, first, length, wind, sets):
    '''One run of a chain under every wind sequence of the checked wind= plan: one batch of day kernels for the
    days the sequences use (PopModel.build_pool), every entry checked before the first sequence runs -- a run with
    a failing day is a failed member and is added nowhere -- then per sequence the chain (run_sequence; with
    pool_kernels=False an evaluation of the model over days=sequence, the A/B leg) and every set's feed with the
    run's length, and after the last the close of the run's group in every WeatherShare.  -> False for a failed
    member.  wind['build_s'] / wind['draw_s'] collect the host time of the builds (which end in a synchronise) and
    of the enqueueing of the draws.'''
    args = mcmc.model_args(theta)
    seqs = wind['sequences']
    recorded = pm.days

    def parameter_failure(e):
        return isinstance(e, (AssertionError, ValueError)) or (isinstance(e, L.HipError)
                                                               and e.code in mcmc._PARAMETER_ERRORS)
    t0 = time.perf_counter()
    try:
        pm.build_pool(*args, wind['used'], [int(s[0]) for s in seqs])
        pm.check_pool()
    except (AssertionError, ValueError, L.HipError) as e:
        if not parameter_failure(e):
            raise
        return False
    t1 = time.perf_counter()
    wind['build_s'].append(t1 - t0)
    for j, seq in enumerate(seqs):
        try:
            if wind['pool_kernels']:
                pm.run_sequence([int(d) for d in seq])
            else:
                pm.days = [int(d) for d in seq]
                try:
                    pm.evaluate(*args, want_stats=False)
                finally:
                    pm.days = recorded
        except (AssertionError, ValueError, L.HipError) as e:
            if not parameter_failure(e):
                raise
            if j == 0:
                return False
            raise RuntimeError('wind: draw %d of the run at row %d failed after %d draws of it were added (%s)'
                               % (j, first, j, e))
        member = types.SimpleNamespace(theta=theta, first=first, length=length, lam=None)
        for fs in sets:
            fs.feed(member)
    for fs in sets:
        if getattr(fs, 'weather', None) is not None:
            fs.weather.close_group(length)
    wind['draw_s'].append(time.perf_counter() - t1)
    return True


def _evaluate_runs(pm, rows, run_list, model_cols, evaluate, want_obs, locinfo, sets=(), wind=None):
    '''one chain: evaluate every run and feed it to the chain's sets (_FieldSet) in the order given, each in the
    FEED_ORDER of its kind.  With a 'sites' set the models of the plan's later release days are evaluated with the
    base model -- with a 'compare' or 'ranking' set those of all plans' (its `lagged`), each once -- and a member for which any
    of them fails is a failed member and is added nowhere.  With an origin= on the 'days' set the models of its
    hypotheses' later release days are evaluated too; a model the plan shares is evaluated once, over the days its
    longest reader needs.  The solver's FFT size follows the days evaluated, so where the findings reach further than
    the plan's output days the plan's maps can differ in their last bits from a run without origin= (never where
    the plan needs at least as many days).  wind: the checked plan of wind=; every run is then evaluated under each of
    its sequences (_evaluate_wind_run) and a member is (run, draw).  -> (expected per run or None, failed)'''
    expected = []
    failed = 0
    kinds = {fs._kind: fs for fs in sets}
    plan, both = kinds.get('sites'), kinds.get('compare')
    if both is None:                   # a 'ranking' set carries the same models: those of every plan's later days
        both = kinds.get('ranking')
    origin = getattr(kinds.get('days'), 'origin', None)
    for first, length in run_list:
        theta = rows[first, model_cols]
        if wind is not None:
            ok = _evaluate_wind_run(pm, theta, first, length, wind, sets)
            failed += not ok
            expected.append(True if ok else None)
            continue
        if evaluate is not None:
            exp = evaluate(theta)
            if exp is None:
                failed += 1
            expected.append(exp)
            continue
        try:
            pm.evaluate(*mcmc.model_args(theta), want_stats=False)
            if origin is not None:     # each later release day's model once, over the days its longest reader needs
                need = {lag: origin.days[-1] - lag + 1 for lag in origin.lagged}
                if plan is not None:
                    for lag in (both.lagged if both is not None else plan._source.lagged):
                        need[lag] = max(need.get(lag, 0), plan._source.days[-1] - lag + 1)
                models = dict(both.lagged if both is not None else plan._source.lagged if plan is not None else {})
                models.update(origin.lagged)
                for lag, n in sorted(need.items()):
                    models[lag].evaluate(*mcmc.model_args(theta), ndays=n, want_stats=False)
            elif both is not None:
                for lag, m in sorted(both.lagged.items()):
                    m.evaluate(*mcmc.model_args(theta), ndays=plan._source.days[-1] - lag + 1, want_stats=False)
            elif plan is not None:
                plan._source.evaluate_lagged(*mcmc.model_args(theta))
        except (AssertionError, ValueError):
            failed += 1
            expected.append(None)
            continue
        except L.HipError as e:
            if e.code not in mcmc._PARAMETER_ERRORS:
                raise
            failed += 1
            expected.append(None)
            continue
        member = types.SimpleNamespace(theta=theta, first=first, length=length, lam=None)
        for fs in sets:
            fs.feed(member)
        expected.append(mcmc.expected_observations(pm, locinfo) if want_obs else True)
    return expected, failed


def _check_request(q):
    '''Everything of posterior_predictive's arguments (q: a namespace of them) that can fail before any evaluation,
    in a fixed order -- of two bad arguments the earlier one is reported.  -> q, with the checked plans beside the
    arguments: cr_frac / cr_levels, in_plan, ct_plan, nb_plan, px_plan, rw_plan / rw_names, ex_thr / ex_levels, pk_thr / pk_levels,
    mc_batches, mc_b / mc_halves, pt_thr / pt_conn / pt_levels, pw_thr / pw_conn / pw_days / pw_levels, rp_plan, s_names, dp_plan / dp_edges, levels, a_thr / a_levels, plans [(name, W, in_days, labels)], site_plan,
    cmp_plan, the loaded chains `prepared` [(rows, runs, model columns, observation columns, source)], `pms` (the
    models) and want_obs.'''
    pm0 = (q.pop_model[0] if q.pop_model else None) if isinstance(q.pop_model, (list, tuple)) else q.pop_model
    days, thresholds = q.days, q.thresholds
    q.cr_frac = q.cr_levels = q.in_plan = q.ct_plan = q.rw_plan = q.ex_thr = q.ex_levels = None
    q.pk_thr = q.pk_levels = q.mc_batches = q.pt_thr = q.pt_conn = q.pt_levels = q.rp_plan = q.nb_plan = None
    q.md_plan = q.pw_thr = q.pw_conn = q.pw_days = q.pw_levels = q.px_plan = q.or_plan = None

    def ndays0():                     # the model is touched only where an option needs it
        return None if pm0 is None else len(pm0.days)

    def check_core_range_arg():
        q.cr_frac, q.cr_levels = check_core_range(q.core_range, days)

    def check_information_arg():
        q.in_plan = check_information(q.information, ndays0(), q.evaluate)

    def check_catch_arg():
        q.ct_plan = check_catch(q.catch, ndays0(), q.emergence, q.evaluate)

    def check_reweight_arg():
        q.rw_plan = check_reweight(q.reweight, None if pm0 is None else pm0.rad_dist,
                                   None if pm0 is None else pm0.rad_res, ndays0())
        check_peak_thresholds(thresholds)
        nd = len(days) if days is not None else (ndays0() if pm0 is not None else 1)
        if not 1 <= nd <= MAX_REWEIGHT_SLOTS:
            raise ValueError('reweight= takes 1..%d days, got %d' % (MAX_REWEIGHT_SLOTS, nd))

    def check_excursion_arg():
        q.ex_thr, q.ex_levels = check_excursion(q.excursion)
        if days is not None:
            check_arrival_days(days)

    def check_peak_arg():
        q.pk_thr, q.pk_levels = check_peak(q.peak)
        if days is not None:
            check_arrival_days(days)

    def check_mc_error_arg():
        q.mc_batches = mc_error_plan(q.mc_error)
        check_mc_thresholds(thresholds)

    def check_neighbourhood_arg():
        cell_m = None if pm0 is None else float(pm0.rad_dist) / int(pm0.rad_res)
        q.nb_plan = check_neighbourhood(q.neighbourhood, ndays0(), cell_m, q.evaluate)

    def check_proximity_arg():
        cell_m = None if pm0 is None else float(pm0.rad_dist) / int(pm0.rad_res)
        q.px_plan = check_proximity(q.proximity, ndays0(), cell_m, q.evaluate)

    def check_origin_arg():
        if isinstance(q.origin, dict) and isinstance(q.origin.get('known'), str) and q.origin['known'] == 'sites':
            plan = getattr(q, 'sites', None)              # known='sites': the release sites of the run's own plan
            if not isinstance(plan, dict) or 'sites' not in plan:
                raise ValueError("origin: known='sites' takes the sites of the run's own sites= plan, and there is none")
            q.origin = dict(q.origin, known=[tuple(s) for s in plan['sites']])
        q.or_plan = check_origin(q.origin, None if pm0 is None else pm0.rad_dist, None if pm0 is None else pm0.rad_res,
                                 ndays0())
    # the options that need the device, in the order in which they are checked: (name, False switches it off too,
    # its check).  check_information, check_catch, check_neighbourhood and check_proximity refuse evaluate= themselves,
    # after the argument's shape.
    for name, or_false, check in (('core_range', True, check_core_range_arg),
                                  ('information', False, check_information_arg), ('catch', False, check_catch_arg),
                                  ('reweight', False, check_reweight_arg), ('excursion', True, check_excursion_arg),
                                  ('peak', True, check_peak_arg), ('mc_error', True, check_mc_error_arg),
                                  ('neighbourhood', False, check_neighbourhood_arg),
                                  ('proximity', False, check_proximity_arg), ('origin', False, check_origin_arg)):
        arg = getattr(q, name, None)  # a request put together by hand may not know the later options
        if arg is None or (or_false and arg is False):
            continue
        if q.evaluate is not None and name not in ('information', 'catch', 'neighbourhood', 'proximity'):
            raise ValueError('%s= needs the device: not with evaluate=' % name)
        check()
    if q.representative is not None and q.representative is not False:
        if q.evaluate is not None:
            raise ValueError('representative= needs the device: not with evaluate=')
        if not q.ex_thr:
            raise ValueError('representative= compares the members of the excursion maps: it needs excursion=')
        q.rp_plan = check_representative(q.representative)
    q.rw_names = q.rw_plan['names'] if q.rw_plan is not None else None
    q.s_names = check_sens_params(q.sensitivity) if q.sensitivity is not None and q.sensitivity is not False else None
    q.levels = (check_levels(q.quantiles) if q.quantiles is not None else []) or None
    if q.levels:
        bin_edges(q.bins, q.edges)    # a bad edge definition
    q.a_thr = q.a_levels = None
    if q.arrival is not None:
        q.a_thr = check_arrival_thresholds(q.arrival)
        q.a_levels = check_levels(q.arrival_levels)
        if days is not None:
            check_arrival_days(days)
    for what, of, have in (('quantiles', 'quantiles', q.levels), ('arrival', 'arrival', q.a_thr),
                           ('excursion', 'excursion', q.ex_thr),
                           ('contrast', 'compare', getattr(q, 'compare', None) is not None)):
        if what in _reweight_maps(q) and not have:
            raise ValueError("reweight: maps=%r reweights the maps of %s=, and there is none" % (what, of))
    wanted = [(name, arg, plan) for name, arg, plan in (('emergence', q.emergence, emergence_plan),
                                                        ('exposure', q.exposure, exposure_plan)) if arg is not None]
    q.plans = [(name,) + plan(arg) for name, arg, plan in wanted]      # bad projection arguments
    q.site_plan = None
    if q.sites is not None:           # a bad release plan: its cells, days and lags against the model if there is one
        q.site_plan = sites_plan(q.sites, pm0)
        if pm0 is None:
            q.site_plan = None
        else:
            for what, tp in (('catch', q.ct_plan), ('information', q.in_plan)):
                off = [t for t in tp['traps'] if t[0] not in q.site_plan[1]] if tp is not None else []
                if off:
                    raise ValueError('%s: trap %r is not on an output day of the release plan %r'
                                     % (what, off[0], list(q.site_plan[1])))
    q.cmp_plan = None
    if q.compare is not None:         # a bad plan B, or one without a plan A to compare with
        q.cmp_plan = contrast_plan(q.compare, q.sites, pm0)
        check_contrast_thresholds(thresholds)
        if pm0 is None:
            q.cmp_plan = None
    q.rk_plan = None
    if getattr(q, 'ranking', None) is not None:       # bad further plans, or none to rank them with
        q.rk_plan = ranking_plan(q.ranking, q.sites, pm0)
        check_contrast_thresholds(thresholds)
        if pm0 is None:
            q.rk_plan = None
    q.wind_plan = None
    if getattr(q, 'wind', None) is not None:          # a weather ensemble: what it cannot go with, then its own plan
        season = 'its observations belong to the recorded season'
        single = 'its member counts and chain rows assume one member per run'
        for name, why in (('evaluate', 'it needs the device'), ('locinfo', season), ('reweight', season),
                          ('origin', season), ('mc_error', single), ('representative', single),
                          ('sensitivity', single), ('dependence', single)):
            arg = getattr(q, name, None)
            if arg is not None and arg is not False:
                raise ValueError('wind= does not go with %s=: %s' % (name, why))
        if pm0 is None:
            raise ValueError('wind= needs a PopModel')
        q.wind_plan = check_wind(q.wind, pm0)
        late = [('sites', q.site_plan[2] if q.site_plan else ()), ('compare', q.cmp_plan[2] if q.cmp_plan else ())]
        late += [('ranking', ranked[2]) for ranked in (q.rk_plan['plans'] if q.rk_plan else ())]
        for name, lags in late:
            if any(int(lag) > 0 for lag in lags):
                raise ValueError('wind= does not go with a plan of %s= that releases after day 0: the models of '
                                 'the later release days carry their own wind' % name)
    chains = q.chains
    if isinstance(chains, (str, os.PathLike)) or (isinstance(chains, tuple) and len(chains) == 2
                                                   and not isinstance(chains[0], (str, os.PathLike, tuple))):
        chains = [chains]
    loaded = [load_chain(c) for c in chains]
    q.want_obs = q.locinfo is not None
    model_want = model_names()
    obs_want = nuisance_names()
    if q.want_obs:
        obs_want = obs_want + ['sent_obs_probs_{}'.format(k) for k in q.locinfo.sent_ids]
    q.prepared = []
    for trace, names, src in loaded:
        mcols = _columns(names, model_want)
        ocols = _columns(names, obs_want) if q.want_obs else None
        rows, rl = runs(trace, mcols, q.burn, q.thin)
        q.prepared.append((rows, rl, mcols, ocols, src))
    if q.rw_plan is not None:         # row log-weights that do not fit the chains
        check_reweight_rows(q.rw_plan, [len(p[0]) for p in q.prepared])
    q.mc_b = q.mc_halves = None
    if q.mc_batches:                  # a chain shorter than the batches asked for
        q.mc_b, q.mc_halves = mc_batch_plan([len(p[0]) for p in q.prepared], q.mc_batches)
    q.pms = list(q.pop_model) if isinstance(q.pop_model, (list, tuple)) else [q.pop_model]
    if q.evaluate is None and (not q.pms or q.pms[0] is None):
        raise ValueError('a PopModel is needed without evaluate=')
    if (q.a_thr or q.pk_thr is not None or q.ex_thr or q.cr_frac) and q.evaluate is None and days is None:
        check_arrival_days(range(len(q.pms[0].days)))
    if q.evaluate is None:            # projections past the model's days
        q.plans = [(name,) + plan(arg, len(q.pms[0].days)) for name, arg, plan in wanted]
    if q.patches is not None and q.patches is not False:       # after every other check
        if q.evaluate is not None:
            raise ValueError('patches= needs the device: not with evaluate=')
        q.pt_thr, q.pt_conn, q.pt_levels = check_patches(q.patches, days)
        if days is None:
            check_arrival_days(range(len(q.pms[0].days)))
    if q.modes is not None and q.modes is not False:           # after every other check
        if q.evaluate is not None:
            raise ValueError('modes= needs the device: not with evaluate=')
        nd = len(q.pms[0].days)
        q.md_plan = check_modes(q.modes, nd)
        if isinstance(q.md_plan['days'], str):
            check_modes(q.modes, list(range(nd)) if days is None else list(days))     # 'all': the summary's days
        if q.site_plan is not None and len(q.site_plan[1]) > MAX_MODE_DAYS:
            raise ValueError('modes: the release plan has %d output days, at most %d fit'
                             % (len(q.site_plan[1]), MAX_MODE_DAYS))
    if q.pathways is not None and q.pathways is not False:     # after every other check
        if q.evaluate is not None:
            raise ValueError('pathways= needs the device: not with evaluate=')
        q.pw_thr, q.pw_conn, q.pw_days, q.pw_levels = check_pathways(q.pathways)
        nd = len(q.pms[0].days)
        if q.pw_days is not None and q.pw_days[-1] >= nd:
            raise ValueError('pathways: the model has %d days, day %d is not among them' % (nd, q.pw_days[-1]))
        if q.pw_days is None:                                  # the summary's days
            check_arrival_days(range(nd) if days is None else days)
    q.dp_plan = q.dp_edges = None
    if q.dependence is not None and q.dependence is not False:           # after every other check
        if q.evaluate is not None:
            raise ValueError('dependence= needs the device: not with evaluate=')
        q.dp_plan = check_dependence(q.dependence)
        nd = len(q.pms[0].days)
        if q.dp_plan['days'] is not None and q.dp_plan['days'][-1] >= nd:
            raise ValueError('dependence: the model has %d days, day %d is not among them' % (nd, q.dp_plan['days'][-1]))
        # one set of edges for every chain's handle: from the pooled runs of all chains
        q.dp_edges = pooled_dependence_edges(q.prepared, q.dp_plan['params'], q.dp_plan['bins'])
    return q


def _build_sets(sets, q, pm, chain, nruns, late):
    '''the sets of one chain on the model pm, appended to `sets` in the order in which a member is fed to them: the
    day fields', one per projection, the release plan's, the contrast's and the ranking's.  A set is in `sets` before it is built,
    so that the caller can close whatever a failure leaves.  late: {lag: model} of the later release days or None.'''
    def begin(fs, kind, source, name=None, **kw):
        sets.append(fs.fed_from(kind, source, name, **kw))
        return fs
    ct, info, nb, px = q.ct_plan, q.in_plan, q.nb_plan, q.px_plan
    day_traps = dict(catch=ct and (ct['traps'],), information=info and (info['traps'],),
                     neighbourhood=nb and (nb['windows'],), proximity=px and (px['windows'],))
    day = begin(_FieldSet(), 'days', pm, owns=False, **day_traps)
    day._late = late                   # the origin maps read the models of their later release days from here
    day.build(q, chain, nruns)
    for name, W, in_days, labels in q.plans:
        traps = (ct['emergence'], labels) if name == 'emergence' and ct is not None and ct['emergence'] else None
        begin(ProjectedMaps(W, in_days, labels, None), 'projection', Projection(pm, W, in_days), name,
              catch=traps).build(q, chain, nruns)
    if q.site_plan is not None:
        rs = ReleaseSites(pm, q.sites['sites'], q.site_plan[1], late)
        # the plan's own neighbourhood maps: over the windows whose day is one of its output days
        on_plan = [t for t in nb['windows'] if t[0] in rs.days] if nb else []
        px_plan = [t for t in px['windows'] if t[0] in rs.days] if px else []     # the proximity maps likewise
        fs = begin(ProjectedMaps(None, None, None, None), 'sites', rs,
                   **dict(day_traps, neighbourhood=(on_plan,) if on_plan else None,
                          proximity=(px_plan,) if px_plan else None))
        fs.labels, fs.plan = list(rs.days), rs.describe()
        fs.build(q, chain, nruns)
        if q.cmp_plan is not None:
            rb = ReleaseSites(pm, q.compare['sites'], q.site_plan[1], late)
            fs = begin(_FieldSet(), 'compare', rb, against=rs)
            fs.lagged, fs.plan = late, rb.describe()
            fs.build(q, chain, nruns)
        if getattr(q, 'rk_plan', None) is not None:
            group = _RankedPlans()
            fs = begin(_FieldSet(), 'ranking', group, against=rs)
            plans = q.ranking['plans'] if isinstance(q.ranking, dict) else q.ranking
            for p in plans:
                group.plans.append(ReleaseSites(pm, p['sites'], q.site_plan[1], late))
            fs.lagged, fs.plan = late, [rs.describe()] + group.describe()
            fs.build(q, chain, nruns)


def posterior_predictive(pop_model, chains, burn=0, thin=1, days=None, thresholds=(), locinfo=None,
                         cell_area=None, seed=0, evaluate=None, quantiles=None, bins=DEFAULT_BINS, edges=None,
                         arrival=None, arrival_levels=(0.05, 0.5, 0.95), emergence=None, exposure=None, sites=None,
                         sensitivity=None, compare=None, mc_error=None, peak=None, excursion=None, reweight=None,
                         catch=None, information=None, core_range=None, patches=None, representative=None,
                         neighbourhood=None, modes=None, dependence=None, pathways=None, proximity=None,
                         origin=None, ranking=None, wind=None):
    '''Posterior predictive spread of one or more chains (`Sampler.save` files or (trace, names) pairs). Burn and
    thin apply per chain; consecutive rows with identical model parameters are one evaluation weighted by the
    run's length.

    pop_model: one PopModel or a list -- with several, one host thread per model runs its chains, each chain into
        its own summary, and the summaries are merged in chain order (the result does not depend on the
        interleaving).

    locinfo: observations for the observation-level predictive (every row: the rates of its run's evaluation with
        its own nuisance parameters).

    evaluate(theta) -> expected observations or None: no device, no summary.

    quantiles: levels in (0, 1]; each chain then also fills a SpreadHistogram (bins / edges as bin_edges) with the
        same weights, merged in chain order into `histogram`.

    arrival: thresholds (1..4, finite, > 0, strictly increasing); each chain then also fills ArrivalMaps over the
        summary's days (strictly increasing, at most 32) with the same weights, merged in chain order into
        `arrival`; arrival_levels: the levels of its saved arrival-day quantile maps.

    emergence: dict(collection_day=C, obs_days=None) (emergence_plan); exposure: model days [D1, D2, ...]
        (exposure_plan); each chain then also applies that Projection after every evaluation and adds its outputs,
        with the same weights, to a SpreadSummary.for_projection (same thresholds) and, with quantiles, a
        SpreadHistogram.for_projection (same edges), merged in chain order into `emergence` / `exposure`
        (ProjectedMaps).

    sites: dict(sites=[(east_m, north_m, amount[, lag_days]), ...], days=None) (sites_plan); each chain then also
        builds one ReleaseSites (the models of the later release days, lagged_models, once per model), evaluates
        those models with every member, applies the plan and adds its outputs, with the same weights, to a
        SpreadSummary.for_projection (same thresholds), with quantiles a SpreadHistogram.for_projection (same
        edges) and with arrival an ArrivalMaps.for_projection (same thresholds), merged in chain order into
        `sites` (ProjectedMaps with `plan` and `arrival`).

    sensitivity: True (all 15 model parameters) or names from mcmc.MODEL_BLOCK (check_sens_params); each chain
        then also fills a SensitivityMaps over the summary's days with every run's theta and length, after the
        summary, merged in chain order into `sensitivity`, and every projection and plan asked for gets a
        SensitivityMaps.for_projection of its own, fed after its summary.

    compare: dict(sites=[...]) (contrast_plan), a second release plan B on the output days of sites= (plan A,
        required); each chain then also builds a ReleaseSites for B and one PlanContrast(A, B, thresholds) -- the
        thresholds then have to be finite, > 0 and strictly increasing -- the models of the later release days
        built once per model for the union of both plans' lags and each evaluated once per member; after A's
        applies and adds B is applied and the contrast added with the same weight, merged in chain order into
        `contrast` (`compare_plan`: plan B).

    ranking: dict(plans=[dict(sites=[...]), ...], names=None, levels=(0.05, 0.5, 0.95)) or the bare list of plans
        (ranking_plan; bad arguments fail before any evaluation, directly after compare='s): 1..7 further release
        plans on the output days of sites= (plan A, required, plan 0 of the ranking): which of the named plans does
        best where, and how surely?  Each chain then also builds a ReleaseSites per further plan and one
        PlanRanking([A, ...], thresholds, names) -- the thresholds then have to be finite, > 0, strictly increasing
        and at most 4 -- the models of the later release days built once per model for the union of the lags of
        sites=, compare= and every ranked plan and each evaluated once per member; after A's applies and adds and
        the compare set the further plans are applied and the ranking added with the run's length, merged in
        chain order into `ranking` (`ranking_plans`: every plan, A's first).  It ranks the plans the caller names:
        no plan is searched for, proposed or recommended; pairwise planes for all pairs, per-rank count planes and
        the Monte Carlo error, reweighting or sensitivity of these maps are not computed.  Without ranking=
        nothing is built, called or written.

    mc_error: True (20 batches per chain) or dict(batches=B), B even and >= 4 (mc_batch_plan; not with evaluate=,
        and every chain needs at least B rows after burn and thin); each chain then also fills two MonteCarloError
        sequences beside its summary, same days and thresholds (finite, strictly increasing), the rows before the
        chain's half into the first and the rest into the second, a run that straddles the half split there -- and
        two per projection and plan asked for; at the end every sequence is finished, the split R-hat maps taken
        over all 2 x chains sequences and the sequences merged in chain order into `mc_error` (`mc_error.rhat`:
        the R-hat maps; None with more than 8 chains or a sequence left with fewer than two batches by failed
        members). The contrast gets none.

    peak: thresholds [t_0, ...] (0..4, finite, > 0, strictly increasing) or dict(thresholds=[...], levels=(0.05,
        0.5, 0.95)) (check_peak; not with evaluate=); each chain then also fills a PeakPosterior over the
        summary's days (strictly increasing, at most 32) with the same weights -- per member the PeakMaps add,
        then a SpreadSummary.for_projection of the peak field (the summary's thresholds) and with quantiles a
        SpreadHistogram.for_projection of it (same edges) -- merged in chain order into `peak`; with sites= the
        plan gets a PeakPosterior of its own outputs, fed after the plan's apply (`sites.peak`). Emergence and
        exposure get none here (PeakMaps.for_projection takes them); sensitivity, contrast and Monte Carlo error
        of the peak maps are not computed.

    excursion: thresholds [t_0, ...] (1..4, finite, > 0, strictly increasing) or dict(thresholds=[...],
        levels=(0.9, 0.95)), the levels in (0.5, 1] (check_excursion; not with evaluate=); each chain then also
        fills one ExcursionMaps over the summary's days (strictly increasing, at most 32), reserved to the chain's
        number of runs and fed the same weights after the summary, merged in chain order into `excursion`
        (`excursion_levels`: the levels of its saved regions and areas); with sites= the plan gets an
        ExcursionMaps.for_projection of its own outputs (`sites.excursion`). Emergence and exposure get none here
        (ExcursionMaps.for_projection takes them); sensitivity, contrast, Monte Carlo error and quantiles of the
        excursion maps are not computed.

    reweight: {name: spec, ...} with 1..4 names (check_reweight; not with evaluate=), the maps under new
        observations by importance reweighting of the members, without a new chain. spec = dict(probes=[(east_m,
        north_m, day, kind, rate[, n]), ...]) (check_probes): the member's log-weight is the log-likelihood of the
        probes under its own fields (probes_loglik on one gather of all probes of all scenarios per member); or
        dict(log_weights=[one 1-D array per chain]), one entry per row after burn and thin: a run's log-weight is
        the log of its rows' mean weight (run_log_weight). Bad cells, days, kinds, rates and lengths fail before
        any evaluation. Each chain then also fills one ReweightedSummary over the summary's days (at most 32) and
        thresholds (finite, > 0, strictly increasing), fed right after the summary with the run's length, merged
        in chain order into `reweight`; every emergence=, exposure= and sites= asked for gets a
        ReweightedSummary.for_projection of its own, fed after its summary. reweight['options'] = dict(maps=
        ('quantiles', 'arrival')) (a subset of the two; 'quantiles' needs quantiles=, 'arrival' needs arrival=)
        also reweights the quantile and the arrival maps: each chain then fills a ReweightedHistogram on the edges of
        quantiles= and a ReweightedArrival on the thresholds of arrival=, fed the same log-weights right after the
        ReweightedSummary, merged in chain order into `reweight_histogram` / `reweight_arrival`; the projections get
        a ReweightedHistogram.for_projection, the plan both. 'excursion' among the maps (needs excursion=) keeps
        per member of the excursion maps the run's log-weights and, once the chains are merged, builds
        `reweight_excursion` = {name: ReweightedExcursion} over `excursion` -- and over the plan's, as
        `sites.reweight_excursion` -- from the kept masks, the members in the merged add order; nothing is added to
        the evaluation of a member. 'contrast' among the maps (needs compare=) reweights the paired contrast:
        each chain fills a ReweightedContrast of plan A against plan B on the run's thresholds, fed the run's
        log-weights and length right after the PlanContrast, merged in chain order into `reweight_contrast`; the
        per-member coverage rows stay the PlanContrast's, and save() weights them by the members' log-weights
        (reweighted_coverage_difference). The ranking of ranking= is not reweighted. Without `maps` nothing of
        this is built or called.
        Peak, range, patch, pathway and Monte Carlo error maps and the histograms inside the
        neighbourhood and proximity posteriors get none. `reweight_info` carries per scenario the diagnostics of the row
        weights (reweight_diagnostics); a UserWarning where ess < min_ess (reweight['options'] = dict(min_ess=50))
        -- importance reweighting degrades as the new data disagree with the posterior -- and a ValueError naming
        a scenario that is left without weight. Without reweight= no call is added and `reweight` is None.

    catch: dict(traps=[(day, rate[, n]), ...], levels=(0.5, 0.95), emergence=[(obs_day, rate[, n]), ...])
        (check_catch; not with evaluate=; bad arguments fail before any evaluation), the probability that a trap
        of effort `rate` on model day `day` catches at least n, per cell, under the package's Poisson observation
        model. Each chain then also applies one CatchFields over the traps right after the summary's add and adds
        its fields, with the run's length, to a SpreadSummary.for_projection whose thresholds are the levels; with
        mc_error= to two MonteCarloError.for_projection of its own, with reweight= to a
        ReweightedSummary.for_projection fed the same log-weights; merged in chain order into `catch` (a
        CatchPosterior). The `emergence` key needs emergence= and puts a CatchPosterior over the emergence
        projection's outputs, the trap's day one of its labels, into `emergence.catch`: sentinel fields measure
        emergence, so this is the forward map of the data the chain was fitted to. With sites= the plan gets one
        of its own over the same traps, whose days have to be output days of the plan, in `sites.catch`.
        Histogram, arrival, peak, excursion, sensitivity and contrast of the catch fields are not computed.
        Without catch= no call is added and `catch` is None.

    information: dict(traps=[(day, rate[, ymax]), ...]) (check_information; not with evaluate=; bad arguments fail
        before any evaluation): per described trap -- effort `rate` on model day `day`, its count observed as 0,
        1, .., ymax and ">= ymax + 1" -- and cell the mutual information in nats between the count and the
        identity of the member: where a reading would change the posterior, and where it would tell nothing. Each
        chain then also applies one InformationFields right after the summary's add and adds its planes, with the
        run's length, to a SpreadSummary.for_projection without thresholds; with reweight= to a
        ReweightedSummary.for_projection fed the same log-weights (`information.gain(e, scenario=name)`: after
        that scenario's observations); merged in chain order into `information` (an InformationPosterior). With
        sites= the plan gets one of its own over the same traps, whose days have to be output days of the plan, in
        `sites.information`. A UserWarning where a trap's largest gain exceeds half of `cap`, the entropy of the
        member weights: the map is then bounded by the ensemble, not by the trap. Histogram, arrival, peak,
        excursion, contrast, sensitivity and Monte Carlo error of these maps are not computed. Without
        information= no call is added and `information` is None.

    core_range: mass fractions [p_0, ...] (1..4, each in (0, 1), strictly increasing) or dict(fractions=[...],
        levels=(0.5, 0.9)), the consensus levels in (0, 1] (check_core_range; not with evaluate=; bad arguments
        fail before any evaluation): per member its own highest-density regions, 0.5 the core and 0.95 the range.
        Each chain then also fills one RangeMaps over the summary's days (strictly increasing, at most 32),
        reserved to the chain's number of runs and fed the run's weight right after the summary's add, merged in
        chain order into `core_range` (`core_range_levels`: the consensus levels of its saved regions); with
        sites= the plan gets a RangeMaps.for_projection of its own outputs (`sites.core_range`). Emergence and
        exposure get none here (RangeMaps.for_projection takes them); sensitivity, contrast, Monte Carlo error and
        reweighting of these maps are not computed. Without core_range= no call is added and `core_range` is None.

    patches: thresholds [t_0, ...] (1..4, finite, > 0, strictly increasing) or dict(thresholds=[...],
        connectivity=8, levels=(0.05, 0.5, 0.95)) (check_patches; not with evaluate=; bad arguments fail before any
        evaluation, after every other argument's): per member the connected components of {v >= t_k} under 4-
        (default) or 8-connectivity -- is the reached area one front or separate foci? Each chain then also fills
        one PatchMaps over the summary's days (strictly increasing, at most 32), reserved to the chain's number of
        runs and fed the run's weight last, merged in chain order into `patches` (`patch_levels`: the levels of
        its saved quantiles); with sites= the plan gets a PatchMaps.for_projection of its own outputs
        (`sites.patches`). Emergence and exposure get none here (PatchMaps.for_projection takes them);
        sensitivity, contrast, Monte Carlo error and reweighting of these maps are not computed. The main patch is
        the largest one, not the one at the release point. Without patches= no call is added and `patches` is
        None.

    representative: True or dict(epsilon=0.02, central=0.5, clusters=3, days='all') (check_representative; needs
        excursion=, not with evaluate=; bad arguments fail before any evaluation): which of the members is the most
        typical one, between which outlines the central share of them lies and which scenarios they fall into, on
        their reached sets {v >= t_k} of the excursion maps. Once the chains are merged one RepresentativeMembers
        is built over `excursion` (`representative`; members in the order of `runs`) and, with sites=, one over
        the plan's (`sites.representative`); nothing is added to the evaluation of a member. days: 'all' for the
        space-time set, or the days whose own planes are saved. It compares members the chain produced: no search
        over plans, no zones and no distance curves; depth variants, outlier fences, other distances and the Monte
        Carlo error of these outputs are not computed. Without representative= no call is added and
        `representative` is None.

    neighbourhood: [(day, radius_m), ...] or dict(windows=[...]) (check_neighbourhood; not with evaluate=; bad
        arguments fail before any evaluation): per window and member the largest value within radius_m of each
        cell on model day `day` -- the disc of the cells with dy^2 + dx^2 <= floor((radius_m / cell_m)^2 + 1e-9),
        at most a half-width of 32 cells, clipped to the domain -- and its ensemble statistics (Schwartz & Sobash
        2017): "are there at least t wasps somewhere within r of this point?". Each chain then also applies one
        NeighbourhoodFields over the windows right after the catch's add and adds its fields, with the run's
        length, to a SpreadSummary.for_projection over `thresholds`; with quantile levels to a
        SpreadHistogram.for_projection, with mc_error= to two MonteCarloError.for_projection of its own, with
        reweight= to a ReweightedSummary.for_projection fed the same log-weights; merged in chain order into
        `neighbourhood` (a NeighbourhoodPosterior; `prob(e, k)` is the map). With sites= the plan gets one of its
        own over the windows whose day is an output day of the plan, in `sites.neighbourhood`; emergence and
        exposure get none. Sums or means over the disc, other footprints, and neighbourhood versions of the
        arrival, peak, excursion, range, patch, sensitivity and contrast maps are not computed. Without
        neighbourhood= no call is added and `neighbourhood` is None.

    modes: True or dict(days=[...] | 'all', count=4, transform='sqrt' | 'raw') (check_modes; not with evaluate=; bad
        arguments fail before any evaluation): in what ways do the members differ?  Each chain then also keeps every
        member's transformed day fields on the device (EnsembleModes over the listed days, or over the summary's
        days for 'all'; at most 8), reserved for the chain's runs before its first evaluation -- a ValueError names
        members x days x cells x 8 B where the device has not that much free -- and fed the run's weight last,
        merged in chain order into `modes` (a ModesPosterior: `explained`, `pattern`, `scores`, `drivers`,
        `extremes`, `reconstruct`; members in the order of `runs`).  Listed days get a decomposition each, 'all' the
        space-time one.  With sites= the plan's outputs (at most 8) get one of their own (`sites.modes`), its planes
        the listed days that are output days.  Rotated or sparse modes, modes of the peak, catch or neighbourhood
        fields and the Monte Carlo error or reweighting of the modes are not computed.  Without modes= no call is
        added and `modes` is None.

    dependence: True (all 15 model parameters, 8 bins), names from mcmc.MODEL_BLOCK, or dict(params=..., bins=8,
        days=...) with bins in 2..16 (check_dependence; not with evaluate=; bad arguments fail before any
        evaluation, after every other argument's): on which parameter does a cell depend, linearly or not?  The bin
        edges of every listed parameter are computed once from the pooled runs of all chains after burn and thin
        (dependence_edges: bins of as nearly equal weight as the distinct values allow) and shared by every chain's
        handle.  Each chain then also fills one DependenceMaps over the summary's days (or `days`) with every run's
        theta and length, right after the sensitivity maps, merged in chain order into `dependence`; every
        emergence=, exposure= and sites= asked for gets a DependenceMaps.for_projection of its own.  A handle holds
        ((2 + params x bins + params) x 8 + 1) bytes per cell and day -- 12.7 GB at R = 400, 18 days, 15 parameters
        and 8 bins -- and a ValueError names the figure where the device has not that much free: `days` and a
        shorter parameter list cut it.  First-order ratios only: interaction, total-effect and Shapley indices,
        two-parameter bins, ratios of the peak, catch, neighbourhood or information fields and the Monte Carlo error
        or reweighting of the ratios are not computed.  Without dependence= no call is added and `dependence` is
        None.

    pathways: thresholds [t_0, ...] (1..4, finite, > 0, strictly increasing) or dict(thresholds=[...],
        connectivity=8, days=None, levels=(0.05, 0.5, 0.95)) (check_pathways; not with evaluate=; bad arguments fail
        before any evaluation, after every other argument's): was a cell reached by the advancing front, by a jump,
        or by the growth of a focus a jump founded?  Each chain then also fills one PathwayMaps over the summary's
        days (or `days`; strictly increasing, at most 32) with the centre cell as its anchor, reserved to the
        chain's number of runs and fed the run's weight right after the patch maps, merged in chain order into
        `pathways` (`pathway_levels`: the levels of its saved quantiles); with sites= the plan gets a
        PathwayMaps.for_projection of its own outputs, anchored at its sites (`sites.pathways`).  Emergence and
        exposure get none: their outputs are not a sequence of days.  Jump distances, zones, a lineage beyond the
        three classes, per-day class planes and the Monte Carlo error, reweighting, sensitivity or contrast of
        these maps are not computed.  Without pathways= no call is added and `pathways` is None.

    proximity: [(day, t[, 'to' | 'in']), ...] or dict(windows=[...], radii_m=[...], levels=(...), ladder=[...])
        (check_proximity; not with evaluate=; bad arguments fail before any evaluation): how far from each cell is
        the nearest ground that holds at least t on model day `day`, and how sure is that?  Per window and member
        the exact Euclidean distance in metres from every cell to the member's own set {v >= t} ('in': to its
        complement, the depth inside the reached ground), far_m = sqrt(2 (N - 1)^2 + 1) cell_m where that set is
        empty.  Each chain then also applies one ProximityFields over the windows right after the neighbourhood's
        add and adds its fields, with the run's length, to a SpreadSummary.for_projection over radii_m (at most 3)
        and far_m; with levels to a SpreadHistogram.for_projection on the ladder of radii (default cell_m 2^(j/4)
        up to the first above far_m), with mc_error= to two MonteCarloError.for_projection of its own, with
        reweight= to a ReweightedSummary.for_projection fed the same log-weights; merged in chain order into
        `proximity` (a ProximityPosterior: `mean`, `sd`, `nearer(e, k)`, `beyond`, `empty_share`, `quantile`,
        `radius(e, level)`).  With sites= the plan gets one of its own over the windows whose day is an output day
        of the plan, in `sites.proximity`; emergence and exposure get none.  A radial profile from the release
        point, mean displacement or dispersal-distance curves, distances between named places, zone totals and a
        search are not computed.  Without proximity= no call is added and `proximity` is None.
    origin: a list of findings (east_m, north_m, day, kind, rate[, n]) or dict(findings=[...], amounts=[...],
        lags=[...], hypotheses=None, prior=None, levels=(0.5, 0.95)) (check_origin; not with evaluate=; bad arguments
        fail before any evaluation): from where, when and in what number did the wasps in these findings start?
        One OriginMaps per chain over the model's day records, fed after the summary with the run's length -- the
        models of the later release days are built once per model, as for sites=, and evaluated with the base
        model -- merged in chain order into `origin`: `log_evidence(h)`, `posterior(h)`, `hypotheses()`,
        `region(level)`, `area(level)`, `mode()`, `at`, `log_bayes_factor`, `log_weights()`, `diagnostics()`.
        Inference about the past by exhaustive evaluation: no plan is chosen, nothing is recommended; a spatially
        varying wind or landscape, several sources at once, the rates themselves, a histogram, arrival or Monte
        Carlo error of these maps and a search for where to put a trap are not computed.  With sites= a lagged
        model that the plan shares is evaluated once over the days its longest reader needs; where the findings
        reach further than the plan, the plan's maps can differ in their last bits from a run without origin=.
        Without origin= nothing is built and `origin` is None.

    wind: dict(draws=8, block=3, seed=0, pool=None, sequences=None, share=True, pool_kernels=True) (check_wind; bad
        arguments fail before any evaluation), a weather ensemble: every map above answers "what if we release like
        this?" under the one recorded order of the wind, and this evaluates every run under `draws` orders of it --
        circular moving-block bootstrap draws of the pool's days (wind_sequences), or the `sequences` given, rows of
        day keys of the model's length ("last year's order", a second season added to wind_data).  Per run one
        batch of day kernels is built for the days the sequences use (PopModel.build_pool) and every sequence runs
        its chain over it (run_sequence; pool_kernels=False evaluates the model over days=sequence instead, the A/B
        leg); every set is fed every draw with the run's length, so a member is (run, draw) and the summary's maps
        are those of the joint ensemble.  With share each set also fills a WeatherShare -- one draw per sequence,
        the group closed with the run's length -- merged in chain order into `weather` (and `sites.weather`, ...):
        the variance over the wind at fixed parameters, the parameters' own and the weather's share of their sum.
        A run with a failing day under any sequence is a failed member and is added nowhere.  Not with evaluate=,
        locinfo=, reweight= or origin= (their observations belong to the recorded season), mc_error=,
        representative=, sensitivity= or dependence= (they assume one member per run), nor with a plan that
        releases after day 0 (the models of the later release days carry their own wind).  Resampling 18 or 30
        recorded days says what a reordering and repetition of that season's weather would do; it is no
        climatology and nothing is generated -- a longer wind_data is the remedy.  A day's kernel keeps the record's
        own next day for its last periods, whatever follows it in a sequence.  `wind`: the plan as evaluated.
        Without wind= no call is added, `weather` is None and every saved file is what it was.'''
    q = types.SimpleNamespace(**locals())
    t0 = time.perf_counter()
    _check_request(q)                 # bad arguments fail before any evaluation
    prepared, pms = q.prepared, q.pms
    nch = len(prepared)
    chain_sets = [[] for _ in range(nch)]      # per chain its _FieldSets, in the order a member is fed to them
    late = {}                                  # per model the models of the plans' later release days
    results = [None] * nch
    errs = []
    wind_plan = q.wind_plan
    if wind_plan is not None:                  # the host time of the runs' kernel batches and of their draws
        wind_plan = dict(wind_plan, build_s=[], draw_s=[])

    def work(p):
        try:
            pm = pms[p]
            for ci in range(p, nch, len(pms)):
                rows, rl, mcols, _o, _s = prepared[ci]
                if evaluate is None:
                    if (q.site_plan is not None or q.or_plan is not None) and p not in late:
                        # once per model, for the union of both plans' release days and the origin hypotheses'
                        lags = set(q.site_plan[2] if q.site_plan else ()) | set(q.cmp_plan[2] if q.cmp_plan else ())
                        for ranked in (q.rk_plan['plans'] if q.rk_plan else ()):
                            lags |= set(ranked[2])
                        lags |= set(q.or_plan['model_lags'] if q.or_plan else ())   # the known lags among them
                        late[p] = lagged_models(pm, sorted(lags))
                    draws = len(wind_plan['sequences']) if wind_plan else 1     # a member is (run, draw)
                    _build_sets(chain_sets[ci], q, pm, ci, len(rl) * draws, late.get(p))
                results[ci] = _evaluate_runs(pm, rows, rl, mcols, evaluate, q.want_obs, locinfo, chain_sets[ci],
                                             wind_plan)
        except BaseException as e:       # re-raised in the caller's thread
            errs.append((p, e))

    if evaluate is None and len(pms) > 1 and nch > 1:
        threads = [threading.Thread(target=work, args=(p,), name='predictive-%d' % p)
                   for p in range(min(len(pms), nch))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    else:
        pms = pms[:1]
        work(0)
    if errs:
        for fs in [fs for sets in chain_sets for fs in sets]:
            fs.close()
    else:                                # per source the chains' sets, merged in chain order into the first chain's
        merged = {sets[0]._name: _merge_chains(sets) for sets in zip(*chain_sets)}
    for sets in chain_sets:              # the accumulators hold what they need: the output fields go, and the plans
        for fs in sets:                  # with the models of their later release days
            fs.release()
    for made in late.values():
        for m in made.values():
            m.close()
    if errs:
        raise errs[0][1]
    day = merged.get('days', _FieldSet())
    if q.rp_plan is not None:         # over the merged excursion maps: the members are those of run_rec below
        settings = {n: q.rp_plan[n] for n in ('epsilon', 'central', 'clusters')}
        try:
            for fs in (day, merged.get('sites')):
                if fs is not None and fs.excursion is not None:
                    fs.representative = RepresentativeMembers(fs.excursion, **settings)
        except BaseException:
            for fs in merged.values():
                fs.close()
            raise
    if q.md_plan is not None:         # the members are those of run_rec below
        md_runs = [(ci, first, length) for ci, p in enumerate(prepared)
                   for (first, length), e in zip(p[1], results[ci][0]) if e is not None
                   for _draw in range(len(wind_plan['sequences']) if wind_plan else 1)]
        for fs in (day, merged.get('sites')):
            if fs is not None and fs.modes is not None:
                fs.modes.runs, fs.modes.chains = md_runs, [p[0][:, p[2]] for p in prepared]
    rw_info = None
    if q.rw_plan is not None:
        import warnings
        rw_plan, rw_maps = q.rw_plan, day.reweight
        diag = {}
        for j, name in enumerate(rw_plan['names']):
            d = reweight_diagnostics([v for sets in chain_sets for v in sets[0]._rw_feed.rows[j]])
            d.update({'members': rw_maps.members(name), 'skipped': rw_maps.skipped(name),
                      'log_total_weight': rw_maps.log_total_weight(name)})
            diag[name] = d
        rw_info = {'names': list(rw_plan['names']), 'probes': list(rw_plan['given']), 'min_ess': rw_plan['min_ess'],
                   'diagnostics': diag}
        if rw_plan.get('maps'):
            rw_info['maps'] = list(rw_plan['maps'])
        empty = [n for n in rw_plan['names'] if diag[n]['members'] == 0]
        if empty:
            for fs in merged.values():
                fs.close()
            raise ValueError('reweight: scenario %r is left without weight (W = 0): no member is compatible with it'
                             % empty[0])
        for n in rw_plan['names']:
            if diag[n]['ess'] < rw_plan['min_ess']:
                warnings.warn('reweight: scenario %r has an effective sample size of %.3g rows (min_ess %g): the '
                              'new data disagree with the posterior, the reweighted maps rest on few members'
                              % (n, diag[n]['ess'], rw_plan['min_ess']), UserWarning)
        try:                          # over the merged excursion maps, the members in the merged add order
            for fs in (day, merged.get('sites')):
                if fs is not None and fs._rw_lam is not None:
                    fs.reweight_excursion = {}
                    for j, n in enumerate(rw_plan['names']):
                        fs.reweight_excursion[n] = fs.excursion.reweighted([lam[j] for lam in fs._rw_lam])
        except BaseException:
            for fs in merged.values():
                fs.close()
            raise
    run_rec = [(ci, first, length) for ci, p in enumerate(prepared)
               for (first, length), e in zip(p[1], results[ci][0]) if e is not None]
    observations = None
    if q.want_obs:
        rates = []
        for ci, (rows, rl, mcols, ocols, _s) in enumerate(prepared):
            for (first, length), exp in zip(rl, results[ci][0]):
                if exp is None:
                    continue
                for r in range(first, first + length):
                    v = rows[r, ocols]
                    rates.append(observation_rates(exp, locinfo, v[:3], v[3:]))
        observations = observation_predictive(rates, locinfo, seed)
    prov = [{'source': p[4], 'rows': int(len(p[0])), 'runs': len(p[1]), 'burn': int(burn), 'thin': int(thin)}
            for p in prepared]
    plan_b = merged.get('compare', _FieldSet())
    if plan_b.reweight_contrast is not None:      # per member of `contrast`, in the merged add order
        plan_b.reweight_contrast.member_log_weights = plan_b._rw_lam
    ranked = merged.get('ranking', _FieldSet())
    res = PredictiveResult(
        summary=day.summary, rows=int(sum(len(p[0]) for p in prepared)), evaluations=sum(len(p[1]) for p in prepared),
        failed=sum(r[1] for r in results), seconds=time.perf_counter() - t0, runs=run_rec, observations=observations,
        provenance=prov, days=None if day.summary is None else day.summary.days, histogram=day.histogram,
        quantiles=q.levels, arrival=day.arrival, arrival_levels=q.a_levels if q.a_thr else None,
        emergence=merged.get('emergence'), exposure=merged.get('exposure'), sites=merged.get('sites'),
        sensitivity=day.sensitivity, contrast=plan_b.contrast, compare_plan=plan_b.plan, mc_error=day.mc_error,
        mc_plan={'batches': q.mc_batches, 'batch_weight': q.mc_b, 'sequences': 2 * nch} if q.mc_b else None,
        peak=day.peak, excursion=day.excursion, excursion_levels=q.ex_levels if q.ex_thr else None,
        reweight=day.reweight, reweight_info=rw_info, catch=day.catch, information=day.information,
        core_range=day.core_range, core_range_levels=q.cr_levels if q.cr_frac else None,
        patches=day.patches, patch_levels=q.pt_levels if q.pt_thr else None,
        representative=day.representative, representative_days=q.rp_plan['days'] if q.rp_plan else None,
        representative_chains=[p[0][:, p[2]] for p in prepared] if q.rp_plan else None,
        neighbourhood=day.neighbourhood, modes=day.modes, dependence=day.dependence, pathways=day.pathways,
        pathway_levels=q.pw_levels if q.pw_thr else None, proximity=day.proximity, origin=day.origin,
        reweight_histogram=day.reweight_histogram, reweight_arrival=day.reweight_arrival,
        reweight_excursion=day.reweight_excursion, ranking=ranked.ranking, ranking_plans=ranked.plan,
        ranking_levels=q.rk_plan['levels'] if q.rk_plan else None, weather=day.weather, wind=wind_plan,
        reweight_contrast=plan_b.reweight_contrast)
    if day.information is not None:   # the stated convention: past cap / 2 the ensemble bounds the map
        warn_information(day.information)
        if 'sites' in merged:
            warn_information(merged['sites'].information, 'information (release plan)')
    if cell_area is not None:
        res.cell_area = float(cell_area)
    return res

#!/usr/bin/env python3
"""Posterior predictive spread of saved MCMC chains (parasitoids_amd/predictive.py): per day and
cell the posterior mean population, its spread and exceedance probabilities, accumulated on the
GPU, plus the observation-level predictive of the reference's Poisson model; with --quantiles also
per-cell quantile maps from device histograms on fixed bin edges (--bins); with --arrival also arrival
probability and arrival-day quantile maps and the reached area per day (--arrival-levels); with --emergence /
--exposure also the posterior maps of the projected emergence after a collection on day C (daily, or binned
into the observation days d1,d2,...) and of the cumulative exposure up to the listed model days, saved as
PREFIX_emergence.npz / PREFIX_exposure.npz; with --sites also the posterior maps of a release plan -- several
release sites, some released days later -- saved as PREFIX_sites.npz (with --arrival including its arrival maps
and, in the json, its reached-area curve); with --sensitivity also the posterior sensitivity maps -- per day and
cell the correlation of the population with every listed model parameter (default: all 15), the share of the
posterior variance a linear dependence on them explains and the dominant parameter -- saved as PREFIX_sens.npz
(and PREFIX_NAME_sens.npz for every projection and plan asked for); with --compare-sites (and --sites) also the
paired contrast of the two release plans, member by member -- the posterior mean and spread of A - B, P(A > B),
P(A < B), per threshold where A reaches it and B does not (and the reverse), and the posterior of the difference
of the covered areas -- saved as PREFIX_contrast.npz; with --rank-sites (once per further plan, and --sites) also
the ranking of the named plans, member by member -- per plan P(it alone is best) and its regret against the best,
per threshold where it alone, some plan or every plan reaches it, and the posterior of the covered areas' order
-- saved as PREFIX_ranking.npz; with --peak also the posterior peak maps -- per cell the
highest density within the window, the day of the peak and the number of days at or above each listed density
(--peak-levels: the levels of the peak-day and duration quantile maps) -- saved as PREFIX_peak.npz (and, with
--sites, PREFIX_sites_peak.npz for the plan); with --excursion also the joint excursion sets -- per listed
density and day the region all of which is reached at the same time with a given probability, the region surely
not reached and the credible band of the contour between them (--excursion-levels: the credible levels of the saved
regions and areas, each in (0.5, 1]) -- saved as PREFIX_excur.npz (and, with --sites, PREFIX_sites_excur.npz for the
plan); with --core-range also the core-range maps -- per listed mass fraction and day the probability that a cell lies
in the member's own highest-density region holding that share of its wasps, 0.5 the core and 0.95 the range
(--core-range-levels: the consensus levels of the saved regions' areas, each in (0, 1]) -- saved as PREFIX_range.npz
(and, with --sites, PREFIX_sites_range.npz for the plan); with --patches also the patch maps -- per listed density
and day the probability that a cell lies in the member's main patch (the largest connected component of the cells at
or above the density) or in a satellite, and the posterior of the patch count (--patch-connectivity 4 or 8,
--patch-levels: the levels of the saved quantiles) -- saved as PREFIX_patch.npz (and, with --sites,
PREFIX_sites_patch.npz for the plan); with --pathways also the pathway maps -- per listed density the probability
that a cell was reached by the front that grew from the release, as a founding cell of a detached focus (a jump) or by
the growth of such a focus, and the posterior of the number of foci founded and of the area each pathway took
(--pathway-connectivity 4 or 8, --pathway-levels: the levels of the saved quantiles) -- saved as PREFIX_pathway.npz
(and, with --sites, PREFIX_sites_pathway.npz for the plan, anchored at its sites); with --representative (and --excursion) also the representative members -- on
the members' reached sets at the excursion densities, over all days at once, every member's inclusion depth, the
deepest member, the central band that holds --representative-central of the weight, and K scenarios by k-medoids on
the area two members disagree on, each with its share and its conditional probability map; the run behind the
deepest member and behind every medoid goes into the json -- saved as PREFIX_repr.npz (and, with --sites,
PREFIX_sites_repr.npz for the plan); with --reweight / --reweight-file also the maps under new observations without a new chain -- up to four
named scenarios, each a list of probe observations 'east,north,day,kind,rate[,n]' (kind: count with the number
found n, none, found; rate: the expected number found per wasp in the cell) or a .npy file of one log-weight per
chain row after burn and thin (several chains: concatenated in chain order), by importance reweighting of the
members, with the effective sample size of every scenario in the json -- saved as PREFIX_reweight.npz (and
PREFIX_NAME_reweight.npz for every projection and plan asked for), and with --reweight-maps quantiles,arrival the
reweighted quantile maps of --quantiles and arrival maps of --arrival as PREFIX_reweight_quantiles.npz and
PREFIX_reweight_arrival.npz, and with excursion among them the excursion regions of --excursion under every
scenario, from the members' kept masks, as PREFIX_reweight_excur.npz, and with contrast among them the paired
contrast of --compare-sites under every scenario as PREFIX_reweight_contrast.npz; with --catch also the catch-probability maps --
per trap 'DAY,RATE[,N]' and cell the posterior mean, sd and the probability (--catch-levels) that a trap of effort
RATE on model day DAY catches at least N wasps; --catch-emergence: traps over the emergence days of --emergence --
saved as PREFIX_catch.npz (and PREFIX_emergence_catch.npz, PREFIX_sites_catch.npz); with --neighbourhood also the
neighbourhood maps -- per window 'DAY,RADIUS_M' and cell the posterior mean, sd and, per threshold, the probability
that at least that many wasps stand somewhere within RADIUS_M of the cell on model day DAY -- saved as
PREFIX_nbhd.npz (and PREFIX_sites_nbhd.npz over the windows on the plan's output days); with --proximity also the
proximity maps -- per window 'DAY,T[,in]' and cell the posterior mean and sd of the distance in metres to the nearest
ground that holds at least T wasps on model day DAY ('in': the depth inside it), per --proximity-radii the
probability of such ground within that radius and per --proximity-levels the quantiles -- saved as PREFIX_prox.npz
(and PREFIX_sites_prox.npz over the windows on the plan's output days); with --information also the
information maps -- per described trap 'DAY,RATE[,YMAX]' and cell the mutual information in nats between the trap's
count (observed as 0, 1, .., YMAX and more) and the identity of the member: where a reading would change what we
believe -- saved as PREFIX_information.npz (and PREFIX_sites_information.npz).  Kalbar wind and
LocInfo as scripts/run_mcmc.py loads them; --synthetic uses the synthetic Kalbar-like observations.
Without --chain a short chain is sampled first (--samples) and saved next to --out.

    python scripts/run_predictive.py --chain c.npz [...] [--burn 0] [--thin 1] [--rad-res 400]
        [--mode auto] [--thresholds 1,10] [--out PREFIX] [--synthetic] [--chains-parallel]
        [--quantiles 0.05,0.5,0.95] [--bins 1e-8,1e6,16] [--arrival 1,10] [--arrival-levels 0.05,0.5,0.95]
        [--emergence C[:d1,d2,...]] [--exposure d1,d2,...]
        [--sites 'E,N,AMOUNT[,LAG];...'] [--sites-days d1,d2,...] [--sensitivity [name,name,...]]
        [--dependence [name,name,...]] [--dependence-bins 8]
        [--compare-sites 'E,N,AMOUNT[,LAG];...'] [--rank-sites 'E,N,AMOUNT[,LAG];...' ...] [--rank-names a,b,c]
        [--peak 1,10] [--peak-levels 0.05,0.5,0.95]
        [--excursion 1,10] [--excursion-levels 0.9,0.95]
        [--core-range 0.5,0.95] [--core-range-levels 0.5,0.9]
        [--patches 1,10] [--patch-connectivity 8] [--patch-levels 0.05,0.5,0.95]
        [--pathways 1,10] [--pathway-connectivity 8] [--pathway-levels 0.05,0.5,0.95]
        [--representative [K]] [--representative-epsilon 0.02] [--representative-central 0.5]
        [--reweight 'NAME:east,north,day,kind,rate[,n];...'] [--reweight-file NAME=weights.npy]
        [--reweight-maps quantiles,arrival,contrast,excursion]
        [--catch 'DAY,RATE[,N];...'] [--catch-levels 0.5,0.95] [--catch-emergence 'OBSDAY,RATE[,N];...']
        [--information 'DAY,RATE[,YMAX];...'] [--neighbourhood 'DAY,RADIUS_M;...']
        [--proximity 'DAY,T[,in];...'] [--proximity-radii 100,400,1600] [--proximity-levels 0.05,0.5,0.95]
        [--modes [K]] [--modes-days d1,d2|all] [--modes-transform sqrt|raw]
        [--origin 'EAST,NORTH,DAY,KIND,RATE[,N];...'] [--origin-amounts 0.1,1,10] [--origin-lags 0,2]
        [--origin-levels 0.5,0.95] [--origin-prior file.npy] [--origin-known 'EAST,NORTH,AMOUNT[,LAG];...' | sites]
        [--wind-draws K] [--wind-block 3] [--wind-seed 0] [--wind-pool d1,d2,...] [--wind-plain]

With --wind-draws K a weather ensemble: every run is evaluated under K orders of the wind record, drawn by a circular
moving-block bootstrap (--wind-block days per block, --wind-seed, --wind-pool the days drawn from), over one batch of
day kernels per run (--wind-plain: every sequence as a model of its own, the A/B leg); the maps are those of the joint
ensemble, PREFIX_weather.npz holds per day the variance over the wind, the parameters' own and the weather's share,
and the line gains wind_build_ms_per_run, wind_ms_per_member and weather_ms_per_member.  The observation-level
predictive is left out: the observations belong to the recorded order.

With --origin the origin maps: for findings 'EAST,NORTH,DAY,KIND,RATE[,N]' (metres from the domain centre, model day,
count | none | found, the rate and for a count the number found) the posterior of where, when (--origin-lags) and in
what number (--origin-amounts, multiples of the release number) the population started, saved as PREFIX_origin.npz
with the hypothesis masses, the mode, the areas of the regions at --origin-levels and the diagnostics under
predictive.origin of the json.  With --origin-known the releases that are facts -- 'EAST,NORTH,AMOUNT[,LAG];...', or
the word sites for those of --sites -- lie in the background of every finding: the hypotheses are those of a second
source, PREFIX_origin.npz gains known, null_rows and background_last, and the json a second_source entry (the log
Bayes factor second source : known releases alone).
"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_reweight(ap, probes, files):
    '''the --reweight / --reweight-file flags -> ({name: dict(probes=[...])}, {name: path}); a malformed flag is an
    argument error (the cells, days and rates are checked against the model later)'''
    specs, paths = {}, {}
    for text in probes or []:
        name, sep, body = text.partition(':')
        if not sep or not name.strip() or not body.strip():
            ap.error("--reweight takes 'NAME:east,north,day,kind,rate[,n];...', got %r" % text)
        if name.strip() in specs:
            ap.error('--reweight names scenario %r twice' % name.strip())
        rows = []
        for item in body.split(';'):
            if not item.strip():
                continue
            f = [v.strip() for v in item.split(',')]
            if len(f) not in (5, 6) or f[3] not in ('count', 'none', 'found') or (f[3] == 'count') != (len(f) == 6):
                ap.error("--reweight probe %r: east,north,day,kind,rate[,n] with kind count (and n), none or found"
                         % item)
            try:
                rows.append((float(f[0]), float(f[1]), int(f[2]), f[3], float(f[4])) + ((int(f[5]),) if len(f) == 6 else ()))
            except ValueError:
                ap.error('--reweight probe %r: numbers expected' % item)
        specs[name.strip()] = dict(probes=rows)
    for text in files or []:
        name, sep, path = text.partition('=')
        if not sep or not name.strip() or not path.strip():
            ap.error('--reweight-file takes NAME=weights.npy, got %r' % text)
        if name.strip() in specs or name.strip() in paths:
            ap.error('--reweight-file names scenario %r twice (reweight)' % name.strip())
        paths[name.strip()] = path.strip()
    if len(specs) + len(paths) > 4:
        ap.error('at most 4 --reweight / --reweight-file scenarios')
    return specs, paths


NB_REPS = 5          # timed applies of the neighbourhood handles per member


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chain', nargs='+', default=None)
    ap.add_argument('--burn', type=int, default=0)
    ap.add_argument('--thin', type=int, default=1)
    ap.add_argument('--rad-res', type=int, default=400)
    ap.add_argument('--mode', default='auto', choices=['exact', 'fold', 'fast', 'auto'])
    ap.add_argument('--thresholds', default='1,10')
    ap.add_argument('--out', default='predictive_out/pp')
    ap.add_argument('--synthetic', action='store_true')
    ap.add_argument('--wind-draws', type=int, default=0,
                    help='weather ensemble: every run under K resampled orders of the wind record (default: off)')
    ap.add_argument('--wind-block', type=int, default=3, help='days per block of the moving-block bootstrap')
    ap.add_argument('--wind-seed', type=int, default=0)
    ap.add_argument('--wind-pool', default='', help='day keys d1,d2,... drawn from (default: the whole record)')
    ap.add_argument('--wind-plain', action='store_true',
                    help='evaluate every sequence as a model of its own instead of over one batch of kernels (A/B)')
    ap.add_argument('--chains-parallel', action='store_true',
                    help='one PopModel and host thread per chain (mcmc.run_parallel style)')
    ap.add_argument('--samples', type=int, default=60, help='without --chain: length of the chain sampled first')
    ap.add_argument('--seed', type=int, default=1000)
    ap.add_argument('--quantiles', default='', help='quantile levels in (0, 1], e.g. 0.05,0.5,0.95 (default: off)')
    ap.add_argument('--bins', default='1e-8,1e6,16', help='histogram edges LO,HI,PER_DECADE (with --quantiles)')
    ap.add_argument('--arrival', default='', help='arrival thresholds, e.g. 1,10 (default: off)')
    ap.add_argument('--arrival-levels', default='0.05,0.5,0.95',
                    help='arrival-day quantile levels in (0, 1] (with --arrival)')
    ap.add_argument('--emergence', default='', help='collection day C, or C:d1,d2,... with the observation days '
                                                    '(days post release; default: off)')
    ap.add_argument('--exposure', default='', help='model days d1,d2,... of the cumulative exposure (default: off)')
    ap.add_argument('--sites', default='', help="release plan 'E,N,AMOUNT[,LAG];...': metres east and north of the "
                                                "domain centre, multiples of the release number, days after the "
                                                'first release (default: off)')
    ap.add_argument('--sites-days', default='', help='output model days d1,d2,... of the release plan '
                                                     '(default: all, at most 32)')
    ap.add_argument('--compare-sites', default='', help="a second release plan 'E,N,AMOUNT[,LAG];...' compared with "
                                                        '--sites member by member on its output days (default: off)')
    ap.add_argument('--rank-sites', action='append', default=[],
                    help="a further release plan 'E,N,AMOUNT[,LAG];...' ranked with --sites member by member on its "
                         'output days; may be repeated, one plan per use, at most 7 (default: off)')
    ap.add_argument('--rank-names', default='', help='names a,b,c,... of the ranked plans, that of --sites first '
                                                     '(default: plan0,plan1,...)')
    ap.add_argument('--sensitivity', nargs='?', const='', default=None,
                    help='posterior sensitivity maps to the listed model parameters, e.g. sig_x,sig_y,mu_r '
                         '(no list: all 15; default: off)')
    ap.add_argument('--dependence', nargs='?', const='', default=None,
                    help='posterior dependence maps -- the correlation ratio eta^2 of every cell on each listed model '
                         'parameter, e.g. sig_x,sig_y (no list: all 15; default: off); a handle holds '
                         '((2 + params x bins + params) x 8 + 1) B per cell and day')
    ap.add_argument('--dependence-bins', type=int, default=8, metavar='B',
                    help='bins per parameter of --dependence, 2..16 (default: 8)')
    ap.add_argument('--mc-error', nargs='?', const=20, default=None, type=int, metavar='B',
                    help='Monte Carlo error maps (MCSE, ESS, split R-hat) from B batches per chain, B even and >= 4 '
                         '(no number: 20; default: off)')
    ap.add_argument('--peak', nargs='?', const='', default=None,
                    help='posterior peak maps with the listed duration thresholds, e.g. 1,10 (no list: peak value '
                         'and peak day only; default: off)')
    ap.add_argument('--peak-levels', default='0.05,0.5,0.95',
                    help='levels in (0, 1] of the peak-day and duration quantile maps (with --peak)')
    ap.add_argument('--excursion', default='', help='joint excursion sets at the listed densities, e.g. 1,10 '
                                                    '(default: off)')
    ap.add_argument('--excursion-levels', default='0.9,0.95',
                    help='credible levels in (0.5, 1] of the saved excursion regions and areas (with --excursion)')
    ap.add_argument('--core-range', default='', help='core-range maps at the listed mass fractions in (0, 1), e.g. '
                                                     '0.5,0.95 (default: off)')
    ap.add_argument('--core-range-levels', default='0.5,0.9',
                    help='consensus levels in (0, 1] of the saved core-range areas (with --core-range)')
    ap.add_argument('--patches', default='', help='patch maps at the listed densities, e.g. 1,10 (default: off)')
    ap.add_argument('--patch-connectivity', type=int, default=4, help='4 or 8 neighbours (with --patches)')
    ap.add_argument('--patch-levels', default='0.05,0.5,0.95',
                    help='levels in (0, 1] of the saved patch-count and area quantiles (with --patches)')
    ap.add_argument('--pathways', default='', help='pathway maps at the listed densities, e.g. 1,10 (default: off)')
    ap.add_argument('--pathway-connectivity', type=int, default=4, help='4 or 8 neighbours (with --pathways)')
    ap.add_argument('--pathway-levels', default='0.05,0.5,0.95',
                    help='levels in (0, 1] of the saved foci and area quantiles (with --pathways)')
    ap.add_argument('--representative', nargs='?', const=3, type=int, default=None, metavar='K',
                    help='representative members on the excursion sets: inclusion depth, the deepest member, the '
                         'central band and K scenarios (default 3, 1..8); needs --excursion (default: off)')
    ap.add_argument('--representative-epsilon', type=float, default=0.02,
                    help='share of its own cells a member may have outside another and still count as inside it, a '
                         'multiple of 0.001 in [0, 0.5] (with --representative)')
    ap.add_argument('--representative-central', type=float, default=0.5,
                    help='share of the weight the central band holds, a multiple of 0.001 in (0, 1] (with '
                         '--representative)')
    ap.add_argument('--catch', default='', help="traps 'DAY,RATE[,N];...': per cell the probability that a trap of "
                    'effort RATE on model day DAY catches at least N (default 1) (default: off)')
    ap.add_argument('--catch-levels', default='0.5,0.95', help='levels of the catch maps (with --catch)')
    ap.add_argument('--catch-emergence', default='', help="traps 'OBSDAY,RATE[,N];...' over the emergence days of "
                    '--emergence (with --catch)')
    ap.add_argument('--modes', nargs='?', const=4, type=int, default=None, metavar='K',
                    help='ensemble modes: the K (1..8, default 4) leading weighted principal components of the '
                         "members' transformed day fields, saved as PREFIX_modes.npz")
    ap.add_argument('--modes-days', default='all', help="days 'd1,d2,...' (at most 8) with a decomposition each, or "
                                                        "'all': the space-time decomposition (with --modes)")
    ap.add_argument('--modes-transform', default='sqrt', choices=('sqrt', 'raw'),
                    help='the transform of the fields before the modes are taken (with --modes)')
    ap.add_argument('--neighbourhood', default='', help="windows 'DAY,RADIUS_M;...': per cell the probability of at "
                    'least each of --thresholds somewhere within RADIUS_M of it on model day DAY (default: off)')
    ap.add_argument('--proximity', default='', help="windows 'DAY,T[,in];...': per cell the distance in metres to the "
                    "nearest ground that holds at least T wasps on model day DAY, 'in': the depth inside it "
                    '(default: off)')
    ap.add_argument('--proximity-radii', default='', help='up to 3 radii in metres, increasing: per cell the '
                    'probability of such ground within each (with --proximity)')
    ap.add_argument('--proximity-levels', default='', help='quantile levels of the distance, e.g. 0.05,0.5,0.95 '
                    '(with --proximity)')
    ap.add_argument('--origin', default='', help="findings 'EAST,NORTH,DAY,KIND,RATE[,N];...' (KIND count | none | "
                    'found): the posterior of the origin of the population they come from (default: off)')
    ap.add_argument('--origin-amounts', default='', help='the ladder of founding numbers in multiples of the release '
                    'number, e.g. 0.1,1,10 (with --origin; default 1)')
    ap.add_argument('--origin-lags', default='', help='release days after the first model day, e.g. 0,2 (with '
                    '--origin; default 0)')
    ap.add_argument('--origin-levels', default='', help='posterior mass of the saved regions, e.g. 0.5,0.95 (with '
                    '--origin)')
    ap.add_argument('--origin-prior', default='', help='an N x N .npy log-prior plane, -inf where the origin cannot '
                    'be (with --origin; default flat)')
    ap.add_argument('--origin-known', default='', help="releases that are facts, 'EAST,NORTH,AMOUNT[,LAG];...' or the "
                    'word sites for those of --sites: every finding also catches their wasps, and the hypotheses are '
                    'those of a second source (with --origin; default none)')
    ap.add_argument('--information', default='', help="described traps 'DAY,RATE[,YMAX];...': per cell the mutual "
                    'information in nats between the count of a trap of effort RATE on model day DAY, observed as '
                    '0, 1, .., YMAX (default 0) and more, and the identity of the member (default: off)')
    ap.add_argument('--reweight', action='append', default=None, metavar='NAME:PROBES',
                    help="a reweighting scenario of probe observations 'NAME:east,north,day,kind,rate[,n];...' "
                         '(repeatable; at most 4 scenarios with --reweight-file; default: off)')
    ap.add_argument('--reweight-file', action='append', default=None, metavar='NAME=NPY',
                    help='a reweighting scenario from a .npy of one log-weight per chain row after burn and thin '
                         '(repeatable)')
    ap.add_argument('--reweight-maps', default='', metavar='quantiles,arrival,contrast,excursion',
                    help='with --reweight / --reweight-file: also reweight the quantile maps (needs --quantiles), '
                         'the arrival maps (needs --arrival), the excursion regions (needs --excursion) and the paired '
                         'contrast of two plans (needs --compare-sites), saved as PREFIX_reweight_quantiles.npz / '
                         'PREFIX_reweight_arrival.npz / PREFIX_reweight_excur.npz / PREFIX_reweight_contrast.npz '
                         '(default: off)')
    args = ap.parse_args()
    rw_specs, rw_files = parse_reweight(ap, args.reweight, args.reweight_file)
    rw_maps = [m.strip() for m in args.reweight_maps.split(',') if m.strip()]
    if rw_maps and not (rw_specs or rw_files):
        ap.error('--reweight-maps reweights more maps of a scenario: give --reweight or --reweight-file too')
    if [m for m in rw_maps if m not in ('quantiles', 'arrival', 'contrast', 'excursion')] \
            or len(set(rw_maps)) != len(rw_maps):
        ap.error("--reweight-maps takes a subset of 'quantiles,arrival,contrast,excursion', got %r" % args.reweight_maps)
    for m in rw_maps:
        of = 'compare_sites' if m == 'contrast' else m
        if not (getattr(args, of) or '').strip():
            ap.error('--reweight-maps %s reweights the maps of --%s: give --%s too'
                     % (m, of.replace('_', '-'), of.replace('_', '-')))
    if args.compare_sites and not args.sites:
        ap.error('--compare-sites names plan B and needs plan A: give --sites too')
    if args.rank_sites and not args.sites:
        ap.error('--rank-sites names further plans and needs plan A: give --sites too')
    if args.rank_names and not args.rank_sites:
        ap.error('--rank-names names the plans of --rank-sites: give --rank-sites too')
    warnings.simplefilter('ignore', RuntimeWarning)
    from parasitoids_amd import ParasitoidModel as PM
    from parasitoids_amd import mcmc
    from parasitoids_amd.pop_model import PopModel
    from parasitoids_amd.predictive import (bin_edges, check_arrival_thresholds, check_contrast_thresholds,
                                            check_core_range, check_dependence, check_excursion, check_levels, check_peak,
                                            check_sens_params, contrast_plan,
                                            emergence_plan, exposure_plan, mc_error_plan, posterior_predictive,
                                            sites_plan)
    mc_error = None
    if args.mc_error is not None:        # a bad --mc-error fails before any work
        mc_error = dict(batches=args.mc_error)
        mc_error_plan(mc_error)
    sens = None
    if args.sensitivity is not None:     # bad --sensitivity names fail before any work
        sens = check_sens_params([n.strip() for n in args.sensitivity.split(',') if n.strip()] or None)
    depend = None
    if args.dependence is not None:      # bad --dependence names or bins fail before any work
        depend = check_dependence(dict(params=[n.strip() for n in args.dependence.split(',') if n.strip()] or None,
                                       bins=args.dependence_bins))
    levels = check_levels([float(q) for q in args.quantiles.split(',') if q.strip()])
    bins = tuple(float(b) for b in args.bins.split(','))
    bin_edges(bins)                      # a bad --bins fails before any work
    arrival = [float(t) for t in args.arrival.split(',') if t.strip()]
    a_levels = check_levels([float(q) for q in args.arrival_levels.split(',') if q.strip()])
    if arrival:
        check_arrival_thresholds(arrival)   # as do bad --arrival thresholds
    peak = None
    if args.peak is not None:            # as do bad --peak thresholds or levels
        peak = dict(thresholds=[float(t) for t in args.peak.split(',') if t.strip()],
                    levels=[float(q) for q in args.peak_levels.split(',') if q.strip()])
        check_peak(peak)
    excursion = None
    if args.excursion:                   # as do bad --excursion thresholds or levels
        excursion = dict(thresholds=[float(t) for t in args.excursion.split(',') if t.strip()],
                         levels=[float(q) for q in args.excursion_levels.split(',') if q.strip()])
        check_excursion(excursion)
    core_range = None
    if args.core_range:                  # as do bad --core-range fractions or levels
        core_range = dict(fractions=[float(t) for t in args.core_range.split(',') if t.strip()],
                          levels=[float(q) for q in args.core_range_levels.split(',') if q.strip()])
        check_core_range(core_range)
    representative = None
    if args.representative is not None:  # as do bad --representative settings, or none without --excursion
        from parasitoids_amd.predictive import check_representative
        if not excursion:
            ap.error('--representative needs --excursion')
        representative = check_representative(dict(clusters=args.representative, epsilon=args.representative_epsilon,
                                                   central=args.representative_central))
    patches = None
    if args.patches:                     # as do bad --patches thresholds, connectivity or levels
        from parasitoids_amd.predictive import check_patches
        patches = dict(thresholds=[float(t) for t in args.patches.split(',') if t.strip()],
                       connectivity=args.patch_connectivity,
                       levels=[float(q) for q in args.patch_levels.split(',') if q.strip()])
        check_patches(patches)
    pathways = None
    if args.pathways:                    # as do bad --pathways thresholds, connectivity or levels
        from parasitoids_amd.predictive import check_pathways
        pathways = dict(thresholds=[float(t) for t in args.pathways.split(',') if t.strip()],
                        connectivity=args.pathway_connectivity,
                        levels=[float(q) for q in args.pathway_levels.split(',') if q.strip()])
        check_pathways(pathways)
    emergence = exposure = None
    if args.emergence:
        cday, _, obs = args.emergence.partition(':')
        emergence = dict(collection_day=int(cday), obs_days=[int(d) for d in obs.split(',') if d.strip()] or None)
    if args.exposure:
        exposure = [int(d) for d in args.exposure.split(',') if d.strip()]
    sites = None
    if args.sites:
        sites = dict(sites=[tuple(float(v) if n < 3 else int(v) for n, v in enumerate(site.split(',')))
                            for site in args.sites.split(';') if site.strip()],
                     days=[int(d) for d in args.sites_days.split(',') if d.strip()] or None)
        sites_plan(sites)                # a bad --sites fails before any work; against the model below
    compare = None
    if args.compare_sites:
        compare = dict(sites=[tuple(float(v) if n < 3 else int(v) for n, v in enumerate(site.split(',')))
                              for site in args.compare_sites.split(';') if site.strip()])
        contrast_plan(compare, sites)    # as does a bad --compare-sites
        check_contrast_thresholds([float(t) for t in args.thresholds.split(',') if t.strip()])
    ranking = None
    if args.rank_sites:
        from parasitoids_amd.predictive import ranking_plan
        ranking = dict(plans=[dict(sites=[tuple(float(v) if n < 3 else int(v) for n, v in enumerate(site.split(',')))
                                          for site in plan.split(';') if site.strip()]) for plan in args.rank_sites])
        if args.rank_names:
            ranking['names'] = [n.strip() for n in args.rank_names.split(',')]
        try:
            ranking_plan(ranking, sites)     # as do bad --rank-sites or --rank-names
        except ValueError as e:
            ap.error('--rank-sites: %s' % e)
        check_contrast_thresholds([float(t) for t in args.thresholds.split(',') if t.strip()])
    catch = None
    if args.catch:                       # as do bad --catch traps or levels
        from parasitoids_amd.predictive import check_catch, parse_traps
        catch = dict(traps=parse_traps(args.catch),
                     levels=[float(q) for q in args.catch_levels.split(',') if q.strip()])
        if args.catch_emergence:
            catch['emergence'] = parse_traps(args.catch_emergence)
        check_catch(catch, None, emergence)
    elif args.catch_emergence:
        ap.error('--catch-emergence needs --catch')
    information = None
    if args.information:                 # as do bad --information traps
        from parasitoids_amd.predictive import check_information, parse_traps
        information = dict(traps=parse_traps(args.information))
        check_information(information)
    neighbourhood = None
    if args.neighbourhood:               # as do bad --neighbourhood windows or radii beyond the largest disc
        from parasitoids_amd.predictive import check_neighbourhood, parse_windows
        neighbourhood = parse_windows(args.neighbourhood)
        check_neighbourhood(neighbourhood, None, 10000.0 / args.rad_res)
    proximity = None
    if args.proximity:                   # as do bad --proximity windows, radii or levels
        from parasitoids_amd.predictive import check_proximity, parse_prox_windows
        proximity = dict(windows=parse_prox_windows(args.proximity),
                         radii_m=[float(x) for x in args.proximity_radii.split(',') if x.strip()],
                         levels=[float(x) for x in args.proximity_levels.split(',') if x.strip()] or None)
        check_proximity(proximity, None, 10000.0 / args.rad_res)
    origin = None
    if args.origin:                      # as do bad --origin findings, amounts, lags, levels or prior
        from parasitoids_amd.predictive import origin_request
        try:
            origin = origin_request(args.origin, args.origin_amounts, args.origin_lags, args.origin_levels,
                                    args.origin_prior, 10000.0, args.rad_res, args.origin_known,
                                    sites['sites'] if sites else None)
        except ValueError as e:
            ap.error('--origin: %s' % e)
    elif args.origin_known:
        ap.error('--origin-known needs --origin')
    wd, days = PM.get_wind_data(os.path.join(ROOT, 'parasitoids_amd', 'data', 'kalbar'), 30, '00:00')
    modes = None
    if args.modes is not None:           # as do bad --modes settings
        from parasitoids_amd.predictive import check_modes
        md_days = args.modes_days if args.modes_days == 'all' else [int(d) for d in args.modes_days.split(',') if d.strip()]
        modes = check_modes(dict(count=args.modes, days=md_days, transform=args.modes_transform), len(days))

    def make_pm():
        return PopModel(wd, days, domain_info=(10000.0, args.rad_res), r_number=130000, mode=args.mode)
    plans = ([emergence_plan(emergence, len(days))] if emergence else []) \
        + ([exposure_plan(exposure, len(days))] if exposure else [])     # bad projections fail before any work too
    pm = make_pm()
    if sites:
        if sites['days'] is None:
            sites['days'] = list(range(min(len(days), 32)))
        sites_plan(sites, pm)
        if compare:
            contrast_plan(compare, sites, pm)
        if ranking:
            ranking_plan(ranking, sites, pm)
    if args.synthetic:
        li = mcmc.synthetic_locinfo(pm, args.rad_res, seed=9)
    else:
        from parasitoids_amd.Data_Import import LocInfo
        li = LocInfo('kalbar', (-27.947131, 152.584171), (10000.0, args.rad_res))   # Run.py:129
    cell_area = (10000.0 / args.rad_res) ** 2
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    chains = args.chain
    bayes_rate = None
    if not chains:
        smp = mcmc.Sampler(pm, li, cell_area, seed=args.seed)
        r = smp.run(args.samples)
        bayes_rate = r['evaluations_this_run'] * 3600.0 / r['seconds']
        chains = [args.out + '_chain.npz']
        smp.save(chains[0])
    pms = [pm] + ([make_pm() for _ in chains[1:]] if args.chains_parallel else [])
    thr = [float(t) for t in args.thresholds.split(',') if t.strip()]
    reweight = None
    if rw_specs or rw_files:             # a bad probe fails before any evaluation; a file is split by the chains' rows
        import numpy as np
        from parasitoids_amd.predictive import check_reweight, load_chain as _load
        reweight = dict(rw_specs)
        nrows = [len(_load(c)[0][args.burn::args.thin]) for c in chains]
        for name, path in rw_files.items():
            lw = np.asarray(np.load(path), dtype=np.float64).ravel()
            if lw.size != sum(nrows):
                ap.error('--reweight-file %s: %d log-weights, the chains have %d rows after burn and thin'
                         % (path, lw.size, sum(nrows)))
            reweight[name] = dict(log_weights=np.split(lw, np.cumsum(nrows)[:-1]))
        if rw_maps:
            reweight['options'] = dict(maps=tuple(rw_maps))
        rw_plan = check_reweight(reweight, pm.rad_dist, pm.rad_res, len(days))
    wind = None
    if args.wind_draws:                  # a bad pool or count fails before any evaluation (check_wind)
        wind = dict(draws=args.wind_draws, block=args.wind_block, seed=args.wind_seed,
                    pool=[int(d) for d in args.wind_pool.split(',') if d.strip()] or None,
                    pool_kernels=not args.wind_plain)
    t0 = time.perf_counter()
    res = posterior_predictive(pms if len(pms) > 1 else pm, chains, burn=args.burn, thin=args.thin,
                               thresholds=thr, locinfo=None if wind else li, cell_area=cell_area, seed=args.seed,
                               **({'wind': wind} if wind else {}),
                               quantiles=levels or None, bins=bins, arrival=arrival or None, arrival_levels=a_levels,
                               emergence=emergence, exposure=exposure, sites=sites, sensitivity=sens,
                               compare=compare, mc_error=mc_error, peak=peak, excursion=excursion,
                               **({'reweight': reweight} if reweight else {}),
                               **({'ranking': ranking} if ranking else {}),
                               **({'catch': catch} if catch else {}),
                               **({'information': information} if information else {}),
                               **({'neighbourhood': neighbourhood} if neighbourhood else {}),
                               **({'proximity': proximity} if proximity else {}),
                               **({'origin': origin} if origin else {}),
                               **({'core_range': core_range} if core_range else {}),
                               **({'patches': patches} if patches else {}),
                               **({'pathways': pathways} if pathways else {}),
                               **({'modes': modes} if modes else {}),
                               **({'dependence': depend} if depend else {}),
                               **({'representative': representative} if representative else {}))
    dt = time.perf_counter() - t0
    # accumulate-kernel time: the same members once more with HIP events around every add
    from parasitoids_amd.predictive import (ArrivalMaps, ExcursionMaps, MonteCarloError, PeakMaps, PlanContrast, Projection,
                                            ReleaseSites, SensitivityMaps, SpreadHistogram, SpreadSummary,
                                            lagged_models, load_chain, runs)
    ME = MonteCarloError(pm, res.mc_plan['batch_weight'], None, thr) if mc_error else None
    X = SensitivityMaps(pm, sens) if sens else None
    DM = None
    if depend:                           # the result's own edges: the same planes are written
        from parasitoids_amd.predictive import DependenceMaps
        DM = DependenceMaps(pm, depend['params'], res.dependence.edges)
    RB = XC = SC = None
    union = {}
    RR = []
    XR = None
    if compare or ranking:               # as the driver: one model per release day of any plan, shared by all
        lags = set(sites_plan(sites, pm)[2]) | set(contrast_plan(compare, sites, pm)[2] if compare else ())
        for ranked in (ranking_plan(ranking, sites, pm)['plans'] if ranking else ()):
            lags |= set(ranked[2])
        union = lagged_models(pm, sorted(lags))
        RS = ReleaseSites(pm, sites['sites'], sites['days'], union)
        if compare:
            RB = ReleaseSites(pm, compare['sites'], sites['days'], union)
        if ranking:
            from parasitoids_amd.predictive import PlanRanking
            RR = [ReleaseSites(pm, p['sites'], sites['days'], union) for p in ranking['plans']]
            XR = PlanRanking([RS] + RR, thr, ranking.get('names'))
            XR.profile(True)
    else:
        RS = ReleaseSites.with_lagged_models(pm, sites['sites'], sites['days']) if sites else None
    if compare:                          # and the plan's own summary to set the contrast's add against
        XC = PlanContrast(RS, RB, thr)
        SC = SpreadSummary.for_projection(RS, thr)
        XC.profile(True)
        SC.profile(True)
    XW = []                              # the reweighted contrast: the request's scenarios, then four (the first's log-weights)
    if compare and reweight and 'contrast' in rw_maps:
        from parasitoids_amd.predictive import ReweightedContrast
        XW = [ReweightedContrast(RS, RB, rw_plan['names'], thr)]
        if len(rw_plan['names']) != 4:
            XW.append(ReweightedContrast(RS, RB, ['s0', 's1', 's2', 's3'], thr))
        for h in XW:
            h.profile(True)
    projections = [Projection(pm, W, in_days) for W, in_days, _labels in plans]
    H = SpreadHistogram(pm, None, bins) if levels else None
    A = ArrivalMaps(pm, arrival) if arrival else None
    PK = PeakMaps(pm, peak['thresholds']) if peak else None
    EX = ExcursionMaps(pm, excursion['thresholds']) if excursion else None
    RG = None
    if core_range:
        from parasitoids_amd.predictive import RangeMaps
        RG = RangeMaps(pm, core_range['fractions'])
    RW = RWF = None
    if reweight:
        from parasitoids_amd.predictive import ReweightedSummary, _ReweightFeed
        RW = ReweightedSummary(pm, rw_plan['names'], None, thr)
        RWF = _ReweightFeed(rw_plan, 0)
        RW.profile(True)
    RWM = []                             # the reweighted quantile and arrival maps, fed the same log-weights
    if reweight and rw_maps:
        from parasitoids_amd.predictive import ReweightedArrival, ReweightedHistogram
        if 'quantiles' in rw_maps:
            RWM.append(ReweightedHistogram(pm, rw_plan['names'], None, bins))
        if 'arrival' in rw_maps:
            RWM.append(ReweightedArrival(pm, rw_plan['names'], arrival))
        for m in RWM:
            m.profile(True)
    CF = CP = None
    if catch:                            # and a Projection of as many outputs: the same bytes, a plain streaming pass
        from parasitoids_amd.predictive import CatchFields
        import numpy as np
        CF = CatchFields(pm, catch['traps'])
        Wc = np.zeros((CF.nout, len(CF.in_days)))
        Wc[np.arange(CF.nout), [CF.in_days.index(t[0]) for t in CF.traps]] = 1.0
        CP = Projection(pm, Wc, CF.in_days)
        CF.profile(True)
        CP.profile(True)
    NF = NP = None
    NW = []
    if neighbourhood:                    # and a Projection of as many outputs: the same bytes, a plain streaming pass;
        from parasitoids_amd.predictive import NeighbourhoodFields      # and every window alone: cost against radius
        import numpy as np
        NF = NeighbourhoodFields(pm, neighbourhood)
        Wn = np.zeros((NF.nout, len(NF.in_days)))
        Wn[np.arange(NF.nout), [NF.in_days.index(t[0]) for t in NF.windows]] = 1.0
        NP = Projection(pm, Wn, NF.in_days)
        NW = [NeighbourhoodFields(pm, [t]) for t in NF.windows]
    PF = None
    if proximity:                        # the set and the row pass apart from the column pass
        from parasitoids_amd.predictive import ProximityFields
        PF = ProximityFields(pm, proximity['windows'])
    IF = IC = None
    if information:                      # and a CatchFields of as many planes over the same days: the same bytes
        from parasitoids_amd.predictive import CatchFields, InformationFields
        IF = InformationFields(pm, information['traps'])
        IC = CatchFields(pm, [(t[0], t[1], 1 + k % 16) for e, t in enumerate(IF.traps) for k in range(t[2] + 3)][:32])
        IF.profile(True)
        IC.profile(True)
    WS = None
    if wind:                             # the draw and the close of the variance split, beside the summary's add
        from parasitoids_amd.predictive import WeatherShare
        WS = WeatherShare(pm)
        WS.profile(True)
    with SpreadSummary(pm, None, thr) as S:
        S.profile(True)
        if H is not None:
            H.profile(True)
        if A is not None:
            A.profile(True)
        if PK is not None:
            PK.profile(True)
        if EX is not None:
            EX.reserve(8)
            EX.profile(True)
        if RG is not None:
            RG.reserve(8)
            RG.profile(True)
        if X is not None:
            X.profile(True)
        if DM is not None:
            DM.profile(True)
        if ME is not None:
            ME.profile(True)
        for P in projections:
            P.profile(True)
        if RS is not None:
            RS.profile(True)
        n = 0
        for c in chains[:1]:
            trace, names, _ = load_chain(c)
            cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
            rows, rl = runs(trace, cols, args.burn, args.thin)
            for first, length in rl[:8]:
                try:
                    pm.evaluate(*mcmc.model_args(rows[first, cols]), want_stats=False)
                    if compare or ranking:
                        for lag, m in sorted(union.items()):       # each once per member, not once per plan
                            m.evaluate(*mcmc.model_args(rows[first, cols]), ndays=sites['days'][-1] - lag + 1,
                                       want_stats=False)
                    elif RS is not None:
                        RS.evaluate_lagged(*mcmc.model_args(rows[first, cols]))
                except Exception:
                    continue
                S.add(length)
                if WS is not None:       # groups of two draws: the timing does not depend on what the draws are
                    WS.add()
                    if WS.open_draws == 2:
                        WS.close_group(length)
                if RG is not None:
                    RG.add(length)
                if CF is not None:
                    CF.apply()
                    CP.apply()
                if IF is not None:
                    IF.apply()
                    IC.apply()
                if NF is not None:
                    # the first member warms the kernels up untimed; every later one is timed NB_REPS times, the
                    # handles taking turns
                    for rep in range(NB_REPS if n else 1):
                        for h in [NF, NP] + NW:
                            h.apply()
                    if n == 0:
                        for h in [NF, NP] + NW:
                            h.profile(True)
                if PF is not None:       # the first member warms the kernels up untimed
                    PF.apply()
                    if n == 0:
                        PF.profile(True)
                if RW is not None:
                    lam = RWF.log_weights(pm, first, length)
                    RW.add(lam, length)
                    for m in RWM:
                        m.add(lam, length)
                if ME is not None:
                    ME.add(length)
                if X is not None:
                    X.add(rows[first, cols], length)
                if DM is not None:
                    DM.add(rows[first, cols], length)
                if H is not None:
                    H.add(length)
                if A is not None:
                    A.add(length)
                if PK is not None:
                    PK.add(length)
                if EX is not None:
                    EX.add(length)
                for P in projections:
                    P.apply()
                if RS is not None:
                    RS.apply()
                if XC is not None:
                    RB.apply()
                    SC.add(length)
                    XC.add(length)
                    for h in XW:
                        h.add([lam[j % len(lam)] for j in range(len(h.scenarios))], length)
                if XR is not None:
                    for R in RR:
                        R.apply()
                    XR.add(length)
                n += 1
        ms, launches = S.profile()
    if WS is not None:
        ws_ms, ws_adds, ws_close_ms, ws_closes = WS.profile()
        ws_bytes = WS.nbytes
        WS.close()
    if H is not None:
        h_ms, h_launches = H.profile()[:2]
        H.close()
        res.histogram.profile(True)     # every quantile launch of the saved maps
    if A is not None:
        a_ms, a_launches = A.profile()[:2]
        A.close()
        res.arrival.profile(True)       # every map launch of the save
    if PK is not None:
        pk_ms, pk_launches = PK.profile()[:2]
        pk_bytes = PK.nbytes
        PK.close()
        res.peak.maps.profile(True)     # every map launch of the save
    if EX is not None:
        ex_ms, ex_launches = EX.profile()[:2]
        EX.close()
        res.excursion.profile(True)     # the finalize and every map launch of the save
    if representative:
        res.representative.overlap.profile(True)     # every pair table and subset plane of the save
    if modes:
        from parasitoids_amd.predictive import EnsembleModes
        res.modes.modes.profile(True)                # every table and combine of the save
        with EnsembleModes(pm, res.modes.days, modes['transform']) as MD:    # the add alone: the last member, 5 times
            MD.reserve(5)
            MD.profile(True)
            for _ in range(5):
                MD.add(1)
            md_add_ms, md_adds = MD.profile()[:2]
    if RG is not None:
        rg_ms, rg_launches = RG.profile()[:2]
        RG.close()
        res.core_range.profile(True)    # every map launch of the save
    if CF is not None:
        cf_ms, cf_launches = CF.profile()
        cp_ms, cp_launches = CP.profile()
        cf_bytes = CF.nbytes
        CF.close()
        CP.close()
    if IF is not None:
        if_ms, if_launches = IF.profile()
        ic_ms, ic_launches = IC.profile()
        if_bytes, if_planes = IF.nbytes, IF.nout
        IF.close()
        IC.close()
    if NF is not None:
        nf_ms, nf_launches = NF.profile()
        np_ms, np_launches = NP.profile()
        nw_ms = [h.profile() for h in NW]
        nf_bytes, nf_cells = NF.nbytes, list(NF.cells)
        for h in [NF, NP] + NW:
            h.close()
    if PF is not None:
        pf_row_ms, pf_launches, pf_col_ms, _ = PF.profile()
        pf_bytes, pf_strip = PF.nbytes, PF.strip
        PF.close()
    if RW is not None:
        rw_ms, rw_launches = RW.profile()
        rw_bytes = RW.nbytes
        RW.close()
    rwm_ms = rwm_members = 0
    rwm_detail = {}
    for m in RWM:                        # add and rescale launches of both handles, per member
        add_ms, adds, _q, _n, sc_ms, scs = m.profile()
        rwm_ms += add_ms + sc_ms
        rwm_members = max(rwm_members, adds)
        rwm_detail[m._prefix] = {'add_ms': round(add_ms / max(adds, 1), 4), 'rescales': scs,
                                 'rescale_ms': round(sc_ms / max(scs, 1), 4), 'bytes': m.nbytes}
        m.close()
    if X is not None:
        x_ms, x_launches = X.profile()
        x_bytes = X.nbytes
        X.close()
    if DM is not None:
        dm_ms, dm_launches = DM.profile()
        DM.close()
    if ME is not None:
        me_ms, me_launches, me_close_ms, me_closes = ME.profile()
        me_members, me_bytes = ME.members, ME.nbytes
        ME.close()
    p_ms = sum(P.profile()[0] for P in projections)
    p_launches = sum(P.profile()[1] for P in projections)
    p_bytes = sum(P.nbytes for P in projections)
    for P in projections:
        P.close()
    if RS is not None:
        s_ms, s_launches = RS.profile()
        s_bytes, s_groups, s_nsite = RS.nbytes, len(RS.groups), len(RS.sites)
    if XC is not None:
        c_ms, c_launches = XC.profile()
        cs_ms, cs_launches = SC.profile()
        c_bytes = XC.nbytes
        xw_report = [{'scenarios': len(h.scenarios), 'add_ms_per_member': round(h.profile()[0] / max(h.profile()[1], 1), 4),
                      'launches_timed': h.profile()[1], 'bytes': h.nbytes} for h in XW]
        for h in XW + [XC, SC, RB]:
            h.close()
    if XR is not None:
        r_ms, r_launches = XR.profile()
        r_bytes = XR.nbytes
        for h in [XR] + RR:
            h.close()
    for h in union.values():
        h.close()
    if RS is not None:
        RS.close()
    npz, js = res.save(args.out, {'chains': chains, 'burn': args.burn, 'thin': args.thin, 'rad_res': args.rad_res,
                                  'mode': args.mode, 'synthetic': bool(args.synthetic)})
    ncell = (2 * args.rad_res + 1) ** 2
    nday = len(res.summary.days)
    per = ms / max(launches, 1)
    out = {'metric': 'posterior predictive members/hour (Kalbar wind, %s observations)'
                     % ('synthetic' if args.synthetic else 'Kalbar field'),
           'value': round(3600.0 * res.evaluations / dt, 1), 'unit': 'members/hour',
           'rows': res.rows, 'evaluations': res.evaluations, 'failed': res.failed, 'seconds': round(dt, 3),
           'accumulate_ms_per_member': round(per, 4), 'accumulate_launches_timed': launches,
           'accumulate_GBps': round((8 + 32 + 8 * len(thr)) * ncell * nday / (per * 1e-3) / 1e9, 1) if per > 0 else None,
           'days': nday, 'thresholds': thr, 'chains': len(chains), 'chains_parallel': len(pms) > 1,
           'bayes_evaluations_per_hour': None if bayes_rate is None else round(bayes_rate, 1),
           'outputs': [npz, js]}
    if wind:                             # a member is (run, draw); the builds' host time ends in a synchronise
        w = res.wind
        members = (res.evaluations - res.failed) * len(w['sequences'])
        out['wind_draws'] = len(w['sequences'])
        out['wind_pool_kernels'] = w['pool_kernels']
        out['wind_members'] = members
        out['runs_per_hour'] = out['value']
        out['value'] = out['wind_members_per_hour'] = round(3600.0 * members / dt, 1)
        out['wind_ms_per_member'] = round(1e3 * dt / max(members, 1), 4)
        out['wind_build_ms_per_run'] = round(1e3 * sum(w['build_s']) / max(len(w['build_s']), 1), 4)
        out['weather_ms_per_member'] = round(ws_ms / max(ws_adds, 1), 4)
        out['weather_close_ms_per_run'] = round(ws_close_ms / max(ws_closes, 1), 4)
        out['weather_bytes'] = ws_bytes
        out['outputs'] += ['%s_weather.npz' % args.out]
    if catch:
        out['catch_ms_per_member'] = round(cf_ms / max(cf_launches, 1), 4)
        out['catch_launches_timed'] = cf_launches
        out['catch_outputs'] = len(catch['traps'])
        out['catch_projection_ms_per_member'] = round(cp_ms / max(cp_launches, 1), 4)   # same nout, same bytes
        out['catch_bytes'] = cf_bytes
        out['outputs'] += ['%s_catch.npz' % args.out] \
            + (['%s_emergence_catch.npz' % args.out] if catch.get('emergence') else []) \
            + (['%s_sites_catch.npz' % args.out] if sites else [])
    if neighbourhood:
        out['nbhd_ms_per_member'] = round(nf_ms / max(nf_launches, 1), 4)
        out['nbhd_launches_timed'] = nf_launches
        out['nbhd_windows'] = [list(t) for t in neighbourhood]
        out['nbhd_cells'] = nf_cells
        out['nbhd_projection_ms_per_member'] = round(np_ms / max(np_launches, 1), 4)     # same nout, same bytes
        out['nbhd_window_ms'] = [round(ms_ / max(k_, 1), 4) for ms_, k_ in nw_ms]        # every window alone
        out['nbhd_bytes'] = nf_bytes
        out['outputs'] += ['%s_nbhd.npz' % args.out] \
            + (['%s_sites_nbhd.npz' % args.out] if res.sites is not None and res.sites.neighbourhood is not None else [])
    if proximity:
        out['prox_row_ms_per_member'] = round(pf_row_ms / max(pf_launches, 1), 4)
        out['prox_col_ms_per_member'] = round(pf_col_ms / max(pf_launches, 1), 4)
        out['prox_launches_timed'] = pf_launches
        out['prox_windows'] = [list(t) for t in proximity['windows']]
        out['prox_strip'] = pf_strip
        out['prox_bytes'] = pf_bytes
        out['outputs'] += ['%s_prox.npz' % args.out] \
            + (['%s_sites_prox.npz' % args.out] if res.sites is not None and res.sites.proximity is not None else [])
    if origin:
        out['origin_hypotheses'] = [list(h) for h in res.origin.pairs]
        out['origin_bytes'] = int(res.origin.nbytes)
        out['outputs'] += ['%s_origin.npz' % args.out]
    if information:
        out['information_ms_per_member'] = round(if_ms / max(if_launches, 1), 4)
        out['information_launches_timed'] = if_launches
        out['information_planes'] = if_planes
        out['information_catch_ms_per_member'] = round(ic_ms / max(ic_launches, 1), 4)   # as many catch outputs
        out['information_bytes'] = if_bytes
        out['information_cap'] = res.information.cap
        out['information_max_gain'] = [float(res.information.gain(e).max()) for e in range(len(res.information.traps))]
        out['outputs'] += ['%s_information.npz' % args.out] + (['%s_sites_information.npz' % args.out] if sites else [])
    if reweight:
        out['reweight_ms_per_member'] = round(rw_ms / max(rw_launches, 1), 4)
        out['reweight_launches_timed'] = rw_launches
        out['reweight_scenarios'] = list(res.reweight.scenarios)
        out['reweight_bytes'] = rw_bytes
        if rw_maps:
            out['reweight_maps'] = rw_maps
            out['reweight_maps_ms_per_member'] = round(rwm_ms / max(rwm_members, 1), 4)
            out['reweight_maps_detail'] = rwm_detail
            out['outputs'] += ['%s_reweight_%s.npz' % (args.out, 'excur' if m == 'excursion' else m) for m in rw_maps
                               if m != 'contrast']
        out['reweight_diagnostics'] = res.reweight_info['diagnostics']
        out['outputs'] += ['%s_reweight.npz' % args.out] + ['%s_%s_reweight.npz' % (args.out, n) for n, on in
                                                            (('emergence', emergence), ('exposure', exposure),
                                                             ('sites', sites)) if on]
    if levels:
        out['histogram_add_ms_per_member'] = round(h_ms / max(h_launches, 1), 4)
        out['quantile_ms_total'] = round(res.histogram.profile()[2], 3)
        out['histogram_bytes'] = res.histogram.nbytes
    if arrival:
        out['arrival_add_ms_per_member'] = round(a_ms / max(a_launches, 1), 4)
        out['arrival_maps_ms_total'] = round(res.arrival.profile()[2], 3)
        out['arrival_bytes'] = res.arrival.nbytes
    if peak:
        out['peak_ms_per_member'] = round(pk_ms / max(pk_launches, 1), 4)
        out['peak_launches_timed'] = pk_launches
        out['peak_maps_ms_total'] = round(res.peak.maps.profile()[2], 3)
        out['peak_bytes'] = pk_bytes
        out['outputs'] += ['%s_peak.npz' % args.out] + (['%s_sites_peak.npz' % args.out] if sites else [])
    if excursion:
        ex_prof = res.excursion.profile()
        out['excur_ms_per_member'] = round(ex_ms / max(ex_launches, 1), 4)
        out['excur_launches_timed'] = ex_launches
        out['excur_finalize_ms'] = round(ex_prof[2], 3)          # once, over all res.excursion.members members
        out['excur_members'] = res.excursion.members
        out['excur_maps_ms_total'] = round(ex_prof[4], 3)
        out['excur_map_launches'] = ex_prof[5]
        out['excur_bytes'] = res.excursion.nbytes
        out['outputs'] += ['%s_excur.npz' % args.out] + (['%s_sites_excur.npz' % args.out] if sites else [])
    if core_range:
        out['range_ms_per_member'] = round(rg_ms / max(rg_launches, 1), 4)
        out['range_launches_timed'] = rg_launches
        out['range_fractions'] = core_range['fractions']
        out['range_members'] = res.core_range.members
        out['range_maps_ms_total'] = round(res.core_range.profile()[2], 3)
        out['range_bytes'] = res.core_range.nbytes
        out['outputs'] += ['%s_range.npz' % args.out] + (['%s_sites_range.npz' % args.out] if sites else [])
    if representative:
        rp_prof = res.representative.overlap.profile()
        out['repr_pairs_ms'] = round(rp_prof[0], 3)              # over repr_pairs_calls planes, the save's
        out['repr_pairs_calls'] = rp_prof[1]
        out['repr_subset_ms'] = round(rp_prof[2], 3)
        out['repr_subset_launches'] = rp_prof[3]
        out['repr_members'] = res.excursion.members
        out['repr_bytes'] = res.representative.overlap.nbytes
        out['outputs'] += ['%s_repr.npz' % args.out] + (['%s_sites_repr.npz' % args.out] if sites else [])
    if modes:
        md_prof = res.modes.modes.profile()
        out['modes_table_ms'] = round(md_prof[4] / max(md_prof[5], 1), 3)     # per table call of the save, by HIP events
        out['modes_table_calls'] = md_prof[5]
        out['modes_combine_ms'] = round(md_prof[6] / max(md_prof[7], 1), 3)
        out['modes_add_ms_per_member'] = round(md_add_ms / max(md_adds, 1), 4)
        out['modes_members'] = res.modes.modes.members
        out['modes_bytes'] = res.modes.modes.nbytes
        out['modes'] = modes
        out['outputs'] += ['%s_modes.npz' % args.out] + (['%s_sites_modes.npz' % args.out] if sites else [])
    if patches:
        out['patch_thresholds'] = patches['thresholds']
        out['patch_connectivity'] = patches['connectivity']
        out['patch_members'] = res.patches.members
        out['patch_bytes'] = res.patches.nbytes
        out['outputs'] += ['%s_patch.npz' % args.out] + (['%s_sites_patch.npz' % args.out] if sites else [])
    if pathways:
        out['pathway_thresholds'] = pathways['thresholds']
        out['pathway_connectivity'] = pathways['connectivity']
        out['pathway_members'] = res.pathways.members
        out['pathway_bytes'] = res.pathways.nbytes
        out['outputs'] += ['%s_pathway.npz' % args.out] + (['%s_sites_pathway.npz' % args.out] if sites else [])
    if sens:
        x_per = x_ms / max(x_launches, 1)
        out['sensitivity_add_ms_per_member'] = round(x_per, 4)
        out['sensitivity_launches_timed'] = x_launches
        # nominal: every pair of cells updated; pairs the member does not move skip their co-moments
        out['sensitivity_add_nominal_GBps'] = round((8 + 32 + 16 * len(sens)) * ncell * nday / (x_per * 1e-3) / 1e9, 1) \
            if x_per > 0 else None
        out['sensitivity_bytes'] = x_bytes
        out['sensitivity_params'] = len(sens)
        out['outputs'] += ['%s_sens.npz' % args.out]
    if depend:
        dm_per = dm_ms / max(dm_launches, 1)
        out['dependence_add_ms_per_member'] = round(dm_per, 4)
        out['dependence_launches_timed'] = dm_launches
        # nominal: every pair of cells updated; pairs that are 0 in the member skip their planes
        out['dependence_add_nominal_GBps'] = round((8 + 32 + 16 * len(depend['params'])) * ncell * nday
                                                   / (dm_per * 1e-3) / 1e9, 1) if dm_per > 0 else None
        out['dependence_bytes'] = res.dependence.nbytes
        out['dependence_params'] = len(depend['params'])
        out['dependence_bins'] = res.dependence.nbin
        out['outputs'] += ['%s_depend.npz' % args.out]
    if mc_error:
        # the add launches of one member (one per piece of its weight) and its share of the close launches
        out['mcerr_add_ms_per_member'] = round(me_ms / max(me_members, 1), 4)
        out['mcerr_close_ms_per_member'] = round(me_close_ms / max(me_members, 1), 4)
        out['mcerr_add_launches_timed'] = me_launches
        out['mcerr_close_launches_timed'] = me_closes
        out['mcerr_close_ms_per_launch'] = round(me_close_ms / max(me_closes, 1), 4)
        out['mcerr_bytes'] = me_bytes
        out['mc_error'] = dict(res.mc_plan, used_weight=res.mc_error.used_weight,
                               discarded_weight=res.mc_error.discarded_weight,
                               rhat=res.mc_error.rhat is not None)
        out['outputs'] += ['%s_mcerr.npz' % args.out]
    if projections:
        out['project_ms_per_member'] = round(p_ms / max(n, 1), 4)       # every projection's apply of one member
        out['project_launches_timed'] = p_launches
        out['project_bytes'] = p_bytes                                   # the output fields
        out['outputs'] += ['%s_%s.npz' % (args.out, name) for name, on in (('emergence', emergence),
                                                                             ('exposure', exposure)) if on]
    if sites:
        out['sites_ms_per_member'] = round(s_ms / max(n, 1), 4)        # every group's apply of one member
        out['sites_launches_timed'] = s_launches
        out['sites_bytes'] = s_bytes                                    # the output fields
        out['sites'] = {'sites': s_nsite, 'groups': s_groups, 'days': len(sites['days'])}
        out['outputs'] += ['%s_sites.npz' % args.out]
    if compare:
        out['contrast_add_ms_per_member'] = round(c_ms / max(c_launches, 1), 4)
        out['contrast_launches_timed'] = c_launches
        out['contrast_plan_summary_add_ms_per_member'] = round(cs_ms / max(cs_launches, 1), 4)
        # what every add must move: both plans' fields, 16 B per cell and output
        out['contrast_read_GBps'] = round(16 * ncell * len(sites['days']) / (c_ms / max(c_launches, 1) * 1e-3) / 1e9, 1) \
            if c_ms > 0 else None
        out['contrast_bytes'] = c_bytes
        if xw_report:
            # what every add must move: both plans' fields and one mean per scenario, 16 + 8 J B per cell and output
            out['reweight_contrast_add_ms_per_member'] = xw_report[0]['add_ms_per_member']
            for rec in xw_report:
                ms_add = rec['add_ms_per_member']
                rec['read_GBps'] = round((16 + rec['scenarios'] * 8) * ncell * len(sites['days'])
                                         / (ms_add * 1e-3) / 1e9, 1) if ms_add > 0 else None
            out['reweight_contrast_detail'] = xw_report
            out['outputs'] += ['%s_reweight_contrast.npz' % args.out]
        out['outputs'] += ['%s_contrast.npz' % args.out]
    if ranking:
        out['ranking_add_ms_per_member'] = round(r_ms / max(r_launches, 1), 4)
        out['ranking_launches_timed'] = r_launches
        out['ranking_plans'] = 1 + len(ranking['plans'])
        # what every add must move: every plan's fields, 8 B per plan, cell and output
        out['ranking_read_GBps'] = round(8 * (1 + len(ranking['plans'])) * ncell * len(sites['days'])
                                         / (r_ms / max(r_launches, 1) * 1e-3) / 1e9, 1) if r_ms > 0 else None
        out['ranking_bytes'] = r_bytes
        out['outputs'] += ['%s_ranking.npz' % args.out]
    print(json.dumps(out))
    res.summary.close()
    if res.histogram is not None:
        res.histogram.close()
    if res.arrival is not None:
        res.arrival.close()
    if res.sensitivity is not None:
        res.sensitivity.close()
    if res.dependence is not None:
        res.dependence.close()
    if res.mc_error is not None:
        res.mc_error.close()
    for pr in (res.representative, res.emergence, res.exposure, res.sites, res.contrast, res.ranking, res.peak, res.excursion, res.catch, res.information,
               res.core_range, res.patches, res.pathways, res.neighbourhood, res.modes, res.proximity, res.origin):
        if pr is not None:
            pr.close()
    for p in pms:
        p.close()


if __name__ == '__main__':
    main()

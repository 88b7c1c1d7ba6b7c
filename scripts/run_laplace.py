#!/usr/bin/env python3
"""MAP estimate and normal approximation of the reference's Bayesian model (Bayes_MAP.py --MAP /
--norm; parasitoids_amd/laplace.py), with the delta-method spread maps built on the GPU.  Kalbar wind
and LocInfo as scripts/run_mcmc.py loads them; --synthetic uses the synthetic Kalbar-like observations
(labelled as such).  Prints one JSON line: evaluations, failed points, seconds per stage, the
accumulator's kernel times and, for comparison, the evaluation rate of the single-chain sampler of
the same build in the same process.

    python scripts/run_laplace.py (--MAP | --norm) [--synthetic] [--rad-res 400] [--mode auto]
        [--days 0,5,17] [--thresholds 1,10] [--start-chain c.npz ...] [--maxeval 60] [--out PREFIX]
"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    group = ap.add_mutually_exclusive_group(required=True)
    group.add_argument('--MAP', action='store_true', help='find the maximum a posteriori estimate')
    group.add_argument('--norm', action='store_true', help='MAP, then the normal approximation and its maps')
    ap.add_argument('--synthetic', action='store_true')
    ap.add_argument('--rad-res', type=int, default=400, help='Bayes_MAP.py uses 200')
    ap.add_argument('--mode', default='auto', choices=['exact', 'fold', 'fast', 'auto'])
    ap.add_argument('--days', default='', help='model days of the maps (default all)')
    ap.add_argument('--thresholds', default='1,10')
    ap.add_argument('--start-chain', nargs='+', default=None, help='start at the best row of these chains')
    ap.add_argument('--maxeval', type=int, default=60, help='model evaluations of the MAP search')
    ap.add_argument('--sampler-samples', type=int, default=40, help='sampler iterations timed for comparison')
    ap.add_argument('--out', default='laplace_out/laplace')
    args = ap.parse_args()
    warnings.simplefilter('ignore', RuntimeWarning)
    from parasitoids_amd import ParasitoidModel as PM
    from parasitoids_amd import laplace as LA
    from parasitoids_amd import mcmc
    from parasitoids_amd.pop_model import PopModel
    wd, days = PM.get_wind_data(os.path.join(ROOT, 'parasitoids_amd', 'data', 'kalbar'), 30, '00:00')
    pm = PopModel(wd, days, domain_info=(10000.0, args.rad_res), r_number=130000, mode=args.mode)
    if args.synthetic:
        li = mcmc.synthetic_locinfo(pm, args.rad_res, seed=9)
    else:
        from parasitoids_amd.Data_Import import LocInfo
        li = LocInfo('kalbar', (-27.947131, 152.584171), (10000.0, args.rad_res))   # Run.py:129
    cell_area = (10000.0 / args.rad_res) ** 2
    start = LA.start_from_chain(args.start_chain, li) if args.start_chain else None
    params = {'rad_res': args.rad_res, 'mode': args.mode, 'synthetic': bool(args.synthetic),
              'start_chain': args.start_chain, 'maxeval': args.maxeval}
    r = LA.find_map(pm, li, cell_area, start=start, maxeval=args.maxeval)
    outputs = list(r.save(args.out + '_map', params))
    out = {'metric': 'MAP%s (Kalbar wind, %s observations)' % (' + normal approximation' if args.norm else '',
                                                               'synthetic' if args.synthetic else 'Kalbar field'),
           'rad_res': args.rad_res, 'mode': args.mode,
           'map': {'evaluations': r.evaluations, 'failed': r.failed, 'seconds': round(r.seconds, 3),
                   'logp_start': r.logp_start, 'logp': r.logp, 'lnL': r.lnL, 'AIC': r.AIC, 'k': r.k}}
    if args.norm:
        sel = [int(d) for d in args.days.split(',') if d.strip()] or None
        thr = [float(t) for t in args.thresholds.split(',') if t.strip()]
        res = LA.normal_approx(pm, li, cell_area, at=r, days=sel, thresholds=thr, profile=True)
        prof = res.spread.profile()
        ndays = len(res.spread.days)
        ncell = (2 * args.rad_res + 1) ** 2
        nm = len(LA.FREE_MODEL)
        add_ms = prof['add_ms'] / max(prof['add_launches'], 1)
        fin_ms = prof['finalize_ms'] / max(prof['finalize_launches'], 1)
        add_gb = 24.0 * ncell * ndays / 1e9                                  # record 8 B + J read/write 16 B
        fin_gb = (nm + 1 + 1 + len(thr)) * 8.0 * ncell * ndays / 1e9         # J + centre in, var + exc out
        outputs += res.save(args.out + '_norm', params)
        st = res.seconds['stencil']
        out['norm'] = {'evaluations': res.evaluations, 'failed': res.failed,
                       'seconds': {k: round(v, 3) for k, v in res.seconds.items()},
                       'stencil_evaluations_per_hour': round(3600.0 * res.evaluations / st, 1) if st > 0 else None,
                       'pd': bool(res.pd), 'held': res.held, 'days': ndays, 'thresholds': thr,
                       'profile': prof, 'add_ms': round(add_ms, 4), 'finalize_ms': round(fin_ms, 4),
                       'add_GB': round(add_gb, 3), 'finalize_GB': round(fin_gb, 3),
                       'add_GBps': round(add_gb / (add_ms * 1e-3), 1) if add_ms > 0 else None,
                       'finalize_GBps': round(fin_gb / (fin_ms * 1e-3), 1) if fin_ms > 0 else None}
        res.spread.close()
    if args.sampler_samples > 0:
        smp = mcmc.Sampler(pm, li, cell_area, seed=1000)
        s = smp.run(args.sampler_samples)
        out['sampler_evaluations_per_hour'] = round(s['evaluations_this_run'] * 3600.0 / s['seconds'], 1)
    out['outputs'] = outputs
    print(json.dumps(out))
    pm.close()


if __name__ == '__main__':
    main()

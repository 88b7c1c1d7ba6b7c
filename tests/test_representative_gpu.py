"""GPU tests of the representative members (ps_overlap_*, predictive.MemberOverlap / RepresentativeMembers): the
pair table of every plane against the integer matrix product of the members' bits (overlap_ref), with and without
the live window; member counts around the tile edges of the pair kernel, built by merging; the last real cell of the
last mask word; empty and wide windows; the subset counts; add order; members added later; posterior_predictive with
representative=; and the refusals.  Kalbar wind, the members, weights and helpers of test_arrival_gpu.py: at
R = 128 (N = 257) as at R = 64 (N = 129) the last mask word holds one real cell and 63 pad bits.  Integers
everywhere: every comparison is exact."""
import json
import warnings

import numpy as np
import pytest

import excur_ref
import overlap_ref as R
import test_arrival_gpu as TA

pytestmark = pytest.mark.gpu

MEMBERS, WEIGHTS, THR, THR4 = TA.MEMBERS, TA.WEIGHTS, TA.THR, TA.THR4
_pop_model, _evaluate, _fields = TA._pop_model, TA._evaluate, TA._fields
# four more, between and around the five: nine distinct members
MORE = [((165.0, 145.0, 0.22), 1.05), ((178.0, 150.0, 0.15), 1.2), ((155.0, 142.0, 0.25), 1.3),
        ((190.0, 165.0, 0.05), 0.95)]


def _bits(fields, slot, t):
    """[M, ncell] bool of the members' [nslot, N, N] fields on one slot"""
    return excur_ref.bits(np.asarray(fields)[:, slot], t)


def _popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def _check_tables(E, O, fields, thr):
    """pairs() of every plane, with and without the window, against the reference -> {(k, day): I}"""
    M = E.members
    out = {}
    for k, t in enumerate(thr):
        for s, d in enumerate(E.days):
            I = out[k, d] = R.table(_bits(fields, s, t))
            got = O.pairs(k, d)
            assert got.dtype == np.uint32 and got.shape == (M, M)
            assert np.array_equal(got.astype(np.int64), I), (k, d)
            assert np.array_equal(got, got.T)
            whole = O.pairs(k, d, window=False)
            assert whole.dtype == np.uint32 and np.array_equal(whole, got), (k, d)
    return out


@pytest.mark.parametrize('prob_model', [False, True])
def test_pairs_match_the_matrix_product_of_the_bits(prob_model):
    from parasitoids_amd.predictive import ExcursionMaps, MemberOverlap
    pm = _pop_model(prob_model=prob_model)
    scale = 1.0 / 130000 if prob_model else 1.0
    thr = [t * scale for t in THR]
    fields = []
    with ExcursionMaps(pm, thr) as E, MemberOverlap(E) as O:
        assert O.N == 257 and O.tile >= 1 and O.thresholds == thr and O.days == E.days
        for mem, w in zip(MEMBERS, WEIGHTS):
            _evaluate(pm, mem)
            E.add(w)
            fields.append(_fields(pm, E.days))
        tables = _check_tables(E, O, fields, thr)
        for (k, d), I in tables.items():
            for m in range(5):
                assert I[m, m] == _popcount(E.mask(m, k, d)), (m, k, d)
        assert O._info()[0] == 5 and O.nbytes >= 5 * 5 * 4 + E.pitch * 4
        # not vacuous: at the low threshold the members overlap on the last day, and they are not the same set
        I = tables[0, E.days[-1]]
        assert 0 < I[0, 1] <= min(I[0, 0], I[1, 1]) and len(set(np.diagonal(I).tolist())) == 5
    pm.close()


def test_member_counts_around_the_tile_edges_by_merging():
    from parasitoids_amd.predictive import ExcursionMaps, MemberOverlap, RepresentativeMembers
    pm = _pop_model(R=64)
    days = [1, 4]
    nine = MEMBERS + MORE
    w9 = [1, 3, 1, 2, 1, 2, 1, 1, 4]
    fields = []
    with ExcursionMaps(pm, THR, days) as E9, ExcursionMaps(pm, THR, days) as E5, ExcursionMaps(pm, THR, days) as E2:
        for i, (mem, w) in enumerate(zip(nine, w9)):
            _evaluate(pm, mem)
            for E, n in ((E9, 9), (E5, 5), (E2, 2)):
                if i < n:
                    E.add(w)
            fields.append(_fields(pm, days))
        with MemberOverlap(E9) as O:
            tile = O.tile
        assert tile == 64
        for M, tail in ((tile + 1, E2), (2 * tile + 3, E5)):
            reps, rest = divmod(M, 9)
            assert rest == tail.members
            idx = list(range(9)) * reps + list(range(rest))
            with ExcursionMaps(pm, THR, days) as big:
                for _ in range(reps):
                    big.merge(E9)
                big.merge(tail)
                assert big.members == M
                f = [fields[i] for i in idx]
                w = [w9[i] for i in idx]
                with RepresentativeMembers(big, clusters=2) as rep:
                    tables = _check_tables(big, rep.overlap, f, THR)
                    assert rep.weights.tolist() == w
                    B = {d: _bits(f, s, THR[0]) for s, d in enumerate(days)}
                    R.check_plane(rep, 0, 4, tables[0, 4], {4: B[4]}, w, K=2)
                    R.check_plane(rep, 0, 'all', tables[0, 1] + tables[0, 4], B, w, K=2)
                    assert rep.pairs(0, 'all').dtype == np.int64
    pm.close()


def test_the_last_real_cell_of_the_last_mask_word_counts():
    from parasitoids_amd.predictive import ExcursionMaps, MemberOverlap, ReleaseSites
    Rr, N = 64, 129
    res = 10000.0 / Rr
    pm = _pop_model(R=Rr)
    out = [1, 3]
    sites = [(Rr * res, -Rr * res, 1.0)]             # the release point in the last cell: row N - 1, column N - 1
    fields = []
    with ReleaseSites(pm, sites, out) as S, ExcursionMaps.for_projection(S, THR) as E, MemberOverlap(E) as O:
        assert S.sites[0]['drow'] == Rr and S.sites[0]['dcol'] == Rr
        for mem, w in zip(MEMBERS[:3], WEIGHTS[:3]):
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                S.evaluate(TA.HP, mem[0], TA.DLP, mem[1], TA.NPER)
            E.add(w)
            fields.append(np.array([S.field(e) for e in range(len(out))]))
        tables = _check_tables(E, O, fields, THR)
        B = _bits(fields, 1, THR[0])
        assert B.shape[1] == N * N == 260 * 64 + 1 and B[:, -1].sum() >= 2       # the last cell, in two members or more
        assert not np.array_equal(R.table(B[:, :-1]), tables[0, 3])              # dropping it changes the table
    pm.close()


def test_an_empty_and_a_wide_live_window():
    from parasitoids_amd.predictive import ExcursionMaps, RepresentativeMembers
    pm = _pop_model(R=64)
    thr = [THR4[0], 1e12]                           # a wide window, and a threshold above every field
    days = [0, 5]
    fields = []
    with ExcursionMaps(pm, thr, days) as E, RepresentativeMembers(E) as rep:
        for mem, w in zip(MEMBERS, WEIGHTS):
            _evaluate(pm, mem)
            E.add(w)
            fields.append(_fields(pm, days))
        tables = _check_tables(E, rep.overlap, fields, thr)
        W = sum(WEIGHTS)
        for d in days + ['all']:
            assert not rep.pairs(1, d).any()
            assert rep.depth_counts(1, d)[0].tolist() == [W] * 5 and rep.median(1, d) == 0
            assert np.array_equal(rep.depth(1, d), np.ones(5)) and np.array_equal(rep.jaccard(1, d), np.ones((5, 5)))
        assert np.array_equal(rep.band(1, 5), -np.ones((129, 129), dtype=np.int8))
        B = {d: _bits(fields, s, thr[0]) for s, d in enumerate(days)}
        live = np.flatnonzero(B[5].any(0)) // 64
        assert live[-1] - live[0] + 1 > (129 * 129 // 64 + 1) // 2, 'the window is not wide'
        R.check_plane(rep, 0, 5, tables[0, 5], {5: B[5]}, WEIGHTS)
        R.check_plane(rep, 0, 'all', tables[0, 0] + tables[0, 5], B, WEIGHTS)
    pm.close()


def test_subset_counts():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import ExcursionMaps, MemberOverlap
    pm = _pop_model()
    days = [2, 5]
    fields = []
    rng = np.random.default_rng(5)
    with ExcursionMaps(pm, THR, days) as E, MemberOverlap(E) as O:
        for mem, w in zip(MEMBERS, WEIGHTS):
            _evaluate(pm, mem)
            E.add(w)
            fields.append(_fields(pm, days))
        for k, t in enumerate(THR):
            for s, d in enumerate(days):
                B = _bits(fields, s, t)
                got = O.subset_counts(k, d, WEIGHTS)
                assert got.dtype == np.uint32 and got.shape == (257, 257)
                assert np.array_equal(got, E.counts(k, d)), (k, d)
                assert not O.subset_counts(k, d, [0] * 5).any()
                for _ in range(3):
                    sel = rng.integers(0, 4, 5)
                    want = R.subset_counts(B, sel).reshape(257, 257)
                    assert np.array_equal(O.subset_counts(k, d, sel).astype(np.int64), want), (k, d, sel)
        big = O.subset_counts(0, 5, [0xfffffffe, 0, 0, 0, 0])                # the largest sum there is
        assert np.array_equal(big.astype(np.int64), 0xfffffffe * _bits(fields, 1, THR[0])[0].reshape(257, 257))
        for bad in ([1] * 4, [1] * 6, [0xfffffffe, 1, 0, 0, 0], [-1, 0, 0, 0, 0], [0.5] * 5):
            with pytest.raises(ValueError):
                O.subset_counts(0, 5, bad)
        u32 = np.array([0xfffffffe, 1, 0, 0, 0], dtype=np.uint32)
        out = np.empty((257, 257), dtype=np.uint32)
        import ctypes as C
        p = C.POINTER(C.c_uint32)
        lib = L.load()
        assert lib.ps_overlap_subset(O._h, 0, 1, 5, u32.ctypes.data_as(p), out.ctypes.data_as(p)) == L.PS_ERR_BAD_ARG
        assert lib.ps_overlap_subset(O._h, 0, 1, 4, u32.ctypes.data_as(p), out.ctypes.data_as(p)) == L.PS_ERR_BAD_ARG
        assert lib.ps_overlap_subset(O._h, 0, 1, 5, None, out.ctypes.data_as(p)) == L.PS_OK     # every member, its weight
        assert np.array_equal(out, E.counts(0, 5))
    pm.close()


def test_add_order_permutes_the_table_and_relabels_the_answers():
    from parasitoids_amd.predictive import ExcursionMaps, RepresentativeMembers
    pm = _pop_model(R=64)
    days = [2, 5]
    nine = MEMBERS + MORE
    w9 = [1, 3, 1, 2, 1, 2, 1, 1, 5]
    perm = [4, 0, 8, 2, 6, 1, 7, 3, 5]               # member j of the second handle is member perm[j] of the first
    with ExcursionMaps(pm, THR, days) as A, ExcursionMaps(pm, THR, days) as P, \
            RepresentativeMembers(A, clusters=2) as ra, RepresentativeMembers(P, clusters=2) as rp:
        for mem, w in zip(nine, w9):
            _evaluate(pm, mem)
            A.add(w)
        for j in perm:
            _evaluate(pm, nine[j])
            P.add(w9[j])
        assert rp.weights.tolist() == [w9[j] for j in perm]
        medians = centrals = scenarios = 0
        for k in range(2):
            for d in days + ['all']:
                I = ra.pairs(k, d)
                assert np.array_equal(rp.pairs(k, d), I[perm][:, perm]), (k, d)
                da = ra.depth_counts(k, d)[0]
                assert np.array_equal(rp.depth_counts(k, d)[0], da[perm])
                # equal depths go by index, so the labels decide between them: the median and the central set are
                # compared where no two of the depths that decide them are equal
                top = np.sort(da)[::-1]
                assert da[perm[rp.median(k, d)]] == top[0]
                if top[0] > top[1]:
                    medians += 1
                    assert perm[rp.median(k, d)] == ra.median(k, d)
                ca = ra.central(k, d)
                if len(set(top[:len(ca) + 1].tolist())) == min(len(ca) + 1, 9):
                    centrals += 1
                    assert [perm[j] for j in rp.central(k, d)] == ca
                    assert np.array_equal(rp.band(k, days[1], d), ra.band(k, days[1], d))
                # nested plumes make equal costs common (a weighted median on a line): whatever the labels decide,
                # the cost is the same, and where the medoids are the same members so are the clusters
                sa, sp = ra.scenarios(k, d), rp.scenarios(k, d)
                D = R.distance(I)
                back = [perm[j] for j in sp['medoids']]
                assert R.cost(D, w9, back) == sp['cost'] == sa['cost'] and sp['costs_by_k'] == sa['costs_by_k']
                if sorted(back) == sorted(sa['medoids']) and all(D[i][back[0]] != D[i][back[1]] for i in range(9)):
                    scenarios += 1
                    assert (sorted(sorted(perm[j] for j in g) for g in sp['members'])
                            == sorted(sorted(g) for g in sa['members']))
                    assert sorted(sp['cluster_weight']) == sorted(sa['cluster_weight'])
                    c = [sorted(perm[j] for j in g) for g in sp['members']].index(sa['members'][0])
                    assert np.array_equal(rp.scenario_map(k, days[1], c, d), ra.scenario_map(k, days[1], 0, d))
        assert medians > 0 and centrals > 0 and scenarios > 0, 'equal depths or costs on every plane: nothing compared'
    pm.close()


def test_members_added_later_are_in_the_next_answer():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import ExcursionMaps, RepresentativeMembers
    import ctypes as C
    pm = _pop_model(R=64)
    days = [3]
    fields = []
    with ExcursionMaps(pm, THR, days) as E, RepresentativeMembers(E) as rep:
        for mem, w in zip(MEMBERS[:2], WEIGHTS[:2]):
            _evaluate(pm, mem)
            E.add(w)
            fields.append(_fields(pm, days))
        first = rep.pairs(0, 3)
        assert first.shape == (2, 2) and np.array_equal(first.astype(np.int64), R.table(_bits(fields, 0, THR[0])))
        for mem, w in zip(MEMBERS[2:], WEIGHTS[2:]):            # the masks grow past their first block: they move
            _evaluate(pm, mem)
            E.add(w)
            fields.append(_fields(pm, days))
        tables = _check_tables(E, rep.overlap, fields, THR)
        assert rep.pairs(0, 3).shape == (5, 5) and rep.weights.tolist() == WEIGHTS     # the cache went with the members
        R.check_plane(rep, 0, 3, tables[0, 3], {3: _bits(fields, 0, THR[0])}, WEIGHTS)
        out = np.empty((5, 5), dtype=np.uint32)
        lib = L.load()
        rc = lib.ps_overlap_pairs(rep.overlap._h, 0, 0, 2, 1, out.ctypes.data_as(C.POINTER(C.c_uint32)))
        assert rc == L.PS_ERR_BAD_ARG and b'expected' in lib.ps_last_error()          # a stale member count
    pm.close()


def _csr(f, key, N):
    from scipy import sparse
    return sparse.csr_matrix((f[key + '_data'], f[key + '_ind'], f[key + '_indptr']), shape=(N, N)).toarray()


def test_posterior_predictive_with_representative_members_and_a_release_plan(tmp_path):
    from parasitoids_amd import mcmc
    from parasitoids_amd import predictive as PR
    from test_peak_gpu import _chain
    Rr, N = 64, 129
    res_m = 10000.0 / Rr
    out = [0, 1, 2, 3, 5]
    trace, names = _chain([2, 1, 3, 1, 2])
    chains = [(trace[:5], names), (trace[5:], names)]
    arg = dict(sites=[(0.0, 0.0, 0.6), (13 * res_m, 6 * res_m, 0.5, 2)], days=out)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        one = _pop_model(R=Rr, mode='exact')
        res = PR.posterior_predictive(one, chains, thresholds=[1, 10], excursion=[1, 10], sites=arg,
                                      representative=dict(clusters=2))
        plain = PR.posterior_predictive(one, chains, thresholds=[1, 10], excursion=[1, 10])
    assert plain.representative is None and plain.representative_days is None
    assert res.failed == 0 and len(res.runs) == 6 and res.representative_days == 'all'
    rep, rs = res.representative, res.sites.representative
    assert rep.excursion is res.excursion and rs.excursion is res.sites.excursion
    assert rep.settings == rs.settings == dict(epsilon=0.02, central=0.5, clusters=2)
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    fields, plan_f, weights = [], [], []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        with PR.ReleaseSites.with_lagged_models(one, arg['sites'], out) as P:
            for ci, first, weight in res.runs:
                P.evaluate(*mcmc.model_args(chains[ci][0][first, cols]))
                fields.append(_fields(one, rep.days))
                plan_f.append(np.array([P.field(e) for e in range(len(out))]))
                weights.append(weight)
    assert weights == [2, 1, 2, 1, 1, 2] and rep.weights.tolist() == weights == rs.weights.tolist()
    want = {}
    for name, r, f in (('', rep, fields), ('sites_', rs, plan_f)):
        assert r.days == (list(range(6)) if not name else out)
        for k, t in enumerate([1.0, 10.0]):
            B = {d: _bits(f, s, t) for s, d in enumerate(r.days)}
            I = sum(R.table(b) for b in B.values())
            want[name, k] = R.check_plane(r, k, 'all', I, B, weights, K=2)
            d0 = r.days[2]
            R.check_plane(r, k, d0, R.table(B[d0]), {d0: B[d0]}, weights, K=2)
    npz, js = res.save(str(tmp_path / 'a' / 'pp'))
    plain.save(str(tmp_path / 'p' / 'pp'))
    assert not (tmp_path / 'p' / 'pp_repr.npz').exists()
    meta = json.load(open(js))['predictive']
    for name, r, blk in (('', rep, meta['representative']), ('sites_', rs, meta['sites']['representative'])):
        keys = {'days', 'repr_weights', 'repr_thresholds', 'repr_days'}
        with np.load(str(tmp_path / 'a' / ('pp_%srepr.npz' % name))) as fz:
            assert fz['repr_weights'].tolist() == weights and fz['repr_days'].tolist() == r.days
            for k in range(2):
                ref = want[name, k]
                tag = '%d_all' % k
                assert fz['repr_depth_' + tag].dtype == np.int64 and fz['repr_depth_' + tag].tolist() == ref['depth']
                got = r.depth_counts(k, 'all')
                assert np.array_equal(fz['repr_in_' + tag], got[1]) and np.array_equal(fz['repr_cont_' + tag], got[2])
                assert int(fz['repr_median_' + tag]) == ref['median']
                assert fz['repr_central_' + tag].tolist() == ref['central']
                assert np.array_equal(fz['repr_pairs_' + tag], r.pairs(k, 'all'))
                sc = ref['scenarios']
                assert fz['repr_medoids_' + tag].tolist() == sc['medoids']
                assert fz['repr_assign_' + tag].tolist() == sc['assignment']
                assert fz['repr_cluster_weight_' + tag].tolist() == sc['cluster_weight']
                assert fz['repr_costs_' + tag].tolist() == sc['costs_by_k']
                keys |= {'repr_%s_%s' % (n, tag) for n in ('depth', 'in', 'cont', 'median', 'central', 'pairs',
                                                           'medoids', 'assign', 'cluster_weight', 'costs')}
                for d in r.days:
                    key = '%d_band%d' % (d, k)
                    assert fz[key].dtype == np.int8 and np.array_equal(fz[key], r.band(k, d, 'all')), key
                    keys.add(key)
                    for c in range(2):
                        key = '%d_scen%d_%d' % (d, k, c)
                        m = r.scenario_map(k, d, c, 'all')
                        assert np.array_equal(_csr(fz, key, N), np.where(m >= 1e-8, m, 0.0)), key
                        keys |= {'%s_%s' % (key, t) for t in ('data', 'ind', 'indptr')}
            assert set(fz.files) == keys
        assert blk['epsilon'] == 0.02 and blk['central'] == 0.5 and blk['clusters'] == 2 and blk['days'] == 'all'
        assert blk['members'] == 6 and blk['total_weight'] == 9 and blk['thresholds'] == [1.0, 10.0]
        assert [(p['threshold'], p['plane']) for p in blk['planes']] == [(0, 'all'), (1, 'all')]
        for p in blk['planes']:
            ref = want[name, p['threshold']]
            assert p['median']['member'] == ref['median'] and p['central'] == ref['central']
            assert [m['member'] for m in p['medoids']] == ref['scenarios']['medoids']
            assert p['costs_by_k'] == ref['scenarios']['costs_by_k']
            for who in [p['median']] + p['medoids']:
                ci, first, length = res.runs[who['member']]
                run = who['run']
                assert (run['chain'], run['first_row'], run['length']) == (ci, first, length)
                assert list(run['params']) == [m[0] for m in mcmc.MODEL_BLOCK]
                assert list(run['params'].values()) == chains[ci][0][first, cols].tolist()
    for r in (res, plain):
        if r.representative is not None:
            r.representative.close()
        for acc in (r.summary, r.excursion, r.sites):
            if acc is not None:
                acc.close()
    one.close()


def test_handle_refusals():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import ExcursionMaps, MemberOverlap, RepresentativeMembers, SpreadSummary
    pm = _pop_model(R=64)
    days = [1, 4]
    with ExcursionMaps(pm, THR, days) as E, MemberOverlap(E) as O:
        with pytest.raises(L.HipError) as err:
            O.pairs(0, 1)                                # no member yet
        assert err.value.code == L.PS_ERR_STATE
        with pytest.raises(L.HipError) as err:
            O.subset_counts(0, 1, np.zeros(0, dtype=np.int64))
        assert err.value.code == L.PS_ERR_STATE
        with RepresentativeMembers(E) as rep, pytest.raises(ValueError):
            rep.depth(0, 1)
        _evaluate(pm, MEMBERS[0])
        E.add(2)
        assert O.pairs(0, 1).shape == (1, 1)
        for k, d in ((2, 1), (-1, 1), (0, 2), (0, 0), (0, 'all')):
            with pytest.raises(ValueError):
                O.pairs(k, d)
            with pytest.raises(ValueError):
                O.subset_counts(k, d, [1])
        import ctypes as C
        lib = L.load()
        out = np.empty((1, 1), dtype=np.uint32)
        p = out.ctypes.data_as(C.POINTER(C.c_uint32))
        for k, s in ((2, 0), (0, 2), (-1, 0), (0, -1)):
            assert lib.ps_overlap_pairs(O._h, k, s, 1, 1, p) == L.PS_ERR_BAD_ARG
        h = L._VP()
        assert lib.ps_overlap_create(L.default_device(), 257, E._h, C.byref(h)) == L.PS_ERR_BAD_ARG and not h
        assert O.pairs(1, 4, window=False).shape == (1, 1)       # the handle is still usable
        with SpreadSummary(pm, days) as S, pytest.raises(ValueError):
            MemberOverlap(S)                                     # not excursion maps
        ms0, n0, ms1, n1 = O.profile(True)
        O.pairs(0, 4)
        O.subset_counts(0, 4, [2])
        ms0, n0, ms1, n1 = O.profile()
        assert n0 == 1 and n1 == 1 and ms0 > 0 and ms1 > 0
    closed = ExcursionMaps(pm, THR, days)
    O = MemberOverlap(closed)
    closed.close()
    with pytest.raises(ValueError):
        O.pairs(0, 1)
    with pytest.raises(ValueError):
        O.subset_counts(0, 1, [1])
    with pytest.raises(ValueError):
        MemberOverlap(closed)
    O.close()
    pm.close()

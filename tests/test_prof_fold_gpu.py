"""GPU tests of the two host-side mechanisms every device handle shares (csrc/ps_common.h): the launch profiler
PsProf, which folds finished event pairs into running totals once 256 are pending, and the last-operation event
PsLastOp, which orders a handle's operations across streams.  300 profiled launches -- more than the pending
limit, so a fold happens during the run -- on a handle whose file never folded before (SpreadSummary), on a
two-channel one (SpreadHistogram) and on one that always folded (CatchFields): no launch is lost or counted twice
and the results are those of an unprofiled twin, bit for bit.  Then a chain of fields sources over three streams
without a host synchronisation against the same chain read back after every step.  Kalbar wind, R = 64, 3 days:
an add takes microseconds."""
import math

import numpy as np
import pytest

from test_arrival_gpu import MEMBERS, THR, _pop_model, _evaluate

pytestmark = pytest.mark.gpu

ADDS = 300          # > 256, the pending limit of a channel


@pytest.fixture(scope='module')
def pm():
    """one small model, MEMBERS[0] evaluated"""
    pm = _pop_model(R=64, ndays=3)
    _evaluate(pm, MEMBERS[0])
    yield pm
    pm.close()


def test_a_summary_folds_during_the_adds_and_loses_no_launch(pm):
    from parasitoids_amd.predictive import SpreadSummary
    with SpreadSummary(pm, None, THR) as S, SpreadSummary(pm, None, THR) as T:
        S.profile(True)
        for _ in range(ADDS):
            S.add(1)
            T.add(1)
        ms, n = S.profile()
        assert n == ADDS and math.isfinite(ms) and ms > 0
        assert S.profile() == (ms, n)                              # folded pairs: neither lost nor counted twice
        assert S.profile(False) == (ms, n)
        for _ in range(10):
            S.add(1)
            T.add(1)
        assert S.profile() == (ms, ADDS)                           # off: nothing is timed
        assert T.profile() == (0.0, 0)                             # never on
        assert S.total_weight == T.total_weight == ADDS + 10
        for d in S.days:
            assert np.array_equal(S.mean(d), T.mean(d)) and np.array_equal(S.variance(d), T.variance(d)), d
        assert S.mean(S.days[-1]).max() > 0


def test_a_two_channel_histogram_counts_adds_and_quantile_calls_apart(pm):
    from parasitoids_amd.predictive import SpreadHistogram
    with SpreadHistogram(pm) as H, SpreadHistogram(pm) as G:
        H.profile(True)
        for _ in range(ADDS):
            H.add(1)
            G.add(1)
        calls = [(1, 0.5), (2, 0.5), (2, 0.95)]
        got = [H.quantile(d, p) for d, p in calls]
        add_ms, adds, q_ms, qs = H.profile()
        assert (adds, qs) == (ADDS, len(calls))
        assert math.isfinite(add_ms) and add_ms > 0 and math.isfinite(q_ms) and q_ms > 0
        assert H.profile() == (add_ms, adds, q_ms, qs)
        for (d, p), q in zip(calls, got):
            assert np.array_equal(q, G.quantile(d, p)), (d, p)
        assert got[-1].max() > 0
        assert G.profile() == (0.0, 0, 0.0, 0)


def test_catch_fields_still_count_every_apply(pm):
    from parasitoids_amd.predictive import CatchFields
    with CatchFields(pm, [(1, 1.0), (2, 0.5, 3)]) as CF:
        CF.profile(True)
        for _ in range(ADDS):
            CF.apply()
        ms, n = CF.profile()
        assert n == ADDS == CF.applies and math.isfinite(ms) and ms > 0
        assert CF.profile() == (ms, n)


def test_a_chain_over_three_streams_needs_no_host_synchronisation():
    """projection -> catch fields -> summary: the projection runs on the solver's stream, the other two on their
    own, ordered by the sources' wait and mark alone; the twin chain reads every step back before the next"""
    from parasitoids_amd.predictive import CatchFields, Projection, SpreadSummary
    pm = _pop_model(R=64, ndays=3)
    W = np.array([[1.0, 0.5, 0.0], [0.0, 1.0, 2.0]])
    traps = [(0, 1e-3), (1, 1e-2, 2), (1, 1.0)]
    levels = [0.5, 0.95]

    def chain():
        P = Projection(pm, W, [0, 1, 2])
        CF = CatchFields.for_projection(P, traps)
        return P, CF, SpreadSummary.for_projection(CF, levels)
    PA, CA, SA = chain()
    PB, CB, SB = chain()
    for member, w in zip(MEMBERS[:3], (1, 3, 2)):
        _evaluate(pm, member)
        PA.apply()
        CA.apply()
        SA.add(w)
        PB.apply()
        PB.field(0)
        CB.apply()
        CB.field(0)
        SB.add(w)
        SB.mean(0)
    assert SA.total_weight == SB.total_weight == 6.0
    for e in range(len(traps)):
        assert np.array_equal(CA.field(e), CB.field(e)), e
        assert np.array_equal(SA.mean(e), SB.mean(e)) and np.array_equal(SA.variance(e), SB.variance(e)), e
        for k in range(len(levels)):
            assert np.array_equal(SA.exceedance(e, k), SB.exceedance(e, k)), (e, k)
    assert SA.mean(2).max() > 0 and SA.variance(2).max() > 0      # the members differ: the summary is not trivial
    for h in (SA, SB, CA, CB, PA, PB):
        h.close()
    pm.close()

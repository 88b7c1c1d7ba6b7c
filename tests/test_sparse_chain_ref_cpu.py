"""CPU checks of the exact sparse-chain reference (sparse_chain_ref) that the broadband GPU tests
lean on: it agrees with the FFT oracle (oracle.calcsol.get_solutions) wherever that is affordable,
its inputs fill the spectrum where the Gaussian day kernels of the other GPU tests do not, and the
geometry of every register-resident FFT size does what test_broadband_gpu.py needs of it."""
import numpy as np
import pytest
from scipy import fft as sfft

import sparse_chain_ref as SR
from oracle import calcsol as OC


def _against_oracle(N, state, kernels):
    K = max(k.shape[0] for k in kernels)
    nd = len(kernels)
    ref = [state]
    trace = {}
    OC.get_solutions(ref, [None] + kernels, list(range(nd + 1)), nd + 1, N, np.array([K, K]), trace=trace)
    days = SR.exact_chain(state, kernels, N)
    worst = 0.0
    for d, day in enumerate(days):
        assert day.flag == bool(trace['flags'][d]), d
        raw = np.abs(SR.raw_dense(day, N) - trace['raw'][d]).max()
        assert raw < 1e-15, (d, raw)
        assert ref[d + 1].nnz == day.nnz
        sol = abs(SR.sol_csr(day, N) - ref[d + 1].tocsr()).max()
        assert sol < 1e-15, (d, sol)
        assert abs(float(day.sum + day.delta * day.nnz) - 1.0) < 1e-15
        worst = max(worst, raw, sol)
    return [d.flag for d in days], worst


@pytest.mark.parametrize('N,m', [(101, 20),       # P = 121
                                 (301, 51),       # P = 352
                                 (501, 72),       # P = 573 = 3 x 191: generic torus
                                 (701, 100)])     # P = 801
@pytest.mark.parametrize('kind', ['wide', 'band', 'one_sided'])
@pytest.mark.parametrize('chain', ['clean', 'edge'])
def test_exact_chain_against_oracle(N, m, kind, chain):
    K = 2 * m + 1
    rng = np.random.default_rng([N, m, len(kind), int(chain == 'edge')])
    nd = 2 if chain == 'clean' else 4
    if chain == 'clean':
        state = SR.clean_state(rng, N, N // 2 - nd * m - 2)
    else:
        state = SR.edge_state(rng, N)
    kernels = [SR.sparse_kernel(rng, K, 6, kind) for _ in range(nd)]
    if chain == 'edge' and kind == 'band':
        kernels[0] = SR.sparse_kernel(rng, K, 6, 'wide')    # a band kernel need not push anything over the edge
    flags, worst = _against_oracle(N, state, kernels)
    assert any(flags) == (chain == 'edge')
    print('N=%d K=%d %s %s: max |oracle - exact| = %.2e' % (N, K, kind, chain, worst))


@pytest.mark.parametrize('chain', ['clean', 'edge'])
def test_exact_chain_against_oracle_on_a_register_resident_torus(chain):
    '''The very chains of the GPU test at L = 1008 (six days with all three kernel kinds; three flagged days).'''
    N, K, state, kernels = SR.fast_geometry(1008, chain)
    assert N + K // 2 == 1008
    flags, worst = _against_oracle(N, state, kernels)
    assert any(flags) == (chain == 'edge')
    print('L=1008 %s: max |oracle - exact| = %.2e' % (chain, worst))


def test_sparse_kernels_are_broadband_and_gaussian_kernels_are_not():
    '''Why test_broadband_gpu.py exists: on the 1008 torus an 8-point kernel leaves (almost) no frequency bin
    below 1e-3, the Gaussian day kernel of the bit-identity tests leaves over 90 % of them below 1e-6 -- an
    error confined to those bins cannot move a field value by more than about 1e-6 / L^2.'''
    from parasitoids_amd import synthetic
    P = 1008
    rng = np.random.default_rng(1008)
    k = SR.sparse_kernel(rng, 401, 8, 'wide')
    mag = np.abs(sfft.fft2(OC.wrap_kernel(k, (P, P))))
    share = (mag < 1e-3).mean()
    print('8-point wide kernel: share of bins below 1e-3 = %.2e' % share)
    assert share < 0.01
    _, kernels, _ = synthetic.make_stack(R=400, K=401, ndays=1, seed=7, sigma=(6.0, 12.0), shift=10)
    mag = np.abs(sfft.fft2(OC.wrap_kernel(kernels[0], (P, P))))
    share = (mag < 1e-6).mean()
    print('Gaussian kernel, sigma 6..12: share of bins below 1e-6 = %.3f' % share)
    assert share > 0.90


def test_size_list_matches_the_header():
    sizes = SR.rs_sizes()
    assert sizes == sorted(set(sizes)) and sizes[0] == 1008 and 5184 in sizes and 10000 in sizes


@pytest.mark.parametrize('L', SR.rs_sizes(), ids=str)
def test_geometry_of_every_register_resident_size(L):
    '''What test_broadband_gpu.py takes for granted, per size: N odd, the fast torus is the reference torus,
    the clean chains raise no flag, the edge chains raise at least one, and every nonzero of every reference
    field is >= 1e-6 (asserted inside exact_chain).'''
    for chain in ('clean', 'edge'):
        N, K, state, kernels = SR.fast_geometry(L, chain)
        assert N % 2 == 1 and K % 2 == 1 and N + K // 2 == L
        assert len(kernels) == (6 if chain == 'clean' else 3)
        days = SR.exact_chain(state, kernels, N)
        flags = [d.flag for d in days]
        assert any(flags) == (chain == 'edge'), flags
        assert all(d.nnz == len(d.vals) and d.nnz > 0 for d in days)
    m = SR.fold_m(L)
    for N in (L - 3 * m, L - 3 * m - 40):         # both ends of the size search of the fold test
        assert N % 2 == 1
        for chain in ('clean', 'edge'):
            K, state, kernels = SR.fold_geometry(L, N, chain)
            assert N + 3 * (K // 2) <= L
            days = SR.exact_chain(state, kernels, N)
            assert any(d.flag for d in days) == (chain == 'edge')


@pytest.mark.parametrize('N,K,nd,direct', SR.AWKWARD_CASES, ids=lambda v: str(v))
def test_geometry_of_the_awkward_pads(N, K, nd, direct):
    state, chains = SR.awkward_geometry(N, K, nd)
    assert N % 2 == 1 and sorted(chains) == ['band', 'wide']
    for kind, kernels in chains.items():
        days = SR.exact_chain(state, kernels, N)       # asserts the >= 1e-6 condition
        assert len(days) == nd and (days[0].flag or kind != 'wide')


def test_geometry_of_the_auto_mode_chains():
    """'edge' flags every day, 'late' has a clean prefix of two days; both against the oracle as well."""
    for start, want in (('edge', [True] * 4), ('late', [False, False, True, True])):
        state, kernels = SR.auto_geometry(start)
        flags, _ = _against_oracle(SR.AUTO_N, state, kernels)
        assert flags == want

"""Scoring checkpoints at their fixed points on the GPU (ssnode.sample_tuning_curves_table, csrc/ssn_fpsample.hip, analyzers/distdiff.py
with dynamics='fixed-point'): the fp64 W table against ssn_build_w_f64, the verdict and select kernels against a numpy restatement
of the rule, the batched sampler against the existing per-draw device path (bit for bit) and against the CPU oracle, its
independence of the grouping into rounds and launches, the scorer and the command line.

The shapes are the smallest that cover the cases: N = 13 (2N = 26), four stimuli, 40 candidates, NZ = 12, five parameter sets
(`ssnode.DEFAULT_PARAMS` times SCALES) of which three come up short and two fill with rejections in front of their last row (all
code 2, asym_power), plus one asym_tanh set whose max_iter sits in a wide gap of the step counts (two rejections, code 1).
`oracle_case` establishes exactly that on the CPU oracle before anything is compared."""
import collections
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ssn_numpy as on
from tc_gan_amd import clib, ssnode
from tc_gan_amd.analyzers import distdiff
from tc_gan_amd.clib import libssnode
from test_distdiff import ks_numerators

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, M = 13, 26
BANDWIDTHS = [0, .125, .5, 1]
CONTRAST = [20.0]
SMOOTHNESS = .25 / 8
CANDIDATES, NZ = 40, 12
SITES = [6, 2]
SCALES = [dict(J=1), dict(J=3), dict(J=4, S=2), dict(J=6, S=2), dict(J=.5)]
THETAS = [{k: ssnode.DEFAULT_PARAMS[k] * sc.get(k, 1) for k in 'JDS'} for sc in SCALES]
POWER = dict(io_type='asym_power', dt=5e-4, rate_stop_at=200, max_iter=20000)
TANH = dict(io_type='asym_tanh', max_iter=2100)
TANH_NZ = 30
STIM = dict(N=N, bandwidths=BANDWIDTHS, smoothness=SMOOTHNESS, contrast=CONTRAST)
PROBES = dict(sample_sites=SITES, include_inhibitory_neurons=True)


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype).contiguous()


def _oracle_candidates(theta, solver):
    """Every one of the 40 candidates on the CPU oracle: (verdict, largest step count, states (NB, 2N))."""
    exts = on.stimulus_input(BANDWIDTHS, np.linspace(-.5, .5, N), SMOOTHNESS, CONTRAST, [0.])
    rs = np.random.RandomState(0)
    out = []
    for _ in range(CANDIDATES):
        z = rs.rand(1, M, M)[0]
        W = on.generate_weight(N, theta['J'], theta['D'], theta['S'], z)
        sols = [on.fixed_point(W, e, r0=np.zeros(M), k=.01, n=2.2, **solver) for e in exts]
        failed = [s.error for s in sols[::-1] if s.error]
        out.append((failed[0] if failed else 0, max(s.steps for s in sols), np.array([s.x for s in sols])))
    return out


def _expected(cands, nz):
    """accepted, used, rejections (2,), draw_index (nz,), states of the accepted candidates, from every candidate's verdict."""
    ok = [i for i, c in enumerate(cands) if c[0] == 0][:nz]
    used = ok[-1] + 1 if len(ok) == nz else len(cands)
    front = [c[0] for c in cands[:used]]
    return dict(accepted=len(ok), used=used, rejections=[front.count(1), front.count(2)],
                draw_index=ok + [-1] * (nz - len(ok)), x=np.array([cands[i][2] for i in ok]))


@pytest.fixture(scope='module')
def oracle_case():
    """The expected outcome per set from the CPU oracle, after checking that the inputs still make the cases."""
    power = [_oracle_candidates(th, POWER) for th in THETAS]
    free = _oracle_candidates(THETAS[0], dict(TANH, max_iter=20000))
    steps = np.sort([c[1] for c in free])
    below, above = steps[steps <= TANH['max_iter']].max(), steps[steps > TANH['max_iter']].min()
    assert all(c[0] == 0 for c in free) and (steps > TANH['max_iter']).sum() == 2
    assert TANH['max_iter'] - below >= 200 and above - TANH['max_iter'] >= 200          # no candidate near the limit
    tanh = _oracle_candidates(THETAS[0], TANH)
    exp = [_expected(c, NZ) for c in power]
    exp_tanh = _expected(tanh, TANH_NZ)
    assert [sum(c[0] == 0 for c in cs) for cs in power] == [7, 10, 22, 27, 7]
    assert [e['accepted'] for e in exp] == [7, 10, 12, 12, 7]                           # short sets and full sets
    assert [e['used'] for e in exp] == [40, 40, 19, 16, 40]
    assert all(e['rejections'][1] > 0 for e in exp[2:4])                                 # rejections in front of the last row
    assert all(e['rejections'][0] == 0 for e in exp) and exp_tanh['rejections'] == [2, 0]   # both codes occur
    assert exp_tanh['accepted'] == TANH_NZ and exp_tanh['used'] == TANH_NZ + 2
    return collections.namedtuple('Case', 'power tanh')(exp, exp_tanh)


# ---- 1. the W table in fp64 ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_sites,sets,draws', [(13, 5, 7), (5, 3, 5), (12, 2, 3)])
def test_w_table_f64_has_the_bits_of_build_w_f64(n_sites, sets, draws):
    m = 2 * n_sites                                             # 26 and 10: no multiples of 4 (scalar path); 24: vectors of 4
    rs = np.random.RandomState(n_sites)
    thetas = [{k: ssnode.DEFAULT_PARAMS[k] * (1 + 0.3 * (rs.rand(2, 2) - 0.5)) for k in 'JDS'} for _ in range(sets)]
    table = ssnode._theta_table(thetas)
    z = _dev(rs.rand(draws, m, m), torch.float64)
    W = torch.full((sets, draws, m, m), float('nan'), device='cuda', dtype=torch.float64)
    dtable = _dev(table, torch.float64)
    clib.check(libssnode.ssn_build_w_table_f64(z.data_ptr(), dtable.data_ptr(), W.data_ptr(), sets, draws,
                                               n_sites, clib.stream_ptr()), 'ssn_build_w_table_f64')
    dp = clib.double_ptr
    for s, th in enumerate(thetas):
        want = torch.full((draws, m, m), float('nan'), device='cuda', dtype=torch.float64)
        J, D, S = (np.ascontiguousarray(th[k], dtype='float64').reshape(4) for k in 'JDS')
        clib.check(libssnode.ssn_build_w_f64(z.data_ptr(), J.ctypes.data_as(dp), D.ctypes.data_as(dp), S.ctypes.data_as(dp),
                                             want.data_ptr(), draws, n_sites, clib.stream_ptr()), 'ssn_build_w_f64')
        got, want = W[s].cpu().numpy(), want.cpu().numpy()
        assert np.isfinite(want).all()
        np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64), err_msg='set {}'.format(s))


# ---- 2. the verdict and select kernels alone ----------------------------------------------------------------------------

def _select_reference(codes, x, set_of, cand0, nz, probes, state):
    """The rule restated: updates `state` (out, accepted, used, rejections, draw_index) in place, returns the verdicts."""
    A, R, NB = codes.shape
    verdict = np.zeros((A, R), dtype=np.int64)
    for a in range(A):
        for b in range(R):
            for s in reversed(range(NB)):
                code = codes[a, b, s] if codes[a, b, s] != 0 else (0 if np.isfinite(x[a, b, s]).all() else 1)
                if code:
                    verdict[a, b] = code
                    break
    out, accepted, used, rejections, draw_index = state
    for a in range(A):
        row = set_of[a]
        if accepted[row] >= nz:
            continue
        used[row] = cand0 + R
        for b in range(R):
            if verdict[a, b] == 0:
                out[row, accepted[row]] = x[a, b][:, probes].reshape(-1)
                draw_index[row, accepted[row]] = cand0 + b
                accepted[row] += 1
                if accepted[row] == nz:
                    used[row] = cand0 + b + 1
                    break
            elif verdict[a, b] in (1, 2):
                rejections[row, verdict[a, b] - 1] += 1
    return verdict


def _planted(rs, A, R, NB, m, dtype, p_fail):
    """codes and states with planted failures: codes 1 and 2, NaN / +inf / -inf in states whose code is 0, several failing
    stimuli per candidate."""
    codes = np.where(rs.rand(A, R, NB) < p_fail, rs.randint(1, 3, (A, R, NB)), 0).astype(np.int32)
    x = rs.rand(A, R, NB, m).astype(dtype) * 50
    bad = np.array([np.nan, np.inf, -np.inf])
    for a, b, s in zip(*np.nonzero(rs.rand(A, R, NB) < p_fail)):
        x[a, b, s, rs.randint(m)] = bad[rs.randint(3)]
    return codes, x


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('R', [1, 63, 64, 65, 257, 300])
def test_select_kernel_equals_the_rule(R, dtype):
    rs = np.random.RandomState(R)
    nz, NB, m, rows = 7, 5, 6, 9
    tdtype = torch.float64 if dtype == 'float64' else torch.float32
    probes = np.array([4, 0, 5], dtype=np.int32)
    set_of = np.array([7, 0, 3, 8, 5, 2], dtype=np.int32)                       # rows 1, 4, 6 belong to no set of the round
    A, C = len(set_of), NB * len(probes)
    p_fail = 0.05 if R > 8 else 0.0
    state = [np.full((rows, nz, C), np.nan, dtype=dtype), np.zeros(rows, np.int32), np.zeros(rows, np.int32),
             np.zeros((rows, 2), np.int32), np.full((rows, nz), -1, np.int32)]
    state[1][3] = nz                                                             # a set complete before the round
    state[2][3], state[3][3], state[4][3] = 11, [2, 1], np.arange(nz) + 1
    dstate = [_dev(s, tdtype if i == 0 else torch.int32) for i, s in enumerate(state)]
    fn = libssnode.ssn_fp_select_f64 if dtype == 'float64' else libssnode.ssn_fp_select_f32
    cand0 = 0
    seen_order = False
    for call in range(2):                                                        # `have` carried over two calls
        codes, x = _planted(rs, A, R, NB, m, dtype, p_fail)
        codes[1], x[1, :, NB - 1, 2] = 2, np.nan                                 # a set with no success at all
        if R > 8:
            codes[0, 1] = [0, 2, 0, 1, 0]                                        # reversed order: stimulus 3 (code 1) comes first
            codes[0, 2], x[0, 2, 4, 0], x[0, 2, 2, 1] = [2, 0, 0, 0, 0], np.inf, -np.inf      # a non-finite state comes first: 1
            codes[3, 0] = 0                                                      # success at the very first candidate
            x[3, 0] = np.abs(np.nan_to_num(x[3, 0], nan=1.0, posinf=1.0, neginf=1.0))
        want_v = _select_reference(codes, x, set_of, cand0, nz, probes, state)
        if R > 8:
            assert want_v[0, 1] == 1 and want_v[0, 2] == 1 and want_v[3, 0] == 0 and (want_v[1] == 2).all()
            seen_order = True
        verdict = torch.full((A, R), -9, device='cuda', dtype=torch.int32)
        dc, dx = _dev(codes, torch.int32), _dev(x, tdtype)
        dp, ds = _dev(probes, torch.int32), _dev(set_of, torch.int32)            # (held: a temporary's memory would be reused)
        rc = fn(dc.data_ptr(), dx.data_ptr(), A, R, NB, m, dp.data_ptr(), len(probes), ds.data_ptr(), cand0, nz, verdict.data_ptr(), *[t.data_ptr() for t in dstate],
                clib.stream_ptr())
        clib.check(rc, 'ssn_fp_select')
        np.testing.assert_array_equal(verdict.cpu().numpy(), want_v)
        for name, got, want in zip(('out', 'accepted', 'used', 'rejections', 'draw_index'), dstate, state):
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg='{} after call {}'.format(name, call))
        cand0 += R
    assert seen_order or R <= 8
    assert state[1][0] == 0 and state[1][3] == nz and state[2][3] == 11          # no success at all; the complete set untouched
    if R >= 257:
        assert (state[1][[7, 3, 8, 5, 2]] == nz).all() and (state[2][[7, 8, 5, 2]] < 2 * R).all()
    assert (state[1] + state[3].sum(axis=1) == state[2])[[7, 0, 8, 5, 2]].all()


def test_select_kernel_sweeps_states_that_are_not_16_byte_aligned():
    """fp32 at an offset of one element: the scalar form of the verdict pass."""
    rs = np.random.RandomState(5)
    A, R, NB, m, nz = 2, 70, 3, 6, 5
    codes, x = _planted(rs, A, R, NB, m, 'float32', 0.08)
    probes, set_of = np.array([1], np.int32), np.array([1, 0], np.int32)
    state = [np.full((2, nz, NB), np.nan, 'float32'), np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros((2, 2), np.int32),
             np.full((2, nz), -1, np.int32)]
    want_v = _select_reference(codes, x, set_of, 3, nz, probes, state)
    buf = torch.zeros(x.size + 1, device='cuda', dtype=torch.float32)
    dx = buf[1:]
    dx.copy_(_dev(x, torch.float32).reshape(-1))
    assert dx.data_ptr() % 16 == 4
    dstate = [_dev(np.full((2, nz, NB), np.nan, 'float32'), torch.float32), *[torch.zeros(s, device='cuda', dtype=torch.int32) for s in (2, 2, (2, 2))],
              torch.full((2, nz), -1, device='cuda', dtype=torch.int32)]
    verdict = torch.empty((A, R), device='cuda', dtype=torch.int32)
    dc, dp, ds = _dev(codes, torch.int32), _dev(probes, torch.int32), _dev(set_of, torch.int32)
    clib.check(libssnode.ssn_fp_select_f32(dc.data_ptr(), dx.data_ptr(), A, R, NB, m, dp.data_ptr(), 1, ds.data_ptr(), 3, nz,
                                           verdict.data_ptr(), *[t.data_ptr() for t in dstate], clib.stream_ptr()), 'ssn_fp_select_f32')
    np.testing.assert_array_equal(verdict.cpu().numpy(), want_v)
    for got, want in zip(dstate, state):
        np.testing.assert_array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize('R', [1, 7, 65])
def test_verdict_pass_reads_the_last_partial_vector_by_element(R):
    """fp32, one set, one stimulus of 6 values, odd R: 6 R = 2 (mod 4) values in all, so the aligned sweep ends in half a vector
    (and every second candidate starts in the middle of one).  The planted values sit in the array's last two elements."""
    rs = np.random.RandomState(R)
    NB, m, nz = 1, 6, 3
    assert (R * NB * m) % 4 == 2
    for plant in (None, -1, -2):
        codes = np.zeros((1, R, NB), np.int32)
        x = (rs.rand(1, R, NB, m) * 50).astype('float32')
        if plant is not None:
            x.reshape(-1)[plant] = [np.nan, np.inf][plant]
        probes, set_of = np.array([5, 4], np.int32), np.array([0], np.int32)
        state = [np.full((1, nz, 2), np.nan, 'float32'), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros((1, 2), np.int32),
                 np.full((1, nz), -1, np.int32)]
        dstate = [_dev(s, torch.float32 if i == 0 else torch.int32) for i, s in enumerate(state)]
        want_v = _select_reference(codes, x, set_of, 0, nz, probes, state)
        assert want_v[0, R - 1] == (0 if plant is None else 1)
        dc, dx, dp, ds = _dev(codes, torch.int32), _dev(x, torch.float32), _dev(probes, torch.int32), _dev(set_of, torch.int32)
        assert dx.data_ptr() % 16 == 0 and dx.numel() == R * m          # exactly the values: nothing behind them belongs to x
        verdict = torch.full((1, R), -9, device='cuda', dtype=torch.int32)
        clib.check(libssnode.ssn_fp_select_f32(dc.data_ptr(), dx.data_ptr(), 1, R, NB, m, dp.data_ptr(), 2, ds.data_ptr(), 0, nz,
                                               verdict.data_ptr(), *[t.data_ptr() for t in dstate], clib.stream_ptr()), 'ssn_fp_select_f32')
        np.testing.assert_array_equal(verdict.cpu().numpy(), want_v)
        for got, want in zip(dstate, state):
            np.testing.assert_array_equal(got.cpu().numpy(), want)


# ---- 3. against the existing device path, bit for bit -------------------------------------------------------------------

def _table(dtype, solver=POWER, thetas=THETAS, nz=NZ, **kw):
    return ssnode.sample_tuning_curves_table(thetas, NZ=nz, seed=0, dtype=dtype, max_candidates=CANDIDATES,
                                             **dict(dict(STIM, **PROBES), **dict(solver, **kw)))


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('variant', [0, 2])
def test_table_equals_the_per_draw_device_path(oracle_case, dtype, variant):
    from tc_gan_amd.gradient_expressions.utils import subsample_neurons
    from tc_gan_amd.networks.ssn import device_rand
    tdtype = torch.float64 if dtype == 'float64' else torch.float32
    tab = _table(dtype, variant=variant)
    assert tab.variant == variant and tab.candidates == CANDIDATES
    z = device_rand(np.random.RandomState(0), (CANDIDATES, M, M), tdtype)
    W = torch.empty((len(THETAS), CANDIDATES, M, M), device='cuda', dtype=tdtype)
    build = libssnode.ssn_build_w_table_f64 if dtype == 'float64' else libssnode.ssn_build_w_table_f32
    dtable = _dev(ssnode._theta_table(THETAS), tdtype)
    clib.check(build(z.data_ptr(), dtable.data_ptr(), W.data_ptr(), len(THETAS), CANDIDATES, N,
                     clib.stream_ptr()), 'ssn_build_w_table')
    zh, Wh = z.cpu().numpy(), W.cpu().numpy()
    exts = ssnode._stimulus_rows(N, BANDWIDTHS, SMOOTHNESS, CONTRAST)
    full = 0
    for s in range(len(THETAS)):
        zs, xs, info = ssnode.find_fixed_points_batched(NZ, zip(zh, Wh[s]), exts, dtype=dtype, variant=variant, k=.01, n=2.2, **POWER)
        got = len(zs)
        assert tab.accepted[s] == got
        want = subsample_neurons(np.asarray(xs), SITES, track_offset_identity=True, include_inhibitory_neurons=True)
        np.testing.assert_array_equal(tab.tunings[s, :got], want)
        assert np.isnan(tab.tunings[s, got:]).all()
        where = [int(np.nonzero((zh == zi).all(axis=(1, 2)))[0][0]) for zi in zs]
        np.testing.assert_array_equal(tab.draw_index[s], where + [-1] * (NZ - got))
        assert list(tab.rejections[s]) == [info.counter[1], info.counter[2]]
        assert tab.accepted[s] + tab.rejections[s].sum() == tab.used[s]
        if got == NZ:
            assert tab.used[s] == NZ + info.rejections
            full += 1
        else:
            assert tab.used[s] == CANDIDATES
    assert 0 < full < len(THETAS)
    if dtype == 'float64':                                   # (fp32 may judge a borderline candidate differently: not asserted)
        assert [int(a) for a in tab.accepted] == [e['accepted'] for e in oracle_case.power]


# ---- 4. against the CPU oracle ------------------------------------------------------------------------------------------

def _check_against(tab, s, exp):
    assert tab.accepted[s] == exp['accepted'] and tab.used[s] == exp['used']
    assert list(tab.rejections[s]) == exp['rejections'] and list(tab.draw_index[s]) == exp['draw_index']
    want = on.subsample_neurons(exp['x'], SITES, track_offset_identity=True, include_inhibitory_neurons=True)
    got = tab.tunings[s, :exp['accepted']]
    with np.errstate(invalid='ignore', divide='ignore'):
        rel = np.where(want == got, 0.0, np.abs(got - want) / np.abs(want))
    print('set {}: largest relative difference to the oracle {:.3g}'.format(s, rel.max()))
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=0)
    assert np.isnan(tab.tunings[s, exp['accepted']:]).all()


def test_table_equals_the_cpu_oracle(oracle_case):
    tab = _table('float64')
    assert tab.tunings.shape == (5, NZ, 4 * 4) and tab.tunings.dtype == np.float64 and tab.candidates == CANDIDATES
    assert tab.variant == libssnode.ssn_solver_fast_path(M, 4, 8)
    for s, exp in enumerate(oracle_case.power):
        _check_against(tab, s, exp)
    # the oracle's own sampler for the sets that fill (it draws until NZ rows are found)
    for s in (2, 3):
        zs, xs, counter = on.sample_fixed_points(NZ=NZ, seed=0, N=N, bandwidths=BANDWIDTHS, smoothness=SMOOTHNESS, contrast=CONTRAST,
                                                 **dict(THETAS[s], **POWER))
        np.testing.assert_array_equal(xs, oracle_case.power[s]['x'])
        assert [counter[1], counter[2]] == oracle_case.power[s]['rejections']
    # code 1: asym_tanh with max_iter inside the gap of the step counts
    tanh = _table('float64', solver=TANH, thetas=THETAS[:1], nz=TANH_NZ)
    _check_against(tanh, 0, oracle_case.tanh)
    assert list(tanh.rejections[0]) == [2, 0]


def test_one_set_equals_sample_tuning_curves(oracle_case):
    s = 3
    tab = _table('float64', thetas=[THETAS[s]])
    tunings, (zs, xs, info) = ssnode.sample_tuning_curves(track_offset_identity=True, NZ=NZ, seed=0, **dict(dict(STIM, **PROBES), **dict(THETAS[s], **POWER)))
    assert tab.accepted[0] == NZ == tunings.shape[1] and tab.used[0] == NZ + info.rejections
    assert list(tab.rejections[0]) == [info.counter[1], info.counter[2]] == oracle_case.power[s]['rejections']
    rs = np.random.RandomState(0)
    stream = [rs.rand(1, M, M)[0] for _ in range(int(tab.used[0]))]
    np.testing.assert_array_equal(np.array([stream[i] for i in tab.draw_index[0]]), zs)
    np.testing.assert_allclose(tab.tunings[0], tunings.T, rtol=1e-9, atol=0)


# ---- 5. independence of the grouping ------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_result_does_not_depend_on_the_grouping(dtype):
    base = _table(dtype, round_draws=CANDIDATES, max_draws_per_launch=4096)
    assert (base.accepted < NZ).any() and (base.accepted == NZ).any()
    for round_draws, budget in itertools.product([5, 12, 40], [40, 4096]):
        tab = _table(dtype, round_draws=round_draws, max_draws_per_launch=budget)
        for name in tab._fields:
            np.testing.assert_array_equal(getattr(tab, name), getattr(base, name),
                                          err_msg='{} with round_draws={} max_draws_per_launch={}'.format(name, round_draws, budget))


def test_sampling_stops_drawing_when_every_set_is_full():
    tab = _table('float64', thetas=THETAS[2:4], round_draws=5)
    assert (tab.accepted == NZ).all() and list(tab.used) == [19, 16] and tab.candidates == 20


# ---- 6. the scorer ------------------------------------------------------------------------------------------------------

CFG = dict(num_sites=N, bandwidths=BANDWIDTHS, contrasts=CONTRAST, smoothness=SMOOTHNESS, probes=SITES + [s + N for s in SITES])
FP = dict(dynamics='fixed-point', max_candidates=CANDIDATES, solver_options=dict(max_iter=POWER['max_iter']))


@pytest.fixture(scope='module')
def truth():
    from tc_gan_amd.networks.dataset import dataset_by_ssnode
    return dataset_by_ssnode(num_sites=N, bandwidths=BANDWIDTHS, contrasts=CONTRAST, truth_size=NZ, truth_seed=0, sample_sites=SITES,
                             include_inhibitory_neurons=True,
                             true_ssn_options=dict(THETAS[3], smoothness=SMOOTHNESS, max_iter=POWER['max_iter']))


def test_fixed_point_scores(oracle_case, truth):
    assert truth.shape == (NZ, 16)
    res = distdiff.score_parameter_sets(CFG, THETAS, truth, draws=NZ, seed=0, return_samples=True, **FP)
    C = 16
    assert res['num'].shape == (5, C + 4 * 4) and res['dynamics'] == 'fixed-point' and res['candidates'] == CANDIDATES
    assert res['solver_variant'] == libssnode.ssn_solver_fast_path(M, 4, 8)
    np.testing.assert_array_equal(res['accepted'], [e['accepted'] for e in oracle_case.power])
    np.testing.assert_array_equal(res['used'], [e['used'] for e in oracle_case.power])
    np.testing.assert_array_equal(res['rejections'], [e['rejections'] for e in oracle_case.power])
    np.testing.assert_array_equal(res['n'][:, :C], np.repeat(res['accepted'][:, None], C, axis=1))
    assert (res['n'][:, C:] <= res['accepted'][:, None]).all()
    tfeat = distdiff._features(_dev(truth, torch.float32), 1, 4, 4).cpu().numpy()
    for s in range(5):
        got = int(res['accepted'][s])
        assert np.isfinite(res['tuning_curves'][s, :got]).all() and np.isnan(res['tuning_curves'][s, got:]).all()
        assert np.isnan(res['features'][s, got:]).all()
        for cols, samples, ref in ((slice(0, C), res['tuning_curves'][s], truth.astype('float32')), (slice(C, None), res['features'][s], tfeat)):
            want_num, want_n, want_m = ks_numerators(samples, ref)
            np.testing.assert_array_equal(res['num'][s, cols], want_num)
            np.testing.assert_array_equal(res['n'][s, cols], want_n)
            np.testing.assert_array_equal(res['m'][cols], want_m)
    # the truth's own parameters, seed and size: the truth's curves
    np.testing.assert_array_equal(res['num'][3], 0)
    assert (res['KSD'][3] == 0).all() and (res['num'][[0, 1, 2, 4], :C] > 0).any()
    np.testing.assert_array_equal(res['tuning_curves'][3], truth.astype('float32'))


def test_default_dynamics_is_the_fixed_time_path():
    from test_distdiff_gpu import CFG as FT_CFG, _looped, _thetas
    from tc_gan_amd.networks.fixed_time_sampler import FixedTimeTuningCurveSampler, new_JDS
    cfg = dict(FT_CFG, gen_kernel='tile')
    thetas = _thetas(3, 21)
    ref = FixedTimeTuningCurveSampler.from_dict(dict(cfg, batchsize=16, seed=4, **new_JDS)).sample()
    res = distdiff.score_parameter_sets(cfg, thetas, ref, draws=5, seed=2, max_draws_per_launch=10, return_samples=True)
    same = distdiff.score_parameter_sets(cfg, thetas, ref, draws=5, seed=2, max_draws_per_launch=10, return_samples=True,
                                         dynamics='fixed-time', solver_options=dict(max_iter=3), max_candidates=1)
    curves, num, n, m = _looped(cfg, thetas, ref, 5, 2)                          # the samplers themselves, KS on the host
    C = ref.shape[1]
    np.testing.assert_array_equal(res['tuning_curves'], curves)
    np.testing.assert_array_equal(res['num'][:, :C], num)
    np.testing.assert_array_equal(res['n'][:, :C], n)
    assert sorted(res) == sorted(same) and not {'accepted', 'used', 'rejections', 'candidates', 'solver_variant', 'dynamics'} & set(res)
    for key in res:
        np.testing.assert_array_equal(np.asarray(res[key], dtype=object if key in ('stat', 'note') else None),
                                      np.asarray(same[key], dtype=object if key in ('stat', 'note') else None), err_msg=key)


# ---- 7. the command line ------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def tiny_run(tmp_path_factory):
    from tc_gan_amd.run import bptt_moments
    from tc_gan_amd.networks.fixed_time_sampler import new_JDS
    tmp = tmp_path_factory.mktemp('moments')
    cfg = tmp / 'config.json'
    cfg.write_text(json.dumps(dict(num_sites=20, true_ssn_options={k: (new_JDS[k] * 1.05).tolist() for k in 'JDS'})))
    bptt_moments.main(['--n_bandwidths', '4', '--seqlen', '40', '--skip-steps', '30', '--iterations', '3', '--quiet', '--truth_size', '16',
                       '--dataset-provider', 'fixedtime', '--gen-kernel', 'tile', '--batchsize', '4', '--sample-sites', '0,0.5',
                       '--gen-moments-record-interval', '1', '--datastore', str(tmp / 'run'), '--load-config', str(cfg)])
    assert json.load(open(str(tmp / 'run' / 'exit.json')))['good']
    return str(tmp / 'run')


def test_command_line_writes_the_fixed_point_tables(tiny_run, tmp_path):
    import pandas
    out, plain = tmp_path / 'fp', tmp_path / 'plain'
    subprocess.run([sys.executable, os.path.join(ROOT, 'run.py'), 'tc_gan.analyzers.distdiff', '--', tiny_run, '--dynamics', 'fixed-point',
                    '--draws', '6', '--max-candidates', '12', '--output', str(out)], check=True, timeout=300)
    assert sorted(os.listdir(str(out))) == ['distdiff.csv', 'distdiff.json', 'rejections.csv']
    table = pandas.read_csv(str(out / 'distdiff.csv'), float_precision='round_trip')
    rej = pandas.read_csv(str(out / 'rejections.csv'))
    meta = json.load(open(str(out / 'distdiff.json')))
    steps = meta['gen_steps']
    C = 4 * 2
    assert len(steps) == 3 and list(table.columns) == ['gen_step', 'stat', 'KSD', 'n', 'm'] and len(table) == 3 * (C + 4 * 2)
    assert list(rej.columns) == ['gen_step', 'accepted', 'used', 'code1', 'code2'] and list(rej['gen_step']) == steps
    assert ((rej['accepted'] + rej['code1'] + rej['code2']) == rej['used']).all() and (rej['accepted'] <= 6).all()
    for key in ('accepted', 'used', 'rejections', 'candidates', 'solver_variant'):
        assert key in meta, key
    assert meta['dynamics'] == 'fixed-point' and meta['arguments']['dynamics'] == 'fixed-point' and meta['accepted'] == list(rej['accepted'])
    assert meta['rejections'] == [[int(a), int(b)] for a, b in zip(rej['code1'], rej['code2'])] and meta['candidates'] <= 12
    assert meta['solver_options']['io_type'] == 'asym_power' and meta['solver_options']['max_iter'] == 100000
    raw = table[table['stat'].str.startswith('tc_')]
    np.testing.assert_array_equal(raw['n'].to_numpy().reshape(3, C), np.repeat(rej['accepted'].to_numpy()[:, None], C, axis=1))
    # without the flag: the files and the keys of the fixed-time scorer, nothing of the new mode
    distdiff.main([tiny_run, '--draws', '6', '--output', str(plain)])
    assert sorted(os.listdir(str(plain))) == ['distdiff.csv', 'distdiff.json']
    meta = json.load(open(str(plain / 'distdiff.json')))
    assert sorted(meta) == ['arguments', 'bandwidths', 'chunk', 'chunks', 'contrasts', 'draws', 'features', 'gen_kernel', 'gen_steps', 'note',
                            'probes']
    assert sorted(meta['arguments']) == ['draws', 'gen_kernel', 'max_draws_per_launch', 'output', 'rundir', 'save_tuning_curves', 'seed',
                                         'steps']
    assert meta['gen_kernel'] == 'tile'
    again = distdiff.calc_distdiff(tiny_run, draws=6)
    back = pandas.read_csv(str(plain / 'distdiff.csv'), float_precision='round_trip')
    np.testing.assert_array_equal(back['KSD'].to_numpy(), again['KSD'].reshape(-1))
    assert (back['n'] == 6).all()

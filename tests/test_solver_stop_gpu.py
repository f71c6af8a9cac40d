"""The stop protocol of every fixed-point solver kernel: stop codes, stop steps, the newest state and the one before it.

Inputs.  Every case solves B = 3 weight draws x NB stimuli given PER DRAW, the rows scaled by the contrast ladder
LADDER[:NB] rolled by 3 b for draw b, from r = 0 with dt = 8e-4, at most T = 48 steps, atol = 0.5.  The ladder puts every
outcome into ONE workgroup: contrast 0 converges at step 1, contrast 2000 is beyond the rate bound after step 1, the
middle contrasts converge at steps 2 .. 39 or (asym_power / asym_linear, rate_stop_at = 200) cross the bound at steps
2 .. 4, and the largest bounded ones (asym_tanh) or one slow pair (asym_power, 2N = 104, NB = 11) run to max_iter.  A
stimulus therefore freezes at step 1 beside neighbours that run to the end, in both stimulus groups of the matrix-core
kernels, with the second group absent (NB = 4), ragged (NB = 5, 11, 12) or alone in a second workgroup (NB = 9), and
with an idle half in the two-draw kernel (B = 3 and B = 1).  `_reference` asserts on the CPU oracle that the ladder
still does this before any kernel is judged.

Test 1 (exact).  `max_iter = k, atol = 0` for k = 0 .. T gives the kernel's own fixed-step trajectory; the stop rule of
ssnode.c (first step with max |r1 - r0| < atol: code 0; else first step with max r1 >= rate_stop_at: code 2; else code 1
at max_iter; convergence wins at the same step) is replayed on it on the host in the kernel's number format, and a
stopped run must return exactly these codes and steps, x = traj[steps] and x_prev = traj[steps - 1], bit for bit.
With an unbounded I/O function the pairs beyond the rate bound overflow the number format some steps after they would
have stopped (stop steps 1 .. 4); the fixed-step assertions cover a pair while its state is finite, and the test
asserts that every replayed stop lies before the overflow.

Test 2 (against the fp64 C oracle).  States at 1e-4 (fp32) / 1e-9 (fp64) relative; codes and steps EQUAL for every pair
whose decision is not borderline in the oracle: a pair is left out if at some step up to its stop the oracle's
max |r1 - r0| / atol, or max r1 / rate_stop_at, lies within DELTA of 1.
Measured on one MI355X over all fp32 cases below, at the steps where the oracle's value is within a factor 2 of its
threshold: the kernel's per-step max |r1 - r0| deviates from the oracle's by at most 1.66e-4 relative and its max r1 by at
most 1.9e-5; DELTA32 = four times the larger, rounded up to one significant digit = 7e-4 (every case prints its own
figures and asserts that they stay below DELTA32).  fp64: DELTA64 = 1e-9 and no pair is left out.  Pairs left out by
the oracle at DELTA32, against the cap of one quarter (`test_ladder_gives_mixed_outcomes_on_the_oracle`):

    (N, NB)       (52, 11)  (76, 12)  (100, 8)  (100, 4)  (101, 9)  (104, 5)  (102, 8)
    asym_power    1 of 33   0 of 36   0 of 24   1 of 12   0 of 27   0 of 15   0 of 24
    asym_linear   1 of 33   1 of 36   0 of 24   1 of 12   0 of 27   0 of 15   0 of 24
    asym_tanh     1 of 33   1 of 36   0 of 24   1 of 12   0 of 27   0 of 15   0 of 24

Test 3.  `ssnode.sample_tuning_curves_table` in fp32 at N = 53 (2N = 106, the smallest size at which the library
picks a matrix-core solver), 5 sets x 40 candidates = 200 pairs in the first launch: variant 5.  On the oracle 10, 8,
27, 26 and 2 of the 40 candidates converge for all four stimuli; sets 2 and 3 fill (12 rows) at candidate 14, the
others come up short; 30, 32, 13, 14 and 38 draws mix code 0 and code 2; every code is unchanged when W is scaled by
1 +- 1e-5, which is what makes exact equality of the counts fair to an fp32 kernel (`sampler_case` asserts all of
it).  The asym_tanh set (`new_JDS` with D x 0.75: no rate above 60, so that fp32 can resolve atol = 1e-5 everywhere):
200 candidates in one launch, variant 6; max_iter = 2500 lies inside the gap 1270 .. 3804 of the oracle's step counts,
candidate 190 is beyond it (code 1) and 195 rows fill at candidate 196.  The rates are compared at 1e-4 relative plus
what the stop rule leaves open (`_check_table3`): the solver's atol and the spread of the oracle's own states over the
atol window that fp32 rounding of |r1 - r0| amounts to (`_expected3`), 6e-4 .. 7e-3 at the largest.
"""
import collections

import numpy as np
import pytest

from oracle import ssn_numpy as on
from test_solver_gpu import RTOL32, RTOL64, _oracle_batch
from test_fixedpoint_score_gpu import POWER, _expected

pytestmark = pytest.mark.gpu
P = on.DEFAULT_PARAMS

LADDER = [0, 5, 20, 40, 55, 65, 75, 85, 100, 150, 2000, 30]
B, T, DT, ATOL, STOP_AT = 3, 48, 8e-4, 0.5, 200.
SHAPES = [(52, 11), (76, 12), (100, 8), (100, 4), (101, 9), (104, 5)]
DELTA32 = 7e-4
DELTA64 = 1e-9
UNBOUNDED = ('asym_power', 'asym_linear')

Case = collections.namedtuple('Case', 'io_type N NB variant dtype B')


def _cases():
    some, few = [(52, 11), (100, 8), (100, 4)], [(52, 11), (104, 5)]
    out = [Case(io, N, NB, 5, 'float32', B) for io in UNBOUNDED for N, NB in SHAPES]
    out += [Case('asym_power', N, NB, v, 'float32', B) for v in (0, 1, 2, 3, 4) for N, NB in some]
    out += [Case('asym_linear', N, NB, v, 'float32', B) for v in (0, 1, 2, 3, 4) for N, NB in few]
    out += [Case('asym_tanh', N, NB, v, 'float32', B) for v in (5, 6, 7, 8) for N, NB in SHAPES]
    out += [Case('asym_tanh', N, NB, 2, 'float32', B) for N, NB in [(52, 11), (100, 8), (104, 5)]]
    out += [Case('asym_tanh', 100, 8, 8, 'float32', 1)]           # one draw: the other half of its workgroup idles
    out += [Case('asym_power', 102, 8, 0, 'float64', B), Case('asym_tanh', 52, 11, 0, 'float64', B),
            Case('asym_tanh', 102, 8, 2, 'float64', B), Case('asym_power', 52, 11, 2, 'float64', B)]
    return out


CASES = _cases()
IDS = ['{}-N{}-NB{}-v{}-{}-B{}'.format(*c) for c in CASES]


def _inputs(N, NB):
    """W (B, 2N, 2N) and the per-draw stimuli (B, NB, 2N) of a shape, in fp64."""
    jds = on.new_JDS()
    zs = np.random.RandomState(N * 31 + NB).rand(B, 2 * N, 2 * N)
    Ws = np.stack([on.generate_weight(N, jds['J'], jds['D'], jds['S'], z) for z in zs])
    rows = on.stimulus_input(np.linspace(0.0625, 1, NB), np.linspace(-.5, .5, N), P['smoothness'], contrasts=[1.0])
    contrast = np.array([np.roll(LADDER[:NB], 3 * b) for b in range(B)], dtype=float)
    return Ws, rows[None] * contrast[:, :, None]


def _replay(traj, atol, stop_at, max_iter):
    """The stop rule of ssnode.c on a fixed-step trajectory (T + 1, B, NB, 2N), in the trajectory's own number format:
    codes and steps (B, NB).  `stop_at` None: no rate test (asym_tanh)."""
    dt = traj.dtype.type
    with np.errstate(invalid='ignore', over='ignore'):
        moving = (np.abs(traj[1:max_iter + 1] - traj[:max_iter]) >= dt(atol)).any(axis=-1)         # (max_iter, B, NB)
        beyond = (traj[1:max_iter + 1] >= dt(stop_at)).any(axis=-1) if stop_at is not None else np.zeros_like(moving)
    stop = ~moving | beyond
    codes = np.ones(traj.shape[1:3], dtype=np.int32)
    steps = np.full(traj.shape[1:3], max_iter, dtype=np.int32)
    for b, s in zip(*np.nonzero(stop.any(axis=0))):
        k = int(np.argmax(stop[:, b, s]))
        codes[b, s], steps[b, s] = (2 if moving[k, b, s] else 0), k + 1
    return codes, steps


def _at(traj, steps):
    """traj[steps[b, s], b, s] for every pair."""
    b, s = np.indices(steps.shape)
    return traj[steps, b, s]


_REFERENCE = {}


def _reference(oracle_lib, io_type, N, NB):
    """The fp64 C oracle on a shape, computed once: its fixed-step trajectory (one Euler step at a time from the state
    before, which is the arithmetic of `max_iter = k` from r = 0; the end state is compared with that call), and the codes
    and steps of the stopped run.  Asserts that the ladder still gives the mixed outcomes the tests are about."""
    key = (io_type, N, NB)
    if key in _REFERENCE:
        return _REFERENCE[key]
    Ws, exts = _inputs(N, NB)
    free = dict(hard=np.inf) if io_type in UNBOUNDED else {}
    stopped = dict(hard=STOP_AT) if io_type in UNBOUNDED else {}
    traj = np.zeros((T + 1, B, NB, 2 * N))
    with np.errstate(all='ignore'):
        for k in range(1, T + 1):
            for b in range(B):
                traj[k, b] = _oracle_batch(oracle_lib, Ws[b:b + 1], exts[b], io_type, 1, 0.0, dt=DT, r0=traj[k - 1, b:b + 1],
                                           **free)[0][0]
    runs = [_oracle_batch(oracle_lib, Ws[b:b + 1], exts[b], io_type, T, ATOL, dt=DT, **stopped) for b in range(B)]
    x, codes, steps = (np.concatenate([r[i] for r in runs]) for i in range(3))
    # the chained trajectory is the oracle's own: states, codes and steps of the stopped run follow from it by the rule
    rcodes, rsteps = _replay(traj, ATOL, STOP_AT if io_type in UNBOUNDED else None, T)
    np.testing.assert_array_equal(codes, rcodes)
    np.testing.assert_array_equal(steps, rsteps)
    np.testing.assert_array_equal(x, _at(traj, steps))
    if np.isfinite(traj[T]).all():
        whole = [_oracle_batch(oracle_lib, Ws[b:b + 1], exts[b], io_type, T, 0.0, dt=DT, **free)[0] for b in range(B)]
        np.testing.assert_array_equal(np.concatenate(whole), traj[T])
    # the inputs still make the case: a freeze at step 1 beside pairs that run on, and (NB >= 8) several codes and steps
    assert steps.min(axis=1).max() == 1 and steps.max(axis=1).min() >= 6 and steps.max() >= 20, steps
    if NB >= 8:
        assert len(set(steps.flat)) >= 6, steps
        assert len(set(codes.flat)) >= 2, codes
        assert all(len(set(steps[b][:8])) >= 3 for b in range(B)), steps
    with np.errstate(all='ignore'):
        dmax = np.abs(traj[1:] - traj[:-1]).max(axis=-1)                    # [k - 1]: step k
        rmax = traj[1:].max(axis=-1)
    ref = dict(Ws=Ws, exts=exts, traj=traj, codes=codes, steps=steps, dmax=dmax, rmax=rmax)
    _REFERENCE[key] = ref
    return ref


def _borderline(ref, io_type, delta):
    """Pairs (B, NB) whose decision at some step up to their stop is within `delta` of a threshold in the oracle."""
    k = np.arange(1, T + 1)[:, None, None]
    upto = k <= ref['steps'][None]
    with np.errstate(all='ignore'):
        near = np.abs(ref['dmax'] / ATOL - 1) <= delta
        if io_type in UNBOUNDED:
            near |= np.abs(ref['rmax'] / STOP_AT - 1) <= delta
    return (near & upto).any(axis=0)


@pytest.mark.parametrize('N,NB', SHAPES + [(102, 8)])
@pytest.mark.parametrize('io_type', ['asym_power', 'asym_linear', 'asym_tanh'])
def test_ladder_gives_mixed_outcomes_on_the_oracle(oracle_lib, io_type, N, NB):
    """The reference alone: the outcomes are mixed (asserted in `_reference`), and at most a quarter of the pairs is
    borderline at DELTA32 while the rest still shows every code."""
    ref = _reference(oracle_lib, io_type, N, NB)
    out = _borderline(ref, io_type, DELTA32)
    print('{} 2N = {} NB = {}: {} of {} pairs within {} of a threshold; codes {} steps {}'.format(
        io_type, 2 * N, NB, out.sum(), out.size, DELTA32, sorted(set(ref['codes'].flat)), sorted(set(ref['steps'].flat))))
    assert 4 * out.sum() <= out.size
    assert set(ref['codes'][~out].flat) == set(ref['codes'].flat)
    assert not _borderline(ref, io_type, DELTA64).any()


# ---- the kernels ----------------------------------------------------------------------------------------------------

_RUNS = {}
Run = collections.namedtuple('Run', 'x prev codes steps')


def _solve(case, dW, dE, **kw):
    from tc_gan_amd import clib, ssnode
    opts = dict(max_iter=T, atol=ATOL, dt=DT, io_type=case.io_type, dtype=case.dtype, variant=case.variant, want_prev=True,
                return_torch=True)
    if case.io_type in UNBOUNDED:
        opts['rate_stop_at'] = STOP_AT
    opts.update(kw)
    try:
        return ssnode.fixed_points_batch(dW, dE, P['k'], P['n'], **opts)
    except clib.SSNLibraryError as e:
        if 'no instantiation' in str(e):
            pytest.skip('variant {} has no instantiation for 2N = {}, NB = {}'.format(case.variant, 2 * case.N, case.NB))
        raise


def _host(res):
    return Run(*(t.cpu().numpy() for t in (res.x, res.x_prev, res.codes, res.steps)))


def _kernel_runs(case):
    """Everything a case launches, once: the fixed-step runs k = 0 .. T (atol = 0, no rate bound) and the stopped runs.
    The inputs go to the device once; results come back after the last launch."""
    if case in _RUNS:
        if _RUNS[case] is None:
            pytest.skip('variant {} has no instantiation for 2N = {}, NB = {}'.format(case.variant, 2 * case.N, case.NB))
        return _RUNS[case]
    import torch
    tdtype = torch.float32 if case.dtype == 'float32' else torch.float64
    Ws, exts = _inputs(case.N, case.NB)
    dW = torch.as_tensor(Ws[:case.B]).to('cuda', tdtype).contiguous()
    dE = torch.as_tensor(exts[:case.B]).to('cuda', tdtype).contiguous()
    free = dict(atol=0.0, **(dict(rate_stop_at=np.inf) if case.io_type in UNBOUNDED else {}))
    try:
        fixed = [_solve(case, dW, dE, max_iter=k, **free) for k in range(T + 1)]
    except pytest.skip.Exception:
        _RUNS[case] = None
        raise
    runs = dict(fixed=[_host(r) for r in fixed])
    runs['stop'] = _host(_solve(case, dW, dE))
    median = max(1, int(np.median(runs['stop'].steps)))
    runs['median'] = median
    runs['stop_median'] = _host(_solve(case, dW, dE, max_iter=median))
    runs['stop_wide'] = _host(_solve(case, dW, dE, atol=1e9))
    if case.B > 1:
        runs['alone'] = _host(_solve(case, dW[1:2], dE[1:2]))
    runs['traj'] = np.stack([r.x for r in runs['fixed']])
    _RUNS[case] = runs
    return runs


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(got, want, what, pairs=None):
    got, want = _bits(got), _bits(want)
    if pairs is not None:
        got, want = got[pairs], want[pairs]
    np.testing.assert_array_equal(got, want, err_msg=what)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_stopped_runs_replay_the_fixed_step_trajectory_exactly(case):
    runs = _kernel_runs(case)
    traj = runs['traj']
    # the fixed-step runs themselves, for every pair whose state is still finite (see the module docstring)
    finite = np.isfinite(traj).all(axis=-1)                                      # (T + 1, B, NB)
    alive = np.logical_and.accumulate(finite, axis=0)
    overflow_at = np.where(alive.all(axis=0), T + 1, np.argmin(alive, axis=0))   # first step with a non-finite state
    assert alive[0].all() and not traj[0].any() and not runs['fixed'][0].prev.any()
    for k, r in enumerate(runs['fixed']):
        ok = alive[k]
        np.testing.assert_array_equal(r.codes[ok], 1, err_msg='codes of max_iter = {}, atol = 0'.format(k))
        np.testing.assert_array_equal(r.steps[ok], k, err_msg='steps of max_iter = {}, atol = 0'.format(k))
        _same_bits(r.prev, traj[max(k - 1, 0)], 'x_prev of max_iter = {} against x of max_iter = {}'.format(k, k - 1), ok)
    stop_at = STOP_AT if case.io_type in UNBOUNDED else None
    for name, atol, max_iter in (('stop', ATOL, T), ('stop_median', ATOL, runs['median']), ('stop_wide', 1e9, T)):
        codes, steps = _replay(traj, atol, stop_at, max_iter)
        assert (steps < overflow_at).all(), 'a pair overflows before it stops'
        got = runs[name]
        what = ' (atol = {}, max_iter = {}; replayed codes\n{}\nsteps\n{})'.format(atol, max_iter, codes, steps)
        np.testing.assert_array_equal(got.codes, codes, err_msg='codes' + what)
        np.testing.assert_array_equal(got.steps, steps, err_msg='steps' + what)
        _same_bits(got.x, _at(traj, steps), 'x against traj[steps]' + what)
        _same_bits(got.prev, _at(traj, steps - 1), 'x_prev against traj[steps - 1]' + what)
        if name == 'stop_median':
            assert (codes == 1).any() and (codes != 1).any()                # max_iter cuts through a mixed workgroup
        if name == 'stop_wide':
            assert (codes == 0).all() and (steps == 1).all()                # convergence wins over the rate bound
            if stop_at is not None and case.NB >= 11:                       # ... also for the pair beyond it (contrast 2000)
                assert (traj[1] >= stop_at).any(axis=-1).any()
    # the verdicts of a draw do not depend on its batch (two-draw kernel: the draw moves to the other half)
    if case.B > 1:
        for name in Run._fields:
            got, want = getattr(runs['alone'], name)[0], getattr(runs['stop'], name)[1]
            if got.dtype.kind == 'f':
                _same_bits(got, want, name + ' of draw 1 solved alone')
            else:
                np.testing.assert_array_equal(got, want, err_msg=name + ' of draw 1 solved alone')


def _deviation(ref, traj, io_type, nb):
    """Largest relative deviation of the kernel's per-step max |r1 - r0|, and of its max r1, from the oracle's, over the
    steps at which the oracle's value is within a factor 2 of its threshold."""
    t64 = traj.astype(np.float64)
    with np.errstate(all='ignore'):
        pairs = [(np.abs(t64[1:] - t64[:-1]).max(axis=-1), ref['dmax'][:, :nb], ATOL)]
        if io_type in UNBOUNDED:
            pairs.append((t64[1:].max(axis=-1), ref['rmax'][:, :nb], STOP_AT))
        out = []
        for got, want, threshold in pairs:
            close = (want >= threshold / 2) & (want <= threshold * 2)
            out.append((np.abs(got - want) / want)[close].max() if close.any() else 0.0)
    return out + [0.0] * (2 - len(out))


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_codes_steps_and_states_against_the_oracle(oracle_lib, case):
    ref = _reference(oracle_lib, case.io_type, case.N, case.NB)
    runs = _kernel_runs(case)
    nb = case.B
    traj, got = runs['traj'], runs['stop']
    rtol, delta = (RTOL32, DELTA32) if case.dtype == 'float32' else (RTOL64, DELTA64)
    # states: after T fixed steps -- for a pair that the oracle stops at the rate bound, at that step (beyond the bound
    # the unbounded I/O functions amplify any rounding difference step by step, up to overflow)
    upto = np.where(ref['codes'][:nb] == 2, ref['steps'][:nb], T)
    np.testing.assert_allclose(_at(traj, upto), _at(ref['traj'][:, :nb], upto), rtol=rtol, atol=rtol * 1e-2)
    dev = _deviation(ref, traj, case.io_type, nb)
    print('{}: max |r1 - r0| deviates by {:.3g}, max r1 by {:.3g} (relative, near the thresholds); delta {}'.format(
        '{}-N{}-NB{}-v{}-{}-B{}'.format(*case), dev[0], dev[1], delta))
    out = _borderline(ref, case.io_type, delta)[:nb]
    keep = ~out
    print('left out {} of {} pairs'.format(out.sum(), out.size))
    assert 4 * out.sum() <= out.size
    assert set(ref['codes'][:nb][keep].flat) == set(ref['codes'][:nb].flat)
    if case.dtype == 'float64':
        assert not out.any()
    assert max(dev) <= delta, 'the kernel deviates from the oracle by more than the margin of the exclusion'
    what = ' (pairs left out:\n{}\noracle codes\n{}\nsteps\n{})'.format(out.astype(int), ref['codes'][:nb], ref['steps'][:nb])
    np.testing.assert_array_equal(got.codes[keep], ref['codes'][:nb][keep], err_msg='codes' + what)
    np.testing.assert_array_equal(got.steps[keep], ref['steps'][:nb][keep], err_msg='steps' + what)


# ---- the fixed-point sampler on the kernel it really runs -------------------------------------------------------------

N3, M3 = 53, 106
BANDWIDTHS3, CONTRAST3, SMOOTHNESS3 = [0, .125, .5, 1], [20.0], .25 / 8
NZ3, CANDIDATES3 = 12, 40
SITES3 = [26, 22]
SCALES3 = [dict(J=1), dict(J=.5), dict(J=.6, S=2), dict(J=.4, S=2), dict(J=.3, S=.5)]
THETAS3 = [{k: on.DEFAULT_PARAMS[k] * sc.get(k, 1) for k in 'JDS'} for sc in SCALES3]
THETA3_TANH = dict(on.new_JDS(), D=on.new_JDS()['D'] * .75)
TANH3 = dict(io_type='asym_tanh', max_iter=2500)
TANH3_CANDIDATES, TANH3_NZ = 200, 195


def _oracle_candidates3(oracle_lib, theta, count, io_type, max_iter, scale=1.0, dt=8e-4, hard=1000., atol=1e-5):
    """codes, steps (count, NB) and states of the first `count` candidates of the stream on the CPU oracle."""
    rs = np.random.RandomState(0)
    Ws = np.stack([on.generate_weight(N3, theta['J'], theta['D'], theta['S'], rs.rand(1, M3, M3)[0]) for _ in range(count)])
    exts = on.stimulus_input(BANDWIDTHS3, np.linspace(-.5, .5, N3), SMOOTHNESS3, CONTRAST3, [0.])
    x, codes, steps = _oracle_batch(oracle_lib, Ws * scale, exts, io_type, max_iter, atol, dt=dt, hard=hard)
    return codes, steps, x


def _verdicts3(codes, steps, x):
    """[(verdict, largest step count, states)] per candidate: the code of the last stimulus that failed (the order in
    which `find_fixed_points` reports it), a non-finite "converged" state counting as code 1."""
    out = []
    for c, st, xs in zip(codes, steps, x):
        failed = [int(ci) if ci else 1 for ci, xi in zip(c[::-1], xs[::-1]) if ci or not np.isfinite(xi).all()]
        out.append((failed[0] if failed else 0, int(st.max()), xs))
    return out


def _expected3(oracle_lib, theta, count, nz, opts):
    """What the oracle expects of a set (`_expected` of the scorer's tests), after checking that no code changes when W is
    scaled by 1 +- 1e-5, plus `slack`: how far the stop rule itself leaves an accepted state open in fp32.  r1 is rounded
    to fp32, so the |r1 - r0| that a kernel compares with atol = 1e-5 is off by up to half an ulp h of the largest rate:
    it stops where an exact test with some atol in [1e-5 - h, 1e-5 + h] would, and `slack` is the distance between the
    oracle's states at these two."""
    codes, steps, x = _oracle_candidates3(oracle_lib, theta, count, **opts)
    for scale in (1 - 1e-5, 1 + 1e-5):
        np.testing.assert_array_equal(_oracle_candidates3(oracle_lib, theta, count, scale=scale, **opts)[0], codes)
    exp = _expected(_verdicts3(codes, steps, x), nz)
    rows = [i for i in exp['draw_index'] if i >= 0]
    h = float(np.spacing(np.float32(exp['x'].max()))) / 2
    assert h < 1e-5, 'the accepted rates are too large for fp32 to resolve atol = 1e-5'
    early, late = (_oracle_candidates3(oracle_lib, theta, count, atol=a, **opts) for a in (1e-5 + h, 1e-5 - h))
    assert (early[0][rows] == 0).all() and (late[0][rows] == 0).all()
    exp.update(codes=codes, slack=np.abs(early[2][rows] - late[2][rows]), h=h)
    return exp


def _sampler_case(oracle_lib):
    power_opts = dict(io_type='asym_power', max_iter=POWER['max_iter'], dt=POWER['dt'], hard=POWER['rate_stop_at'])
    exp = [_expected3(oracle_lib, th, CANDIDATES3, NZ3, power_opts) for th in THETAS3]
    assert all(set(e['codes'].flat) == {0, 2} for e in exp)
    assert [sum(not c.any() for c in e['codes']) for e in exp] == [10, 8, 27, 26, 2]
    assert [e['accepted'] for e in exp] == [10, 8, 12, 12, 2] and [e['used'] for e in exp] == [40, 40, 14, 14, 40]
    assert [sum(set(c) == {0, 2} for c in e['codes']) for e in exp] == [30, 32, 13, 14, 38]
    # asym_tanh: max_iter inside a wide gap of the step counts
    limit = TANH3['max_iter']
    steps = np.sort(_oracle_candidates3(oracle_lib, THETA3_TANH, TANH3_CANDIDATES, 'asym_tanh', 8000)[1].max(axis=1))
    below, above = steps[steps <= limit].max(), steps[steps > limit].min()
    assert limit - below >= 200 and above - limit >= 200 and (steps > limit).sum() == 1
    exp_tanh = _expected3(oracle_lib, THETA3_TANH, TANH3_CANDIDATES, TANH3_NZ, dict(io_type='asym_tanh', max_iter=limit))
    assert exp_tanh['accepted'] == TANH3_NZ and exp_tanh['rejections'] == [1, 0]
    return collections.namedtuple('SamplerCase', 'power tanh')(exp, exp_tanh)


@pytest.fixture(scope='module')
def sampler_case(oracle_lib):
    """What the CPU oracle expects per set, after checking that the inputs still make the cases and that no code depends
    on the last digits of W."""
    return _sampler_case(oracle_lib)


def _table3(thetas, nz, candidates, solver, **kw):
    from tc_gan_amd import ssnode
    return ssnode.sample_tuning_curves_table(
        thetas, NZ=nz, seed=0, N=N3, bandwidths=BANDWIDTHS3, smoothness=SMOOTHNESS3, contrast=CONTRAST3, sample_sites=SITES3,
        include_inhibitory_neurons=True, dtype='float32', round_draws=candidates, max_candidates=candidates, **dict(solver, **kw))


def _check_table3(tab, s, exp):
    """Counts and indices equal the oracle's; the rates are within 1e-4 relative of it, plus what the stop rule leaves
    open: in fp32 the `slack` of `_expected3`, and in any format the solver's atol = 1e-5 -- a rate below atol passes the
    stop test whatever it does, so the value the oracle holds for a silenced neuron (it decays by dt / tau per step, to
    1e-16 .. 1e-85 for the widest stimuli, below the fp32 range) only records the step at which the oracle stopped."""
    assert tab.accepted[s] == exp['accepted'] and tab.used[s] == exp['used']
    assert list(tab.rejections[s]) == exp['rejections'] and list(tab.draw_index[s]) == exp['draw_index']
    want, slack = (on.subsample_neurons(a, SITES3, track_offset_identity=True, include_inhibitory_neurons=True)
                   for a in (exp['x'], exp['slack']))
    got = tab.tunings[s, :exp['accepted']]
    assert np.isfinite(got).all() and np.isnan(tab.tunings[s, exp['accepted']:]).all()
    diff = np.abs(got - want)
    allowed = 1e-4 * np.abs(want) + slack + 1e-5
    big = np.abs(want) >= 1
    print('set {}: h = {:.3g}; largest difference to the oracle {:.3g} absolute, {:.3g} relative among the rates >= 1, {:.3g} '
          'of what is allowed (slack up to {:.3g})'.format(s, exp['h'], diff.max(), (diff / np.abs(want))[big].max(),
                                                          (diff / allowed).max(), slack.max()))
    worst = np.unravel_index(np.argmax(diff / allowed), diff.shape)
    assert (diff <= allowed).all(), 'row {} column {}: {!r} against the oracle\'s {!r}, slack {!r}'.format(
        worst[0], worst[1], got[worst], want[worst], slack[worst])


def _variant_for(pairs, nb, solver):
    import ctypes
    from tc_gan_amd import ssnode
    from tc_gan_amd.clib import libssnode
    unbounded = solver['io_type'] in UNBOUNDED
    p = ssnode._params(solver['io_type'], P['k'], P['n'], tau=P['tau'], dt=solver.get('dt', 8e-4), max_iter=solver['max_iter'],
                       atol=1e-5, rate_hard_bound=solver['rate_stop_at'] if unbounded else P['rate_hard_bound'])
    return libssnode.ssn_solve_batch_variant_for(pairs, nb, M3, 4, ctypes.byref(p))


def test_fp32_table_runs_the_fp32_matrix_core_solver_and_equals_the_oracle(sampler_case):
    tab = _table3(THETAS3, NZ3, CANDIDATES3, POWER)
    assert tab.variant == 5 == _variant_for(len(THETAS3) * CANDIDATES3, len(BANDWIDTHS3), POWER)
    assert tab.tunings.shape == (5, NZ3, 4 * 4) and tab.candidates == CANDIDATES3
    for s, exp in enumerate(sampler_case.power):
        _check_table3(tab, s, exp)
    tile = _table3(THETAS3, NZ3, CANDIDATES3, POWER, variant=2)
    assert tile.variant == 2
    for name in ('accepted', 'used', 'rejections', 'draw_index'):
        np.testing.assert_array_equal(getattr(tile, name), getattr(tab, name), err_msg=name)


def test_fp32_table_runs_the_split_solver_for_asym_tanh_and_counts_its_code_1_rejections(sampler_case):
    tab = _table3([THETA3_TANH], TANH3_NZ, TANH3_CANDIDATES, TANH3)
    assert tab.variant == 6 == _variant_for(TANH3_CANDIDATES, len(BANDWIDTHS3), TANH3)
    _check_table3(tab, 0, sampler_case.tanh)
    tile = _table3([THETA3_TANH], TANH3_NZ, TANH3_CANDIDATES, TANH3, variant=2)
    for name in ('accepted', 'used', 'rejections', 'draw_index'):
        np.testing.assert_array_equal(getattr(tile, name), getattr(tab, name), err_msg=name)

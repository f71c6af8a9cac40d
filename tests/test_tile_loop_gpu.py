"""The step loop of the fp32 NB = 1 tile solver: slot rotation, buffer parity, unconditional stores, FMA block.

Common setup: fp32, one stimulus per draw (NB = 1), B = 5 draws from `new_JDS`, through `ssnode.fixed_points_batch`, with
variant 3 (split tile) and with the library's own choice, at

    N    2N   C    what it exercises
    100  200  25   exact, mixed kernel
    99   198  25   ragged last column group: a column pair with one half masked
    86   172  25   light wave with 4 real rows
    73   146  19   5-row light wave with its own odd row

Test 1: `max_iter = k, atol = 0` for k = 0 .. 7 from a random non-zero r0 equals k one-step calls, each fed the `x` of the
call before, bit for bit, and `x_prev` of the k-step call is the `x` of step k - 1: every phase of the three-slot flag cycle
and both buffer parities, with the read-back of x_prev from LDS.  The state after 7 steps is within RTOL32 of the fp64 oracle.
Test 2: five contrasts (0, 20, 65, 150, 2000), one per draw, at atol = 0.5, T = 48 stop at different steps within one
launch; the stop rule of ssnode.c is replayed (`_replay` of test_solver_stop_gpu) on the kernel's own fixed-step trajectory
(48 chained one-step calls) and codes, steps, x and x_prev must be exact.  The CPU oracle is asked first whether these
inputs give a code 0 and a code 2 (asym_power, rate_stop_at = 200), a code 0 and a code 1 (asym_tanh).
Test 3: draw 1 solved alone equals draw 1 inside the batch, bit for bit.
Test 4: asym_power without a rate bound, 2N = 198, T = 12, one draw at contrast 2000 beside four at contrast 20.  On the
fp64 oracle contrast 2000 alone peaks near 1e13 within 12 steps (at every bandwidth of the default set) and does not leave the
fp32 range, so the draw also starts from r0 x 1e18: its first step is beyond the range, the test asserts that its result is
not finite, and that the other four draws are finite and carry exactly the bits they have in a batch without it.
"""
import numpy as np
import pytest

from oracle import ssn_numpy as on
from test_solver_gpu import RTOL32, _oracle_batch
from test_solver_stop_gpu import _at, _replay, _same_bits

pytestmark = pytest.mark.gpu
P = on.DEFAULT_PARAMS

B = 5
SIZES = [100, 99, 86, 73]
VARIANTS = [3, None]
KMAX = 7
CONTRASTS = [0., 20., 65., 150., 2000.]
T, ATOL, STOP_AT = 48, 0.5, 200.
IO_TYPES = ['asym_tanh', 'asym_power']

_SETUP = {}
_RUNS = {}


def _setup(N):
    """W (B, 2N, 2N), the stimulus row at contrast 1 (1, 2N) and a random non-zero r0 (B, 1, 2N), the latter two already
    rounded to fp32; device copies beside them."""
    if N in _SETUP:
        return _SETUP[N]
    import torch
    jds = on.new_JDS()
    rs = np.random.RandomState(1000 + N)
    Ws = np.stack([on.generate_weight(N, jds['J'], jds['D'], jds['S'], z) for z in rs.rand(B, 2 * N, 2 * N)])
    row = on.stimulus_input([1.0], np.linspace(-.5, .5, N), P['smoothness'], contrasts=[1.0]).astype(np.float32)
    r0 = (rs.rand(B, 1, 2 * N) * 20 + 0.05).astype(np.float32)
    s = dict(Ws=Ws, row=row, r0=r0, dW=torch.as_tensor(Ws).to('cuda', torch.float32).contiguous(),
             drow=torch.as_tensor(row).cuda(), dr0=torch.as_tensor(r0).cuda())
    s['dladder'] = (s['drow'][None] * torch.tensor(CONTRASTS, device='cuda', dtype=torch.float32)[:, None, None]).contiguous()
    _SETUP[N] = s
    return s


def _solve(dW, dE, variant, **kw):
    from tc_gan_amd import ssnode
    opts = dict(dtype='float32', variant=variant, want_prev=True, return_torch=True)
    opts.update(kw)
    return ssnode.fixed_points_batch(dW, dE, P['k'], P['n'], **opts)


def _host(res):
    return tuple(t.cpu().numpy() for t in (res.x, res.x_prev, res.codes, res.steps))


def _chain(dW, dE, variant, dr0, steps, **kw):
    """The kernel's own fixed-step trajectory (steps + 1, B, 1, 2N): one-step calls, each from the `x` of the call before."""
    xs = [dr0]
    for _ in range(steps):
        xs.append(_solve(dW, dE, variant, r0=xs[-1], max_iter=1, atol=0.0, **kw).x)
    return np.stack([x.cpu().numpy() for x in xs])


@pytest.mark.parametrize('variant', VARIANTS, ids=['v3', 'auto'])
@pytest.mark.parametrize('N', SIZES)
def test_k_steps_in_one_call_equal_k_one_step_calls(oracle_lib, N, variant):
    s = _setup(N)
    dE = s['drow'] * 20.0
    chain = _chain(s['dW'], dE, variant, s['dr0'], KMAX)
    assert np.isfinite(chain).all() and (chain[1:] != chain[:-1]).any(axis=-1).all()
    for k in range(KMAX + 1):
        x, prev, codes, steps = _host(_solve(s['dW'], dE, variant, r0=s['dr0'], max_iter=k, atol=0.0))
        np.testing.assert_array_equal(codes, 1, err_msg='codes of max_iter = {}'.format(k))
        np.testing.assert_array_equal(steps, k, err_msg='steps of max_iter = {}'.format(k))
        _same_bits(x, chain[k], 'x of max_iter = {} against {} one-step calls'.format(k, k))
        _same_bits(prev, chain[max(k - 1, 0)], 'x_prev of max_iter = {} against the x of step {}'.format(k, k - 1))
    want = _oracle_batch(oracle_lib, s['Ws'], s['row'].astype(np.float64) * 20.0, 'asym_tanh', KMAX, 0.0,
                         r0=s['r0'].astype(np.float64))[0]
    np.testing.assert_allclose(chain[KMAX], want, rtol=RTOL32, atol=RTOL32 * 1e-2)


def _oracle_ladder(oracle_lib, N, io_type):
    """Codes of the ladder on the CPU oracle: the inputs must give both outcomes the test is about."""
    s = _setup(N)
    hard = dict(hard=STOP_AT) if io_type == 'asym_power' else {}
    runs = [_oracle_batch(oracle_lib, s['Ws'][b:b + 1], s['row'].astype(np.float64) * CONTRASTS[b], io_type, T, ATOL, **hard)
            for b in range(B)]
    return np.concatenate([r[1] for r in runs]), np.concatenate([r[2] for r in runs])


def _ladder_runs(N, variant, io_type):
    key = (N, variant, io_type)
    if key not in _RUNS:
        s = _setup(N)
        import torch
        zero = torch.zeros_like(s['dr0'])
        free = dict(rate_stop_at=np.inf) if io_type == 'asym_power' else {}
        stop = dict(rate_stop_at=STOP_AT) if io_type == 'asym_power' else {}
        traj = _chain(s['dW'], s['dladder'], variant, zero, T, io_type=io_type, **free)
        batch = _host(_solve(s['dW'], s['dladder'], variant, max_iter=T, atol=ATOL, io_type=io_type, **stop))
        alone = _host(_solve(s['dW'][1:2], s['dladder'][1:2], variant, max_iter=T, atol=ATOL, io_type=io_type, **stop))
        _RUNS[key] = dict(traj=traj, batch=batch, alone=alone)
    return _RUNS[key]


@pytest.mark.parametrize('io_type', IO_TYPES)
@pytest.mark.parametrize('variant', VARIANTS, ids=['v3', 'auto'])
@pytest.mark.parametrize('N', SIZES)
def test_draws_stop_at_different_steps_within_one_launch(oracle_lib, N, variant, io_type):
    ocodes, osteps = _oracle_ladder(oracle_lib, N, io_type)
    assert {0, 2 if io_type == 'asym_power' else 1} <= set(ocodes.flat), ocodes
    assert len(set(osteps.flat)) >= 3, osteps
    runs = _ladder_runs(N, variant, io_type)
    traj = runs['traj']
    codes, steps = _replay(traj, ATOL, STOP_AT if io_type == 'asym_power' else None, T)
    alive = np.logical_and.accumulate(np.isfinite(traj).all(axis=-1), axis=0)
    overflow_at = np.where(alive.all(axis=0), T + 1, np.argmin(alive, axis=0))
    assert (steps < overflow_at).all(), 'a draw overflows before it stops'
    assert set(codes.flat) == set(ocodes.flat), (codes, ocodes)
    x, prev, gcodes, gsteps = runs['batch']
    what = ' (replayed codes {} steps {})'.format(codes.ravel(), steps.ravel())
    np.testing.assert_array_equal(gcodes, codes, err_msg='codes' + what)
    np.testing.assert_array_equal(gsteps, steps, err_msg='steps' + what)
    _same_bits(x, _at(traj, steps), 'x against traj[steps]' + what)
    _same_bits(prev, _at(traj, steps - 1), 'x_prev against traj[steps - 1]' + what)


@pytest.mark.parametrize('io_type', IO_TYPES)
@pytest.mark.parametrize('variant', VARIANTS, ids=['v3', 'auto'])
@pytest.mark.parametrize('N', SIZES)
def test_draw_1_alone_equals_draw_1_in_the_batch(N, variant, io_type):
    runs = _ladder_runs(N, variant, io_type)
    for name, got, want in zip(('x', 'x_prev', 'codes', 'steps'), runs['alone'], runs['batch']):
        if got.dtype.kind == 'f':
            _same_bits(got[0], want[1], name + ' of draw 1 solved alone')
        else:
            np.testing.assert_array_equal(got[0], want[1], err_msg=name + ' of draw 1 solved alone')


@pytest.mark.parametrize('variant', VARIANTS, ids=['v3', 'auto'])
def test_an_overflowing_draw_keeps_its_inf_and_nan_to_itself(variant):
    import torch
    N, steps, bad = 99, 12, 2
    s = _setup(N)
    opts = dict(io_type='asym_power', rate_stop_at=np.inf, atol=0.0, max_iter=steps)
    contrast = torch.full((B, 1, 1), 20.0, device='cuda')
    calm = _host(_solve(s['dW'], s['drow'][None] * contrast, variant, r0=s['dr0'], **opts))
    contrast[bad] = 2000.0
    r0 = s['dr0'].clone()
    r0[bad] *= 1e18
    wild = _host(_solve(s['dW'], (s['drow'][None] * contrast).contiguous(), variant, r0=r0, **opts))
    others = [b for b in range(B) if b != bad]
    assert np.isfinite(calm[0]).all() and np.isfinite(calm[1]).all()
    assert not np.isfinite(wild[0][bad]).all(), 'the draw was meant to overflow'
    for name, got, want in zip(('x', 'x_prev'), wild[:2], calm[:2]):
        assert np.isfinite(got[others]).all(), name
        _same_bits(got[others], want[others], name + ' of the draws beside the overflowing one')
    np.testing.assert_array_equal(wild[2][others], 1)
    np.testing.assert_array_equal(wild[3][others], steps)

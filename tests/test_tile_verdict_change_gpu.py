"""The verdict byte of the fp32 NB = 1 tile solver is stored only when it changes (csrc/ssn_tile.hip: a wave keeps the byte it
stored last per parity of the state buffer in a scalar register and stores under a scalar branch).  What the other tests of the
loop leave open is a byte that goes 1 -> 0 -> 1: both changes have to be stored, in the word of the right parity.

Inputs.  One draw, one stimulus, asym_power without a rate bound, W = 0 but for one excitatory row e and one inhibitory row i
of two different waves that drive each other, W[e, i] = -3 and W[i, e] = +3, ext_e = 12, ext_i = 6; every other row is its own
scalar recurrence with ext = 4 + 8 row / (2N - 1), as in test_tile_verdict_gpu.py.  Every row starts at the kernel's own fixed
point (2000 steps of the same kernel from r = 0) but for
  * row e, 0.5 above it: it relaxes over some 17 steps, and row i (eps_I = 0.4 against eps_E = 0.05) first runs after it,
    overshoots, turns round and follows it down.  With atol = 1e-2 row i moves by 20, 11, 5.3, 1.7 atol in steps 1-4, by 0.49
    atol at its turning point in step 5 and by 1.7, 2.4, 2.6 ... atol afterwards (fp64 model of the pair), falls below atol for
    good after step 20, and row e after step 17: the byte of row i's wave goes 1 -> 0 -> 1 while row e's wave keeps the solve
    alive, and from step 18 on row i's wave ALONE keeps it alive, with the 1 it stored again after step 5.  (Under eps_I = 0.4
    the pair is overdamped: one turning point, of row i; row e does not turn.)
  * a slowly relaxing row s of a third wave, whose last moving step is 8.
`shift` = 1 starts from the state after one step instead, so that the turning point falls on a step of the other parity.

Expected values: `_replay` of test_solver_stop_gpu (the stop rule of ssnode.c) on the kernel's own trajectory of chained one-step
calls; codes, steps, x and x_prev of the stopped run are exact.  Asserted from that replay, so that the case is what it claims:
row i's wave reports 1, then 0, then 1 again before the stop; while it reports 0 another wave moves; and at the last moving step
it moves alone.  max_iter = 40 and 41 (the stop comes before), and max_iter = the step count itself and one less, odd and even.

    2N    kernel (the library's choice)                   rows e / s / i
    200   solve_tile_mixed6_kernel, waves from rows 0, 56, 104, 152        3 / 60 / 160
    146   solve_tile_mixed_kernel at C = 19, waves from rows 0, 56, 112    3 / 60 / 120
"""
import collections

import numpy as np
import pytest

from oracle import ssn_numpy as on
from test_solver_stop_gpu import _at, _replay, _same_bits

pytestmark = pytest.mark.gpu
P = on.DEFAULT_PARAMS

DT, ATOL, T = 8e-4, 1e-2, 44
EPS = (DT / P['tau'][0], DT / P['tau'][1])
WAVE_START = {200: (0, 56, 104, 152), 146: (0, 56, 112)}
ROWS = {200: (3, 60, 160), 146: (3, 60, 120)}            # e, s, i
COUPLING, EXT_E, EXT_I, KICK, SLOW_LAST = 3.0, 12.0, 6.0, 0.5, 8

Case = collections.namedtuple('Case', 'M shift max_iter')
# max_iter 'steps': the replayed step count itself (the stop at exactly max_iter); 'steps-1': one less (code 1)
CASES = [Case(M, shift, mi) for M in (200, 146) for shift in (0, 1) for mi in (40, 41, 'steps', 'steps-1')]


def _wave(M, row):
    return sum(row >= s for s in WAVE_START[M]) - 1


_STATE = {}


def _setup(M):
    """W and ext on the device, the start state and the chained one-step trajectory, once per size."""
    import torch
    from tc_gan_amd import ssnode
    if M in _STATE:
        return _STATE[M]
    e, s, i = ROWS[M]
    assert e < M // 2 <= i and s < M // 2 and len({_wave(M, r) for r in (e, s, i)}) == 3
    W = np.zeros((1, M, M), dtype=np.float32)
    W[0, e, i], W[0, i, e] = -COUPLING, COUPLING
    ext = 4.0 + 8.0 * np.arange(M) / (M - 1)
    ext[e], ext[i] = EXT_E, EXT_I
    dW = torch.as_tensor(W).cuda()
    dE = torch.as_tensor(ext[None], dtype=torch.float32).cuda()

    def solve(r0, **kw):
        return ssnode.fixed_points_batch(dW, dE, P['k'], P['n'], r0=r0, dt=DT, io_type='asym_power', rate_stop_at=np.inf,
                                         dtype='float32', variant=None, want_prev=True, return_torch=True, **kw)

    fixed = solve(torch.zeros((1, 1, M), device='cuda', dtype=torch.float32), max_iter=2000, atol=0.0).x.cpu().numpy()[0, 0]
    r0 = fixed.astype(np.float64)
    r0[e] += KICK
    r0[s] += ATOL / (EPS[0] * (1 - EPS[0]) ** (SLOW_LAST - 0.5))
    chain = [torch.as_tensor(r0[None, None].astype(np.float32)).cuda()]
    for _ in range(T + 1):
        chain.append(solve(chain[-1], max_iter=1, atol=0.0).x)
    traj = torch.stack(chain).cpu().numpy()                                      # (T + 2, 1, 1, M)
    _STATE[M] = (solve, chain, traj)
    return _STATE[M]


@pytest.mark.parametrize('c', CASES, ids=['2N{}-shift{}-T{}'.format(*c) for c in CASES])
def test_a_byte_that_changes_back_is_stored_both_times(c):
    M = c.M
    e, s, i = ROWS[M]
    solve, chain, traj = _setup(M)
    traj = traj[c.shift:c.shift + T + 1]
    codes, steps = _replay(traj, ATOL, None, T)
    code, nsteps = int(codes[0, 0]), int(steps[0, 0])
    moving = np.abs(traj[1:, 0, 0] - traj[:-1, 0, 0]) >= np.float32(ATOL)        # [m - 1]: step m, per row
    wave_of = np.array([_wave(M, r) for r in range(M)])
    bits = np.stack([moving[:, wave_of == w].any(axis=1) for w in range(len(WAVE_START[M]))], axis=1)   # (T, waves)
    wi = _wave(M, i)
    line = ''.join(str(int(b)) for b in bits[:nsteps, wi])
    print('2N=%d shift %d: replayed code %d steps %d; byte of wave %d per step %s; rows moving per step %s'
          % (M, c.shift, code, nsteps, wi, line, moving[:nsteps].sum(axis=1).tolist()))
    # ---- the case is what it claims, from the replay ----
    assert code == 0 and 12 < nsteps < 40
    assert sorted(np.flatnonzero(moving[:nsteps].any(axis=0)).tolist()) == sorted([e, s, i])
    zeros = [m for m in range(nsteps - 1) if not bits[m, wi]]
    assert zeros and bits[:zeros[0], wi].all() and zeros[0] >= 2, line            # 1 ... 1, then 0
    assert bits[zeros[-1] + 1:nsteps - 1, wi].all() and zeros[-1] < nsteps - 3, line          # ... and 1 again up to the stop
    assert all(bits[m].any() for m in zeros)                                     # another wave keeps the solve alive meanwhile
    assert np.flatnonzero(bits[nsteps - 2]).tolist() == [wi] and not bits[nsteps - 1].any()   # the last mover, alone
    assert (zeros[0] + 1 + c.shift) % 2 == 1                                     # shift moves the turning point to the other parity
    assert not moving[SLOW_LAST - c.shift:, s].any() and moving[SLOW_LAST - c.shift - 1, s]

    # ---- the stopped run ----
    max_iter = {'steps': nsteps, 'steps-1': nsteps - 1}.get(c.max_iter, c.max_iter)
    want_codes, want_steps = _replay(traj, ATOL, None, max_iter)
    assert int(want_codes[0, 0]) == (1 if c.max_iter == 'steps-1' else 0)
    res = solve(chain[c.shift], max_iter=max_iter, atol=ATOL)
    np.testing.assert_array_equal(res.codes.cpu().numpy(), want_codes, err_msg='codes (replayed steps {})'.format(nsteps))
    np.testing.assert_array_equal(res.steps.cpu().numpy(), want_steps, err_msg='steps')
    _same_bits(res.x.cpu().numpy(), _at(traj, want_steps), 'x against traj[steps]')
    _same_bits(res.x_prev.cpu().numpy(), _at(traj, want_steps - 1), 'x_prev against traj[steps - 1]')

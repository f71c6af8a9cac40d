"""The per-wave stop verdict of the fp32 NB = 1 tile solver: one byte per wave in one word per parity of the state buffer.

What the other tests of this loop leave open is a step at which ONE wave alone decides the verdict, and a different wave
one step earlier: a wrong byte index, a byte that is not overwritten every step, or the word of the other parity.

Inputs.  One draw, one stimulus, W = 0: every row is its own scalar recurrence r <- r + (f(ext_i) - r) eps_i with
eps_E = dt / tau_E = 0.0503 (rows < N) and eps_I = 0.4, so the distance to the fixed point shrinks by (1 - eps) per step
and |r_m - r_{m-1}| = eps (1 - eps)^(m-1) |d0| for a row that starts d0 off it.  ext_i = 4 + 8 i / (2N - 1), rates
0.2 .. 2.4.  Every row starts at its own fixed point, taken from 1000 steps of the same kernel from r = 0 (where the
recurrence has stalled in fp32: those rows do not move at all), but for
  * row j, d0 = atol / (eps (1 - eps)^(k - 1/2)): step k moves it by atol / sqrt(1 - eps) and step k + 1 by
    atol sqrt(1 - eps), 2.5 % (E) or 23 % (I) on either side of atol = 1e-3, against 2.4e-4 that one fp32 ulp of a rate
    of 2 is of atol.  Row j alone moves at step k, nothing moves at step k + 1: code 0, steps = k + 1;
  * a partner row in ANOTHER wave (the same wave at 2N = 32, which has one), with k - 2 for k: its wave reports
    "moving" up to step k - 2 and has to report "still" from then on, while row j's wave goes on alone.
j runs over the first and the last row of every wave's row range (56 rows per wave); k = 4 and 9, max_iter = 16.

Rate bound (asym_power, rate_stop_at = S).  ext_j = 30 (fixed point f = 17.8), r0_j = f / 4 and S = f - (f - r0_j)
(1 - eps)^(k - 1/2): row j is below S after step k - 1 and above it after step k, by (f - S)(1 / sqrt(1 - eps) - 1) and
(f - S)(1 - sqrt(1 - eps)), at least 0.03, and S >= 6.6 is above every other rate.  The partner row's last moving step is
k + 3, so another wave still reports "moving" when row j's wave alone reports the bound: code 2, steps = k.  The
mirror: the main case under asym_power with S = 100, which no row reaches: code 0, steps = k + 1.

Boundaries: the stop at exactly max_iter (k = max_iter - 1, max_iter = 16 and 15), where the verdict of the last step
is the loop's own, and the stop at step 1 (every row at its fixed point).

Expected values: `_replay` of test_solver_stop_gpu (the stop rule of ssnode.c) on the kernel's own trajectory of chained
one-step calls; codes, steps, x and x_prev of the stopped run are exact.  Before that, on the CPU: the fp64 oracle,
started from ITS fixed point plus the same offsets, must give the designed code and step count (the design is right
before a kernel is asked), and on the trajectory the deciding step must belong to row j alone (and the step at which the
partner's wave falls still must be the designed one).  The oracle from the kernel's start state must give the replayed code
and a step count within 1 of the replayed one.

Checked once against two deliberately wrong builds of the loop: reading the verdict word of the other parity fails all 420
cases, every wave storing to byte 0 fails 277 of them; the parent commit's three-slot protocol passes all.

    2N    kernel (variant 3 and the library's choice / variant 4)
    200   mixed kernel, 4 waves / all-register, 4 waves
    146   C = 19, 3 waves, 5-row light wave / all-register, 3 waves
    104   all-register, 2 waves (every variant)
    32    one wave, C = 4: the masked state store without a pad float (every variant)
"""
import collections

import numpy as np
import pytest

from oracle import ssn_numpy as on
from test_solver_gpu import _oracle_batch
from test_solver_stop_gpu import _at, _replay, _same_bits

pytestmark = pytest.mark.gpu
P = on.DEFAULT_PARAMS

DT, ATOL, T = 8e-4, 1e-3, 16
EPS = (DT / P['tau'][0], DT / P['tau'][1])
WAVE_ROWS = 56
ROWS = {200: [0, 55, 56, 111, 112, 167, 168, 199], 146: [0, 55, 56, 111, 112, 145], 104: [0, 55, 56, 103], 32: [0, 31]}
VARIANTS = [3, 4, None]
KS = [4, 9]
EXT_BOUND, NO_BOUND = 30.0, 100.0

Case = collections.namedtuple('Case', 'kind M variant j k max_iter')


def _cases():
    out = []
    for M, rows in ROWS.items():
        for v in VARIANTS:
            out += [Case(kind, M, v, j, k, T) for kind in ('last', 'bound', 'mirror') for j in rows for k in KS]
            out += [Case('last', M, v, j, mi - 1, mi) for j in (rows[0], rows[-1]) for mi in (T, T - 1)]
            out += [Case('still', M, v, 0, 0, T)]
    return out


CASES = _cases()
IDS = ['{}-2N{}-v{}-row{}-k{}-T{}'.format(*c) for c in CASES]


def _eps(M, row):
    return EPS[0] if row < M // 2 else EPS[1]


def _partner(M, j):
    """A row of another wave than row j's (the wave behind it, cyclically); with one wave, another row."""
    waves = -(-M // WAVE_ROWS)
    if waves == 1:
        return (j + 7) % M
    return min(((j // WAVE_ROWS + 1) % waves) * WAVE_ROWS + 3, M - 1)


Design = collections.namedtuple('Design', 'io_type ext offsets start stop_at code steps partner partner_last')


def _design(c):
    """Inputs and the designed outcome of a case.  `offsets`: {row: d0} added to the fixed point; `start`: {row: r0} that
    replaces it (the rate-bound row)."""
    M = c.M
    ext = 4.0 + 8.0 * np.arange(M) / (M - 1)
    if c.kind == 'still':
        return Design('asym_tanh', ext, {}, {}, None, 0, 1, None, None)
    p = _partner(M, c.j)
    assert p != c.j and (M <= WAVE_ROWS or p // WAVE_ROWS != c.j // WAVE_ROWS)

    def d0(row, last):            # last moving step `last`
        e = _eps(M, row)
        return ATOL / (e * (1 - e) ** (last - 0.5))

    if c.kind == 'bound':
        ext[c.j] = EXT_BOUND
        e = _eps(M, c.j)
        f = P['k'] * EXT_BOUND ** P['n']
        stop_at = f - 0.75 * f * (1 - e) ** (c.k - 0.5)
        assert stop_at > 6.5 and 0.75 * f * (1 - e) ** (c.k - 0.5) * (1 - np.sqrt(1 - e)) > 0.03
        return Design('asym_power', ext, {p: d0(p, c.k + 3)}, {c.j: f / 4}, stop_at, 2, c.k, p, c.k + 3)
    io_type, stop_at = ('asym_power', NO_BOUND) if c.kind == 'mirror' else ('asym_tanh', None)
    return Design(io_type, ext, {c.j: d0(c.j, c.k), p: d0(p, c.k - 2)}, {}, stop_at, 0, c.k + 1, p, c.k - 2)


def _start(fixed, d):
    r0 = np.array(fixed, dtype=np.float64)
    for row, off in d.offsets.items():
        r0[row] += off
    for row, val in d.start.items():
        r0[row] = val
    return r0


def _oracle(oracle_lib, c, d, r0):
    hard = dict(hard=d.stop_at) if d.stop_at is not None else {}
    _, codes, steps = _oracle_batch(oracle_lib, np.zeros((1, c.M, c.M)), d.ext[None], d.io_type, c.max_iter, ATOL, dt=DT,
                                    r0=r0[None, None], **hard)
    return int(codes[0, 0]), int(steps[0, 0])


_ORACLE_FIXED = {}


def _oracle_fixed(oracle_lib, d):
    """The fp64 oracle's fixed point for W = 0: 800 steps from r = 0, (1 - eps_E)^800 = 1e-18."""
    key = (d.io_type, d.ext.tobytes())
    if key not in _ORACLE_FIXED:
        M = d.ext.size
        free = dict(hard=np.inf) if d.io_type == 'asym_power' else {}
        _ORACLE_FIXED[key] = _oracle_batch(oracle_lib, np.zeros((1, M, M)), d.ext[None], d.io_type, 800, 0.0, dt=DT, **free)[0][0, 0]
    return _ORACLE_FIXED[key]


_DEVICE = {}
_KERNEL_FIXED = {}


def _solve(c, d, r0, **kw):
    import torch
    from tc_gan_amd import ssnode
    if c.M not in _DEVICE:
        _DEVICE[c.M] = torch.zeros((1, c.M, c.M), device='cuda', dtype=torch.float32)
    opts = dict(dt=DT, io_type=d.io_type, dtype='float32', variant=c.variant, want_prev=True, return_torch=True)
    if d.io_type == 'asym_power':
        opts['rate_stop_at'] = np.inf
    opts.update(kw)
    ext = torch.as_tensor(d.ext[None], dtype=torch.float32).cuda()
    return ssnode.fixed_points_batch(_DEVICE[c.M], ext, P['k'], P['n'], r0=r0, **opts)


def _kernel_fixed(c, d):
    """The kernel's own fixed point: 1000 steps from r = 0, (1 - eps_E)^1000 = 3e-23 of the way left."""
    import torch
    key = (c.M, c.variant, d.io_type, d.ext.tobytes())
    if key not in _KERNEL_FIXED:
        res = _solve(c, d, torch.zeros((1, 1, c.M), device='cuda', dtype=torch.float32), max_iter=1000, atol=0.0)
        _KERNEL_FIXED[key] = res.x.cpu().numpy()[0, 0]
    return _KERNEL_FIXED[key]


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_one_wave_decides_the_verdict(oracle_lib, c):
    import torch
    d = _design(c)
    # ---- on the CPU, before the kernel is asked: the design gives the outcome it is meant to give ----
    assert _oracle(oracle_lib, c, d, _start(_oracle_fixed(oracle_lib, d), d)) == (d.code, d.steps)

    # ---- the kernel's own trajectory: chained one-step calls from its fixed point plus the offsets ----
    r0 = _start(_kernel_fixed(c, d), d).astype(np.float32)
    state = torch.as_tensor(r0[None, None]).cuda()
    chain = [state]
    for _ in range(T):
        chain.append(_solve(c, d, chain[-1], max_iter=1, atol=0.0).x)
    traj = torch.stack(chain).cpu().numpy()                                   # (T + 1, 1, 1, M)
    codes, steps = _replay(traj, ATOL, d.stop_at, c.max_iter)
    code, nsteps = int(codes[0, 0]), int(steps[0, 0])
    moving = np.abs(traj[1:, 0, 0] - traj[:-1, 0, 0]) >= np.float32(ATOL)     # [m - 1]: step m
    print('{}: replayed code {} steps {}; rows moving per step {}'.format(IDS[CASES.index(c)], code, nsteps,
                                                                         moving[:c.max_iter].sum(axis=1).tolist()))
    assert (code, nsteps) == (d.code, d.steps)
    if c.kind == 'still':
        assert not moving.any()
    elif c.kind == 'bound':
        beyond = traj[1:, 0, 0] >= np.float32(d.stop_at)
        assert np.flatnonzero(beyond[nsteps - 1]).tolist() == [c.j] and not beyond[:nsteps - 1].any()
        assert moving[nsteps - 1, d.partner] and moving[nsteps - 1, c.j]      # another wave still reports "moving"
    else:
        # the step before the stop belongs to row j alone; the partner's wave fell still at the designed step
        assert np.flatnonzero(moving[nsteps - 2]).tolist() == [c.j] and not moving[nsteps - 1].any()
        assert moving[d.partner_last - 1, d.partner] and not moving[d.partner_last:, d.partner].any()
        assert sorted(np.flatnonzero(moving[:c.max_iter].any(axis=0)).tolist()) == sorted([c.j, d.partner])
    ocode, osteps = _oracle(oracle_lib, c, d, r0.astype(np.float64))
    assert ocode == code and abs(osteps - nsteps) <= 1, (ocode, osteps)

    # ---- the stopped run ----
    kw = dict(rate_stop_at=d.stop_at) if d.stop_at is not None else {}
    res = _solve(c, d, state, max_iter=c.max_iter, atol=ATOL, **kw)
    got_codes, got_steps = res.codes.cpu().numpy(), res.steps.cpu().numpy()
    np.testing.assert_array_equal(got_codes, codes, err_msg='codes (replayed steps {})'.format(nsteps))
    np.testing.assert_array_equal(got_steps, steps, err_msg='steps')
    _same_bits(res.x.cpu().numpy(), _at(traj, steps), 'x against traj[steps]')
    _same_bits(res.x_prev.cpu().numpy(), _at(traj, steps - 1), 'x_prev against traj[steps - 1]')

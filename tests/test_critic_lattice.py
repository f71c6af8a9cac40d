"""oracle/critic_lattice.py on the CPU: the lattice cases ARE lattice cases (every GEMM operand a bf16 number, every partial sum
an fp32 number), the hand-written chains equal torch autograd on oracle/gan_torch.py, rounding the operands to bf16 changes
nothing, the cases are not trivial (units active and inactive, dense gradients, K tails that carry weight, a second chain that
is not zero), and the kernel defects the GPU module (tests/test_critic_lattice_gpu.py) is meant to see change the expected
values."""
import functools

import numpy as np
import pytest
import torch

from oracle import critic_lattice as cl
from oracle import gan_torch as og

CASES = [(name, family) for name in cl.CASES for family in 'AB']
IDS = ['%s-%s' % c for c in CASES]
EXACT = ('D', 'stats', 'flat', 'gx', 'gx_mean', 'accuracy')


@functools.lru_cache(maxsize=None)
def _case(name, family):
    return cl.make_case(name, family)


@functools.lru_cache(maxsize=None)
def _expected(name, family):
    return cl.evaluate(_case(name, family))


def _changed(a, b):
    return int((np.asarray(a) != np.asarray(b)).sum())


def test_round_bf16_modes():
    x = np.array([1.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -9, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 1 + 2.0 ** -7, 0.0,
                  3 + 2.0 ** -7, 1 + 2.0 ** -8 + 2.0 ** -20], dtype=np.float32)
    u = 2.0 ** -7
    np.testing.assert_array_equal(cl.round_bf16(x, 'rne'), [1, 1, 1 + 2 * u, 1, -1, -(1 + 2 * u), 1 + u, 0, 3, 1 + u])
    np.testing.assert_array_equal(cl.round_bf16(x, 'trunc'), [1, 1, 1 + u, 1, -1, -(1 + u), 1 + u, 0, 3, 1])
    np.testing.assert_array_equal(cl.round_bf16(x, 'away'), [1, 1 + u, 1 + 2 * u, 1 + u, -(1 + u), -(1 + 2 * u), 1 + u, 0, 3 + 2 * u, 1 + u])
    # against torch's own conversion (round to nearest even) on random fp32 numbers
    r = np.random.RandomState(0).randn(10000).astype(np.float32) * 100
    np.testing.assert_array_equal(cl.round_bf16(r), torch.from_numpy(r).to(torch.bfloat16).to(torch.float32).numpy())
    assert cl.is_bf16(cl.round_bf16(r)) and not cl.is_bf16(r)
    assert cl.lsb(np.array([0.0, 6.0, -0.75, 40.0])) == 0.25


@pytest.mark.parametrize('name,family', CASES, ids=IDS)
def test_case_is_on_the_lattice(name, family):
    bits, names = cl.check_lattice(_case(name, family))
    L = len(cl.CASES[name]['layers'])
    # every GEMM of the update, of the forward and of the generator side's input gradient went through the check
    want = 3 * (L + 1) + (L - 1) + 2 * L + (L + 1) + (2 * L if family == 'B' else 0)
    assert len(names) == want and len(set(names)) == want, names
    assert bits < 24


@pytest.mark.parametrize('name,family', CASES, ids=IDS)
def test_hand_written_chains_equal_autograd(name, family):
    case, want = _case(name, family), _expected(name, family)
    kw = dict(nonlinearity=case['nonlinearity'])
    ps = [og.t64(p).clone().requires_grad_(True) for p in case['params']]

    def cond(c):
        if c is None:
            return None
        c = np.array(c, dtype=np.float64)
        if case['hide_cell_type']:
            c[:, 2] = 0.0                              # cwgan.py:178-187
        return og.t64(c)
    tg, td, tp = (og.t64(case[k]) for k in ('xg', 'xd', 'xp'))
    cg, cd, cp = (cond(case[k]) for k in ('cg', 'cd', 'cp'))
    loss = og.critic_loss(ps, tg, td, tp, cg, cd, cp, case['lmd'], **kw)
    flat = np.concatenate([g.numpy().ravel() for g in torch.autograd.grad(loss, ps)])
    scale = max(1.0, np.abs(flat).max())
    np.testing.assert_allclose(want['flat'], flat, rtol=1e-12, atol=1e-12 * scale)
    np.testing.assert_allclose(want['stats'][3], float(loss.detach()), rtol=1e-12)
    with torch.no_grad():
        dg, dd = og.critic_forward(ps, tg, cg, **kw)[:, 0].numpy(), og.critic_forward(ps, td, cd, **kw)[:, 0].numpy()
    np.testing.assert_allclose(want['D'], np.concatenate([dg, dd]), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(want['stats'][:2], [dg.mean(), dd.mean()], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(want['accuracy'], dg.mean() - dd.mean(), rtol=1e-12, atol=1e-12)
    x = tg.clone().requires_grad_(True)
    gx, = torch.autograd.grad(-og.critic_forward(ps, x, cg, **kw).mean(), x)
    np.testing.assert_allclose(want['gx'], gx.numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(want['gx_mean'], dg.mean(), rtol=1e-12, atol=1e-12)
    # the penalty itself: mean (||g|| - 1)^2 of autograd's input gradient
    xp = tp.clone().requires_grad_(True)
    g, = torch.autograd.grad(og.critic_forward(ps, xp, cp, **kw).sum(), xp)
    np.testing.assert_allclose(want['stats'][2], float(((g.norm(2, dim=1) - 1) ** 2).mean()), rtol=1e-12)


@pytest.mark.parametrize('name,family', CASES, ids=IDS)
def test_rounding_the_operands_changes_nothing(name, family):
    want, got = _expected(name, family), cl.evaluate(_case(name, family), rounding='rne')
    for key in EXACT:
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    # ... and every expected value is an fp32 number: the GPU can return it
    for key in ('D', 'flat', 'gx', 'accuracy', 'gx_mean'):
        a = np.asarray(want[key])
        np.testing.assert_array_equal(a.astype(np.float32).astype(np.float64), a, err_msg=key)
    np.testing.assert_array_equal(want['stats'][:2].astype(np.float32), want['stats'][:2])


@pytest.mark.parametrize('name,family', CASES, ids=IDS)
def test_case_is_not_trivial(name, family):
    case, out = _case(name, family), _expected(name, family)
    linear = case['nonlinearity'] == 'linear'
    for a in out['active']:
        assert linear or 0.2 <= a <= 0.8, out['active']
    for (kind, sl), p in zip(cl.tensor_slices(case), case['params']):
        # (a linear critic's bias gradient is the chain's value times the sum of the upstream: exactly zero)
        if not (linear and kind == 'b'):
            assert (out['flat'][sl] != 0).mean() >= 0.25, (kind, sl, (out['flat'][sl] != 0).mean())
    W = case['params'][0:-1:2]
    for l, w in enumerate(W):
        # a contraction over 72 or 132 units: the K tail beyond the last whole tile of 64 carries weight
        if w.shape[0] in (72, 132):
            assert (w[-16:] != 0).any(), ('forward', l)
        if w.shape[1] in (72, 132):
            assert (w[:, -16:] != 0).any(), ('backward', l)
    if len(case['params'][-1]) in (72, 132):
        assert (np.asarray(case['params'][-1])[-16:] != 0).any()
    if family == 'B':
        for e in out['e']:
            assert (e != 0).mean() >= 0.04
        # (a linear critic's input gradient is the same for every row)
        assert linear or len(np.unique(out['norms'])) >= 3, np.unique(out['norms'])
        assert out['stats'][2] > 0
    # rows that differ from each other
    assert len(np.unique(out['D'])) >= 8 and len(np.unique(out['gx'], axis=0)) >= (1 if linear else 4)


MUTATIONS = [
    ('tails', 'A', ('drop_tail', 'fwd2w'), 'both'),       # K = 72: the 8 beyond a tile of 64, and 8 more
    ('tails', 'A', ('drop_tail', 'fwd3w'), 'both'),       # K = 100
    ('tails', 'A', ('drop_tail', 'outw'), 'D'),         # K = 132: the output GEMM (D alone depends on it)
    ('tails', 'A', ('drop_tail', 'bwd3w'), 'flat'),      # K = 132, backward chain
    ('tails', 'A', ('drop_tail', 'gW2w'), 'flat'),       # K = the 192 stacked rows: a weight gradient that loses its last rows
    ('tails', 'B', ('drop_tail', 'gW1p'), 'flat'),       # ... and one of the penalty half
    ('tails', 'B', ('drop_tail', 'e2'), 'flat'),
    ('c3', 'B', ('drop_tail', 'gW3w'), 'flat'),          # the last split-K slice
    ('c3', 'B', ('drop_tail', 'fwd2p'), 'flat'),
    ('c3', 'A', ('mask_shift', 2), 'flat'), ('c3', 'B', ('mask_shift', 3), 'flat'), ('ragged', 'B', ('mask_shift', 1), 'flat'),
    ('odd', 'A', ('mask_shift', 2), 'flat'),
    ('c3', 'A', ('swap_n', None), 'flat'), ('ragged', 'B', ('swap_n', None), 'flat'), ('one', 'A', ('swap_n', None), 'flat'),
    ('c3', 'A', ('transpose', 2), 'flat'), ('c3', 'B', ('transpose', 3), 'flat'), ('c3par', 'B', ('transpose', 2), 'flat'),
]


@pytest.mark.parametrize('name,family,mutation,moves', MUTATIONS, ids=['%s-%s-%s-%s' % (m[0], m[1], m[2][0], m[2][1]) for m in MUTATIONS])
def test_kernel_defects_change_the_expected_values(name, family, mutation, moves):
    """A K tail dropped in one GEMM, slopes taken from the neighbouring row, 1/ng and 1/nd swapped, a weight read the wrong way
    round: each moves more than one element of the flat gradient (and of D, where the forward is hit) -- the exact comparison of
    the GPU module cannot miss it."""
    want = _expected(name, family)
    got = cl.evaluate(_case(name, family), rounding='rne', mutate=mutation)
    for key in ('flat', 'D'):
        if moves in (key, 'both'):
            assert _changed(got[key], want[key]) > 1, (mutation, key)
        else:
            np.testing.assert_array_equal(got[key], want[key])


def test_tie_case_tells_the_rounding_modes_apart():
    case = cl.make_tie_case()
    d = {}
    for mode in ('rne', 'trunc', 'away'):
        d[mode], ties = cl.tie_forward(case, mode)
        if mode == 'rne':
            # every x and every non-zero weight is a tie; so is a good part of h_1 under the kernels' own rounding
            assert ties['x'] == 1.0 and ties['W'] == 1.0 / cl.NX and ties['h'] >= 0.25, ties
        # whatever the mode, the rounded operands are few-bit numbers: D is an fp32 number
        np.testing.assert_array_equal(d[mode].astype(np.float32).astype(np.float64), d[mode])
    exact, _ = cl.tie_forward(case, None)
    for a, b in (('rne', 'trunc'), ('rne', 'away'), ('trunc', 'away')):
        assert _changed(d[a], d[b]) > len(d[a]) // 2, (a, b)
    assert _changed(d['rne'], exact) > len(exact) // 2

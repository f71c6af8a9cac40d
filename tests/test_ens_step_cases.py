"""No GPU: the cases of oracle/ens_step_cases.py -- the restatements against independent forms (math.fsum, power-of-two probes of
the one-workgroup sum, torch fp64 autograd of the moment loss, gan_torch's update rules with zero regularisation, central
differences of the regularised loss), the conditions of every case, and the sensitivity of the checks of
tests/test_ens_step_gpu.py to a list of defects."""
import math

import numpy as np
import pytest
import torch

from oracle import ens_step_cases as ec
from oracle import gan_torch as og
from oracle import gen_step_cases as gc

TINY = 2.0 ** -53


def _id(c):
    return '-'.join(str(v) for v in c)


# ------------------------------------------------------------------ restatements against independent forms
def test_block_sum_adds_in_the_stated_order_and_is_within_its_bound_of_fsum():
    """Powers of two more than 53 bits apart show who is added to whom (1 + 2^-53 rounds back to 1)."""
    assert ec.block_sum([]) == 0 and ec.block_sum([3.0]) == 3 and ec.block_sum(np.ones(1000)) == 1000
    x = np.zeros(513)
    x[[0, 256, 512]] = [1, TINY, TINY]                 # thread 0 adds in the order of the index: (1 + tiny) + tiny
    assert ec.block_sum(x) == 1
    x[[0, 256, 512]] = [TINY, TINY, 1]                 # (tiny + tiny) + 1
    assert ec.block_sum(x) == 1 + 2 * TINY
    x = np.zeros(256)
    x[[0, 1, 129]] = [1, TINY, TINY]                   # off = 128 joins threads 1 and 129 before off = 1 joins 0 and 1
    assert ec.block_sum(x) == 1 + 2 * TINY
    x = np.zeros(256)
    x[[0, 128, 129]] = [1, TINY, TINY]                 # off = 128: thread 0 takes thread 128 alone
    assert ec.block_sum(x) == 1
    assert ec.block_sum(x) == float(gc.tree256(gc.strided_partials(x, 1))[0])
    rs = np.random.RandomState(0)
    for n in (1, 255, 256, 257, 513, 1542):
        v = rs.randn(n) * 10.0 ** rs.uniform(-3, 3, n)
        assert abs(ec.block_sum(v) - math.fsum(v)) <= ec.depth(n) * TINY * math.fsum(np.abs(v))
    assert ec.depth(256) == 9 and ec.depth(257) == 10 and ec.depth(513) == 11


@pytest.mark.parametrize('c', [ec.MOM_CASES[4], ec.MOM_CASES[10], ec.MOM_CASES[-2], ec.MOM_CASES[-1]], ids=_id)
def test_moment_oracle_is_the_autograd_of_the_moment_loss(c):
    """m, s and gx of the oracle against torch fp64: gx = d L0 / d x of L0 = mean(w (moments - data moments)^2) per member."""
    x, o = ec.mom_inputs(c), ec.mom_oracle(c)
    for k, sl in enumerate(ec._rows(c.K, c.B)):
        xt = torch.tensor(x['x'][sl], dtype=torch.float64, requires_grad=True)
        m = xt.mean(dim=0)
        s = ((xt - m) ** 2).mean(dim=0)                                      # (the centred form: no cancellation)
        dm, w = torch.tensor(x['dm'][k]), torch.tensor(x['w'][k])
        L0 = (w[0] * (m - dm[0]) ** 2 + w[1] * (s - dm[1]) ** 2).sum() / (2.0 * c.D)
        gx, = torch.autograd.grad(L0, xt)
        assert (np.abs(o['m'][k] - m.detach().numpy()) <= o['allowed_m'][k]).all()
        assert (np.abs(o['s'][k] - s.detach().numpy()) <= o['allowed_s'][k]).all()
        assert (np.abs(o['gx'][sl] - gx.numpy()) <= o['allowed_gx'][sl]).all()
        if c.kind == 'free':
            assert ec.moment_loss(x['x'][sl], x['dm'][k], x['w'][k]) == pytest.approx(L0.item(), rel=1e-9)


def test_apply_step_reg_without_regularisation_is_gan_torch_and_its_terms_are_the_loss_derivatives():
    rs = np.random.RandomState(5)
    p, g = rs.uniform(-1, 1, 9), rs.randn(9)
    p[3] = 0.0
    h = gc.APPLY_HYPER
    zero = (0.0, 0.0, 0.0, 0.0)
    for rule, step, kw in (('adam', og.adam_step, dict(beta1=h['beta1'], beta2=h['beta2'], eps=h['epsilon_adam'])),
                           ('rmsprop', og.rmsprop_step, dict(rho=h['rho'], eps=h['epsilon_rmsprop'])), ('sgd', og.sgd_step, {})):
        sa, sb, q, r = {}, {}, p, p
        for _ in range(2):                                                  # two steps: the moments carry
            u, q, g2 = ec.apply_step_reg(rule, q, g, sa, 0.03, zero, -0.9, 0.9)
            r = np.clip(step(r, g, sb, 0.03, **kw), -0.9, 0.9)
            assert np.array_equal(q, r) and np.array_equal(g2, g)
        assert all(np.array_equal(sa[k], sb[k]) for k in sb)
    # the penalties are the derivative of l2 p^2 + l1 |p| (central differences away from 0; 0 at p = 0 for l1)
    l2p, l1p, l2d, l1d, lr = 0.07, 0.03, 0.4, 0.2, 0.05
    _, _, g2 = ec.apply_step_reg('sgd', p, g, {}, lr, (l2p, l1p, 0.0, 0.0))
    loss = lambda v: l2p * v * v + l1p * np.abs(v)
    d = 1e-6
    nz = p != 0
    np.testing.assert_allclose((g2 - g)[nz], ((loss(p + d) - loss(p - d)) / (2 * d))[nz], rtol=1e-8, atol=1e-9)
    assert (g2 - g)[3] == 0
    # the decays act on the old value, after the rule: sgd's update moves by -lr (l2_decay p0 + l1_decay sign p0)
    u0, _, _ = ec.apply_step_reg('sgd', p, g, {}, lr, (l2p, l1p, 0.0, 0.0))
    u1, _, _ = ec.apply_step_reg('sgd', p, g, {}, lr, (l2p, l1p, l2d, l1d))
    np.testing.assert_allclose(u1 - u0, -lr * (l2d * p + l1d * np.sign(p)), rtol=0, atol=1e-15)
    un, _, _ = ec.apply_step_reg('sgd', p, g, {}, lr, (l2p, l1p, l2d, l1d), defect='decay-from-new-value')
    np.testing.assert_allclose(un - u0, -lr * (l2d * u0 + l1d * np.sign(u0)), rtol=0, atol=1e-15)
    assert ec.adam_a_t(0.05, 1) == pytest.approx(0.05 * math.sqrt(1 - 0.999) / (1 - 0.9))


def test_gen_grads_restated_layout_split_and_loss():
    """grads = [dV (nv), dJ (4), dD (4), dS (4)] per member: a part that is non-zero in one (pq, t) lands in grads[nv + 4 t + pq]
    of its member alone; nv = 2 splits at m = N and nv = 1 is the sum; the loss is formed from the ROUNDED penalties."""
    c = ec.EnsGG(ec.ENTRIES[3], 2, 2, 2, 1, 4, 0)
    base = dict(scale_dyn=0.125, scale_rate=0.125, dyn=np.full((4, 1, 4), 0.1, dtype='float32').astype('float64'),
                rate=np.ones((4, 1, 4)), costs=np.array([[1.0, 2.0], [4.0, 8.0]]), l0=np.array([0.5, 0.25]),
                g_ext=np.arange(1.0, 17.0).reshape(4, 1, 4), ext_base=np.ones((4, 1, 4)), zin=np.ones((4, 4)))
    for q in range(4):
        for t in range(3):
            parts = np.zeros((4, 4, 3))
            parts[2:, q, t] = [1.5, 2.0]                                     # member 1
            out = ec.gen_grads_in_order(c, dict(base, parts=parts))
            want = np.zeros((2, 14))
            want[0, :2], want[1, :2] = [1 + 2 + 5 + 6, 3 + 4 + 7 + 8], [9 + 10 + 13 + 14, 11 + 12 + 15 + 16]
            want[1, 2 + 4 * t + q] = 3.5
            assert np.array_equal(out['grads'], want.astype('float32'))
    one = ec.gen_grads_in_order(c._replace(nv=1), dict(base, parts=np.zeros((4, 4, 3))))
    assert one['grads'][:, 0].tolist() == [36.0, 100.0] and one['grads'].shape == (2, 13)
    fd = float(np.float32(np.float64(np.float32(0.1)) * 8 * 0.125))
    assert out['dyn'].tolist() == [fd, fd] and out['rate'].tolist() == [1.0, 1.0]
    assert out['loss'].tolist() == [0.5 + 1.0 * fd + 2.0, 0.25 + 4.0 * fd + 8.0] and out['L0'].tolist() == [0.5, 0.25]


def test_jds16_and_the_member_tables():
    for k in range(3):
        J, D, S = ec.member_jds(k)
        assert all(len(set(a.flat)) == 4 and np.array_equal(a, gc._f32(a)) for a in (J, D, S))
        p = ec.jds16(J, D, S).astype('float64')
        s = S.reshape(4)
        assert p.shape == (16,) and np.array_equal(p[:4], J.reshape(4)) and np.array_equal(p[4:8], D.reshape(4))
        np.testing.assert_allclose(p[8:12], 1 / (2 * s * s), rtol=2 * ec.U)
        np.testing.assert_allclose(p[12:], 1 / s ** 3, rtol=3 * ec.U)
    for a, b in ((0, 1), (1, 2), (0, 2)):
        assert all((x != y).all() for x, y in zip(ec.member_jds(a), ec.member_jds(b)))


def test_ens_gain_is_the_members_two_rounding_gain():
    c = ec.STIM_CASES[1]
    x = ec.ens_stim_inputs(c)
    for k, sl in enumerate(ec._rows(c.K, c.B)):
        assert np.array_equal(x['gain'][sl], gc.hetero_gain(x['v'][k], x['zin'][sl], c.N).astype('float64'))
    vm = np.repeat(np.repeat(x['v'], c.N, axis=1), c.B, axis=0)
    one = (1.0 + vm * x['zin']).astype('float32')
    assert np.array_equal(ec.fused_gain(x['v'], x['zin'], c.K, c.B, c.N), one)


# ------------------------------------------------------------------ the conditions of the cases
def test_the_case_tables_cover_what_they_claim():
    assert len(ec.ENTRIES) == 6
    mom = ec.MOM_CASES
    assert {(c.B, c.D) for c in mom if c.K == 3 and c.kind == 'free'} == {(B, D) for B in (1, 255, 256, 257, 513) for D in (1, 7, 24)}
    assert any(c.kind == 'offset' and c.B > 256 for c in mom) and sum(c.K == 1 for c in mom) == 1
    jd = ec.JDS_CASES
    assert {(c.N, c.B, c.gw) for c in jd if c.K == 3} == {(N, B, g) for N in (1, 16, 17, 52) for B in (1, 3) for g in ('free', 'onehot')}
    assert [N * N for N in ec.JDS_N] == [1, 256, 289, 2704] and sum(c.K == 1 for c in jd) == 1
    gg = ec.GG_CASES
    assert [B * NB * M for B, NB, M in ec.GG_SHAPES] == [30, 256, 270, 1542] and 256 % 18 != 0
    for entry, Ds in ((ec.ENTRIES[2], {1, 24, 257}), (ec.ENTRIES[3], {0})):
        mine = [c for c in gg if c.entry == entry and c.K == 3]
        assert {(c.nv, (c.B, c.NB, c.M)) for c in mine} == {(nv, s) for nv in (0, 1, 2) for s in ec.GG_SHAPES}
        for nv in (0, 1, 2):
            assert {c.D for c in mine if c.nv == nv} == Ds
        assert sum(c.K == 1 for c in gg if c.entry == entry) == 1
    ap = ec.APPLY_CASES
    assert {(c.K, c.P, c.rule) for c in ap if c.K <= 3} == {(K, P, r) for K in (1, 3) for P in (12, 13, 14) for r in gc.RULES}
    big = [c for c in ap if c.K > 3]
    assert len(big) == 1 and big[0].K * big[0].P == 16900 > ec.APPLY_SWEEP == 16384 and all(c.K * c.P < 256 for c in ap if c.K <= 3)
    assert gc.APPLY_RTOL <= ec.TOLERANCE_CAP
    st = ec.STIM_CASES
    assert [(c.K, c.B, c.NB, c.N) for c in st] == [(3, 2, 4, 1), (3, 2, 4, 10), (8, 33, 8, 125), (1, 2, 4, 10)]
    assert 8 * 33 * 8 * 250 == 528000 > ec.STIM_SWEEP == 524288 < 8 * 64 * 8 * 200                # (a sweep shape: K 8, B 64, NB 8, N 100)
    assert all(c.K * c.B * c.NB * 2 * c.N < 256 * 8 for c in st if c.N <= 10)


@pytest.mark.parametrize('c', ec.MOM_CASES, ids=_id)
def test_moments_case_conditions(c):
    x, o = ec.mom_inputs(c), ec.mom_oracle(c)
    assert np.array_equal(x['x'], gc._f32(x['x'])) and x['x'].shape == (c.K * c.B, c.D)
    sq = x['x'] * x['x']
    assert np.array_equal(sq, (x['x'].astype(np.longdouble) ** 2).astype('float64'))        # the fp64 square is exact
    sums = ec.moment_sums_in_order(x['x'], c.K, c.B, c.D)
    m = sums[:, 0] / c.B
    s = sums[:, 1] / c.B - m * m
    assert (np.abs(m - o['m']) <= o['allowed_m']).all() and (np.abs(s - o['s']) <= o['allowed_s']).all()
    xm = x['x'].reshape(c.K, c.B, c.D)
    if c.K > 1:
        assert (np.abs(np.diff(o['m'], axis=0)) > 100 * o['allowed_m'][1:]).all()          # the members differ
    rel = o['allowed_gx'] / o['scale_gx']
    assert (o['scale_gx'] > 0).all() and 0 < rel.max() <= ec.TOLERANCE_CAP
    assert (np.abs(o['m'] - x['dm'][:, 0]) > 1e3 * o['allowed_m']).all() and (np.abs(o['s'] - x['dm'][:, 1]) > 1e3 * o['allowed_s']).all()
    if c.kind == 'offset':
        assert (np.abs(o['m']) > 1e3 * np.sqrt(o['s'])).all() and (o['allowed_s'] > 1e4 * ec.E * o['s']).all()
        assert xm.std(axis=1).min() > 50 * np.spacing(np.float32(100))
    r = ec.defect_ratio(ec.DEFECTS[0], c)
    assert (r is None) == (c.B <= 256) and (r is None or r >= ec.SENSITIVITY), r


@pytest.mark.parametrize('c', ec.JDS_CASES, ids=_id)
def test_jds_grad_case_conditions(c):
    x, res = ec.ens_jds_inputs(c), ec.ens_jds_oracle(c)
    nb = c.K * c.B
    assert len(res) == (1 if c.gw == 'free' else 12) and len(x['jds']) == c.K
    for k, o in enumerate(res):
        assert o['want'].shape == (nb, 4, 3) and 0 <= o['tol'] <= ec.TOLERANCE_CAP
        if c.gw == 'onehot':
            name, p, q, i, j = gc.onehot_places(c.N)[k]
            fed = np.zeros((nb, 4), dtype=bool)
            fed[k % nb, 2 * p + q] = True
            assert (o['want'][~fed] == 0).all() and (o['scale'][~fed] == 0).all() and (o['allowed'][~fed] == 0).all()
            assert (o['want'][fed][:, :2] != 0).all() and ((o['want'][fed][:, 2] != 0).all() == (i != j))
            assert np.count_nonzero(x['gW'][k]) == 1
    if c.gw == 'onehot':
        assert {(k % nb) // c.B for k in range(12)} == set(range(c.K))                      # every member is fed
    for kind in ec.DEFECTS[1:3]:
        r = ec.defect_ratio(kind, c)
        applies = c.N > 1 and (c.K > 1 or kind == ec.DEFECTS[2])
        assert (r is None) == (not applies) and (r is None or r >= ec.SENSITIVITY), (kind, r)


@pytest.mark.parametrize('c', ec.GG_CASES, ids=_id)
def test_gen_grads_case_conditions(c):
    x = ec.gg_inputs(c, 'exact')
    P = c.nv + 12
    if c.nv:
        assert set(np.abs(x['zin']).flat) == {1.0}
        for k in ('g_ext', 'ext_base'):
            mant, _ = np.frexp(x[k])
            assert np.array_equal(mant * 2 ** 12, np.round(mant * 2 ** 12))                 # at most 12 significant bits
        t = x['g_ext'] * x['ext_base'] * x['zin'][:, None, :]
        assert np.array_equal(t, (x['g_ext'].astype(np.longdouble) * x['ext_base'] * x['zin'][:, None, :]).astype('float64'))
    if c.D:
        L = np.longdouble
        for k in range(c.K):
            em, es = x['mom'][k, :c.D].astype(L) - x['dm'][k, 0], x['mom'][k, c.D:].astype(L) - x['dm'][k, 1]
            assert np.array_equal(em.astype('float64'), x['mom'][k, :c.D] - x['dm'][k, 0])
            for w, e in ((x['w'][k, 0], em), (x['w'][k, 1], es)):                           # w e e in 32 bits: exact
                assert np.array_equal((w.astype(L) * e * e).astype('float64').astype(L), w.astype(L) * e * e)
        assert (x['w'] > 0).all()
    fd = np.float32(0.123456789)
    for k in range(c.K):                                                                    # cost x rounded penalty: exact
        for cost in x['costs'][k]:
            assert np.longdouble(cost) * np.longdouble(fd) == np.longdouble(float(cost) * float(fd))
    if c.K > 1:
        assert len({tuple(r) for r in x['costs']}) == c.K
    o = ec.gen_grads_in_order(c, x)
    assert o['grads'].shape == (c.K, P) and np.isfinite(o['grads']).all() and np.isfinite(o['loss']).all()
    x = ec.gg_inputs(c, 'free')
    o, ex = ec.gen_grads_in_order(c, x), ec.gen_grads_exact(c, x)
    assert (np.abs(o['grads'] - ex['grads']) <= ex['grads_allowed']).all()
    assert (np.abs(o['L0'] - ex['L0']) <= ex['L0_allowed']).all()
    for k in ('dyn', 'rate'):
        assert (np.abs(o[k] - ex[k]) <= ec.U * np.abs(ex[k]) * (1 + 1e-6)).all()
    if c.K > 1:
        assert len(set(o['L0'])) == c.K and len(set(o['dyn'])) == c.K
    r = ec.defect_ratio(ec.DEFECTS[0], c)
    assert (r is None) == (c.B * c.NB * c.M <= 256 and c.B <= 256 and c.D <= 256) and (r is None or r >= ec.SENSITIVITY), r
    r = ec.defect_ratio(ec.DEFECTS[1], c)
    assert (r is None) == (c.K == 1) and (r is None or r >= ec.SENSITIVITY), r


@pytest.mark.parametrize('c', ec.APPLY_CASES, ids=_id)
def test_apply_case_conditions(c):
    x = ec.apply_inputs(c)
    tr = ec.apply_trace(c, x)
    n = c.K * c.P
    assert tr['margin'].min() >= ec.APPLY_MARGIN > 4 * ec.apply_tol(2.0)
    assert x['lo'][2] == x['hi'][2] and (np.delete(x['lo'], 2) < np.delete(x['hi'], 2)).all()
    distinct = min(len(set(x['lo'])), len(set(x['hi'])))                                    # they differ element by element
    assert distinct == n or (n > 256 and distinct > 0.999 * n)                              # (float32 draws: a few of 16 900 meet)
    assert (x['p0'] < 0).any() and (x['p0'] > 0).any() and (x['p0'].reshape(c.K, c.P)[:, 1] == 0).all()
    hyp = x['hyp']
    assert hyp.shape == (c.K, 5) and (hyp > 0).all() and len(set(hyp[:, 0])) == c.K and np.array_equal(hyp, gc._f32(hyp))
    assert len({np.float32(ec.adam_a_t(lr, 2)) for lr in hyp[:, 0]}) == c.K
    first = tr['steps'][0]['where']
    assert {-1, 0, 1} <= set(first) and (first == 0).sum() >= n // 3
    assert set(tr['steps'][1]['where']) >= {-1, 0}
    for s in tr['steps']:
        assert np.abs(s['p']).max() < 3.0
        clipped = s['where'] != 0
        assert np.array_equal(s['p'][clipped], np.where(s['where'] < 0, x['lo'], x['hi'])[clipped])
    if c.rule != 'sgd':
        assert (tr['steps'][0]['m'] != 0).all()                                             # the second step starts from moments
    for kind in ec.DEFECTS[4:8]:
        r = ec.defect_ratio(kind, c)
        assert (r is None) == (kind == ec.DEFECTS[7] and c.rule != 'rmsprop') and (r is None or r >= ec.SENSITIVITY), (kind, r)
    r = ec.defect_ratio(ec.DEFECTS[1], c)
    assert (r is None) == (c.K == 1) and (r is None or r >= ec.SENSITIVITY), r
    r = ec.defect_ratio(ec.DEFECTS[8], c)
    assert (r is None) == (n <= ec.APPLY_SWEEP) and (r is None or r >= ec.SENSITIVITY), r


@pytest.mark.parametrize('c', ec.STIM_CASES, ids=_id)
def test_stimulus_case_conditions(c):
    x, o = ec.ens_stim_inputs(c), ec.ens_stim_oracle(c)
    nb = c.K * c.B
    assert o['want'].shape == (nb, c.NB, 2 * c.N) and (o['want'] != 0).all() and 0 < o['tol'] <= ec.TOLERANCE_CAP
    assert x['v'].shape == (c.K, 2) and len(set(x['v'].flat)) == 2 * c.K
    assert (np.abs(x['zin']) < 1).all() and len(set(np.abs(x['zin']).flat)) > x['zin'].size // 2      # generic, not +-1
    r = ec.defect_ratio(ec.DEFECTS[1], c)
    assert (r is None) == (c.K == 1) and (r is None or r >= ec.SENSITIVITY), r
    assert ec.defect_ratio(ec.DEFECTS[3], c) >= ec.SENSITIVITY
    assert ec.defect_ratio(ec.DEFECTS[9], c) is True
    r = ec.defect_ratio(ec.DEFECTS[8], c)
    assert (r is None) == (o['want'].size <= ec.STIM_SWEEP) and (r is None or r >= ec.SENSITIVITY), r


def test_every_defect_applies_somewhere():
    every = [ec.MOM_CASES[-2], ec.JDS_CASES[4], ec.GG_CASES[-3], ec.APPLY_CASES[-1], ec.APPLY_CASES[-2], ec.STIM_CASES[2]]
    for kind in ec.DEFECTS:
        assert any(ec.defect_ratio(kind, c) is not None for c in every), kind

"""No GPU: the cases of oracle/gen_step_cases.py -- the restatements against independent checks (make_W, make_dW, central
differences, gan_torch.stimulus, power-of-two probes of the two summation orders), the conditions of every case, and the
sensitivity of the element-wise checks of tests/test_gen_step_gpu.py to a list of defects."""
import math

import numpy as np
import pytest

from oracle import gan_torch as og
from oracle import gen_step_cases as gc
from oracle import ss_grad_numpy as sg

TINY = 2.0 ** -53


def _id(c):
    return '-'.join(str(v) for v in c)


# ------------------------------------------------------------------ restatements against independent checks
@pytest.mark.parametrize('N,pset', [(1, 'four'), (2, 'wide'), (5, 'four'), (17, 'new'), (101, 'new')])
def test_build_w_restated_is_make_W(N, pset):
    J, D, S = gc.jds_set(pset, fp32=False)
    z = np.random.RandomState(N).rand(2, 2 * N, 2 * N)
    W = gc.build_w(z, J, D, S, N)[0]
    np.testing.assert_allclose(W, sg.make_W(z, J, D, S, N), rtol=1e-12, atol=0)        # (x reaches 800: the reciprocal's rounding, 800 x 2^-52)
    assert (W[:, :, :N] >= 0).all() and (W[:, :, N:] <= 0).all()


@pytest.mark.parametrize('N', [1, 5, 16])
def test_jds_grad_restated_is_make_dW_and_the_central_difference_of_make_W(N):
    """out[b][pq][t] summed over the draws is dL/dtheta_pq of L = sum gW W: against make_dW contracted with gW, and against
    central differences of make_W in every (p, q) and every one of J, D, S."""
    J, D, S = gc.jds_set('four', fp32=False)
    rs = np.random.RandomState(40 + N)
    z, gW = rs.rand(3, 2 * N, 2 * N), rs.randn(3, 2 * N, 2 * N)
    out = gc.jds_grad(gW, z, J, D, S, N)
    assert out.shape == (3, 4, 3)
    tot = out.sum(axis=0)
    for t, which in enumerate('JDS'):
        dW = sg.make_dW(which, z, J, D, S, N)                                           # (nz or 1, M, M, 2, 2)
        np.testing.assert_allclose(tot[:, t].reshape(2, 2), np.einsum('bij,bijpq->pq', gW, np.broadcast_to(dW, (3,) + dW.shape[1:])),
                                   rtol=1e-10, atol=1e-13)
        for p in range(2):
            for q in range(2):
                theta = dict(J=J.copy(), D=D.copy(), S=S.copy())
                h = 1e-6 * theta[which][p, q]
                theta[which][p, q] += h
                up = (gW * sg.make_W(z, theta['J'], theta['D'], theta['S'], N)).sum()
                theta[which][p, q] -= 2 * h
                dn = (gW * sg.make_W(z, theta['J'], theta['D'], theta['S'], N)).sum()
                scale = np.abs(gW).sum() * 1e-6 + abs(tot[2 * p + q, t])
                assert abs((up - dn) / (2 * h) - tot[2 * p + q, t]) <= 1e-5 * scale, (which, p, q)


@pytest.mark.parametrize('N,smooth', [(5, 0.03125), (101, 0.05), (102, 0.03125)])
def test_stimulus_restated_is_gan_torch_stimulus(N, smooth):
    rs = np.random.RandomState(N)
    bw, con = rs.choice([0, 0.0625, 0.25, 1.0], (3, 4)), rs.uniform(0, 40, (3, 4))
    want = og.stimulus(bw, con, smooth, N).numpy()
    np.testing.assert_allclose(gc.stimulus(bw, con, smooth, N), want, rtol=1e-12, atol=0)
    gain = 1 + rs.uniform(-0.5, 0.5, (3, 2 * N))
    np.testing.assert_allclose(gc.stimulus(bw, con, smooth, N, gain), want * gain[:, None, :], rtol=1e-12, atol=0)
    one = gc.stimulus(bw[:, :1], con[:, :1], smooth, 1)                                  # one site: x = -0.5, both populations
    assert one.shape == (3, 1, 2) and np.array_equal(one[..., 0], one[..., 1])


def test_hetero_gain_is_the_two_rounding_form_and_differs_from_one_rounding():
    rs = np.random.RandomState(3)
    v, z = rs.uniform(0.1, 0.5, 2).astype('float32'), rs.uniform(-1, 1, (64, 10)).astype('float32')
    g = gc.hetero_gain(v, z, 5)
    vm = np.repeat(v, 5)[None, :]
    assert g.dtype == np.float32 and np.array_equal(g, np.float32(1) + (vm * z).astype('float32'))
    fused = (1.0 + vm.astype('float64') * z.astype('float64')).astype('float32')         # one rounding, as a contracted fma
    assert (g != fused).any()
    assert np.array_equal(gc.hetero_gain(v[:1], z, 5), np.float32(1) + v[0] * z)
    assert np.array_equal(gc.hetero_gain(np.repeat(v, 5), z, 5), g)


def test_the_summation_orders_restated_add_in_the_stated_order():
    """Powers of two that differ by more than 53 bits show who is added to whom: 1 + 2^-53 rounds back to 1, so a small term
    survives only where it meets another small term first."""
    def pen(x):
        return gc.penalty_means_in_order(np.asarray(x, dtype='float64'), 1.0)[0]
    assert pen([]) == 0 and pen([3.0]) == 3 and pen(np.ones(70000)) == 70000
    assert math.isnan(gc.penalty_means_in_order(np.zeros(0), float('nan'))[0])
    assert gc.penalty_means_in_order(np.ones(5), 0.25)[0] == 1.25
    # one thread strides over the whole grid: n = 65 537 runs 256 workgroups, thread (0, 0) takes elements 0 and 65 536
    x = np.zeros(65537)
    x[[0, 65536, 128]] = [1, TINY, TINY]                                   # (1 + tiny) in thread 0, then + thread 128's tiny
    assert pen(x) == 1
    x[[0, 65536, 128]] = [TINY, TINY, 1]                                   # (tiny + tiny) in thread 0, then + 1
    assert pen(x) == 1 + 2 * TINY
    x = np.zeros(65536)                                                    # the same elements at n = 65 536: three workgroups/threads
    x[[0, 1, 129]] = [1, TINY, TINY]                                       # off = 128 joins threads 1 and 129 before off = 1
    assert pen(x) == 1 + 2 * TINY
    x[[0, 1, 129]] = [0, 0, 0]
    x[[0, 128, 129]] = [1, TINY, TINY]                                     # off = 128: thread 0 takes thread 128 alone
    assert pen(x) == 1
    # the workgroup partials: the same tree over the workgroup index
    x = np.zeros(65536)
    x[[0, 256, 129 * 256]] = [1, TINY, TINY]                               # workgroups 0, 1, 129: 1 and 129 meet first
    assert pen(x) == 1 + 2 * TINY
    x[[0, 256, 129 * 256]] = [0, 0, 0]
    x[[0, 128 * 256, 129 * 256]] = [1, TINY, TINY]
    assert pen(x) == 1
    x = np.zeros(512)                                                      # two workgroups
    x[[0, 256]] = [1, TINY]
    assert pen(x) == 1 and gc.penalty_means_in_order(x, 1.0)[1].tolist() == [1, TINY]
    # gen_grads: at most 128 workgroups; thread b % 256 adds part[b] in the order of b
    parts = np.zeros((513, 4, 3))
    parts[[0, 256, 512], 2, 1] = [1, TINY, TINY]
    args = dict(dmean=0.0, pens=None, dynamics_cost=0.0, rate_cost=0.0, nv=0)
    assert gc.gen_grads_in_order(parts, **args)[0][4 + 2] == 1
    g = np.zeros((1, 1, 2 * 128 * 256 + 2))
    g[0, 0, [0, 128 * 256, 1]] = [1, TINY, TINY]                           # thread (0, 0) takes elements 0 and 128 256 (population E)
    one = np.ones_like(g)
    out, wg = gc.gen_grads_in_order(np.zeros((1, 4, 3)), 0.0, None, 0.0, 0.0, 2, g, one, np.ones((1, g.shape[2])))
    assert wg.shape == (128, 2) and wg[0, 0] == 1 and wg[0, 1] == 0 and out[0] == 1 and out[1] == 0


def test_gen_grads_restated_layout_and_loss():
    """out = [dV (nv), dJ (4), dD (4), dS (4), loss]: a part that is non-zero in one (pq, t) lands in out[nv + 4 t + pq] alone, and
    nv = 1 is the sum of the two populations."""
    for nv in (0, 1, 2):
        for q in range(4):
            for t in range(3):
                parts = np.zeros((2, 4, 3))
                parts[:, q, t] = [1.5, 2.0]
                out = gc.gen_grads_in_order(parts, 0.0, None, 1.0, 1.0, nv, *(np.zeros((2, 1, 4)),) * 2 + (np.zeros((2, 4)),) if nv else ())[0]
                want = np.zeros(nv + 13)
                want[nv + 4 * t + q] = 3.5
                assert np.array_equal(out, want.astype('float32'))
    g = np.arange(1.0, 9.0).reshape(1, 2, 4)
    args = (np.zeros((1, 4, 3)), 2.0, np.array([0.5, 0.25]), 4.0, 8.0)
    two = gc.gen_grads_in_order(*args, 2, g, np.ones_like(g), np.ones((1, 4)))[0]
    one = gc.gen_grads_in_order(*args, 1, g, np.ones_like(g), np.ones((1, 4)))[0]
    assert two[0] == 1 + 2 + 5 + 6 and two[1] == 3 + 4 + 7 + 8 and one[0] == 36 and one[13] == two[14] == -2 + 2 + 2
    sw = gc.gen_grads_in_order(np.arange(24.0).reshape(2, 4, 3), 0.0, None, 0.0, 0.0, 0, swap_jd=True)[0]
    ok = gc.gen_grads_in_order(np.arange(24.0).reshape(2, 4, 3), 0.0, None, 0.0, 0.0, 0)[0]
    assert np.array_equal(sw[0:4], ok[4:8]) and np.array_equal(sw[4:8], ok[0:4]) and np.array_equal(sw[8:], ok[8:])


# ------------------------------------------------------------------ the conditions of the cases
def test_the_case_tables_cover_what_they_claim():
    bw = gc.BUILD_W_CASES
    for entry in gc.ENTRIES[:3]:
        mine = [c for c in bw if c.entry == entry]
        assert {c.N for c in mine} >= {1, 2, 5, 101, 104}
        assert {(c.N, c.pset) for c in mine} >= {(101, 'new'), (104, 'new'), (101, 'wide'), (104, 'wide')}
        assert any(c.shift and (2 * c.N) % 4 == 0 for c in mine)
        assert any(gc.build_w_vec(c) == 4 and c.B * 4 * c.N * c.N > 4 * gc.BW_SWEEP for c in mine)
    for entry in gc.ENTRIES[:2]:
        assert any(gc.build_w_vec(c) == 1 and c.B * 4 * c.N * c.N > gc.BW_SWEEP for c in bw if c.entry == entry)
    for name in ('new', 'four', 'wide'):
        J, D, S = gc.jds_set(name)
        assert len(set(J.flat)) == len(set(D.flat)) == 4 and (len(set(S.flat)) == 4 or name == 'new')
    p = gc.jds_set('new', fp32=False)
    assert 1 / (2 * p[2].min() ** 2) == pytest.approx(800) and np.exp(-800.0) < 2.0 ** -126
    st = gc.STIM_CASES
    for entry in gc.ENTRIES[3:8]:
        mine = [c for c in st if c.entry == entry]
        assert {c.N for c in mine} >= {1, 5, 101} and {c.NB for c in mine} >= {1, 3} and all(c.B >= 2 for c in mine)
    assert {c.nv if c.nv <= 2 else 'M' for c in st if 'hetero' in c.entry and c.N > 1} == {1, 2, 'M'}
    assert any(c.B * c.NB * 2 * c.N > gc.STIM_SWEEP for c in st if c.entry == gc.ENTRIES[3])
    for entry in gc.ENTRIES[8:10]:
        mine = [c for c in gc.JDS_CASES if c.entry == entry]
        assert {c.N for c in mine} == {1, 15, 16, 17, 101} and all(c.B == 3 for c in mine) and {c.gw for c in mine} == {'free', 'onehot'}
    assert 15 * 15 < 256 == 16 * 16 < 17 * 17
    assert gc.PEN_N == (0, 1, 255, 256, 257, 65536, 65537)
    assert any(p.nsamp * p.NB < 256 and p.nsamp for p in gc.PROBE_CASES) and any(p.nsamp == 0 for p in gc.PROBE_CASES)
    assert any(p.nsamp * p.NB > 256 * min(max(-(-p.n // 256), 1), 256) for p in gc.PROBE_CASES)
    assert all(p.nsamp > p.models or p.nsamp <= 1 for p in gc.PROBE_CASES)                  # ids collide
    gg = gc.GG_CASES
    assert {c.nv for c in gg} == {0, 1, 2} and {c.B for c in gg} == {1, 2, 257} and {c.pens for c in gg} == {True, False}
    for nv in (1, 2):
        sizes = {c.B * c.NB * c.M for c in gg if c.nv == nv}
        assert min(sizes) < 256 and 128 * 256 in sizes and any(128 * 256 < s < 128 * 256 + 256 for s in sizes)
        assert {c.pens for c in gg if c.nv == nv} == {True, False}
    assert {(c.n, c.rule) for c in gc.APPLY_CASES} == {(n, r) for n in (13, 14, 15, 256, 300) for r in gc.RULES}


@pytest.mark.parametrize('c', gc.BUILD_W_CASES, ids=_id)
def test_build_w_case_conditions(c):
    x, o = gc.build_w_inputs(c), gc.build_w_oracle(c)
    M = 2 * c.N
    assert o['want'].shape == (c.B, M, M) == o['allowed'].shape and (o['allowed'] > 0).all()
    if gc._is32(c.entry):
        assert all(np.array_equal(x[k], gc._f32(x[k])) for k in ('z', 'J', 'D', 'S'))
    assert 0 < o['tol'] <= gc.TOLERANCE_CAP
    named = gc.build_w_named(c)
    assert named['last'] == o['want'].size - 1 and all(0 <= g < o['want'].size for g in named.values())
    if c.B > 2:                      # the first element of the second sweep, by name, is held relatively
        vec = gc.build_w_vec(c)
        assert named['sweep1-first'] == gc.BW_SWEEP * vec < o['want'].size < 2 * gc.BW_SWEEP * vec
        assert o['normal'].reshape(-1)[[named['sweep0-last'], named['sweep1-first'], named['last']]].all()
    if c.pset != 'wide' and c.N >= 101:
        assert not o['normal'].all()             # the profile underflows somewhere
    if c.pset == 'wide':
        assert o['normal'].all()
    for kind in gc.DEFECTS[:2]:
        r = gc.defect_ratio(kind, c)
        assert r is None or r >= gc.SENSITIVITY, (kind, r)
    assert gc.defect_ratio(gc.DEFECTS[1], c) is not None and (c.N == 1 or gc.defect_ratio(gc.DEFECTS[0], c) is not None)


@pytest.mark.parametrize('c', gc.STIM_CASES, ids=_id)
def test_stimulus_case_conditions(c):
    x, o = gc.stim_inputs(c), gc.stim_oracle(c)
    assert o['want'].shape == (c.B, c.NB, 2 * c.N)
    assert 0.0 in x['bw'] and 1.0 in x['bw'] and 0.0 in x['con'] and (o['want'] == 0).any() and (o['want'] != 0).sum() >= o['want'].size // 2
    assert 0 < o['tol'] <= gc.TOLERANCE_CAP
    named = gc.stim_named(c)
    assert all(0 <= g < o['want'].size for g in named.values()) and (c.B < 800 or 'sweep1-first' in named)
    if 'hetero' in c.entry:
        assert x['v'].size == c.nv and x['gain'].shape == (c.B, 2 * c.N)
        one = (1.0 + np.asarray(gc.hetero_gain(x['v'], x['zin'], c.N) - 1, dtype='float64'))
        assert np.array_equal(one, x['gain'])
    r = gc.defect_ratio(gc.DEFECTS[2], c)
    assert (r is None) == (x['gain'] is None) and (r is None or r >= gc.SENSITIVITY), r


@pytest.mark.parametrize('c', gc.JDS_CASES, ids=_id)
def test_jds_grad_case_conditions(c):
    x, res = gc.jds_inputs(c), gc.jds_oracle(c)
    assert len(res) == (1 if c.gw == 'free' else 12)
    for k, o in enumerate(res):
        assert o['want'].shape == (c.B, 4, 3) and 0 <= o['tol'] <= gc.TOLERANCE_CAP
        if c.gw == 'onehot':
            name, p, q, i, j = gc.onehot_places(c.N)[k]
            fed = np.zeros((c.B, 4), dtype=bool)
            fed[k % c.B, 2 * p + q] = True
            assert (o['want'][~fed] == 0).all() and (o['scale'][~fed] == 0).all() and (o['allowed'][~fed] == 0).all()
            assert (o['want'][fed][:, :2] != 0).all() and ((o['want'][fed][:, 2] != 0).all() == (i != j))
            assert np.count_nonzero(x['gW'][k]) == 1
    if c.gw == 'onehot':
        assert {k % c.B for k in range(12)} == {0, 1, 2}
    r = gc.defect_ratio(gc.DEFECTS[0], c)
    assert (r is None) == (c.N == 1) and (r is None or r >= gc.SENSITIVITY), r


@pytest.mark.parametrize('n', gc.PEN_N)
def test_penalty_case_conditions(n):
    for fp32 in (True, False):
        for call in range(3):
            dyn, rate, sd, sr = gc.penalty_inputs(n, call, fp32)
            assert len(dyn) == len(rate) == n and (not fp32 or np.array_equal(dyn, gc._f32(dyn)))
            for x, s in ((dyn, sd), (rate, sr)):
                got, wg = gc.penalty_means_in_order(x, s)
                want, bound = gc.penalty_bound(x, s)
                assert abs(got - want) <= bound and len(wg) == min(max(-(-n // 256), 1), 256)
                if n > 256:          # the order counts: the plain sum in element order gives other bits somewhere
                    assert bound > 0
            r = gc.defect_ratio(gc.DEFECTS[3], ('penalty', n, call, fp32))
            assert (r is None) == (n <= 256) and (r is None or r >= gc.SENSITIVITY), r
    if n >= 65536:
        sums = {gc.penalty_means_in_order(gc.penalty_inputs(n, k, True)[0], 1.0)[0] != float(np.sum(gc.penalty_inputs(n, k, True)[0])) for k in range(3)}
        assert True in sums


@pytest.mark.parametrize('c', gc.GG_CASES, ids=_id)
def test_gen_grads_case_conditions(c):
    for call in range(3):
        x = gc.gen_grads_inputs(c, call, 'exact')
        kw = dict(g_ext=x.get('g_ext'), ext_base=x.get('ext_base'), zin=x.get('zin'))
        out, wg = gc.gen_grads_in_order(x['parts'], x['dmean'], x['pens'], x['dynamics_cost'], x['rate_cost'], c.nv, **kw)
        assert out.shape == (c.nv + 13,) and np.isfinite(out).all() and (wg is None) == (c.nv == 0)
        pens = x['pens'] if x['pens'] is not None else (0, 0)
        assert float(out[-1]) == -x['dmean'] + 0.75 * pens[0] + 3.0 * pens[1]              # the loss is exact
        if c.nv:
            assert set(np.abs(x['zin']).flat) == {1.0}
            for k in ('g_ext', 'ext_base'):
                m, _ = np.frexp(x[k])
                assert np.array_equal(m * 2 ** 12, np.round(m * 2 ** 12))                   # at most 12 significant bits
    x = gc.gen_grads_inputs(c, 0, 'free')
    kw = dict(g_ext=x.get('g_ext'), ext_base=x.get('ext_base'), zin=x.get('zin'))
    out = gc.gen_grads_in_order(x['parts'], x['dmean'], x['pens'], x['dynamics_cost'], x['rate_cost'], c.nv, **kw)[0]
    want, allowed = gc.gen_grads_exact(x)
    assert (np.abs(out - want) <= allowed).all()
    r = gc.defect_ratio(gc.DEFECTS[3], c)
    assert (r is None) == (c.nv == 0 or c.B * c.NB * c.M <= 256) and (r is None or r >= gc.SENSITIVITY), r
    assert gc.defect_ratio(gc.DEFECTS[4], c) >= gc.SENSITIVITY


@pytest.mark.parametrize('c', gc.APPLY_CASES, ids=_id)
def test_gen_apply_case_conditions(c):
    x = gc.apply_inputs(c)
    tr = gc.apply_trace(c, x)
    assert tr['margin'] >= gc.APPLY_MARGIN > 4 * gc.apply_tol(2.0)
    assert x['lo'][2] == x['hi'][2] and (np.delete(x['lo'], 2) < np.delete(x['hi'], 2)).all()
    assert len(set(x['lo'])) == len(set(x['hi'])) == c.n                                    # they differ element by element
    first = tr['steps'][0]['where']
    assert {-1, 0, 1} <= set(first) and (first == 0).sum() >= c.n // 3                      # lo < update < hi cases exist
    assert set(tr['steps'][1]['where']) >= {-1, 0}
    for s in tr['steps']:
        assert np.abs(s['p']).max() < 2.0
        clipped = s['where'] != 0
        assert np.array_equal(s['p'][clipped], np.where(s['where'] < 0, x['lo'], x['hi'])[clipped])
    assert gc.defect_ratio(gc.DEFECTS[5], c) >= gc.SENSITIVITY


def test_every_defect_applies_somewhere():
    every = list(gc.BUILD_W_CASES[:3]) + [c for c in gc.STIM_CASES if 'amp' in c.entry][:2] + list(gc.JDS_CASES[2:4]) + [('penalty', 257, 0, True)] + list(gc.GG_CASES[-2:]) + list(gc.APPLY_CASES[:1])
    for kind in gc.DEFECTS:
        assert any(gc.defect_ratio(kind, c) is not None for c in every), kind

"""Pin `oracle/gan_torch.euler_ssn_adjoint` and the cases of tests/test_adjoint_elementwise_gpu.py without a GPU: the layout
identities the kernels' header states, finite differences, the conditions every case must meet for an element-wise
comparison to mean something, the fp32 oracle that the fp32 tolerances are taken from -- and, recorded as tests, what the
gradient checks before this module could not see."""
import numpy as np
import pytest
import torch

from oracle import adjoint_cases as ac
from oracle import gan_torch as og
from test_adjoint_elementwise_gpu import DF_ATOL, DF_PLAIN_FROM, DF_RTOL, FP32_ORACLE, SPLIT_EXTRA, TOL32
from test_generator_gpu import GEN, P, _problem

IDS = [ac.case_id(c) for c in ac.CASES]


@pytest.mark.parametrize('c', [c for c in ac.CASES if c.M <= 66], ids=[i for i, c in zip(IDS, ac.CASES) if c.M <= 66])
def test_layout_identities(c):
    """include/ssnode_mi355x.h, section 3: with the stream shifted by one step (slot t holds delta_{t+1}, the last slot zero)
    dL/dW[b] = dsh[b].reshape(NB T, M)^T @ traj[b].reshape(NB T, M), and dL/d ext = sum_t delta_t INCLUDING t = 0, the term the
    shifted stream drops.  1e-12 of the element's (block's) scale; measured <= 2e-15."""
    o = ac.oracle(c)
    e_w = ac.err_weight_grad(ac.weight_grad_of(o['dsh'], o['traj']), o).max()
    e_x = ac.err_g_ext(o['delta'].sum(axis=2), o).max()
    print('identities %s: dL/dW %.1e, dL/d ext %.1e' % (ac.case_id(c), e_w, e_x))
    assert e_w < 1e-12 and e_x < 1e-12
    assert ac.err_g_ext(o['dsh'].sum(axis=2), o).max() > 1e-3           # ... and the t = 0 term is not negligible here
    assert (o['dsh'][:, :, -1] == 0).all() and np.array_equal(o['dsh'][:, :, :-1], o['delta'][:, :, 1:])


def test_finite_differences_in_single_elements():
    """Central differences of the loss in five single elements of W and five of ext, 1e-6 relative: element (M - 1, M - 1), the
    last row and column, the last E row, the last stimulus, the saturated draw."""
    c = ac.Case('float64', 'asym_tanh', 20, 5, 'mid')
    x, o = ac.inputs(c), ac.oracle(c)
    gen, dyn_cost, rate_cost = ac.gen_kwargs(c)
    M, NB, N = c.M, c.NB, c.M // 2

    def loss(W, ext):
        ta, dyn, rate = og.euler_ssn(og.t64(W), og.t64(ext), **gen)
        return float((og.t64(x['G']) * ta).sum() + dyn_cost * dyn + rate_cost * rate)

    worst = 0.0
    for name, idxs in (('W', [(0, M - 1, M - 1), (1, M - 1, 0), (2, N - 1, M - 1), (0, 0, N), (2, 3, 7)]),
                       ('ext', [(0, NB - 1, M - 1), (2, NB - 1, 0), (1, 0, N - 1), (2, 4, N), (0, 2, 5)])):
        want = o['gW'] if name == 'W' else o['g_ext']
        for idx in idxs:
            h = 1e-4 * max(abs(x[name][idx]), 1e-2)
            vals = []
            for sgn in (+1, -1):
                q = {k: x[k].copy() for k in ('W', 'ext')}
                q[name][idx] += sgn * h
                vals.append(loss(q['W'], q['ext']))
            fd = (vals[0] - vals[1]) / (2 * h)
            worst = max(worst, abs(fd / want[idx] - 1))
            np.testing.assert_allclose(want[idx], fd, rtol=1e-6, atol=0, err_msg='%s%r' % (name, idx))
    print('finite differences: worst relative deviation %.1e' % worst)


# ------------------------------------------------------------------ the gap, recorded
def _jds_of(gW, z, jds, N):
    """dL/d(J, D, S) of a given dL/dW through make_W (all draws summed, as the existing tests compare them)."""
    J, D, S = (og.t64(jds[k]).clone().requires_grad_(True) for k in 'JDS')
    return [g.numpy() for g in torch.autograd.grad((og.t64(gW) * og.make_W(og.t64(z), J, D, S, N)).sum(), [J, D, S])]


@pytest.mark.parametrize('N,NB', [(33, 5), (101, 4)])
def test_the_gap_sums_over_dLdW_do_not_see_a_dropped_edge(N, NB):
    """What `test_bptt_gradients_vs_oracle` compares (its inputs: stimulus centred on the ring, sparse G, 50 steps, skip 30; the
    twelve numbers dL/d(J, D, S) at 2e-3 of the largest) does not move when the last row, the last column or the last E row of
    dL/dW is dropped: each of the twelve changes by less than 2e-3 of the largest (measured: below 1e-6), because the edge
    neurons of those inputs are silent -- the smallest row maximum of dL/dW is below 1e-6 of the draw's largest element."""
    B, T, skip, theta = 2, 50, 30, 1.0
    jds, z, bws, con = _problem(N, B, NB, 7 * N + NB, T, skip, theta)
    rs = np.random.RandomState(5)
    G = rs.randn(B, NB, 2 * N) * (rs.rand(B, NB, 2 * N) < 0.1)
    W = og.make_W(og.t64(z), *(og.t64(jds[k]) for k in 'JDS'), N)
    o = og.euler_ssn_adjoint(W, og.stimulus(bws, con, P['smoothness'], N), og.t64(G), 1.0, 0.01, seqlen=T, skip_steps=skip,
                             rate_penalty_threshold=theta, **GEN)
    gW = o['gW'].numpy()
    want = _jds_of(gW, z, jds, N)
    rowmax = np.abs(gW).max(axis=2) / np.abs(gW).max(axis=(1, 2), keepdims=True)[:, :, 0]
    assert rowmax.min() < 1e-6
    for name, sl in (('last row', np.s_[:, 2 * N - 1, :]), ('last column', np.s_[:, :, 2 * N - 1]), ('last E row', np.s_[:, N - 1, :])):
        bad = gW.copy()
        bad[sl] = 0
        moved = max(np.abs(g - w).max() / np.abs(w).max() for g, w in zip(_jds_of(bad, z, jds, N), want))
        print('N = %d, %s dropped: dL/d(J, D, S) move by %.1e of the largest (the test allows 2e-3)' % (N, name, moved))
        assert moved < 2e-3
        # ... nor does "relative to the largest element of the draw" at the 1e-4 of the production-horizon tests
        assert (np.abs(bad - gW).reshape(B, -1).max(axis=1) / np.abs(gW).reshape(B, -1).max(axis=1)).max() < 1e-4


@pytest.mark.parametrize('c', [c for c in ac.CASES if c.dtype == 'float32' and (c.M, c.NB) in ((66, 9), (202, 5))],
                         ids=[i for i, c in zip(IDS, ac.CASES) if c.dtype == 'float32' and (c.M, c.NB) in ((66, 9), (202, 5))])
def test_the_gap_is_closed_on_the_new_inputs_under_the_new_measures(c):
    """The same defects, and four of the sweep, on the inputs of this module under its measures: each exceeds the tolerance of
    the fp32 kernels by a factor of at least 100 (measured: 113 ... 1.4e5; the fp16-split add-on included).  The factor of the
    1.001 defect is 1e-3 / tolerance whatever the inputs: it is applied in a draw that stays in the power-law branch
    (tolerance 3.84e-6 + 5e-6); in the saturated draw of the asym_tanh cases, where the fp32 oracle itself deviates by 6.7e-6
    and the tolerance is 2.7e-5 (+ 5e-6), the same defect stands out by a factor of 31 only."""
    o = ac.oracle(c)
    M, N, NB = c.M, c.M // 2, c.NB
    sat = ac.saturated_draws(c)
    tol = {k: np.where(sat, TOL32[k][1], TOL32[k][0]) + (SPLIT_EXTRA if k != 'weight_grad' else 0.0)
           for k in ('weight_grad', 'delta', 'g_ext')}

    def factor(delta=None, gW=None, g_ext=None):
        """The largest excess over the tolerance of any measure; what a sweep derives from delta follows a defective delta."""
        if delta is not None:
            dsh = ac.shifted(delta)
            gW, g_ext = ac.weight_grad_of(dsh, o['traj']), delta.sum(axis=2)
        else:
            dsh = o['dsh']
        return max((ac.err_weight_grad(o['gW'] if gW is None else gW, o) / tol['weight_grad']).max(),
                   (ac.err_delta(dsh, o) / tol['delta']).max(), (ac.err_g_ext(o['g_ext'] if g_ext is None else g_ext, o) / tol['g_ext']).max())

    assert factor() == 0.0
    found = {}
    for name, sl in (('last row of dL/dW zero', np.s_[:, M - 1, :]), ('last column of dL/dW zero', np.s_[:, :, M - 1]),
                     ('row N - 1 of dL/dW zero', np.s_[:, N - 1, :])):
        bad = o['gW'].copy()
        bad[sl] = 0
        found[name] = factor(gW=bad)
    bad = o['delta'].copy()
    bad[..., M - 1] = 0
    found['neuron M - 1 of delta zero at every step'] = factor(delta=bad)
    bad = o['delta'].copy()
    bad[0, NB - 1, ac.T // 2] *= 1.001
    found['one stimulus of the last group x 1.001 at one step'] = factor(delta=bad)
    found['dL/d ext without its t = 0 term'] = factor(g_ext=o['delta'][:, :, 1:].sum(axis=2))
    unshifted = o['delta'].copy()
    unshifted[:, :, -1] = 0
    found['delta not shifted'] = max((ac.err_delta(unshifted, o) / tol['delta']).max(),
                                     (ac.err_weight_grad(ac.weight_grad_of(unshifted, o['traj']), o) / tol['weight_grad']).max())
    for name, f in found.items():
        print('%s, %s: %.3g x the tolerance' % (ac.case_id(c), name, f))
    assert all(f >= 100 for f in found.values()), found


# ------------------------------------------------------------------ every case of the GPU module
@pytest.mark.parametrize('c', ac.CASES, ids=IDS)
def test_case_conditions_and_fp32_oracle(c):
    """What makes the element-wise comparison of a case meaningful: finite values; every row and every column of dL/dW holds an
    element of at least 0.2 of its own scale sum_k |delta_ki| |x_kj| (measured: rows >= 0.24, columns >= 0.79); every neuron's
    |delta| reaches 1e-4 of the maximum of its (draw, stimulus, step, population) block at some step, for every draw and
    stimulus (measured: >= 2.5e-4); every rate is above 1e-4; with asym_tanh 10 % ... 60 % of the last draw's inputs lie above
    v0 = (r0 / k)^(1 / n), both branches of f' are live, and no other draw reaches v0 (measured: 12 ... 57 %, rates up to 530).  Four cases are drawn
    from a second seed because their first draw misses one of these (`adjoint_cases.RESEED`).
    fp32 cases: the oracle run in float32 stays within the figures the fp32 tolerances are four times of, f'(u) among them:
    under the block measure, and plainly relative on the elements that the GPU module holds plainly."""
    o = ac.oracle(c)
    assert all(np.isfinite(v).all() for v in o.values())
    ratio = np.abs(o['gW']) / o['scale']
    assert ratio.max(axis=2).min() >= 0.2 and ratio.max(axis=1).min() >= 0.2
    d = np.abs(o['delta'])
    sh = d.shape[:-1] + (2, c.M // 2)
    rel = (d.reshape(sh) / d.reshape(sh).max(axis=-1, keepdims=True)).reshape(d.shape)
    assert rel.max(axis=2).min() >= 1e-4
    assert o['traj'].min() > 1e-4
    v0 = (200.0 / ac.GEN['k']) ** (1 / ac.GEN['n'])
    above = (o['u'] > v0).reshape(ac.B, -1).mean(axis=1)
    if c.io_type == 'asym_tanh':
        assert 0.10 <= above[-1] <= 0.60 and (above[:-1] == 0).all() and o['traj'].max() < 1000.0
    else:
        assert o['traj'].max() < 100.0
    if c.dtype == 'float32':
        f = ac.oracle(c, 'float32')
        sat = ac.saturated_draws(c)
        df_block, df_plain = ac.err_df(f['df'], o, np.where(sat, DF_PLAIN_FROM[1], DF_PLAIN_FROM[0]), DF_RTOL, DF_ATOL)
        print('fp32 oracle %s: f\'(u) / block maximum %s, plain relative on the elements held to it %s'
              % (ac.case_id(c), ' '.join('%.1e' % v for v in df_block), ' '.join('%.1e' % v for v in df_plain)))
        for name, err in (('weight_grad', ac.err_weight_grad(f['gW'], o)), ('delta', ac.err_delta(f['dsh'], o)),
                          ('g_ext', ac.err_g_ext(f['g_ext'], o)), ('df', df_block), ('df_plain', df_plain)):
            # (twice the recorded figure: another BLAS may add in another order; the tolerance is four times it)
            assert (err <= 2 * np.where(sat, FP32_ORACLE[name][1], FP32_ORACLE[name][0])).all(), (name, err)

"""The BPTT backward of the fixed-time generator against fp64 autograd ELEMENT BY ELEMENT: the adjoint sweep of every kernel
family, every form of dL/dW, dL/d ext and the per-draw chain to J, D, S, on inputs that drive every neuron
(oracle/adjoint_cases.py; reference semantics: the `theano.grad` of networks/wgan.py:236-242 through the scan of
networks/ssn.py:354-385, 555-576, 598-633).

The other gradient tests compare sums over dL/dW (dL/d(J, D, S)) or dL/dW "relative to its largest element", on inputs whose
edge neurons are silent: a dropped tail row, tail column or ragged stimulus group is invisible to them
(tests/test_adjoint_oracle.py::test_the_gap_*).  Here the sizes are the ones where a tile grid is partly filled, full, or just
exceeded, the stimulus counts leave a ragged last group of four, three draws leave the two-draw kernels a lone draw, and every
error has the scale of its own element (dL/dW: sum_k |delta_ki| |x_kj|) or block (delta, dL/d ext: the largest element of the
same draw, stimulus, step and population).

Tolerances.  fp64: 1e-9, the project's figure.  fp32: FOUR TIMES the deviation of the oracle itself run in float32 on the CPU
(`euler_ssn_adjoint(dtype=float32)`; the convention of tests/test_solver_stop_gpu.py), capped at the project's 1e-4, never
taken from a kernel.  The draw that asym_tanh drives into saturation is worse conditioned than the others -- the fp32 oracle
deviates up to seven times as much there -- so it has figures of its own.  tests/test_adjoint_oracle.py holds the fp32 oracle
to these constants on every case.  The forward of the same runs is held as well: trajectory and time average at the project's
1e-4 relative (fp64: 1e-9), f'(u) under the block measure and, wherever four times the fp32 oracle's plain deviation stays
within 1e-4, plainly relative (`DF_PLAIN_FROM`), each at four times the fp32 oracle's figure (fp64: 1e-9 on every element).
Any error of a launch fails its test; only a refusal that is asked for BEFORE the launch (`forward_variant`,
`gen_backward_fused_supported`) is a skip.
Measured per family on an MI355X: DESIGN.md section 1.
"""
import numpy as np
import pytest
import torch

from oracle import adjoint_cases as ac

pytestmark = pytest.mark.gpu

#                 fp32 oracle against fp64, largest over all cases:   other draws   saturated draw (asym_tanh, last)
FP32_ORACLE = {'weight_grad': (7.5e-6, 4.3e-5),       # |d dL/dW_ij| / sum_k |delta_ki| |x_kj|   (M210-NB1 power / tanh)
               'delta': (9.6e-7, 6.7e-6),             # |d delta| / block maximum                (M66-NB9 power / M258-NB8 tanh)
               'g_ext': (7.1e-7, 8.4e-7),             # |d dL/d ext| / block maximum             (M202-NB4-last power / M106-NB5 tanh)
               # f'(u): a float32 run depends on the order its BLAS adds in; the larger figures of two CPUs (the other's:
               # 6.3e-7 / 2.4e-6 and 1.5e-5 / 1.2e-5)
               'df': (6.9e-7, 9.2e-6),                # |d f'(u)| / block maximum                (M258-NB8 power / tanh)
               'df_plain': (2.4e-5, 2.1e-5)}          # |d f'(u)| / f'(u) where held plainly     (M258-NB8 power / tanh)
TOL32 = {k: tuple(min(4 * v, 1e-4) for v in pair) for k, pair in FP32_ORACLE.items()}
# the fp16-split sweeps (4, 5, 6, 8) and the one-launch backward: the distance tests/test_generator_gpu.py::
# test_split_adjoint_matches_fp32_adjoint_step_by_step allows between them and the fp32 sweep, on delta and dL/d ext
SPLIT_EXTRA = 5e-6
TOL64 = 1e-9
# a dL/dW kernel on the sweep's own (delta, trajectory) against their fp64 product: the bound of
# test_weight_grad_kernels_vs_fp64_matmul (an fp32 dot product, relative to sum |d| |x|)
DOT32, DOT64 = 2e-6, 1e-14

# f'(u), fp32.  The plain 1e-4 relative (atol 1e-9) of the forward cannot hold on every element: u = W r + ext cancels, f'
# is ~ u^1.2 and exactly zero for u <= 0, and the fp32 oracle itself is 1e-2 off in plain relative terms near a zero of u.
# So every element is held under the block-maximum measure ('df'), and the plain relative one ('df_plain') holds wherever
# four times the fp32 oracle's plain deviation stays within 1e-4: on the elements that reach DF_PLAIN_FROM of their block's
# maximum (other draws, saturated draw), at least 99.7 % / 92 % of a draw's elements with f' > 0.  (From 1e-3 / 3e-2 of the
# block's maximum the fp32 oracle is 3.7e-5 / 2.9e-5 off already.)  tests/test_adjoint_oracle.py holds the fp32 oracle to
# both figures on every case.
DF_PLAIN_FROM = (3e-3, 0.1)
DF_RTOL, DF_ATOL = 1e-4, 1e-9

SPLIT = (4, 5, 6, 8)


def tolerance(c, measure, code):
    """(B,) tolerances of one measure for a case and a kernel code."""
    if c.dtype == 'float64':
        return np.full(ac.B, TOL64)
    tol = np.where(ac.saturated_draws(c), TOL32[measure][1], TOL32[measure][0])
    return tol + (SPLIT_EXTRA if measure in ('delta', 'g_ext') and (code in SPLIT or code == 'fused') else 0.0)


def codes(c):
    """The kernel codes that take a case's shape (include/ssnode_mi355x.h, `ssn_gen_params.kernel`), forced one by one; 'fused'
    is the one-launch backward, which answers for its shapes itself."""
    if c.dtype == 'float64':
        return [0]
    return [1] + ([2, 3, 4, 5, 6, 8] if c.NB >= 4 and c.M <= 208 else []) + ['fused']


PARAMS = [(c, code) for c in ac.CASES for code in codes(c)]
RAN = set()             # (family, tile grid) and ('weight_grad', form, tile grid) that ran to the end


def _family(c, code):
    return 'fp64' if c.dtype == 'float64' else {1: 'tile' if c.M <= 208 else 'stream'}.get(code, code)


def _run(c, code):
    from tc_gan_amd import genops
    x, o = ac.inputs(c), ac.oracle(c)
    td = getattr(torch, c.dtype)
    W, ext, G, z = (torch.as_tensor(x[k]).to('cuda', td) for k in ('W', 'ext', 'G', 'z'))
    gen, dyn_cost, rate_cost = ac.gen_kwargs(c)
    skip = gen['skip_steps']
    B, NB, T, M = ac.B, c.NB, ac.T, c.M
    grid, family = ac.tile_grid(c), _family(c, code)
    fp32 = c.dtype == 'float32'
    rtol = 1e-4 if fp32 else TOL64
    # the fp16-split forwards need the rate bound of asym_tanh: with asym_power their adjoint runs on kernel 2's forward, as the
    # library's own rule has it; the one-launch backward runs behind the two-draw forward (networks/ssn.py)
    if code == 'fused':
        fwd_code = (8 if c.io_type == 'asym_tanh' else 2) if NB >= 4 and M <= 208 else 1
    else:
        fwd_code = 2 if code in SPLIT and c.io_type != 'asym_tanh' else code
    gpf = genops.make_gen_params(kernel=fwd_code, **gen)
    gpb = genops.make_gen_params(kernel=0 if code == 'fused' else code, **gen)
    if fp32 and genops.forward_variant(B, NB, M, gpf, save=True) < 0:
        pytest.skip('forward kernel %s refuses %s' % (fwd_code, ac.case_id(c)))
    out = genops.gen_forward(W, ext, gpf, save=True)
    tag = '%s code %s' % (ac.case_id(c), code)
    fig = {}
    traj, df = out['traj'].cpu().numpy().astype('float64'), out['df'].cpu().numpy().astype('float64')
    assert np.isfinite(traj).all() and np.isfinite(df).all()
    fig['traj'] = np.abs(traj / o['traj'] - 1).max()
    if fp32:
        fig['df'], fig['df plain'] = ac.err_df(df, o, np.where(ac.saturated_draws(c), DF_PLAIN_FROM[1], DF_PLAIN_FROM[0]), DF_RTOL, DF_ATOL)
    else:
        fig['df plain'] = ac.err_df(df, o, np.zeros(B), rtol, DF_ATOL)[1]        # fp64: every element, plainly
    c_dyn = dyn_cost / (B * (T - skip - 1) * NB * M) if dyn_cost else 0.0
    c_rate = rate_cost / (B * (T - skip) * NB * M)
    forms = {}
    if code == 'fused':
        xmax = genops.rate_bound(gpb) or float(out['traj'].max()) + 1.0
        if not genops.gen_backward_fused_supported(B, NB, M, gpb, xmax):
            pytest.skip('ssn_gen_backward_fused_supported refuses %s' % ac.case_id(c))
        df0 = out['df'].clone()
        gW, g_ext, dmax = genops.gen_backward_fused(W, out['traj'], out['df'], G, c_dyn, c_rate, gpb, xmax, want_g_ext=True)
        assert torch.equal(df0, out['df'])                       # f'(u) is only read
        forms['fused'] = gW
        true = np.abs(o['dsh']).reshape(B, -1).max(axis=1)
        dsh = None
    else:
        delta, g_ext, dmax = genops.gen_backward(W, out['traj'], out['df'].clone(), G, c_dyn, c_rate, gpb, want_g_ext=True,
                                                 want_dmax=True)
        assert (dmax is not None) == (code in SPLIT)
        dsh = delta.cpu().numpy().astype('float64')
        assert np.isfinite(dsh).all()
        assert (dsh[:, :, -1] == 0).all()                        # the shifted stream ends in a zero slot, exactly
        fig['delta'] = ac.err_delta(dsh, o)
        forms[1] = genops.weight_grad(delta, out['traj'], kernel=1)
        if fp32 and M <= 224:
            forms[2] = genops.weight_grad(delta, out['traj'], kernel=2)
        if dmax is not None and genops.rate_bound(gpb) is not None:
            forms[3] = genops.weight_grad(delta, out['traj'], kernel=3, dmax=dmax, xmax=genops.rate_bound(gpb))
        true = np.abs(dsh).reshape(B, -1).max(axis=1)
    fig['g_ext'] = ac.err_g_ext(g_ext.cpu().numpy().astype('float64'), o)
    own = None if dsh is None else (ac.weight_grad_of(dsh, traj), ac.weight_grad_of(np.abs(dsh), np.abs(traj)))
    for form, gW in forms.items():
        got = gW.cpu().numpy().astype('float64')
        assert np.isfinite(got).all(), (tag, form)
        fig['weight_grad %s' % form] = ac.err_weight_grad(got, o)
        if own is not None:
            fig['dot %s' % form] = ac.err_weight_grad(got, o, *own)
    # the chain through make_W per draw, on the form the generator update takes by default for this sweep
    last = forms['fused'] if code == 'fused' else forms[3] if 3 in forms else forms[2] if 2 in forms else forms[1]
    parts = genops.jds_grad_parts(last, z, x['jds']['J'], x['jds']['D'], x['jds']['S']).cpu().numpy()
    ptol = 2e-3 if fp32 else 1e-8
    fig['parts'] = (np.abs(parts - o['parts']) / (np.abs(o['parts']) + np.abs(o['parts']).max(axis=1, keepdims=True))).max()
    print('ADJ %s family=%s grid=%s %s' % (tag, family, grid, ' '.join(
        '%s=%.2e' % (k.replace(' ', ''), np.max(v)) + ('/%.2e' % np.max(np.where(ac.saturated_draws(c), 0, v)) if np.ndim(v) else '')
        for k, v in fig.items())))
    # ---- forward
    np.testing.assert_allclose(out['time_avg'].cpu().numpy(), o['time_avg'], rtol=rtol, atol=1e-9, err_msg=tag)
    np.testing.assert_allclose(traj, o['traj'], rtol=rtol, atol=1e-9, err_msg=tag)
    if fp32:
        assert (fig['df'] <= tolerance(c, 'df', code)).all(), (tag, fig['df'])
    assert (fig['df plain'] <= tolerance(c, 'df_plain', code)).all(), (tag, fig['df plain'])
    # ---- adjoint
    if dsh is not None:
        assert (fig['delta'] <= tolerance(c, 'delta', code)).all(), (tag, fig['delta'])
    assert (fig['g_ext'] <= tolerance(c, 'g_ext', code)).all(), (tag, fig['g_ext'])
    if dmax is not None:                                         # at least the true maximum and at most 4 x it
        dm = dmax.cpu().numpy().astype('float64')
        assert (dm >= true * (1 - 1e-4)).all() and (dm <= 4 * true).all(), (tag, dm, true)
    # ---- dL/dW, every form
    for form in forms:
        assert (fig['weight_grad %s' % form] <= tolerance(c, 'weight_grad', code)).all(), (tag, form, fig['weight_grad %s' % form])
        if own is not None:
            assert (fig['dot %s' % form] <= (DOT32 if fp32 else DOT64)).all(), (tag, form, fig['dot %s' % form])
    assert fig['parts'] <= ptol, (tag, fig['parts'])
    RAN.add((family, grid))
    RAN.update(('weight_grad', form, grid) for form in forms)


@pytest.mark.parametrize('c,code', PARAMS, ids=['%s-k%s' % (ac.case_id(c), code) for c, code in PARAMS])
def test_backward_elementwise_vs_fp64(c, code):
    _run(c, code)


def test_every_family_and_every_weight_grad_form_ran_on_every_tile_grid():
    """Each adjoint family and each dL/dW form has run to the end at least once per tile grid: a refusal is a skip above, never
    a silent pass, and a family that only skipped or failed on a grid fails here.  Meaningful only after the parametrized test
    above, in the same process; it launches nothing itself."""
    grids32 = (0, 1, 2)
    need = [(f, g) for f in ('tile', 2, 3, 4, 5, 6, 8, 'fused') for g in grids32] + [('stream', 'stream'), ('fp64', 0), ('fp64', 'stream')]
    need += [('weight_grad', form, g) for form in (1, 2, 3) for g in grids32] + [('weight_grad', 1, 'stream'), ('weight_grad', 2, 'stream')]
    missing = [item for item in need if item not in RAN]
    assert not missing, 'never ran to the end: %r' % (missing,)

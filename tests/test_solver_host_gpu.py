"""`ssn_solve_batch_host_f32 / _f64` (host buffers in, host buffers out) against `ssn_solve_batch_f32 / _f64` on device
tensors with the same inputs: same kernel choice and same launch, so r, r_prev, codes and steps are equal bit for bit.

Staged case (2N = 8, B = 3, NB = 2: the whole device image goes through the pinned staging buffer, one copy up and one down),
with a shared and a per-draw ext, with and without r_prev / steps.  Un-staged case: fp64, 2N = 200, B = 27 -- the W block alone is
27 * 200 * 200 * 8 = 8.64 MB, above the 8 MiB staging limit, so every buffer is copied on its own."""
import ctypes

import numpy as np
import pytest

from oracle import ssn_numpy as on

pytestmark = pytest.mark.gpu


def _inputs(dtype, N, B, NB, ext_per_draw, seed):
    rs = np.random.RandomState(seed)
    P, jds = on.DEFAULT_PARAMS, on.new_JDS()
    W = np.stack([on.generate_weight(N, jds['J'], jds['D'], jds['S'], z) for z in rs.rand(B, 2 * N, 2 * N)])
    ext = on.stimulus_input(P['bandwidths'][:NB], np.linspace(-.5, .5, N), P['smoothness'], [20.])
    ext = ext.reshape(NB, 2 * N)
    if ext_per_draw:
        ext = ext[None] * (1. + .1 * rs.rand(B, 1, 1))
    r0 = .1 * rs.rand(B, NB, 2 * N)
    return tuple(np.ascontiguousarray(a, dtype=dtype) for a in (W, ext, r0))


def _params(max_iter):
    from tc_gan_amd import clib
    P = on.DEFAULT_PARAMS
    return clib.SolverParams(io_type=clib.SSN_IO_TANH, max_iter=max_iter, k=P['k'], n=P['n'], tau_E=P['tau'][0], tau_I=P['tau'][1],
                             dt=8e-4, atol=1e-5, rate_soft_bound=200., rate_hard_bound=1000.)


def _host_solve(dtype, W, ext, r0, ext_per_draw, p, outputs):
    from tc_gan_amd import clib
    B, NB, M = r0.shape
    r = r0.copy()
    r_prev = np.full_like(r0, np.nan) if outputs else None
    steps = np.full((B, NB), -7, dtype=np.int32) if outputs else None
    codes = np.full((B, NB), -7, dtype=np.int32)
    fn = clib.libssnode.ssn_solve_batch_host_f32 if dtype == np.float32 else clib.libssnode.ssn_solve_batch_host_f64
    ptr = lambda a: None if a is None else a.ctypes.data
    clib.check(fn(ptr(W), ptr(ext), ext_per_draw, ptr(r), ptr(r_prev), ptr(codes), ptr(steps), B, NB, M, ctypes.byref(p)),
               'ssn_solve_batch_host')
    return r, r_prev, codes, steps


def _device_solve(dtype, W, ext, r0, ext_per_draw, p, outputs):
    import torch
    from tc_gan_amd import clib
    clib.require_gpu()
    B, NB, M = r0.shape
    dW, dE, dR = (torch.as_tensor(a).to('cuda') for a in (W, ext, r0))
    dP = torch.full_like(dR, float('nan')) if outputs else None
    dS = torch.full((B, NB), -7, dtype=torch.int32, device='cuda') if outputs else None
    dC = torch.full((B, NB), -7, dtype=torch.int32, device='cuda')
    fn = clib.libssnode.ssn_solve_batch_f32 if dtype == np.float32 else clib.libssnode.ssn_solve_batch_f64
    ptr = lambda t: None if t is None else t.data_ptr()
    clib.check(fn(ptr(dW), ptr(dE), ext_per_draw, ptr(dR), ptr(dP), ptr(dC), ptr(dS), B, NB, M, ctypes.byref(p),
                  clib.stream_ptr()), 'ssn_solve_batch')
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (dR, dP, dC, dS))


def _check_same(dtype, N, B, NB, ext_per_draw, max_iter, outputs):
    W, ext, r0 = _inputs(dtype, N, B, NB, ext_per_draw, seed=N + B)
    p = _params(max_iter)
    got = _host_solve(dtype, W, ext, r0, ext_per_draw, p, outputs)
    want = _device_solve(dtype, W, ext, r0, ext_per_draw, p, outputs)
    bits = np.uint32 if dtype == np.float32 else np.uint64
    for name, g, w in zip(('r', 'r_prev', 'codes', 'steps'), got, want):
        assert (g is None) == (w is None) == (not outputs and name in ('r_prev', 'steps')), name
        if g is None:
            continue
        if g.dtype == dtype:
            g, w = g.view(bits), w.view(bits)
        np.testing.assert_array_equal(g, w, err_msg=name)
    assert np.isin(got[2], (0, 1, 2)).all() and not np.array_equal(got[0], r0)      # the solve ran and wrote its codes
    if outputs:
        assert (got[3] >= 1).all() and (got[3] <= max_iter).all() and np.isfinite(got[1]).all()


@pytest.mark.parametrize('outputs', [True, False], ids=['prev-steps', 'null-prev-steps'])
@pytest.mark.parametrize('ext_per_draw', [0, 1])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_staged_host_solve_equals_the_device_solve_bit_for_bit(dtype, ext_per_draw, outputs):
    _check_same(dtype, N=4, B=3, NB=2, ext_per_draw=ext_per_draw, max_iter=50, outputs=outputs)


def test_unstaged_host_solve_equals_the_device_solve_bit_for_bit():
    N, B = 100, 27
    assert B * (2 * N) ** 2 * 8 > 8 << 20           # the W block alone is beyond the staging limit
    _check_same(np.float64, N=N, B=B, NB=1, ext_per_draw=1, max_iter=20, outputs=True)

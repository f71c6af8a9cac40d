"""Every kernel of the fixed-point solver against the fp64 C oracle ELEMENT BY ELEMENT, on inputs that drive every neuron
(oracle/solver_cases.py; reference semantics: ODE_STEP and the Euler loops of ext/ssnode.c:64-187).

The other solver tests compare end states with `atol = rtol * 1e-2` after 300 steps from r = 0 under a stimulus centred on
the ring: a quarter of the expected state lies below that atol, the end neurons of the ring among it, and a dropped edge row
or column of the E population is invisible to every parametrization with 2 ... 7 stimuli (tests/test_solver_cases.py::
test_the_gap_*).  Here the sizes are the ones where a tile grid is partly filled, full or just exceeded, the stimulus counts
reach every template instantiation and every grouping of the matrix-core kernels, three draws leave the two-draw kernel a
lone draw, the start state is non-zero, two horizons (24 and 7 steps) end in either state buffer, and with asym_tanh the
last draw runs in the saturating branch.

Every (case, variant) runs `ssnode.fixed_points_batch(..., atol=0, want_prev=True)` with the variant forced (None: the
library's own choice) and asserts codes == 1, steps == T, and x and x_prev (the oracle's state one step earlier) with

    |got - want| <= RTOL |want|      RTOL = 1e-4 (fp32), 1e-9 (fp64): the project's RTOL32 and RTOL64

on EVERY element -- no absolute term, nothing left out; tests/test_solver_cases.py asserts on the oracle that every expected
element is at least 1e-3 of its row's maximum, that a float32 CPU run of the same loop stays within a quarter of RTOL32, and
that nine defects of the kind the old inputs hide exceed the tolerance 100 times here.  A variant that has no instantiation
for a shape must refuse it with the documented error (`sc.REFUSAL`, raised before anything is launched); any other error
fails the test, nothing is skipped.  The last test asserts that every variant ran on every step of its size ladder and that
every template instantiation and stimulus grouping ran (`sc.coverage`).
Measured per family on an MI355X: DESIGN.md section 1, "The solver, element by element".
"""
import numpy as np
import pytest

from oracle import solver_cases as sc

pytestmark = pytest.mark.gpu

PARAMS = [(c, v) for c in sc.CASES for v in sc.variants(c)]
RAN = set()             # the records of `sc.ran` of every (case, variant) that ran to the end
REFUSED = set()         # the variants that refused a shape the documented way


def _solve(c, variant, steps):
    from tc_gan_amd.ssnode import fixed_points_batch
    x = sc.inputs(c)
    return fixed_points_batch(x['W'], x['ext'], sc.P['k'], sc.P['n'], r0=x['r0'], max_iter=steps, atol=0.0, dt=sc.DT,
                              io_type=c.io_type, rate_stop_at=np.inf, dtype=c.dtype, variant=variant, want_prev=True)


@pytest.mark.parametrize('c,variant', PARAMS, ids=['%s-v%s' % (sc.case_id(c), v) for c, v in PARAMS])
def test_solver_elementwise_vs_fp64(oracle_lib, c, variant):
    import torch
    from tc_gan_amd import clib
    tag = '%s variant %s' % (sc.case_id(c), variant)
    if not sc.supported(c, variant):
        with pytest.raises(clib.SSNLibraryError, match=sc.REFUSAL):
            _solve(c, variant, sc.T)
        torch.cuda.synchronize()
        REFUSED.add(variant)
        return
    oracle = sc.oracle(c)
    sat = sc.saturated_draws(c)
    rtol = sc.RTOL[c.dtype]
    fig = {}
    for steps in sc.HORIZONS:
        want, want_prev, wcodes, wsteps = oracle[steps]
        res = _solve(c, variant, steps)         # (any error of the launch propagates: a failure, never a skip)
        assert res.x.shape == want.shape and res.x_prev.shape == want.shape and res.x.dtype == np.dtype(c.dtype)
        np.testing.assert_array_equal(res.codes, wcodes, err_msg=tag)
        np.testing.assert_array_equal(res.steps, wsteps, err_msg=tag)
        assert (res.codes == 1).all() and (res.steps == steps).all(), tag
        assert np.isfinite(res.x).all() and np.isfinite(res.x_prev).all(), tag
        fig[steps] = sc.per_draw_max(sc.rel_err(res.x, want)), sc.per_draw_max(sc.rel_err(res.x_prev, want_prev))
    family, grid, shape = sc.kernel_of(c, variant)
    ex, ep = (np.maximum(*(fig[k][i] for k in sc.HORIZONS)) for i in (0, 1))
    print('SOLVER %s family=%s grid=%s shape=%s x=%.2e x_prev=%.2e saturated: x=%.2e x_prev=%.2e' % (
        tag, family.replace(' ', '_'), grid, str(shape).replace(' ', '_'), ex[~sat].max(), ep[~sat].max(),
        ex[sat].max() if sat.any() else 0.0, ep[sat].max() if sat.any() else 0.0))
    for steps in sc.HORIZONS:
        assert (fig[steps][0] <= rtol).all(), (tag, steps, 'x', fig[steps][0])
        assert (fig[steps][1] <= rtol).all(), (tag, steps, 'x_prev', fig[steps][1])
    RAN.update(sc.ran(c, variant))


def test_every_variant_grid_and_instantiation_ran():
    """Every variant has run to the end on every step of its size ladder, and so has every template instantiation (tile and
    register-stationary: stimuli per workgroup; mixed: rows per lane of the last wave) and every stimulus grouping of the
    matrix-core kernels; every variant that can refuse a shape has done so the documented way.  A (case, variant) that failed
    left no record, so a family that only failed on a grid fails here as well.  Meaningful only after the parametrized test
    above, in the same process; it launches nothing itself."""
    missing = [k for k in sc.coverage() if k not in RAN]
    assert not missing, 'never ran to the end: %r' % (missing,)
    assert REFUSED == {1, 2, 3, 4, 5, 6, 7, 8}

"""What makes tests/test_solver_elementwise_gpu.py fair and sharp, asserted on the oracle alone (no GPU).

1. The gap it closes.  The other solver-vs-oracle tests (tests/test_solver_gpu.py::_inputs, T = 300 steps from r = 0, stimulus
   centred on the ring, `atol = rtol * 1e-2`) leave 24-29 % of the expected end state below their atol wherever every
   bandwidth is <= 0.75 (2 ... 7 stimuli), and the neurons at the ends of the ring hold 1e-22 ... 1e-19 there.  With row
   N - 1, column N - 1 or row 0 of W ZEROED in the oracle, the largest |delta| / (1e-4 |r| + 1e-6) over all elements (above 1:
   the test would notice) is

       (N, NB)     row N - 1   column N - 1   row 0     column 2N - 1   row 2N - 1
       (102, 3)    3.1e-7      5.8e-12        3.1e-7    0.94            6.8e2
       (102, 5)    2.5e-5      7.7e-12        2.5e-5    3.8             1.4e3
       (76, 3)     3.1e-7      5.8e-12        3.1e-7    3.8             1.5e3
       (75, 2)     3.4e-8      4.5e-12        3.4e-8    0.31            3.1e2
       (100, 8)    4.0e3       4.9e3          5.0e3     8.6e3           9.9e3

   so a dropped edge row or column of the E population is invisible to every parametrization with 2 ... 7 stimuli by a
   factor 4e4 ... 1e11 (`test_the_gap_*`; the same figures with asym_tanh and asym_power).

2. The conditions of every case of oracle/solver_cases.py (`test_case_conditions`): inputs exactly representable in the
   case's dtype; the numpy restatement of the Euler loop equal to the C oracle at 1e-12 (x and x_prev, both horizons); every
   element of the expected x and x_prev finite and >= 1e-3 of its (draw, stimulus) maximum; the same loop run in float32 on
   the CPU within 2.5e-5 relative of the fp64 one on every element of the whole trajectory (a quarter of the fp32 tolerance;
   fp32 cases); at least 5 % of the saturated draw's trajectory above the soft rate bound.  Measured over all cases: smallest
   element 2.0e-3 of its maximum, float32 run 1.1e-5 off (1.2e-5 in the saturated draw), 6.6 ... 36 % of a saturated draw
   above the bound.

3. Sharpness (`test_defects_are_seen`): nine defects of the kind the old inputs hide, applied to the oracle itself on the new
   inputs, each measured like the GPU test measures a kernel (|delta| / |want| on x and x_prev at both horizons).  A defect
   confined to one element or one row (zeroed last row, zeroed row N - 1, one neuron's ext dropped, neuron N - 1 stepped with
   the I population's dt / tau) must move EVERY element it concerns by at least 100 times the tolerance.  A defect that
   concerns many elements to different degrees (a zeroed column reaches a neuron through W_ij of any size; two stimuli or two
   draws may give a neuron nearly the same ext; a neuron may be nearly at rest between two steps) must move at least a
   quarter of them by that much, where one such element already fails the GPU test (measured: 55 ... 100 %).  A defect counts
   as seen at an element if x or x_prev moves there at one of the two horizons: a (case, variant) of the GPU module asserts
   all four.  A case that misses gets another seed in `solver_cases.RESEED`.
"""
import numpy as np
import pytest

from oracle import solver_cases as sc
from test_solver_gpu import _inputs as old_inputs

IDS = [sc.case_id(c) for c in sc.CASES]


# ---------------------------------------------------------------------------------------------------------------- 1. the gap
GAP = {  # (N, NB): row N - 1, column N - 1, row 0, column 2N - 1, row 2N - 1
    (102, 3): (3.1e-7, 5.8e-12, 3.1e-7, 0.94, 6.8e2),
    (102, 5): (2.5e-5, 7.7e-12, 2.5e-5, 3.8, 1.4e3),
    (76, 3): (3.1e-7, 5.8e-12, 3.1e-7, 3.8, 1.5e3),
    (75, 2): (3.4e-8, 4.5e-12, 3.4e-8, 0.31, 3.1e2),
    (100, 8): (4.0e3, 4.9e3, 5.0e3, 8.6e3, 9.9e3),
}


def _gap(N, NB, io_type='asym_tanh'):
    """Share of the old test's expected end state below its atol, what the end neurons hold, and the old measure of the five
    zeroed rows / columns."""
    B, steps, M = 6, 300, 2 * N
    Ws, exts = old_inputs(N, B, NB, seed=N * 31 + NB)
    ext, r0 = np.broadcast_to(exts, (B, NB, M)), np.zeros((B, NB, M))
    want = sc.euler(Ws, ext, r0, io_type, steps=steps)[-1]
    seen = []
    for axis, idx in ((1, N - 1), (2, N - 1), (1, 0), (2, M - 1), (1, M - 1)):
        W = Ws.copy()
        W[(slice(None),) * axis + (idx,)] = 0.0
        got = sc.euler(W, ext, r0, io_type, steps=steps)[-1]
        seen.append((np.abs(got - want) / (1e-4 * np.abs(want) + 1e-6)).max())
    narrow = np.asarray(sc.P['bandwidths'][:NB]) < 0.75
    return (want < 1e-6).mean(), want[:, narrow][:, :, [0, N - 1]].max(), seen


@pytest.mark.parametrize('N,NB', [(102, 3), (102, 5), (76, 3), (75, 2)])
def test_the_gap_old_inputs_hide_the_edge_rows_and_columns_of_the_E_population(N, NB):
    below_atol, ends, seen = _gap(N, NB)
    print('GAP N=%d NB=%d below atol %.2f ends %.1e seen %s' % (N, NB, below_atol, ends, ' '.join('%.1e' % v for v in seen)))
    assert 0.16 <= below_atol <= 0.30                   # not compared at all
    assert ends < 1e-14                                 # neurons 0 and N - 1 in every stimulus narrower than 0.75
    assert max(seen[:3]) <= 1e-4                        # below the old acceptance by at least 1e4
    for got, recorded in zip(seen, GAP[N, NB]):
        assert recorded / 3 <= got <= 3 * recorded, (seen, GAP[N, NB])


def test_the_gap_closes_only_where_the_widest_stimulus_is_among_them():
    below_atol, _, seen = _gap(100, 8)
    print('GAP N=100 NB=8 below atol %.2f seen %s' % (below_atol, ' '.join('%.1e' % v for v in seen)))
    assert min(seen) > 1e3
    for got, recorded in zip(seen, GAP[100, 8]):
        assert recorded / 3 <= got <= 3 * recorded, (seen, GAP[100, 8])


# ------------------------------------------------------------------------------------------------------------ 2. every case
FLOOR, F32_CLOSE, SATURATED_SHARE = 1e-3, 2.5e-5, 0.05


def test_case_list():
    assert len(set(sc.CASES)) == len(sc.CASES) and len(set(IDS)) == len(IDS)
    assert not set(sc.RESEED) - set(IDS)
    # every kernel, grid and stimulus grouping the GPU module must see run is reached by some (case, variant)
    reached = {k for c in sc.CASES for v in sc.variants(c) if sc.supported(c, v) for k in sc.ran(c, v)}
    assert not [k for k in sc.coverage() if k not in reached]
    # and every variant refuses somewhere, so that the refusal is seen as well
    for v in (1, 2, 3, 4, 5, 6, 7, 8):
        assert any(not sc.supported(c, v) for c in sc.CASES if v in sc.variants(c)), v


@pytest.mark.parametrize('c', sc.CASES, ids=IDS)
def test_case_conditions(oracle_lib, c):
    x = sc.inputs(c)
    for a in x.values():
        assert np.array_equal(a.astype(c.dtype).astype('float64'), a)
    assert x['ext'].shape == ((c.NB, c.M) if c.shared else (sc.B, c.NB, c.M)) and (x['r0'] > 0).all()
    traj = sc.trajectory(c)
    assert np.isfinite(traj).all()
    sat = sc.saturated_draws(c)
    floor = 1.0
    for k, (want, prev, codes, steps) in sc.oracle(c).items():
        assert (codes == 1).all() and (steps == k).all()
        np.testing.assert_allclose(traj[k], want, rtol=1e-12, atol=0)
        np.testing.assert_allclose(traj[k - 1], prev, rtol=1e-12, atol=0)
        for a in (want, prev):
            assert np.isfinite(a).all()
            floor = min(floor, (a / a.max(axis=-1, keepdims=True)).min())
    share = (traj[1:, sat] > sc.SOFT).mean() if sat.any() else None
    f32 = sc.per_draw_max(np.moveaxis(sc.rel_err(sc.trajectory(c, 'float32'), traj), 0, 1)) if c.dtype == 'float32' else np.zeros(sc.B)
    print('CASE %s floor %.2e float32 run %.2e (saturated draw %.2e) share above the bound %s' % (
        sc.case_id(c), floor, f32[~sat].max(), f32[sat].max() if sat.any() else 0.0, share))
    assert floor >= FLOOR
    assert (f32 <= F32_CLOSE).all(), f32
    if sat.any():
        assert share >= SATURATED_SHARE
        assert c.io_type == 'asym_tanh' and sat[-1] and sat.sum() == 1


# ------------------------------------------------------------------------------------------------------------- 3. sharpness
def _defects(c, x):
    """name -> (keywords of `euler` that differ from the true run, or None for 'x_prev = x'; mask (B, NB, M) of the elements
    the defect concerns; whether every one of them must move)."""
    N, M, NB = c.M // 2, c.M, c.NB
    b, s = 1, NB - 1                                    # an unsaturated draw that is not the first; the last stimulus
    W, ext = x['W'], sc.ext_per_draw(c, x)

    def mask(*idx):
        m = np.zeros((sc.B, NB, M), dtype=bool)
        m[idx] = True
        return m

    def zeroed(axis, i):
        W2 = W.copy()
        W2[(b,) + (slice(None),) * (axis - 1) + (i,)] = 0.0
        return dict(W=W2)

    def reached(col):               # the neurons of draw b that column `col` feeds with at least half its largest weight to their population
        w = np.abs(W[b, :, col]).reshape(2, N)
        return mask(b, slice(None), np.nonzero((w >= 0.5 * w.max(axis=1, keepdims=True)).ravel())[0])

    out = {
        'zeroed last row of one draw': (zeroed(1, M - 1), mask(b, slice(None), M - 1), True),
        'zeroed last column of one draw': (zeroed(2, M - 1), reached(M - 1), False),
        'zeroed row N - 1': (zeroed(1, N - 1), mask(b, slice(None), N - 1), True),
        'zeroed column N - 1': (zeroed(2, N - 1), reached(N - 1), False),
        'neuron N - 1 with the I step': (dict(eps=np.where(np.arange(M) < N - 1, sc.DT / sc.P['tau'][0], sc.DT / sc.P['tau'][1])),
                                         mask(slice(None), slice(None), N - 1), True),
        'x_prev = x': (None, mask(), False),
    }
    e = ext.copy()
    e[b, s, M - 1] = 0.0
    out['one ext dropped'] = (dict(ext=e), mask(b, s, M - 1), True)
    if NB > 1:
        e = ext.copy()
        e[:, s] = ext[:, s - 1]
        out['stimulus s reads s - 1'] = (dict(ext=e), mask(slice(None), s), False)
    if not c.shared:
        e = ext.copy()
        e[b] = ext[b - 1]
        out['draw b reads b - 1'] = (dict(ext=e), mask(b), False)
    return out


@pytest.mark.parametrize('c', sc.CASES, ids=IDS)
def test_defects_are_seen(c):
    x = sc.inputs(c)
    traj = sc.trajectory(c)
    need = 100 * sc.RTOL[c.dtype]
    for name, (changed, concerns, every) in _defects(c, x).items():
        if changed is None:
            worst = np.maximum(*(sc.rel_err(traj[k], traj[k - 1]) for k in sc.HORIZONS))
            concerns = np.ones_like(concerns)
        else:
            kw = dict(W=x['W'], ext=sc.ext_per_draw(c, x), r0=x['r0'], io_type=c.io_type)
            kw.update(changed)
            bad = sc.euler(**kw)
            # seen at one of the horizons, in x or in x_prev: a (case, variant) of the GPU module asserts all four
            worst = np.maximum(*(np.maximum(sc.rel_err(bad[k], traj[k]), sc.rel_err(bad[k - 1], traj[k - 1])) for k in sc.HORIZONS))
        seen = worst[concerns] >= need
        print('DEFECT %s %s: %d of %d concerned elements beyond 100 x tol, smallest %.1e x tol' % (
            sc.case_id(c), name, seen.sum(), seen.size, worst[concerns].min() / sc.RTOL[c.dtype]))
        assert seen.all() if every else seen.mean() >= 0.25, name

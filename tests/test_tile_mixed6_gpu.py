"""`solve_tile_mixed6_kernel` (csrc/ssn_tile.hip): the fp32 NB = 1 tile solver with rows split 56/48/48/48 -- wave 0 a 7-row
tile, waves 1-3 a 6-row tile -- which every size 2N >= MIXED6_MIN_M of the C = 25 grid runs (test_tile_mixed6_build.py holds the
constant to the source).

What is new in it, and what each test here holds it to:

  * the 6-row tile: two register row pairs and a third pair whose columns 0-11 are in VGPRs and 12-24 in LDS, the last of them
    alone in its unit; a transpose-reduce with two masked adds; an LDS image per wave.  One step on integer inputs is exact in
    any order, so the all-register kernel (variant 4) must give the same bits: W with row i = i + 1 (a row that lands in another
    row's lane shows), W that is nonzero only in columns 11 and 12 of every column group (the seam), only in column 24 (the
    last unit), and a dense one.
  * every row, element by element: seven steps on real weights with every neuron driven (oracle/solver_cases.py) against the
    fp64 oracle at RTOL32, x and x_prev, no absolute term.
  * the stop protocol at the new wave boundaries: the design of tests/test_tile_verdict_gpu.py (W = 0, one moving row j whose
    last moving step k is odd or even, a partner row in another wave, expected values from the replayed stop rule) with j the
    first and last row of each wave's new row range.
  * the layout counts on the hardware to spread the 7-row waves of co-resident workgroups over the SIMDs, for speed only:
    8 draws, each repeated 192 times in one launch (two full rounds of three workgroups per CU), must give 192 equal copies
    of what a launch of the 8 alone gives, bit for bit.  No test reads a hardware register.

Sizes: 200, 198 (ragged last column group) and MIXED6_MIN_M.  Wave 3 starts at row 152 and dispatch admits no size below
170, so there is no size at which it has fewer than 8 real rows.
"""
import numpy as np
import pytest

import test_tile_verdict_gpu as tv
from oracle import solver_cases as sc

pytestmark = pytest.mark.gpu

MIXED6_MIN_M = 170                                  # ssn_tile.hip: TILE_MIXED6_MIN_M
SIZES = sorted({200, 198, MIXED6_MIN_M}, reverse=True)
WAVE_START = (0, 56, 104, 152)


# ---- 1. the same bits wherever a workgroup runs -----------------------------------------------------------------------

@pytest.mark.parametrize('M', SIZES)
def test_result_does_not_depend_on_where_a_workgroup_runs(M):
    import torch
    from tc_gan_amd import ssnode
    COPIES, DRAWS = 192, 8
    x = sc.inputs(sc.Case('float32', 'asym_tanh', M, 1, False))
    rs = np.random.RandomState(M)
    W = torch.as_tensor(x['W'][rs.randint(0, sc.B, DRAWS)], dtype=torch.float32).cuda()
    ext = torch.as_tensor(rs.uniform(0.5, 5.0, (DRAWS, 1, M)), dtype=torch.float32).cuda()
    r0 = torch.as_tensor(rs.uniform(0.0125, 5.0, (DRAWS, 1, M)), dtype=torch.float32).cuda()

    def solve(n):
        # atol > 0: draws may stop at their own steps, so codes and steps carry information
        res = ssnode.fixed_points_batch(W.repeat(n, 1, 1), ext.repeat(n, 1, 1), sc.P['k'], sc.P['n'], r0=r0.repeat(n, 1, 1),
                                        max_iter=12, atol=0.05, dt=sc.DT, io_type='asym_tanh', dtype='float32', variant=None,
                                        return_torch=True)
        return [a.cpu().numpy() for a in (res.x, res.codes, res.steps)]

    one, many = solve(1), solve(COPIES)
    print('2N=%d: steps %d..%d, codes %s' % (M, one[2].min(), one[2].max(), np.unique(one[1]).tolist()))
    assert np.isfinite(one[0]).all() and len(np.unique(one[0].view(np.uint32).reshape(DRAWS, -1), axis=0)) == DRAWS
    for a, b in zip(one, many):
        b = b.reshape((COPIES,) + a.shape)
        assert b.shape[0] == COPIES
        np.testing.assert_array_equal(b.view(np.uint32) if b.dtype == np.float32 else b,
                                      np.broadcast_to(a.view(np.uint32) if a.dtype == np.float32 else a, b.shape))


# ---- 2. every row, element by element, against the fp64 oracle -----------------------------------------------------------

@pytest.mark.parametrize('io_type', ['asym_tanh', 'asym_power'])
@pytest.mark.parametrize('M', SIZES)
def test_every_row_against_fp64(oracle_lib, M, io_type):
    from tc_gan_amd.ssnode import fixed_points_batch
    c = sc.Case('float32', io_type, M, 1, False)
    x = sc.inputs(c)
    steps = 7
    want, want_prev, wcodes, wsteps = sc.c_oracle(c, steps)
    assert (want > 0).all() and (want_prev > 0).all()
    res = fixed_points_batch(x['W'], x['ext'], sc.P['k'], sc.P['n'], r0=x['r0'], max_iter=steps, atol=0.0, dt=sc.DT,
                             io_type=io_type, rate_stop_at=np.inf, dtype='float32', variant=None, want_prev=True)
    np.testing.assert_array_equal(res.codes, wcodes)
    np.testing.assert_array_equal(res.steps, wsteps)
    ex, ep = sc.rel_err(res.x, want), sc.rel_err(res.x_prev, want_prev)
    print('2N=%d %s: x %.2e (row %d) x_prev %.2e' % (M, io_type, ex.max(), int(ex.max(axis=(0, 1)).argmax()), ep.max()))
    rtol = sc.RTOL['float32']
    assert (ex <= rtol).all(), np.argwhere(ex > rtol)[:8]
    assert (ep <= rtol).all(), np.argwhere(ep > rtol)[:8]


# ---- 3. the tile forms, exact -----------------------------------------------------------------------------------------

def _integer_w(kind, M):
    i, j = np.meshgrid(np.arange(M), np.arange(M), indexing='ij')
    C = 25
    if kind == 'row':
        return (i + 1.0) * np.ones((M, M))
    dense = (i * 7 + j * 3) % 11 - 3.0
    if kind == 'dense':
        return dense
    cols = {'seam': (11, 12), 'last': (24,)}[kind]
    return np.where(np.isin(j % C, cols), (i * 3 + j) % 13 + 1.0, 0.0)


@pytest.mark.parametrize('kind', ['row', 'seam', 'last', 'dense'])
@pytest.mark.parametrize('M', SIZES)
def test_one_step_on_integers_equals_the_all_register_kernel(M, kind):
    from tc_gan_amd.ssnode import fixed_points_batch
    W = np.stack([_integer_w(kind, M), _integer_w(kind, M).T.copy()])          # (2, M, M)
    r0 = (np.arange(M) * 5 % 7 + 1.0)[None, None].repeat(2, axis=0)             # 1 .. 7
    ext = (np.arange(M) % 9 + 1.0)[None, None].repeat(2, axis=0)
    # every partial sum is an integer below 2^24: |W| <= 200, r <= 7, 200 columns
    assert np.abs(W).max() * 7 * M < 2 ** 24
    v = np.einsum('bij,bsj->bsi', W, r0) + ext
    assert len(np.unique(v[0, 0])) > M // 8 and (v > 0).sum() > M // 2
    opts = dict(r0=r0, max_iter=1, atol=0.0, dt=sc.DT, io_type='asym_power', rate_stop_at=np.inf, dtype='float32', want_prev=True)
    got = fixed_points_batch(W, ext, sc.P['k'], sc.P['n'], variant=None, **opts)
    ref = fixed_points_batch(W, ext, sc.P['k'], sc.P['n'], variant=4, **opts)
    assert np.isfinite(ref.x).all() and (ref.codes == 1).all() and (ref.steps == 1).all()
    bad = np.argwhere(got.x.view(np.uint32) != ref.x.view(np.uint32))
    assert bad.size == 0, (kind, bad[:8].tolist())
    np.testing.assert_array_equal(got.x_prev.view(np.uint32), ref.x_prev.view(np.uint32))
    np.testing.assert_array_equal(got.codes, ref.codes)
    np.testing.assert_array_equal(got.steps, ref.steps)


# ---- 4. the stop protocol at the new wave boundaries --------------------------------------------------------------------

def _wave(row):
    return sum(row >= s for s in WAVE_START) - 1


# a row of another wave than row j's -- and of another 56-row block, which the borrowed design asserts
PARTNER_OF_WAVE = {0: 60, 1: 120, 2: 170, 3: 3}
STOP_ROWS = [0, 55, 56, 103, 104, 151, 152, 199]
STOP_CASES = [tv.Case(kind, 200, None, j, k, tv.T) for kind in ('last', 'bound', 'mirror') for j in STOP_ROWS for k in tv.KS]


@pytest.mark.parametrize('c', STOP_CASES, ids=['{}-row{}-k{}'.format(c.kind, c.j, c.k) for c in STOP_CASES])
def test_one_wave_decides_the_verdict_at_the_new_boundaries(oracle_lib, monkeypatch, c):
    partner = PARTNER_OF_WAVE[_wave(c.j)]
    assert _wave(partner) != _wave(c.j)
    monkeypatch.setattr(tv, '_partner', lambda M, j: partner)
    monkeypatch.setattr(tv, 'CASES', [c])
    monkeypatch.setattr(tv, 'IDS', ['{}-2N{}-v{}-row{}-k{}-T{}'.format(*c)])
    tv.test_one_wave_decides_the_verdict(oracle_lib, c)

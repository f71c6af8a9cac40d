"""The transpose-reduce of `solve_tile_mixed6_kernel` on DPP bank masks (csrc/ssn_tile_core.h: reduce_bank_f32), and the lane map
that goes with it: the lane with bits b5 .. b0 is row group b1 | b4 << 1 | b5 << 2, owns the columns of group
((b3 << 1) | b0) ^ (b2 ? 7 : 0) and finishes row 4 b2 + 2 b3 + b0 of its row group, if the tile has that row.

  1. One step on integer inputs, bit for bit against the all-register kernel (variant 4): r = 1 and W nonzero only in the first
     column of each column group, (i + 1) + 211 c for row i and group c.  Every partial sum is one integer, every row total an
     integer below 2^24 that names its row and, term by term, its column groups: a partial routed to another row, dropped or
     added twice changes it.
  2. The tree.  One nonzero column per (row, column group), so that a lane's partial sum is one product, exact; magnitudes
     10^-3 .. 10^3 and mixed signs, so that the order of the 8-term sum shows in fp32 -- asserted on the CPU: summing adjacent
     groups first, ((0,1),(2,3)),((4,5),(6,7)), changes the bits of at least a quarter of the rows against the kernels' tree,
     ((0,7),(2,5)),((1,6),(3,4)).  On the GPU 1 and 3 steps are bit-identical between the library's choice and variants 3 and 4
     (the all-register kernel keeps the DPP sequence with selects and has the same tree).
  3. The checks of test_tile_mixed6_gpu.py through the new lane map: the stop protocol with the moving row at both ends of every
     wave's range, and 192 copies of 8 draws in one launch equal to a launch of the 8.

Sizes 200, 198 (ragged last column group) and 170 (no column in group 7, 20 in group 6), 8 draws.
"""
import numpy as np
import pytest

import test_tile_mixed6_gpu as t6
from oracle import solver_cases as sc

pytestmark = pytest.mark.gpu

SIZES = [200, 198, 170]
DRAWS, C = 8, 25
TREE = (((0, 7), (2, 5)), ((1, 6), (3, 4)))
ADJACENT = (((0, 1), (2, 3)), ((4, 5), (6, 7)))


def _ncols(M, c):
    return max(0, min(C, M - C * c))


def _solve(W, ext, r0, steps, variant):
    from tc_gan_amd.ssnode import fixed_points_batch
    return fixed_points_batch(W, ext, sc.P['k'], sc.P['n'], r0=r0, max_iter=steps, atol=0.0, dt=sc.DT, io_type='asym_power',
                              rate_stop_at=np.inf, dtype='float32', variant=variant, want_prev=True)


def _assert_same(got, ref, what):
    bad = np.argwhere(got.x.view(np.uint32) != ref.x.view(np.uint32))
    assert bad.size == 0, (what, bad[:8].tolist())
    np.testing.assert_array_equal(got.x_prev.view(np.uint32), ref.x_prev.view(np.uint32), err_msg=what)
    np.testing.assert_array_equal(got.codes, ref.codes, err_msg=what)
    np.testing.assert_array_equal(got.steps, ref.steps, err_msg=what)


# ---- 1. integers ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('M', SIZES)
def test_one_step_on_integers_names_every_row_and_column_group(M):
    W = np.zeros((DRAWS, M, M))
    i = np.arange(M)
    for c in range(8):
        if _ncols(M, c):
            W[:, i, C * c] = (i + 1.0) + 211.0 * c
    W[1::2] = np.transpose(W[1::2], (0, 2, 1)).copy()          # odd draws: the transpose (one dense row per column group)
    r0 = np.ones((DRAWS, 1, M))
    ext = (np.arange(M) % 7 + 1.0)[None, None].repeat(DRAWS, axis=0)
    v = np.einsum('bij,bsj->bsi', W, r0) + ext
    assert np.abs(v).max() < 2 ** 24 and len(np.unique(v[0, 0])) == M
    got, ref = _solve(W, ext, r0, 1, None), _solve(W, ext, r0, 1, 4)
    assert np.isfinite(ref.x).all() and (ref.codes == 1).all() and (ref.steps == 1).all()
    assert len(np.unique(ref.x[0, 0])) > M // 2
    _assert_same(got, ref, 'library against variant 4')


# ---- 2. the tree ---------------------------------------------------------------------------------------------------------

def _tree_sum(p, tree):
    """fp32 sum of p[..., 8] in the order of a nested tuple of column groups."""
    if isinstance(tree, int):
        return p[..., tree]
    return (_tree_sum(p, tree[0]) + _tree_sum(p, tree[1])).astype(np.float32)


_TREE_INPUTS = {}


def _tree_inputs(M):
    if M not in _TREE_INPUTS:
        rs = np.random.RandomState(1000 + M)
        W = np.zeros((DRAWS, M, M), dtype=np.float32)
        col = np.zeros((DRAWS, M, 8), dtype=int)
        val = np.zeros((DRAWS, M, 8), dtype=np.float32)
        i = np.arange(M)
        for c in range(8):
            n = _ncols(M, c)
            if not n:
                continue
            for b in range(DRAWS):
                col[b, :, c] = C * c + rs.randint(0, n, M)
                val[b, :, c] = (10.0 ** rs.uniform(-3, 3, M) * rs.choice([-1.0, 1.0], M)).astype(np.float32)
                W[b, i, col[b, :, c]] = val[b, :, c]
        r0 = (rs.uniform(0.5, 2.0, (DRAWS, 1, M)) * 1e-3).astype(np.float32)
        ext = rs.uniform(0.5, 5.0, (DRAWS, 1, M)).astype(np.float32)
        _TREE_INPUTS[M] = (W, ext, r0, col, val)
    return _TREE_INPUTS[M]


@pytest.mark.parametrize('M', SIZES)
def test_inputs_show_the_order_of_the_sum(M):
    """(needs no GPU; it is here because it is about the inputs of the test below)"""
    W, ext, r0, col, val = _tree_inputs(M)
    assert ((W != 0).sum(axis=2) == sum(1 for c in range(8) if _ncols(M, c))).all()
    b = np.arange(DRAWS)[:, None, None]
    p = (val * r0[b, 0, col]).astype(np.float32)               # the 8 partial sums of every row: one product each
    p[..., [c for c in range(8) if not _ncols(M, c)]] = 0
    tree, adjacent = _tree_sum(p, TREE), _tree_sum(p, ADJACENT)
    differ = (tree.view(np.uint32) != adjacent.view(np.uint32)).mean()
    print('2N=%d: %.0f %% of the rows change bits with adjacent groups first' % (M, 100 * differ))
    assert differ >= 0.25


@pytest.mark.parametrize('steps', [1, 3])
@pytest.mark.parametrize('M', SIZES)
def test_tree_bits_equal_the_kernels_that_keep_the_old_sequence(M, steps):
    W, ext, r0, _, _ = _tree_inputs(M)
    got = _solve(W, ext, r0, steps, None)
    assert np.isfinite(got.x).all() and (got.x > 0).all() and (got.steps == steps).all()
    # (a row whose input is not positive only decays: the rows that carry their sum into the state are the others)
    assert (got.x > got.x_prev).mean() > 0.25
    for variant in (3, 4):
        _assert_same(got, _solve(W, ext, r0, steps, variant), 'library against variant %d, %d steps' % (variant, steps))


# ---- 3. the checks of test_tile_mixed6_gpu.py through the new lane map ------------------------------------------------------

@pytest.mark.parametrize('c', t6.STOP_CASES, ids=['{}-row{}-k{}'.format(c.kind, c.j, c.k) for c in t6.STOP_CASES])
def test_stop_protocol_at_both_ends_of_every_waves_rows(oracle_lib, monkeypatch, c):
    assert sorted({c.j for c in t6.STOP_CASES}) == [0, 55, 56, 103, 104, 151, 152, 199]
    t6.test_one_wave_decides_the_verdict_at_the_new_boundaries(oracle_lib, monkeypatch, c)


@pytest.mark.parametrize('M', SIZES)
def test_192_copies_of_8_draws_equal_a_launch_of_the_8(M):
    t6.test_result_does_not_depend_on_where_a_workgroup_runs(M)

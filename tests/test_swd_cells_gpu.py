"""The sliced Wasserstein match per condition cell on the GPU (csrc/ssn_swd_cells.hip through libssnode_ext2.so) against the
restatement of tests/swd_cells_cases.py: the coefficients bit for bit, loss_cl bit for bit against the kernel-order restatement
and within the derived bound of the exact rational; the one-cell equality with the first companion's match of two sizes, which
guards the restated walk; non-finite values, repeatability, the exact lattice, refusals; the host function.

Cell sizes: an empty cell first, in the middle and last; one and two rows; both sides of the padding of 64 (63, 64, 65) and of
the 256-thread stride (257); the rows of the cells interleaved in x.  Truth sizes: one row, below, at and above the padding
(7, 64, 65), and 1000 (the default truth).  The limits: the largest cell with the largest truth (96 KiB of LDS) beside an empty
cell, and the longest walk of one rank's neighbour (n = 4096, m = 1) beside a cell of one row."""
import ctypes
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import swd_cells_cases as cc
import swd_sizes_cases as zc
from tc_gan_amd import clib
from tc_gan_amd.clib import libssnode_ext, libssnode_ext2
from tc_gan_amd.networks.conditional_sliced_wasserstein import cswd_loss_grad

pytestmark = pytest.mark.gpu

D = 6
#: the cell sizes of a call with C cells
CELL_SIZES = {1: (65,), 3: (0, 257, 0), 18: (0, 1, 2, 63, 64, 65, 257, 1, 0, 0, 2, 65, 64, 63, 1, 257, 2, 0)}


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype).contiguous()


@functools.lru_cache(maxsize=None)
def _case(sizes, m, L, power, kind='generic'):
    """Inputs and restatement of one case, computed once and shared by the tests that need it (read only)."""
    make = cc.generic_inputs if kind == 'generic' else cc.lattice_inputs
    x, cells, y, theta = make(np.random.RandomState(1000 * L + sum(sizes) + m), sizes, m, L, D)
    return x, cells, y, theta, cc.swd_cells(x, cells, y, theta, power)


def _device_match(px, cell_rows, cell_start, py, power):
    """The match alone on float32 numpy projections -> (coef, loss_cl); the outputs are filled beforehand with values the
    kernel does not write."""
    (B, L), (C, m) = px.shape, py.shape[:2]
    pxd, pyd, rows = _dev(px), _dev(py), _dev(cell_rows, torch.int32)
    coef = torch.full((B, L), 7.0, device='cuda')
    loss_cl = torch.full((C, L), -7.0, device='cuda', dtype=torch.float64)
    start = np.ascontiguousarray(cell_start, dtype=np.int32)
    clib.check_ext2(libssnode_ext2.ssnx2_swd_match_cells_f32(
        pxd.data_ptr(), B, rows.data_ptr(), start.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), C, pyd.data_ptr(), m, L, power,
        coef.data_ptr(), loss_cl.data_ptr(), clib.stream_ptr()), 'ssnx2_swd_match_cells_f32')
    return coef.cpu().numpy(), loss_cl.cpu().numpy()


def _check_against_restatement(sizes, m, L, power):
    want = _case(sizes, m, L, power)[4]
    coef, loss_cl = _device_match(want['px'], want['cell_rows'], want['cell_start'], want['py'], power)
    np.testing.assert_array_equal(coef.view(np.uint32), want['coef'].view(np.uint32))
    ordered = cc.loss_cl_in_kernel_order(want['px'], want['cell_rows'], want['cell_start'], want['py'], power)
    np.testing.assert_array_equal(loss_cl.view(np.uint64), ordered.view(np.uint64))
    worst = Fraction(0)
    for c, n in enumerate(sizes):
        for l in range(L):
            exact = want['loss_cl'][c][l]
            err = abs(Fraction(float(loss_cl[c, l])) - exact)
            assert err <= zc.loss_bound(exact, n, m), (c, l, float(err), float(exact))
            if exact:
                worst = max(worst, err / exact)
        if n == 0:                                                # +0, not -0, and nothing else of the cell
            assert (loss_cl[c] == 0).all() and not np.signbit(loss_cl[c]).any()
    print('sizes, m, L, p =', (sizes, m, L, power), 'largest relative error of loss_cl:', float(worst))
    if L >= 2 and D >= 2:                                         # the tied direction: d = 0 at every pair of every cell
        assert (coef[:, L // 2] == 0).all() and (loss_cl[:, L // 2] == 0).all() and not np.signbit(coef[:, L // 2]).any()


@pytest.mark.parametrize('power', [1, 2])
@pytest.mark.parametrize('C', [1, 3, 18])
def test_generic_inputs_bit_for_bit_and_loss_within_the_bound(C, power):
    """Every truth size with every number of directions in one test (the cases are small; an assertion names its case)."""
    for m in (1, 7, 64, 65, 1000):
        for L in (1, 3, 33):
            _check_against_restatement(CELL_SIZES[C], m, L, power)


def test_the_limits():
    for sizes, m in (((4096, 0), 16384), ((1, 4096), 1)):
        for power in (1, 2):
            _check_against_restatement(sizes, m, 2, power)


def test_one_cell_is_the_first_companions_match_bit_for_bit():
    """C = 1, cell_rows the identity: coef and loss_cl[0] are the bits `ssnx_swd_match_sizes_f32` writes on the same inputs.
    The walk is written twice (the two libraries share no header): this holds the two copies together."""
    for n, m, L in ((1, 1, 1), (65, 64, 3), (15, 1000, 33), (300, 257, 3), (1024, 1000, 2)):
        for power in (1, 2):
            _one_cell_case(n, m, L, power)


def _one_cell_case(n, m, L, power):
    x, y, theta = zc.generic_inputs(np.random.RandomState(n + m + L), n, m, L, D)
    px, py = cc.project_rows(x, theta), cc.project_rows(y, theta)
    pxd, pyd = _dev(px), _dev(py)
    coef1 = torch.full((n, L), 7.0, device='cuda')
    loss1 = torch.full((L,), -7.0, device='cuda', dtype=torch.float64)
    clib.check_ext(libssnode_ext.ssnx_swd_match_sizes_f32(pxd.data_ptr(), n, pyd.data_ptr(), m, L, power, coef1.data_ptr(),
                                                          loss1.data_ptr(), clib.stream_ptr()), 'ssnx_swd_match_sizes_f32')
    coef2, loss2 = _device_match(px, np.arange(n), np.array([0, n]), py[None], power)
    assert coef1.cpu().numpy().tobytes() == coef2.tobytes(), (n, m, L, power)
    assert loss1.cpu().numpy().tobytes() == loss2[0].tobytes(), (n, m, L, power)
    assert np.abs(coef2).max() > 0


def test_a_non_finite_value_touches_its_cell_and_direction_only():
    for where in ('x', 'y'):
        for value in (np.nan, np.inf, -np.inf):
            _non_finite_case(where, value)


def _non_finite_case(where, value):
    sizes, m, L = CELL_SIZES[18], 65, 3
    for power in (1, 2):
        clean = _case(sizes, m, L, power)[4]
        px, py = clean['px'].copy(), clean['py'].copy()
        c = 5                                                     # a cell of 65 rows
        rows = clean['cell_rows'][clean['cell_start'][c]:clean['cell_start'][c + 1]]
        if where == 'x':
            px[rows[17], 1] = value
        else:
            py[c, 17, 1] = value
        coef, loss_cl = _device_match(px, clean['cell_rows'], clean['cell_start'], py, power)
        assert np.isnan(loss_cl[c, 1]) and np.isnan(coef[rows, 1]).all()
        keep = np.ones_like(coef, dtype=bool)
        keep[rows, 1] = False
        np.testing.assert_array_equal(coef[keep].view(np.uint32), clean['coef'][keep].view(np.uint32))
        ordered = cc.loss_cl_in_kernel_order(clean['px'], clean['cell_rows'], clean['cell_start'], clean['py'], power)
        keep = np.ones_like(loss_cl, dtype=bool)
        keep[c, 1] = False
        np.testing.assert_array_equal(loss_cl[keep].view(np.uint64), ordered[keep].view(np.uint64))
        want_coef, want_loss = cc.match_cells(px, clean['cell_rows'], clean['cell_start'], py, power)
        assert want_loss[c][1] is None and np.isnan(want_coef[rows, 1]).all()


def test_two_launches_give_the_same_bits():
    for power in (1, 2):
        want = _case(CELL_SIZES[18], 65, 33, power)[4]
        args = (want['px'], want['cell_rows'], want['cell_start'], want['py'], power)
        a, b = _device_match(*args), _device_match(*args)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_lattice_inputs_give_the_exact_loss():
    for sizes, m, L in (((1,), 1, 1), ((2, 0, 4, 2), 8, 2), ((64, 32, 16, 16), 16, 4), ((0, 256), 64, 2)):
        for power in (1, 2):
            want = _case(sizes, m, L, power, 'lattice')[4]
            coef, loss_cl = _device_match(want['px'], want['cell_rows'], want['cell_start'], want['py'], power)
            assert [[Fraction(float(v)) for v in row] for row in loss_cl] == want['loss_cl'], (sizes, m, L, power)
            np.testing.assert_array_equal(coef.view(np.uint32), want['coef'].view(np.uint32))


def test_refusals_write_nothing():
    buf = torch.zeros(64, device='cuda')
    rows = torch.zeros(64, device='cuda', dtype=torch.int32)
    out = torch.zeros(64, device='cuda', dtype=torch.float64)

    def call(B, start, C, m):
        start = np.asarray(start, dtype=np.int32)
        return libssnode_ext2.ssnx2_swd_match_cells_f32(buf.data_ptr(), B, rows.data_ptr(),
                                                        start.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), C, buf.data_ptr(), m, 1,
                                                        2, buf.data_ptr(), out.data_ptr(), clib.stream_ptr())
    for args, what in (((8, [0, 9], 1, 8), 'does not end at B'), ((8, [0, 8], 1, clib.SWD_MAX_TRUTH + 1), '16384 truth rows'),
                       ((8, [0, 8], 1, 0), 'no truth rows'), ((8, [0, 5, 3, 8], 3, 8), 'decreases'),
                       ((8, [1, 8], 1, 8), 'start at 0'), ((5000, [0, 4097, 5000], 2, 8), '4096 generated rows')):
        assert call(*args) == clib.SSN_ERR_BASE + 1 and what in clib.ext2_last_error(), args
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0 and float(buf.abs().sum()) == 0


# ---- the host function ---------------------------------------------------------------------------------------------------

def test_cswd_loss_grad_is_the_restatement():
    for C, m, L in ((18, 65, 33), (3, 1000, 3), (1, 7, 1), (18, 1000, 3)):
        for power in (1, 2):
            _host_case(C, m, L, power)


def _host_case(C, m, L, power):
    sizes = CELL_SIZES[C]
    x, cells, y, theta, want = _case(sizes, m, L, power)
    gx, swd, loss_cl = cswd_loss_grad(_dev(x), cells, _dev(y), _dev(theta), power)
    np.testing.assert_array_equal(gx.cpu().numpy().view(np.uint32), want['gx'].view(np.uint32))
    ordered = cc.loss_cl_in_kernel_order(want['px'], want['cell_rows'], want['cell_start'], want['py'], power)
    assert loss_cl.shape == (C, L) and loss_cl.dtype == np.float64
    np.testing.assert_array_equal(loss_cl.view(np.uint64), ordered.view(np.uint64))
    assert swd == cc.swd_in_host_order(ordered, want['cell_start'])[0]
    np.testing.assert_allclose(swd, want['swd'], rtol=(max(sizes) + m + L + C + 8) * 2.0 ** -52)

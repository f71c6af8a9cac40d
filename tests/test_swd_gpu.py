"""The kernels of the sliced Wasserstein loss on the GPU (csrc/ssn_swd.hip) against the restatement of tests/swd_cases.py: the
coefficients and the gradient bit for bit, the loss per direction equal to the exact value on a lattice and within the derived
bound on generic values, against the scorer's W1 kernel for p = 1, non-finite inputs, repeatability, the refusal.

The shapes are the smallest that cover the paths: B = 1 and 2 (padded to 64), 63, 64 (no padding), 65 (P = 128), 257 and 300 (more
than one sort pair and more than one rank per thread), 1024, 4096 (the largest sort: 48 KiB of LDS); L = 1, 33 (one staged chunk
of the back-projection, partly filled) and 128 (two chunks); D = 1, 6 and 129 (the projection's 128-column staging is crossed,
nine column tiles of the back-projection).  Every B once, every L and D with at least two B."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import swd_cases as sc
from tc_gan_amd import clib
from tc_gan_amd.clib import libssnode
from tc_gan_amd.networks.sliced_wasserstein import swd_loss_grad

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 33, 6), (63, 128, 129), (64, 1, 6), (65, 33, 1), (257, 128, 6), (300, 33, 129), (1024, 128, 6),
          (4096, 1, 6)]
LATTICE_SHAPES = [s for s in SHAPES if (s[0] * s[1]) & (s[0] * s[1] - 1) == 0]
assert LATTICE_SHAPES == [(1, 1, 1), (64, 1, 6), (1024, 128, 6), (4096, 1, 6)]


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype).contiguous()


def _device_chain(x, y, theta, power):
    """The four launches one by one on float32 numpy inputs -> dict(px, py, coef, loss_l, gx) of numpy arrays.  The outputs are
    filled beforehand with values no kernel writes."""
    B, D = x.shape
    L = theta.shape[0]
    xd, yd, td = _dev(x), _dev(y), _dev(theta)
    px = torch.full((B, L), 7.0, device='cuda')
    py = torch.full((B, L), 7.0, device='cuda')
    coef = torch.full((B, L), 7.0, device='cuda')
    gx = torch.full((B, D), 7.0, device='cuda')
    loss_l = torch.full((L,), -7.0, device='cuda', dtype=torch.float64)
    stream = clib.stream_ptr()
    for src, dst in ((xd, px), (yd, py)):
        clib.check(libssnode.ssn_project_rows_f32(src.data_ptr(), B, D, D, td.data_ptr(), L, dst.data_ptr(), stream), 'project')
    clib.check(libssnode.ssn_swd_match_f32(px.data_ptr(), py.data_ptr(), B, L, power, coef.data_ptr(), loss_l.data_ptr(), stream),
               'ssn_swd_match_f32')
    clib.check(libssnode.ssn_swd_backproject_f32(coef.data_ptr(), td.data_ptr(), B, L, D, gx.data_ptr(), stream),
               'ssn_swd_backproject_f32')
    return {k: v.cpu().numpy() for k, v in dict(px=px, py=py, coef=coef, loss_l=loss_l, gx=gx).items()}


def _same_bits(a, b):
    """Equal as numbers with NaN == NaN and -0 == +0 (the kernel takes -0 as +0)."""
    np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('power', [1, 2])
@pytest.mark.parametrize('B,L,D', SHAPES)
def test_generic_inputs_bit_for_bit_and_loss_within_the_bound(B, L, D, power):
    """coef and gx equal the restatement's; |loss_l - exact| <= (B + 2) 2^-52 exact: all terms are non-negative, with one
    rounding per product, per partial sum and for the division (DESIGN 3.16b's derivation)."""
    x, y, theta = sc.generic_inputs(np.random.RandomState(100 + B), B, L, D)
    want = sc.swd(x, y, theta, power)
    got = _device_chain(x, y, theta, power)
    _same_bits(got['px'], want['px'])
    _same_bits(got['py'], want['py'])
    _same_bits(got['coef'], want['coef'])
    _same_bits(got['gx'], want['gx'])
    if D >= 2 and L >= 2:
        assert (want['coef'][:, L // 2] == 0).all() and want['loss_l'][L // 2] == 0     # the tied direction: d = 0 at every rank
        assert (got['coef'][:, L // 2] == 0).all() and got['loss_l'][L // 2] == 0
    worst = Fraction(0)
    for l in range(L):
        exact = want['loss_l'][l]
        err = abs(Fraction(float(got['loss_l'][l])) - exact)
        assert err <= sc.loss_bound(exact, B), (l, float(err), float(exact))
        if exact:
            worst = max(worst, err / exact)
    print('B, L, D, p =', (B, L, D, power), 'largest relative error of loss_l:', float(worst), 'bound', (B + 2) * 2.0 ** -52)
    # the order of the additions: loss_l is the restatement of the thread, wave and block sums bit for bit
    assert np.isfinite(got['loss_l']).all()
    ordered = np.array([sc.loss_in_kernel_order(want['px'][:, l], want['py'][:, l], power) for l in range(L)])
    np.testing.assert_array_equal(got['loss_l'].view(np.uint64), ordered.view(np.uint64))
    # the whole chain as the trainer calls it: the same gradient, the mean of the directions
    gx, loss, loss_l = swd_loss_grad(_dev(x), _dev(y), _dev(theta), power)
    _same_bits(gx.cpu().numpy(), want['gx'])
    np.testing.assert_array_equal(loss_l, got['loss_l'])
    np.testing.assert_allclose(loss, want['loss'], rtol=(B + L + 4) * 2.0 ** -52)


@pytest.mark.parametrize('power', [1, 2])
@pytest.mark.parametrize('B,L,D', LATTICE_SHAPES)
def test_lattice_inputs_give_the_exact_loss(B, L, D, power):
    x, y, theta = sc.lattice_inputs(np.random.RandomState(200 + B), B, L, D)
    want = sc.swd(x, y, theta, power)
    got = _device_chain(x, y, theta, power)
    assert [Fraction(float(v)) for v in got['loss_l']] == want['loss_l']
    _same_bits(got['coef'], want['coef'])
    _same_bits(got['gx'], want['gx'])


@pytest.mark.parametrize('B,L,D', [(65, 33, 1), (257, 128, 6)])
def test_power_one_is_the_scorers_w1(B, L, D):
    """loss_l[l] against wnum / (n m) of ssn_ks_w1_columns_f32 on the same projections (n = m = B): within the sum of the two
    bounds, (B + 2) 2^-52 and (2 B + 2) 2^-52 relative, and one rounding of the scorer's division."""
    x, y, theta = sc.generic_inputs(np.random.RandomState(300 + B), B, L, D)
    got = _device_chain(x, y, theta, 1)
    px = _dev(got['px'])
    truth_sorted = _dev(np.sort(got['py'], axis=0).T)
    m = torch.full((L,), B, device='cuda', dtype=torch.int32)
    n = torch.zeros((1, L), device='cuda', dtype=torch.int32)
    num = torch.zeros((1, L), device='cuda', dtype=torch.int64)
    wnum = torch.zeros((1, L), device='cuda', dtype=torch.float64)
    clib.check(libssnode.ssn_ks_w1_columns_f32(px.data_ptr(), truth_sorted.data_ptr(), m.data_ptr(), 1, B, L, B, n.data_ptr(),
                                               num.data_ptr(), wnum.data_ptr(), clib.stream_ptr()), 'ssn_ks_w1_columns_f32')
    assert (n.cpu().numpy() == B).all()
    w1 = wnum.cpu().numpy()[0] / (float(B) * float(B))
    np.testing.assert_allclose(got['loss_l'], w1, rtol=(3 * B + 5) * 2.0 ** -52, atol=0)


@pytest.mark.parametrize('where,value', [('x', np.nan), ('x', np.inf), ('x', -np.inf), ('y', np.nan)])
def test_a_non_finite_row_makes_everything_nan_and_the_call_returns(where, value):
    B, L, D = 65, 33, 6
    x, y, theta = sc.generic_inputs(np.random.RandomState(5), B, L, D)
    (x if where == 'x' else y)[17, 2] = value
    for power in (1, 2):
        got = _device_chain(x, y, theta, power)
        assert np.isnan(got['loss_l']).all() and np.isnan(got['coef']).all() and np.isnan(got['gx']).all()
        gx, loss, loss_l = swd_loss_grad(_dev(x), _dev(y), _dev(theta), power)
        assert np.isnan(loss) and np.isnan(loss_l).all() and bool(torch.isnan(gx).all())
        want = sc.swd(x, y, theta, power)
        assert np.isnan(want['loss']) and np.isnan(want['gx']).all()


def test_two_launches_give_the_same_bits():
    x, y, theta = sc.generic_inputs(np.random.RandomState(6), 300, 33, 6)
    for power in (1, 2):
        a, b = _device_chain(x, y, theta, power), _device_chain(x, y, theta, power)
        for key in ('coef', 'loss_l', 'gx'):
            assert a[key].tobytes() == b[key].tobytes(), key


def test_more_rows_than_the_sort_holds_are_refused():
    buf = torch.zeros(8, device='cuda')
    out = torch.zeros(8, device='cuda', dtype=torch.float64)
    rc = libssnode.ssn_swd_match_f32(buf.data_ptr(), buf.data_ptr(), clib.SWD_MAX_BATCH + 1, 1, 2, buf.data_ptr(), out.data_ptr(),
                                     clib.stream_ptr())
    assert rc == clib.SSN_ERR_BASE + 1 and '4096 rows' in clib.last_error()
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0 and float(buf.abs().sum()) == 0
    with pytest.raises(ValueError, match='contiguous'):
        swd_loss_grad(torch.zeros(4, 3, device='cuda'), torch.zeros(5, 3, device='cuda'), torch.zeros(2, 3, device='cuda'), 2)

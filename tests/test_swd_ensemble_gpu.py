"""Ensembles of sliced Wasserstein runs on the GPU (csrc/ssn_ens_swd.hip, networks/sliced_wasserstein_ensemble.py,
run/bptt_swd_ensemble.py): the segmented loss kernels give, member by member, the bits of the single-run kernels -- in both forms
of the match, on generic inputs and on lattice inputs full of ties; a value that is not finite in one member reaches no other;
the gradient assembly with a given L0 is the moment ensemble's; every member's tables are its single run's."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import swd_cases as sc
from tc_gan_amd import clib, execution
from tc_gan_amd.clib import libssnode
from tc_gan_amd.loaders import _read_table
from tc_gan_amd.run import bptt_swd, bptt_swd_ensemble as bse

pytestmark = pytest.mark.gpu

INVALID = clib.SSN_ERR_BASE + 1                               # hipErrorInvalidValue


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda').to(dtype).contiguous()


def _stream():
    return clib.stream_ptr()


def _powers(K):
    return [1 + (k + 1) % 2 for k in range(K)]                # 2, 1, 2, 1, 2: mixed over the members


# ---- the launches ---------------------------------------------------------------------------------------------------------

def ens_project(x, y, theta, K, B, L, D):
    px = torch.full((K * B, L), -7.0, device='cuda')
    py = torch.full((K * B, L), -7.0, device='cuda')
    clib.check(libssnode.ssn_ens_swd_project_f32(x.data_ptr(), y.data_ptr(), theta.data_ptr(), K, B, L, D, px.data_ptr(), py.data_ptr(),
                                                 _stream()), 'ssn_ens_swd_project_f32')
    return px, py


def ens_match(px, py, powers, K, B, L, form=clib.SWD_FORM_AUTO):
    coef = torch.full((K * B, L), -7.0, device='cuda')
    loss_l = torch.full((K, L), -7.0, device='cuda', dtype=torch.float64)
    l0 = torch.full((K,), -7.0, device='cuda', dtype=torch.float64)
    clib.check(libssnode.ssn_ens_swd_match_f32(px.data_ptr(), py.data_ptr(), (ctypes.c_int * K)(*powers), K, B, L, form,
                                               coef.data_ptr(), loss_l.data_ptr(), l0.data_ptr(), _stream()), 'ssn_ens_swd_match_f32')
    return coef, loss_l, l0


def ens_backproject(coef, theta, K, B, L, D):
    gx = torch.full((K * B, D), -7.0, device='cuda')
    clib.check(libssnode.ssn_ens_swd_backproject_f32(coef.data_ptr(), theta.data_ptr(), K, B, L, D, gx.data_ptr(), _stream()),
               'ssn_ens_swd_backproject_f32')
    return gx


def solo_project(x, theta, B, L, D):
    out = torch.empty((B, L), device='cuda')
    clib.check(libssnode.ssn_project_rows_f32(x.data_ptr(), B, D, D, theta.data_ptr(), L, out.data_ptr(), _stream()), 'project')
    return out


def solo_match(px, py, power, B, L):
    coef = torch.empty((B, L), device='cuda')
    loss_l = torch.empty(L, device='cuda', dtype=torch.float64)
    clib.check(libssnode.ssn_swd_match_f32(px.data_ptr(), py.data_ptr(), B, L, power, coef.data_ptr(), loss_l.data_ptr(), _stream()),
               'match')
    return coef, loss_l


def solo_backproject(coef, theta, B, L, D):
    gx = torch.empty((B, D), device='cuda')
    clib.check(libssnode.ssn_swd_backproject_f32(coef.data_ptr(), theta.data_ptr(), B, L, D, gx.data_ptr(), _stream()), 'backproject')
    return gx


# ---- inputs ---------------------------------------------------------------------------------------------------------------

def generic_members(seed, K, B, L, D):
    """x, y (K B, D), theta (K, L, D): `swd_cases.generic_inputs` per member, each on its own stream."""
    parts = [sc.generic_inputs(np.random.RandomState(seed + 17 * k), B, L, D) for k in range(K)]
    return tuple(np.concatenate([p[i] for p in parts]) if i < 2 else np.stack([p[2] for p in parts]) for i in range(3))


def lattice_members(seed, K, B, L, D):
    """Multiples of 1/8 from a small range, rows repeated, directions with few non-zero entries: every projection is an exact
    multiple of 1/64 and many of them are equal, within x and between x and y, so the tie rule (by row) decides coef."""
    rs = np.random.RandomState(seed)
    x = (rs.randint(-4, 5, size=(K * B, D)) / 8.0).astype('float32')
    y = (rs.randint(-4, 5, size=(K * B, D)) / 8.0).astype('float32')
    theta = (rs.randint(-8, 9, size=(K, L, D)) / 8.0 * (rs.rand(K, L, D) < 0.5)).astype('float32')
    for k in range(K):
        if B >= 2:
            x[k * B + B - 1] = x[k * B]                       # a repeated row at non-adjacent indices
            y[k * B + B // 2] = x[k * B]                      # a row of x in y
        if B >= 5:
            x[k * B + 3] = x[k * B + 1]
    return x, y, theta


def plant_signed_zeros(px):
    """-0 beside +0 in the columns of px that hold zeros (the projection itself starts from +0 and never gives -0)."""
    px = px.clone()
    zero = (px == 0)
    odd = (torch.arange(px.shape[0], device=px.device) % 2 == 1)[:, None]
    px[zero & odd] = -0.0
    return px


# ---- 1. segmented kernels against the single-run kernels ---------------------------------------------------------------------

SHAPES = [(1, 1, 1), (3, 33, 6), (5, 130, 17), (3, 130, 129)]          # (K, L, D)
BATCHES = [1, 2, 31, 32, 33, 63, 64, 65, 100, 300]


def _check_chain(x, y, theta, K, B, L, D, signed_zeros=False):
    powers = _powers(K)
    xd, yd, td = _dev(x), _dev(y), _dev(theta)
    px, py = ens_project(xd, yd, td, K, B, L, D)
    if signed_zeros:
        px = plant_signed_zeros(px)
    coef, loss_l, l0 = ens_match(px, py, powers, K, B, L)
    gx = ens_backproject(coef, td, K, B, L, D)
    # two launches give the same bits
    again = ens_match(px, py, powers, K, B, L)
    for a, b in zip((coef, loss_l, l0), again):
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    np.testing.assert_array_equal(gx.cpu().numpy(), ens_backproject(coef, td, K, B, L, D).cpu().numpy())
    if B <= clib.SWD_WAVE_MAX_BATCH:                          # both forms of the match
        for form in (clib.SWD_FORM_GENERAL, clib.SWD_FORM_WAVE):
            for a, b in zip((coef, loss_l, l0), ens_match(px, py, powers, K, B, L, form)):
                np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy(), err_msg='form {}'.format(form))
    for k in range(K):
        sl = slice(k * B, (k + 1) * B)
        tk = td[k].contiguous()
        if not signed_zeros:
            np.testing.assert_array_equal(px[sl].cpu().numpy(), solo_project(xd[sl].contiguous(), tk, B, L, D).cpu().numpy())
        np.testing.assert_array_equal(py[sl].cpu().numpy(), solo_project(yd[sl].contiguous(), tk, B, L, D).cpu().numpy())
        c1, l1 = solo_match(px[sl].contiguous(), py[sl].contiguous(), powers[k], B, L)
        np.testing.assert_array_equal(coef[sl].cpu().numpy(), c1.cpu().numpy(), err_msg='coef of member {}'.format(k))
        host = l1.cpu().numpy()
        np.testing.assert_array_equal(loss_l[k].cpu().numpy(), host, err_msg='loss_l of member {}'.format(k))
        assert l0[k].item() == np.cumsum(host)[-1] / L
        np.testing.assert_array_equal(gx[sl].cpu().numpy(), solo_backproject(c1, tk, B, L, D).cpu().numpy())
    return coef, loss_l


@pytest.mark.parametrize('K,L,D', SHAPES)
@pytest.mark.parametrize('B', BATCHES)
def test_segmented_kernels_equal_the_single_run_kernels_member_by_member(K, B, L, D):
    _check_chain(*generic_members(1000 * B + L, K, B, L, D), K, B, L, D)


@pytest.mark.parametrize('K,L,D', SHAPES)
@pytest.mark.parametrize('B', BATCHES)
def test_segmented_kernels_on_lattice_inputs_with_ties(K, B, L, D):
    x, y, theta = lattice_members(B + L, K, B, L, D)
    coef, _ = _check_chain(x, y, theta, K, B, L, D, signed_zeros=True)
    if B >= 5 and D >= 6:
        # the inputs do tie: against the restatement with ties broken the other way, member 0's coefficients differ
        px = sc.project_rows(x[:B], theta[0])
        py = sc.project_rows(y[:B], theta[0])
        assert min(np.unique(px[:, l]).size for l in range(L)) < B
        right, _ = sc.match(px, py, _powers(K)[0])
        wrong, _ = sc.match(px, py, _powers(K)[0], ties='reversed')
        assert (right != wrong).any()


def test_wave_form_is_refused_beyond_one_wave():
    K, B, L = 2, 65, 3
    px = torch.zeros((K * B, L), device='cuda')
    coef, loss_l, l0 = torch.zeros_like(px), torch.zeros((K, L), device='cuda', dtype=torch.float64), torch.zeros(K, device='cuda',
                                                                                                               dtype=torch.float64)
    err = libssnode.ssn_ens_swd_match_f32(px.data_ptr(), px.data_ptr(), (ctypes.c_int * K)(1, 2), K, B, L, clib.SWD_FORM_WAVE,
                                          coef.data_ptr(), loss_l.data_ptr(), l0.data_ptr(), _stream())
    assert err == INVALID and '64 rows' in clib.last_error()


# ---- 2. isolation ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('B', [33, 65])                        # the wave form and the general form
@pytest.mark.parametrize('side', ['x', 'y'])
def test_a_value_that_is_not_finite_stays_in_its_member(B, side):
    K, L, D = 3, 33, 6
    powers = _powers(K)
    x, y, theta = generic_members(5, K, B, L, D)
    td = _dev(theta)

    def chain(xa, ya):
        px, py = ens_project(_dev(xa), _dev(ya), td, K, B, L, D)
        coef, loss_l, l0 = ens_match(px, py, powers, K, B, L)
        return [t.cpu().numpy() for t in (px, py, coef, loss_l, l0, ens_backproject(coef, td, K, B, L, D))]
    clean = chain(x, y)
    bad = [x.copy(), y.copy()]
    target = bad[0] if side == 'x' else bad[1]
    target[B + 2, 1], target[B + 7, 0], target[2 * B - 1, D - 1] = np.nan, np.inf, -np.inf          # member 1
    got = chain(*bad)
    rows = lambda k: slice(k * B, (k + 1) * B)
    for k in (0, 2):
        for a, b, per_row in zip(got, clean, (True, True, True, False, False, True)):
            idx = rows(k) if per_row else k
            np.testing.assert_array_equal(a[idx], b[idx])
            assert np.isfinite(a[idx]).all()
    # member 1: what the single-run kernels give for it alone
    pxk, pyk = _dev(got[0][rows(1)]), _dev(got[1][rows(1)])
    c1, l1 = solo_match(pxk, pyk, powers[1], B, L)
    np.testing.assert_array_equal(got[2][rows(1)], c1.cpu().numpy())
    np.testing.assert_array_equal(got[3][1], l1.cpu().numpy())
    assert np.isnan(got[3][1]).all() and np.isnan(got[2][rows(1)]).all() and np.isnan(got[4][1])


@pytest.mark.parametrize('B', [33, 65])
def test_one_bad_column_spoils_that_column_and_the_members_l0_only(B):
    K, L, D = 3, 33, 6
    powers = _powers(K)
    x, y, theta = generic_members(6, K, B, L, D)
    px, py = ens_project(_dev(x), _dev(y), _dev(theta), K, B, L, D)
    clean = [t.cpu().numpy() for t in ens_match(px, py, powers, K, B, L)]
    px[2 * B + 4, 7] = float('inf')                            # member 2, direction 7
    coef, loss_l, l0 = [t.cpu().numpy() for t in ens_match(px, py, powers, K, B, L)]
    assert np.isnan(loss_l[2, 7]) and np.isnan(coef[2 * B:, 7]).all() and np.isnan(l0[2])
    keep = np.ones(L, dtype=bool)
    keep[7] = False
    np.testing.assert_array_equal(coef[2 * B:][:, keep], clean[0][2 * B:][:, keep])
    np.testing.assert_array_equal(loss_l[2, keep], clean[1][2, keep])
    np.testing.assert_array_equal(coef[:2 * B], clean[0][:2 * B])
    np.testing.assert_array_equal(loss_l[:2], clean[1][:2])
    np.testing.assert_array_equal(l0[:2], clean[2][:2])


# ---- 3. the gradient assembly with a given L0 ----------------------------------------------------------------------------------

def test_gen_grads_with_given_l0_equals_the_moment_assembly():
    """The inputs of test_moments_ensemble_gpu.test_segmented_grads_and_apply_isolate_nan (member 2's penalty rows poisoned).
    loss = L0 + c_dyn dyn + c_rate rate in this order; the compiler may fuse each product into its addition, which saves at most
    one rounding of a non-negative term each: 2 x 2^-53 relative, asserted as 4 x 2^-52."""
    K, B, NB, M, D, nv = 3, 4, 2, 8, 3, 1
    P = nv + 12
    g = torch.Generator().manual_seed(1)
    f = dict(device='cuda', dtype=torch.float32)
    parts = torch.rand((K * B, 4, 3), generator=g, dtype=torch.float64).cuda()
    g_ext, ext_base = torch.rand((K * B, NB, M), generator=g).cuda(), torch.rand((K * B, NB, M), generator=g).cuda()
    zin = (torch.rand((K * B, M), generator=g) * 2 - 1).cuda()
    dyn, rate = torch.rand((K * B, NB, M), generator=g).cuda(), torch.rand((K * B, NB, M), generator=g).cuda()
    dyn[2 * B, 0, 1] = float('nan')                        # member 2 poisoned
    dm = torch.rand((K, 2, D), generator=g, dtype=torch.float64).cuda()
    w = torch.rand((K, 2, D), generator=g, dtype=torch.float64).cuda()
    costs = torch.tensor([[1.0, 0.5], [0.0, 2.0], [1.0, 1.0]], device='cuda', dtype=torch.float64)
    n = B * NB * M
    common = dict(K=K, B=B, nv=nv, NB=NB, M=M, part=parts.data_ptr(), g_ext=g_ext.data_ptr(), ext_base=ext_base.data_ptr(),
                  zin=zin.data_ptr(), dyn_row=dyn.data_ptr(), rate_row=rate.data_ptr(), scale_dyn=1.0 / n, scale_rate=1.0 / n,
                  costs=costs.data_ptr())
    R = int(libssnode.ssn_ens_record_doubles(D, P))
    rec = torch.zeros((K, R), device='cuda', dtype=torch.float64)
    rec[:, 1:1 + 2 * D] = torch.rand((K, 2 * D), generator=g, dtype=torch.float64).cuda()
    grads = torch.empty((K, P), **f)
    a = clib.EnsGrads(D=D, data_moments=dm.data_ptr(), weights=w.data_ptr(), grads=grads.data_ptr(), rec=rec.data_ptr(), rstride=R,
                      **common)
    clib.check(libssnode.ssn_ens_gen_grads_f32(ctypes.byref(a), _stream()), 'ssn_ens_gen_grads_f32')

    R0 = int(libssnode.ssn_ens_record_doubles(0, P))
    assert R0 == 4 + 2 * P
    stride = R0 + 5                                          # (a row may be longer than the record: loss_l rides behind it)
    rec0 = torch.full((K, stride), -3.0, device='cuda', dtype=torch.float64)
    grads0 = torch.empty((K, P), **f)
    l0 = torch.tensor([0.625, float('nan'), 1.75], device='cuda', dtype=torch.float64)
    b = clib.EnsGrads(D=0, grads=grads0.data_ptr(), rec=rec0.data_ptr(), rstride=stride, **common)
    clib.check(libssnode.ssn_ens_gen_grads_l0_f32(ctypes.byref(b), l0.data_ptr(), _stream()), 'ssn_ens_gen_grads_l0_f32')
    np.testing.assert_array_equal(grads0.cpu().numpy(), grads.cpu().numpy())
    got, ref, l0h, c = rec0.cpu().numpy(), rec.cpu().numpy(), l0.cpu().numpy(), costs.cpu().numpy()
    np.testing.assert_array_equal(got[:, 1:3], ref[:, 1 + 2 * D:3 + 2 * D])            # the penalties
    np.testing.assert_array_equal(got[:, 0], l0h)
    assert (got[:, 4:] == -3.0).all()                         # the parameters and gradients are the apply's to write
    want = l0h[0] + c[0, 0] * got[0, 1] + c[0, 1] * got[0, 2]
    assert abs(got[0, 3] - want) <= 4 * 2.0 ** -52 * want
    assert np.isnan(got[1, 3]) and np.isfinite(got[1, 1:3]).all() and np.isfinite(grads0[1].cpu().numpy()).all()   # NaN l0: row 1 only
    assert np.isnan(got[2, 1]) and np.isnan(got[2, 3]) and got[2, 0] == 1.75
    assert np.isfinite(got[0, :4]).all()
    # D != 0 or moment arrays are refused
    bad = clib.EnsGrads(D=D, grads=grads0.data_ptr(), rec=rec0.data_ptr(), rstride=R, **common)
    assert libssnode.ssn_ens_gen_grads_l0_f32(ctypes.byref(bad), l0.data_ptr(), _stream()) == INVALID
    assert 'D must be 0' in clib.last_error()
    assert libssnode.ssn_ens_gen_grads_l0_f32(ctypes.byref(b), None, _stream()) == INVALID


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_limit_and_empty_problems_write_nothing():
    K, B, L, D = 2, 3, 4, 5
    buf = torch.full((K * B * max(L, D),), -7.0, device='cuda')
    dbl = torch.full((K * L,), -7.0, device='cuda', dtype=torch.float64)
    p, d = buf.data_ptr(), dbl.data_ptr()
    two = (ctypes.c_int * K)(1, 2)
    lib = libssnode
    many = (ctypes.c_int * (clib.ENS_SWD_MAX_MEMBERS + 1))(*([1] * (clib.ENS_SWD_MAX_MEMBERS + 1)))
    cases = [
        (lambda: lib.ssn_ens_swd_project_f32(p, p, p, K, clib.SWD_MAX_BATCH + 1, L, D, p, p, None), '4096 rows'),
        (lambda: lib.ssn_ens_swd_match_f32(p, p, two, K, clib.SWD_MAX_BATCH + 1, L, 0, p, d, d, None), '4096 rows'),
        (lambda: lib.ssn_ens_swd_backproject_f32(p, p, K, clib.SWD_MAX_BATCH + 1, L, D, p, None), '4096 rows'),
        (lambda: lib.ssn_ens_swd_project_f32(p, p, p, K, B, clib.W1_MAX_DIRECTIONS + 1, D, p, p, None), '4096 directions'),
        (lambda: lib.ssn_ens_swd_match_f32(p, p, two, K, B, clib.W1_MAX_DIRECTIONS + 1, 0, p, d, d, None), '4096 directions'),
        (lambda: lib.ssn_ens_swd_backproject_f32(p, p, K, B, clib.W1_MAX_DIRECTIONS + 1, D, p, None), '4096 directions'),
        (lambda: lib.ssn_ens_swd_match_f32(p, p, many, clib.ENS_SWD_MAX_MEMBERS + 1, B, L, 0, p, d, d, None), '2048 members'),
        (lambda: lib.ssn_ens_swd_match_f32(p, p, (ctypes.c_int * K)(1, 3), K, B, L, 0, p, d, d, None), 'power other than 1 or 2'),
        (lambda: lib.ssn_ens_swd_match_f32(p, p, (ctypes.c_int * K)(0, 2), K, B, L, 0, p, d, d, None), 'power other than 1 or 2'),
        (lambda: lib.ssn_ens_swd_match_f32(p, p, two, K, B, L, 7, p, d, d, None), 'unknown form'),
        (lambda: lib.ssn_ens_swd_project_f32(p, p, p, -1, B, L, D, p, p, None), 'invalid argument'),
        (lambda: lib.ssn_ens_swd_project_f32(p, p, p, K, B, L, -1, p, p, None), 'invalid argument'),
        (lambda: lib.ssn_ens_swd_match_f32(p, p, two, K, -1, L, 0, p, d, d, None), 'invalid argument'),
        (lambda: lib.ssn_ens_swd_backproject_f32(p, p, K, B, -1, D, p, None), 'invalid argument'),
        (lambda: lib.ssn_ens_swd_project_f32(None, p, p, K, B, L, D, p, p, None), 'invalid argument'),
        (lambda: lib.ssn_ens_swd_project_f32(p, p, p, K, B, L, D, p, None, None), 'invalid argument'),
        (lambda: lib.ssn_ens_swd_match_f32(p, p, None, K, B, L, 0, p, d, d, None), 'invalid argument'),
        (lambda: lib.ssn_ens_swd_match_f32(p, p, two, K, B, L, 0, p, d, None, None), 'invalid argument'),
        (lambda: lib.ssn_ens_swd_backproject_f32(p, None, K, B, L, D, p, None), 'invalid argument'),
    ]
    for call, text in cases:
        assert call() == INVALID
        assert text in clib.last_error(), (text, clib.last_error())
    # K, B or L == 0: success, nothing written
    s = _stream()
    for k, b, l in ((0, B, L), (K, 0, L), (K, B, 0)):
        assert lib.ssn_ens_swd_project_f32(p, p, p, k, b, l, D, p, p, s) == 0
        assert lib.ssn_ens_swd_match_f32(p, p, two, k, b, l, 0, p, d, d, s) == 0
        if l:
            assert lib.ssn_ens_swd_backproject_f32(p, p, k, b, l, D, p, s) == 0
    torch.cuda.synchronize()
    assert (buf == -7.0).all() and (dbl == -7.0).all()


# ---- 5. members equal their single runs ---------------------------------------------------------------------------------------

BASE = ['--n_bandwidths', '8', '--seqlen', '40', '--skip-steps', '30', '--batchsize', '4', '--iterations', '6', '--quiet',
        '--sample-sites', '0,0.5', '--swd-directions', '33']
SHARED = dict(num_sites=20, dataset_provider='fixedtime')
MAXDIFF = {}


def members_for(batchsize):
    """Three members that differ in seed, start values, learning rate, rate_cost, power, direction seed and truth size (whole
    minibatches each)."""
    return [dict(seed=1, J0=0.02, learning_rate=0.01, rate_cost=0.5, swd_power=1, swd_direction_seed=3, truth_size=8 * batchsize),
            dict(seed=2, S0=0.3, learning_rate=0.002, rate_cost=0.5, swd_power=2, swd_direction_seed=0, truth_size=12 * batchsize),
            dict(seed=3, J0=0.015, S0=0.2, learning_rate=0.005, rate_cost=3.0, swd_power=2, swd_direction_seed=11,
                 truth_size=10 * batchsize)]


def _write(path, obj):
    path.write_text(json.dumps(obj))
    return str(path)


def _ensemble(tmp_path, args, members, shared=SHARED):
    d = tmp_path / 'ens'
    bse.main(args + ['--members', _write(tmp_path / 'members.json', members), '--datastore', str(d),
                     '--load-config', _write(tmp_path / 'shared.json', shared)])
    return [str(d / str(i)) for i in range(len(members))]


def _solo(tmp_path, args, shared, member, i, kernel):
    d = tmp_path / 'solo{}'.format(i)
    argv = args + ['--datastore', str(d), '--load-config', _write(tmp_path / 'solo{}.json'.format(i), dict(shared, **member)),
                   '--gen-kernel', kernel]
    try:
        bptt_swd.main(argv)
    except execution.KnownError:
        pass
    return str(d)


def _compare(ens_dir, solo_dir, tag, rtol=1e-6):
    """The moment ensemble's allowance (the fp64 sums over a member's draws may add in another order); 0 is expected."""
    assert json.load(open(os.path.join(ens_dir, 'exit.json'))) == json.load(open(os.path.join(solo_dir, 'exit.json')))
    worst = 0.0
    for name in ('learning', 'generator'):
        ta, tb = _read_table(ens_dir, name), _read_table(solo_dir, name)
        assert list(ta.columns) == list(tb.columns) and len(ta) == len(tb), name
        cols = [c for c in ta.columns if c not in ('train_time',)]
        va, vb = ta[cols].to_numpy(dtype='float64'), tb[cols].to_numpy(dtype='float64')
        with np.errstate(invalid='ignore', divide='ignore'):
            rel = np.abs(va - vb) / np.maximum(np.abs(vb), 1e-300)
        worst = max(worst, float(np.nanmax(rel)) if rel.size else 0.0)
        print('largest relative difference {} {}: {:.3g}'.format(tag, name, worst))
        np.testing.assert_allclose(va, vb, rtol=rtol, atol=0, err_msg='{} {}'.format(tag, name))
    # the first step's forward and loss: the same bits
    assert _read_table(ens_dir, 'learning')['swd'].to_numpy()[0] == _read_table(solo_dir, 'learning')['swd'].to_numpy()[0]
    MAXDIFF[tag] = max(MAXDIFF.get(tag, 0.0), worst)


def _check(tmp_path, args, members, kernel, shared=SHARED, tag=None):
    ens = _ensemble(tmp_path, args + ['--gen-kernel', kernel], members, shared)
    assert json.load(open(str(tmp_path / 'ens' / 'members.json')))['num_members'] == len(members)
    for i, m in enumerate(members):
        info = json.load(open(os.path.join(ens[i], 'info.json')))
        assert info['run_config']['gen_kernel'] == kernel and info['run_config']['swd_power'] == m['swd_power']
        assert np.load(os.path.join(ens[i], 'truth.npy')).shape[0] == m['truth_size']
        _compare(ens[i], _solo(tmp_path, args, shared, m, i, kernel), '{}/{}'.format(tag or kernel, i))
    return ens


def _batch(args, batchsize):
    args = list(args)
    args[args.index('--batchsize') + 1] = str(batchsize)
    return args


@pytest.mark.parametrize('kernel', ['tile', 'mfma-fp32'])
def test_three_members_match_solo(tmp_path, kernel):
    _check(tmp_path, BASE, members_for(4), kernel)


def test_philox_members_match_solo(tmp_path):
    members = [dict(m, z_device_seed=100 + i) for i, m in enumerate(members_for(4))]
    _check(tmp_path, BASE, members, 'tile', tag='philox')


def test_duo_odd_batch_members_match_solo(tmp_path):
    _check(tmp_path, _batch(BASE, 3), members_for(3), 'duo', tag='duo')         # a workgroup of two draws holds two members


def test_single_member_matches_solo(tmp_path):
    _check(tmp_path, BASE, members_for(4)[:1], 'tile', tag='K=1')


def test_batch_beyond_one_wave_runs_the_general_match_form(tmp_path):
    members = [dict(m, truth_size=65 * (2 + i)) for i, m in enumerate(members_for(65))]
    _check(tmp_path, _batch(BASE, 65), members, 'tile', tag='B=65')


def test_member_that_quits_leaves_the_others_unchanged(tmp_path):
    members = members_for(4)
    members[1] = dict(members[1], quit_JDS_threshold=1e-3)
    _check(tmp_path, BASE, members, 'tile', tag='quit')
    assert json.load(open(str(tmp_path / 'ens' / '1' / 'exit.json')))['reason'] == 'JDS_distance'
    assert json.load(open(str(tmp_path / 'ens' / '0' / 'exit.json')))['reason'] == 'end_of_iteration'


def test_distdiff_scores_a_member_directory(tmp_path):
    import pandas
    from tc_gan_amd.analyzers import distdiff
    ens = _ensemble(tmp_path, BASE + ['--gen-kernel', 'tile'], members_for(4))
    distdiff.main([ens[1], '--wasserstein', '--steps', '::3', '--draws', '8'])
    table = pandas.read_csv(os.path.join(ens[1], 'wdist.csv'))
    steps = _read_table(ens[1], 'generator')['gen_step'].to_numpy()[::3]
    scored = table['gen_step'].to_numpy()
    assert sorted(set(scored)) == sorted(int(s) for s in steps)
    per_step = table[table['stat'] == 'sliced_w1']
    assert len(per_step) == len(steps) and np.isfinite(per_step['W1'].to_numpy()).all()

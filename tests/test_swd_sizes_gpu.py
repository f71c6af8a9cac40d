"""The match of two samples of different sizes on the GPU (csrc/ssn_swd_sizes.hip through libssnode_ext.so) against the
restatement of tests/swd_sizes_cases.py: the coefficients bit for bit, the loss per direction bit for bit against the kernel-order
restatement and within the derived bound of the exact rational; non-finite columns, repeatability, the exact lattice; the host
function at M != B and M == B; one update against fp64 autograd; a seeded run with a larger truth minibatch.

The size pairs (n, m): both paddings at and around 64 (63/64, 64/65, 65/64) and at powers of two (256/257, 257/256, 1024/1000),
the 256-thread stride (257, 300), coprime and common-factor sizes, m < n (one or two terms per rank), the longest loop of one
rank (1, 16384) and the largest LDS request (4096, 16384: 96 KiB)."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import swd_cases as sc
import swd_sizes_cases as zc
from oracle import gan_torch as og
from oracle import ssn_numpy as on
from test_moments import JDS, MM_PARAMS
from test_swd_train_gpu import LEARN_RATIO
from tc_gan_amd import clib
from tc_gan_amd.clib import libssnode_ext
from tc_gan_amd.networks.sliced_wasserstein import swd_loss_grad

pytestmark = pytest.mark.gpu

SIZE_PAIRS = [(1, 1), (1, 7), (7, 1), (2, 3), (63, 64), (64, 65), (65, 64), (15, 1000), (256, 257), (257, 256), (300, 257),
              (1024, 1000)]
LIMIT_PAIRS = [(4096, 16384), (1, 16384), (4096, 1)]
D = 6


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype).contiguous()


@functools.lru_cache(maxsize=None)
def _case(n, m, L, power, kind='generic'):
    """Inputs and restatement of one case, computed once and shared by the tests that need it (read only)."""
    make = zc.generic_inputs if kind == 'generic' else zc.lattice_inputs
    x, y, theta = make(np.random.RandomState(1000 * L + n + m), n, m, L, D)
    return x, y, theta, zc.swd(x, y, theta, power)


def _device_match(px, py, power):
    """The match alone on float32 numpy projections -> (coef, loss_l); the outputs are filled beforehand with values the kernel
    does not write."""
    (n, L), m = px.shape, py.shape[0]
    pxd, pyd = _dev(px), _dev(py)
    coef = torch.full((n, L), 7.0, device='cuda')
    loss_l = torch.full((L,), -7.0, device='cuda', dtype=torch.float64)
    clib.check_ext(libssnode_ext.ssnx_swd_match_sizes_f32(pxd.data_ptr(), n, pyd.data_ptr(), m, L, power, coef.data_ptr(),
                                                          loss_l.data_ptr(), clib.stream_ptr()), 'ssnx_swd_match_sizes_f32')
    return coef.cpu().numpy(), loss_l.cpu().numpy()


def _check_against_restatement(n, m, L, power):
    x, y, theta, want = _case(n, m, L, power)
    coef, loss_l = _device_match(want['px'], want['py'], power)
    np.testing.assert_array_equal(coef.view(np.uint32), want['coef'].view(np.uint32))
    ordered = np.array([zc.loss_in_kernel_order(want['px'][:, l], want['py'][:, l], power) for l in range(L)])
    np.testing.assert_array_equal(loss_l.view(np.uint64), ordered.view(np.uint64))
    worst = Fraction(0)
    for l in range(L):
        exact = want['loss_l'][l]
        err = abs(Fraction(float(loss_l[l])) - exact)
        assert err <= zc.loss_bound(exact, n, m), (l, float(err), float(exact))
        if exact:
            worst = max(worst, err / exact)
    print('n, m, L, p =', (n, m, L, power), 'largest relative error of loss_l:', float(worst), 'bound', (n + m + 4) * 2.0 ** -52)
    if L >= 2:                                                    # the tied direction: d = 0 at every pair
        assert (coef[:, L // 2] == 0).all() and loss_l[L // 2] == 0 and not np.signbit(coef[:, L // 2]).any()


@pytest.mark.parametrize('power', [1, 2])
@pytest.mark.parametrize('L', [1, 3, 33])
@pytest.mark.parametrize('n,m', SIZE_PAIRS)
def test_generic_inputs_bit_for_bit_and_loss_within_the_bound(n, m, L, power):
    _check_against_restatement(n, m, L, power)


@pytest.mark.parametrize('power', [1, 2])
@pytest.mark.parametrize('n,m', LIMIT_PAIRS)
def test_the_limits(n, m, power):
    _check_against_restatement(n, m, 2, power)


@pytest.mark.parametrize('where,value', [('x', np.nan), ('x', np.inf), ('x', -np.inf), ('y', np.nan), ('y', np.inf), ('y', -np.inf)])
def test_a_non_finite_value_touches_its_direction_only(where, value):
    n, m, L = 65, 300, 3
    for power in (1, 2):
        clean = _case(n, m, L, power)[3]
        px, py = clean['px'].copy(), clean['py'].copy()
        (px if where == 'x' else py)[17, 1] = value
        coef, loss_l = _device_match(px, py, power)
        assert np.isnan(loss_l[1]) and np.isnan(coef[:, 1]).all()
        for l in (0, 2):
            np.testing.assert_array_equal(coef[:, l].view(np.uint32), clean['coef'][:, l].view(np.uint32))
            assert loss_l[l] == zc.loss_in_kernel_order(px[:, l], py[:, l], power)
        want_coef, want_loss = zc.match(px, py, power)
        assert want_loss[1] is None and np.isnan(want_coef[:, 1]).all()


def test_two_launches_give_the_same_bits():
    for power in (1, 2):
        want = _case(300, 257, 33, power)[3]
        a, b = _device_match(want['px'], want['py'], power), _device_match(want['px'], want['py'], power)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize('power', [1, 2])
@pytest.mark.parametrize('n,m,L', [(1, 1, 1), (2, 8, 2), (64, 16, 4), (256, 1024, 2)])
def test_lattice_inputs_give_the_exact_loss(n, m, L, power):
    want = _case(n, m, L, power, 'lattice')[3]
    coef, loss_l = _device_match(want['px'], want['py'], power)
    assert [Fraction(float(v)) for v in loss_l] == want['loss_l']
    np.testing.assert_array_equal(coef.view(np.uint32), want['coef'].view(np.uint32))


def test_refusals_write_nothing():
    buf = torch.zeros(8, device='cuda')
    out = torch.zeros(8, device='cuda', dtype=torch.float64)
    for n, m, what in ((clib.SWD_MAX_BATCH + 1, 8, '4096 generated rows'), (8, clib.SWD_MAX_TRUTH + 1, '16384 truth rows'),
                       (2, 0, 'no truth rows')):
        rc = libssnode_ext.ssnx_swd_match_sizes_f32(buf.data_ptr(), n, buf.data_ptr(), m, 1, 2, buf.data_ptr(), out.data_ptr(),
                                                    clib.stream_ptr())
        assert rc == clib.SSN_ERR_BASE + 1 and what in clib.ext_last_error()
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0 and float(buf.abs().sum()) == 0


# ---- the host function ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('power', [1, 2])
@pytest.mark.parametrize('n,m,L', [(15, 1000, 33), (300, 257, 33), (65, 64, 3), (1024, 1000, 3)])
def test_swd_loss_grad_at_unequal_sizes_is_the_restatement(n, m, L, power):
    x, y, theta, want = _case(n, m, L, power)
    gx, loss, loss_l = swd_loss_grad(_dev(x), _dev(y), _dev(theta), power, unequal=True)
    np.testing.assert_array_equal(gx.cpu().numpy().view(np.uint32), want['gx'].view(np.uint32))
    ordered = np.array([zc.loss_in_kernel_order(want['px'][:, l], want['py'][:, l], power) for l in range(L)])
    np.testing.assert_array_equal(loss_l.view(np.uint64), ordered.view(np.uint64))
    np.testing.assert_allclose(loss, want['loss'], rtol=(n + m + L + 6) * 2.0 ** -52)


@pytest.mark.parametrize('power', [1, 2])
@pytest.mark.parametrize('B,L', [(65, 33), (300, 3)])
def test_swd_loss_grad_at_equal_sizes_returns_the_bits_of_the_rank_matching(B, L, power):
    """M == B takes the three entry points of libssnode.so whether `unequal` is given or not: `swd_cases.swd`'s gradient and
    its kernel-order loss."""
    x, y, theta = sc.generic_inputs(np.random.RandomState(100 + B), B, L, D)
    want = sc.swd(x, y, theta, power)
    ordered = np.array([sc.loss_in_kernel_order(want['px'][:, l], want['py'][:, l], power) for l in range(L)])
    for unequal in (False, True):
        gx, loss, loss_l = swd_loss_grad(_dev(x), _dev(y), _dev(theta), power, unequal=unequal)
        np.testing.assert_array_equal(gx.cpu().numpy().view(np.uint32), want['gx'].view(np.uint32))
        np.testing.assert_array_equal(loss_l.view(np.uint64), ordered.view(np.uint64))
    with pytest.raises(ValueError, match='unequal=True'):
        swd_loss_grad(_dev(x), _dev(y[:-1]), _dev(theta), power)


# ---- the trainer -----------------------------------------------------------------------------------------------------------

SWD_PARAMS = dict({k: v for k, v in MM_PARAMS.items() if k not in ('lam', 'moment_weights_regularization')}, swd_directions=16)


def test_one_update_with_a_larger_truth_minibatch_vs_oracle():
    """p = 2, sgd, 2N = 20, 16 draws against minibatches of 96 truth rows: the bare loss, the total, the penalties and the
    post-update (J, D, S) with the tolerances of tests/test_swd_train_gpu.py::test_one_sliced_wasserstein_update_vs_oracle.  The
    oracle's loss is the quantile coupling written with repeated rows: each of the 16 sorted projections 6 times against the 96."""
    from tc_gan_amd.analyzers.distdiff import slice_directions
    from tc_gan_amd.networks.sliced_wasserstein import make_sliced_wasserstein
    B, M = 16, 96
    swd, rest = make_sliced_wasserstein(dict(SWD_PARAMS, swd_power=2, batchsize=B, swd_truth_batch=M))
    assert rest == {} and swd.swd_truth_batch == M
    data = np.random.RandomState(5).rand(2 * M, swd.num_mom_conds) * 8
    swd.set_dataset(data)
    info = next(swd.learning())

    N = 10
    zs = og.t64(np.random.RandomState(0).rand(B, 2 * N, 2 * N))
    idx = np.arange(len(data))
    np.random.RandomState(0).shuffle(idx)
    y, theta = data[idx[:M]].astype('float32'), slice_directions(16, swd.num_mom_conds, 0)
    bw = np.tile(np.asarray(MM_PARAMS['bandwidths']), 2)[None].repeat(B, 0)
    con = np.repeat(np.asarray(MM_PARAMS['contrasts']), 3)[None].repeat(B, 0)
    J, Dp, S = (og.t64(JDS[k]).clone().requires_grad_(True) for k in 'JDS')
    ta, dyn, rate = og.euler_ssn(og.make_W(zs, J, Dp, S, N), og.stimulus(bw, con, on.DEFAULT_PARAMS['smoothness'], N),
                                 'asym_tanh', 0.01, 2.2, 10., 1., 0.1, 40, 30, 5.0)
    tc = ta[:, :, torch.as_tensor(np.asarray(swd.gen.probes), dtype=torch.long)].reshape(B, -1)
    px, py = tc @ og.t64(theta).T, og.t64(y) @ og.t64(theta).T
    bare = ((torch.sort(px, dim=0).values.repeat_interleave(M // B, dim=0) - torch.sort(py, dim=0).values) ** 2).mean()
    loss = bare + 1.0 * dyn + 0.01 * rate
    gJ, gD, gS = torch.autograd.grad(loss, [J, Dp, S])
    print('swd', info.swd, float(bare.detach()), 'loss', info.loss, float(loss.detach()))
    np.testing.assert_allclose(info.swd, float(bare.detach()), rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(info.loss, float(loss.detach()), rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(info.dynamics_penalty, float(dyn.detach()), rtol=1e-3, atol=1e-7)
    np.testing.assert_allclose(info.rate_penalty, float(rate.detach()), rtol=1e-3, atol=1e-7)
    assert info.swd_per_direction.shape == (16,)
    for name, g in (('J', gJ), ('D', gD), ('S', gS)):
        want = np.clip(JDS[name] - 0.01 * g.numpy(), 1e-3, 10)
        got = getattr(swd.gen, name)
        np.testing.assert_allclose(got - JDS[name], want - JDS[name], rtol=5e-3, atol=5e-3 * np.abs(want - JDS[name]).max())
    # the step's gradient is the restatement's on the GPU's own tuning curves
    np.testing.assert_array_equal(swd.last_gx.cpu().numpy(), zc.swd(swd.last_x.cpu().numpy(), y, theta, 2)['gx'])


def test_the_whole_truth_every_step_with_fewer_truth_rows_than_draws():
    """swd_truth_batch = -1: 16 draws against a truth of 5 rows, which `random_minibatches` refuses; every step sees all 5."""
    from tc_gan_amd.analyzers.distdiff import slice_directions
    from tc_gan_amd.networks.sliced_wasserstein import make_sliced_wasserstein
    swd, _ = make_sliced_wasserstein(dict(SWD_PARAMS, swd_power=1, batchsize=16, swd_truth_batch=-1))
    data = (np.random.RandomState(6).rand(5, swd.num_mom_conds) * 8).astype('float32')
    swd.set_dataset(data)
    assert swd.minibatch_rows is None
    updates = swd.learning()
    info = next(updates)
    want = zc.swd(swd.last_x.cpu().numpy(), data, slice_directions(16, swd.num_mom_conds, 0), 1)
    np.testing.assert_array_equal(swd.last_gx.cpu().numpy(), want['gx'])
    np.testing.assert_allclose(info.swd, want['loss'], rtol=64 * 2.0 ** -52)
    assert np.isfinite(next(updates).swd)
    np.testing.assert_array_equal(swd.next_minibatch().cpu().numpy(), data)


LEARN_STEPS = 100


def learning_run(truth_batch, steps=LEARN_STEPS):
    """The sliced W1 to the truth at the end parameters (and at the start): the run of
    tests/test_swd_train_gpu.py::learning_run -- 2N = 40, 8 bandwidths, 200 steps of dynamics, truth of 512 rows, start perturbed
    by +30 % / -25 % -- at batchsize 16 with `swd_truth_batch`.  The W1 is the restatement's p = 1 loss of 256 draws on one
    fixed noise stream against 256 truth rows on 64 fixed directions."""
    from tc_gan_amd.analyzers.distdiff import slice_directions
    from tc_gan_amd.networks.dataset import dataset_by_fixedtime
    from tc_gan_amd.networks.fixed_time_sampler import FixedTimeTuningCurveSampler, new_JDS
    from tc_gan_amd.networks.sliced_wasserstein import make_sliced_wasserstein
    true = {k: np.asarray(new_JDS[k], dtype=float) for k in 'JDS'}
    pert = np.array([[1.3, 0.75], [0.75, 1.3]])
    swd, rest = make_sliced_wasserstein(dict(
        num_sites=20, seqlen=200, skip_steps=150, batchsize=16, sample_sites=[0], include_inhibitory_neurons=False,
        bandwidths=[0, 0.0625, 0.125, 0.1875, 0.25, 0.5, 0.75, 1], contrasts=[20.],
        J0=true['J'] * pert, D0=true['D'] * pert, S0=true['S'] * pert, learning_rate=0.01, update_name='adam-wgan',
        swd_directions=64, swd_power=2, swd_truth_batch=truth_batch))
    assert rest == {}
    truth = dataset_by_fixedtime(swd, truth_size=512, truth_seed=42, true_ssn_options={k: true[k] for k in 'JDS'})
    swd.set_dataset(truth)
    theta = slice_directions(64, truth.shape[1], 11)

    def w1():
        jds = dict(zip('JDS', swd.get_gen_param()))
        x = FixedTimeTuningCurveSampler.from_learner(swd, batchsize=256, seed=7, **jds).forward().prober_tuning_curve
        return sc.swd(x.cpu().numpy().astype('float32'), truth[:256].astype('float32'), theta, 1)['loss']
    start = w1()
    updates = swd.learning()
    losses = [next(updates).swd for _ in range(steps)]
    assert np.isfinite(losses).all()
    return start, w1()


def test_seeded_run_with_a_larger_truth_minibatch_ends_no_farther_from_the_truth():
    """Both runs 100 steps at batchsize 16.  The yardstick is the run with swd_truth_batch = 0, which executes the rank-matching
    path alone; the run with 256 truth rows per step must end no higher than twice its final sliced W1 (the factor is for the
    evaluation's own sampling noise at 256 draws).  Measured on MI355X: see DESIGN 3.11e."""
    start0, end0 = learning_run(0)
    start, end = learning_run(256)
    print('sliced W1 to the truth: start', start0, start, 'end with swd_truth_batch = 0:', end0, '256:', end)
    assert start == start0
    assert np.isfinite(end0) and np.isfinite(end) and end <= 2 * end0
    # the yardstick run itself learns: the ratio bound tests/test_swd_train_gpu.py asserts for its run of 64 draws (measured
    # here at 16 draws: 8.9e-4)
    assert end0 <= LEARN_RATIO * start0

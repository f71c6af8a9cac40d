"""The sliced Wasserstein loss of the critic-free trainer (csrc/ssn_swd.hip, networks/sliced_wasserstein.py), the parts that need
no GPU: the restatement the GPU tests compare with (tests/swd_cases.py) against known answers, scipy, fp64 autograd through
torch.sort and a finite difference; how far three deliberate errors move what is checked; the C entry points' refusals, the
header / clib / export agreement, the generated code of the new file, and the command lines."""
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import swd_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tc_gan_amd', 'csrc')


def _unit(rs, L, D):
    g = rs.randn(L, D)
    return (g / np.sqrt((g * g).sum(axis=1, keepdims=True))).astype('float32')


def _torch_loss(x, y, theta, power):
    """The loss in fp64 torch: projections, torch.sort, mean over ranks and directions."""
    px, py = x @ theta.T, y @ theta.T
    d = torch.sort(px, dim=0).values - torch.sort(py, dim=0).values
    return (d.abs() if power == 1 else d * d).mean()


# ---- 1. the restatement against known answers ----------------------------------------------------------------------------

@pytest.mark.parametrize('power', [1, 2])
def test_constant_shift_known_answer(power):
    """x = y + c: every rank moves by c . theta_l, so loss = mean_l |c . theta_l|^p; on a lattice this is exact."""
    rs = np.random.RandomState(0)
    _, y, theta = sc.lattice_inputs(rs, 16, 4, 5)
    c = (rs.randint(-16, 17, size=5) / 8.0).astype('float32')
    got = sc.swd(y + c[None, :], y, theta, power)
    shift = [sum(Fraction(float(a)) * Fraction(float(b)) for a, b in zip(c, th)) for th in theta]
    assert got['loss_l'] == [abs(s) ** power for s in shift]
    assert got['loss'] == float(sum(abs(s) ** power for s in shift) / 4)
    # the coefficients: the same for every row of a direction
    want = [np.sign(float(s)) / 64.0 if power == 1 else 2.0 * float(s) / 64.0 for s in shift]
    np.testing.assert_array_equal(got['coef'], np.tile(np.asarray(want, dtype='float32'), (16, 1)))


def test_restatement_equals_scipy_per_direction():
    wasserstein_distance = pytest.importorskip('scipy.stats').wasserstein_distance
    rs = np.random.RandomState(1)
    worst = 0.0
    for B, L, D in ((1, 3, 2), (7, 5, 3), (64, 9, 6), (300, 4, 40)):
        x, y, theta = sc.generic_inputs(rs, B, L, D)
        got = sc.swd(x, y, theta, 1)
        for l in range(L):
            ref = wasserstein_distance(got['px'][:, l].astype('float64'), got['py'][:, l].astype('float64'))
            worst = max(worst, abs(float(got['loss_l'][l]) - ref))
    print('largest difference to scipy:', worst)
    assert worst <= 1e-12


@pytest.mark.parametrize('power', [1, 2])
def test_restatement_equals_fp64_autograd_through_sort(power):
    """The restatement rounds the projections, the coefficients and the gradient to float32 (2^-24 = 6e-8 relative each) where
    autograd stays in fp64: loss within 1e-6 relative, gradient within 1e-6 of its largest entry (the issue's prototype measured
    4e-8 and 4.4e-8 / 7.3e-8).  Generic rows: no ties, so both sorts order alike."""
    rs = np.random.RandomState(2)
    B, L, D = 50, 16, 7
    x, y, theta = rs.randn(B, D).astype('float32'), (rs.randn(B, D) + 0.5).astype('float32'), _unit(rs, L, D)
    got = sc.swd(x, y, theta, power)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    loss = _torch_loss(xt, torch.tensor(y, dtype=torch.float64), torch.tensor(theta, dtype=torch.float64), power)
    grad, = torch.autograd.grad(loss, xt)
    print('loss', got['loss'], float(loss.detach()), 'gradient difference / largest entry',
          np.abs(got['gx'] - grad.numpy()).max() / np.abs(grad.numpy()).max())
    np.testing.assert_allclose(got['loss'], float(loss.detach()), rtol=1e-6)
    np.testing.assert_allclose(got['gx'], grad.numpy(), rtol=0, atol=1e-6 * np.abs(grad.numpy()).max())


def test_gradient_equals_central_finite_difference_of_the_squared_loss():
    """p = 2: the loss is piecewise quadratic and C^1 in x, so a central difference with h = 1e-4 is off by the fp64 noise of
    the difference (1e-16 / h) and by rank changes inside [x - h, x + h] (h times a coefficient step): 1e-4 of the largest entry."""
    rs = np.random.RandomState(3)
    B, L, D = 12, 8, 4
    x, y, theta = rs.randn(B, D).astype('float32'), (rs.randn(B, D) + 0.5).astype('float32'), _unit(rs, L, D)
    gx = sc.swd(x, y, theta, 2)['gx']
    yt, tt = torch.tensor(y, dtype=torch.float64), torch.tensor(theta, dtype=torch.float64)
    fd = np.empty((B, D))
    h = 1e-4
    for b in range(B):
        for c in range(D):
            up, down = x.astype('float64'), x.astype('float64')
            up[b, c] += h
            down[b, c] -= h
            fd[b, c] = (float(_torch_loss(torch.tensor(up), yt, tt, 2)) - float(_torch_loss(torch.tensor(down), yt, tt, 2))) / (2 * h)
    print('difference / largest entry', np.abs(gx - fd).max() / np.abs(fd).max())
    np.testing.assert_allclose(gx, fd, rtol=0, atol=1e-4 * np.abs(fd).max())


def test_projection_and_backprojection_are_the_sequential_sums():
    rs = np.random.RandomState(5)
    coef, theta = rs.randn(4, 9).astype('float32'), rs.randn(9, 3).astype('float32')
    want = np.empty((4, 3), dtype='float32')
    for r in range(4):
        for c in range(3):
            acc = Fraction(0)
            for l in range(9):
                acc = Fraction(float(acc + Fraction(float(coef[r, l])) * Fraction(float(theta[l, c]))))   # one rounding: an fma
            want[r, c] = np.float32(float(acc))
    np.testing.assert_array_equal(sc.backproject(coef, theta), want)


def test_ties_zero_differences_and_non_finite_columns():
    px = np.array([[2.0], [1.0], [2.0], [-0.0], [1.0]], dtype='float32')           # ranks: rows 3, 1, 4, 0, 2
    py = np.array([[0.0], [1.0], [3.0], [2.0], [0.5]], dtype='float32')             # sorted: 0, 0.5, 1, 2, 3
    coef, loss = sc.match(px, py, 1)
    # d by rank: 0 - 0, 1 - 0.5, 1 - 1, 2 - 2, 2 - 3
    assert loss == [(Fraction(1, 2) + 1) / 5]
    np.testing.assert_array_equal(coef[:, 0], np.array([0, 0.2, -0.2, 0, 0], dtype='float32'))
    assert not np.signbit(coef[[0, 3, 4], 0]).any()                                  # sign(0) = 0: +0
    coef, loss = sc.match(px, py, 2)
    assert loss == [(Fraction(1, 4) + 1) / 5]
    np.testing.assert_array_equal(coef[:, 0], (2.0 * np.array([0, 0.5, -1.0, 0, 0]) * (1.0 / 5.0)).astype('float32'))
    for bad in (np.nan, np.inf, -np.inf):
        for side in (0, 1):
            p = [px.repeat(2, axis=1).copy(), py.repeat(2, axis=1).copy()]
            p[side][2, 1] = bad
            coef, loss = sc.match(p[0], p[1], 2)
            assert loss[1] is None and np.isnan(coef[:, 1]).all() and loss[0] is not None and np.isfinite(coef[:, 0]).all()
            assert np.isnan(sc.backproject(coef, np.ones((2, 3), dtype='float32'))).all()


@pytest.mark.parametrize('power', [1, 2])
def test_loss_in_kernel_order_is_exact_on_a_lattice_and_within_the_bound_elsewhere(power):
    """The restatement of the order of additions against the exact loss of `match`: equal where every operation is exact, inside
    `loss_bound` on generic values; NaN for a column that is not finite.  B below, at and above one term per thread."""
    for B, L, D in ((1, 1, 1), (64, 2, 6), (1024, 4, 6)):
        x, y, theta = sc.lattice_inputs(np.random.RandomState(200 + B), B, L, D)
        want = sc.swd(x, y, theta, power)
        got = [sc.loss_in_kernel_order(want['px'][:, l], want['py'][:, l], power) for l in range(L)]
        assert [Fraction(float(v)) for v in got] == want['loss_l']
    worst = Fraction(0)
    for B, L, D in ((2, 3, 6), (65, 5, 6), (300, 5, 40), (1000, 3, 6)):
        x, y, theta = sc.generic_inputs(np.random.RandomState(100 + B), B, L, D)
        want = sc.swd(x, y, theta, power)
        for l in range(L):
            exact = want['loss_l'][l]
            err = abs(Fraction(float(sc.loss_in_kernel_order(want['px'][:, l], want['py'][:, l], power))) - exact)
            assert err <= sc.loss_bound(exact, B), (B, l)
            if exact:
                worst = max(worst, err / sc.loss_bound(exact, B))
    print('largest error of the restatement: {:.3g} of the bound'.format(float(worst)))
    assert worst > 0                                              # (generic values do round: the order is exercised)
    px = np.array([1.0, np.inf, 2.0], dtype='float32')
    assert np.isnan(sc.loss_in_kernel_order(px, np.ones(3, dtype='float32'), power))
    assert np.isnan(sc.loss_in_kernel_order(np.ones(3, dtype='float32'), [0.0, np.nan, 1.0], power))


# ---- 2. sensitivity: what a wrong restatement would move ---------------------------------------------------------------

def test_deliberate_errors_move_the_checked_quantities_far_beyond_their_tolerances():
    """The GPU tests hold coef and gx to bit equality (tolerance: nothing; one float32 ulp, 2^-23 = 1.2e-7 relative, is the least
    a difference can be) and loss_l to (B + 2) 2^-52 relative.  Measured here at B = 65, L = 33, D = 6, p = 2, on the inputs of
    the GPU tests: ties broken the other way move coef by 0.17 of its largest entry (1.4e6 ulps), a dropped last rank moves
    every loss_l by at least 7e10 times its bound, coefficients left at their ranks move coef by 1.3 times its largest entry
    (1.1e7 ulps).  Asserted with a margin: factors of at least 1e5, 1e9 and 1e6."""
    rs = np.random.RandomState(4)
    B, L, D = 65, 33, 6
    x, y, theta = sc.generic_inputs(rs, B, L, D)
    right = sc.swd(x, y, theta, 2)
    ulp = 2.0 ** -23
    top = np.abs(right['coef']).max()

    tied = sc.swd(x, y, theta, 2, ties='reversed')
    moved = np.abs(tied['coef'] - right['coef']).max() / top
    assert tied['loss_l'] == right['loss_l']                      # (the loss cannot see the tie-break: the coefficients do)
    print('ties reversed: coef moves by', moved, 'of its largest entry, factor', moved / ulp)
    assert moved / ulp >= 1e5
    assert np.abs(tied['gx'] - right['gx']).max() / np.abs(right['gx']).max() / ulp >= 1e5

    dropped = sc.swd(x, y, theta, 2, drop_last=True)
    factors = [float((a - b) / sc.loss_bound(a, B)) for a, b in zip(right['loss_l'], dropped['loss_l']) if a != 0]
    print('last rank dropped: loss_l moves by at least', min(factors), 'times its bound')
    assert len(factors) == L - 1 and min(factors) >= 1e9

    ranked = sc.swd(x, y, theta, 2, scatter='rank')
    moved = np.abs(ranked['coef'] - right['coef']).max() / top
    print('scattered by rank: coef moves by', moved, 'of its largest entry, factor', moved / ulp)
    assert moved / ulp >= 1e6
    assert np.abs(ranked['gx'] - right['gx']).max() / np.abs(right['gx']).max() / ulp >= 1e6


# ---- 3. the library: refusals, declarations, generated code ---------------------------------------------------------------

def test_new_symbols_are_declared():
    from tc_gan_amd import clib
    header = open(os.path.join(ROOT, 'include', 'ssnode_mi355x.h')).read()
    for name in ('ssn_swd_match_f32', 'ssn_swd_backproject_f32'):
        assert name in clib.DECLARED_SYMBOLS and getattr(clib.libssnode, name).argtypes is not None
        assert re.search(r'^int %s\(' % name, header, re.M)
    assert len(clib.libssnode.ssn_swd_match_f32.argtypes) == 8 and len(clib.libssnode.ssn_swd_backproject_f32.argtypes) == 7
    assert int(re.search(r'#define SSN_SWD_MAX_BATCH (\d+)', header).group(1)) == clib.SWD_MAX_BATCH == 4096
    assert 'ssn_swd.hip' in open(os.path.join(CSRC, 'Makefile')).read()
    nm = shutil.which('nm')
    if nm:
        exported = subprocess.run([nm, '-D', '--defined-only', clib.libssnode._name], check=True, stdout=subprocess.PIPE,
                                  universal_newlines=True).stdout
        assert ' T ssn_swd_match_f32' in exported and ' T ssn_swd_backproject_f32' in exported


def test_c_entry_points_refuse_from_the_arguments_alone():
    """Host checks in front of any HIP call: no device needed."""
    from tc_gan_amd import clib
    lib = clib.libssnode
    invalid = clib.SSN_ERR_BASE + 1                  # hipErrorInvalidValue
    assert lib.ssn_swd_match_f32(None, None, clib.SWD_MAX_BATCH + 1, 1, 2, None, None, None) == invalid
    assert '4096 rows' in clib.last_error()
    assert lib.ssn_swd_match_f32(None, None, 4, clib.W1_MAX_DIRECTIONS + 1, 2, None, None, None) == invalid
    assert '4096 directions' in clib.last_error()
    assert lib.ssn_swd_match_f32(None, None, 4, 3, 2, None, None, None) == invalid            # null pointers
    assert 'invalid argument' in clib.last_error()
    assert lib.ssn_swd_match_f32(None, None, -1, 3, 2, None, None, None) == invalid
    assert lib.ssn_swd_match_f32(None, None, 4, -3, 2, None, None, None) == invalid
    for power in (0, 3, -1):
        assert lib.ssn_swd_match_f32(None, None, 0, 0, power, None, None, None) == invalid
    assert lib.ssn_swd_backproject_f32(None, None, 4, clib.W1_MAX_DIRECTIONS + 1, 3, None, None) == invalid
    assert '4096 directions' in clib.last_error()
    assert lib.ssn_swd_backproject_f32(None, None, 4, 5, 3, None, None) == invalid              # null pointers
    assert lib.ssn_swd_backproject_f32(None, None, -1, 5, 3, None, None) == invalid
    assert lib.ssn_swd_backproject_f32(None, None, 4, 5, -3, None, None) == invalid
    # empty problems succeed
    for power in (1, 2):
        assert lib.ssn_swd_match_f32(None, None, 0, 5, power, None, None, None) == 0
        assert lib.ssn_swd_match_f32(None, None, 4, 0, power, None, None, None) == 0
    assert lib.ssn_swd_backproject_f32(None, None, 0, 5, 3, None, None) == 0
    assert lib.ssn_swd_backproject_f32(None, None, 4, 5, 0, None, None) == 0


def test_trainer_refusals_need_no_device(monkeypatch):
    from tc_gan_amd.networks.sliced_wasserstein import DEFAULT_PARAMS, make_sliced_wasserstein
    assert (DEFAULT_PARAMS['swd_directions'], DEFAULT_PARAMS['swd_power'], DEFAULT_PARAMS['swd_direction_seed']) == (128, 2, 0)
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='one GPU'):
        make_sliced_wasserstein({})


def test_direction_draws_continue_one_stream():
    from tc_gan_amd.analyzers.distdiff import draw_slice_directions, slice_directions
    rng = np.random.RandomState(7)
    first, second = draw_slice_directions(rng, 5, 9), draw_slice_directions(rng, 5, 9)
    np.testing.assert_array_equal(first, slice_directions(5, 9, 7))
    g = np.random.RandomState(7).randn(10, 9)[5:]
    np.testing.assert_array_equal(second, (g / np.sqrt((g * g).sum(axis=1))[:, None]).astype('float32'))
    with pytest.raises(ValueError, match='directions'):
        draw_slice_directions(rng, 0, 9)


def test_no_kernel_of_the_new_file_spills_or_uses_scratch(tmp_path):
    """Metadata only.  LDS: the match kernel's static part is 40 bytes (four doubles, one flag) beside the dynamic
    12 P <= 48 KiB the launch asks for; the back-projection's two tiles are 16 x 65 + 64 x 16 floats = 8256 bytes."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = tmp_path / 'ssn_swd.s'
    flags = ['-O3', '-std=c++17', '--offload-arch=gfx950']                       # csrc/Makefile: CXXFLAGS
    subprocess.run([hipcc] + flags + ['-S', '--cuda-device-only', 'ssn_swd.hip', '-o', str(out)], cwd=CSRC, check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(str(out)).read()
    found = re.findall(r'\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)'
                       r'.*?\.sgpr_spill_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+).*?\.wavefront_size:\s+(\d+)', text, re.S)
    lds = {('match' if 'swd_match_kernel' in name else 'backproject' if 'swd_backproject_kernel' in name else name): int(g)
           for g, name, _, _, _, _ in found}
    assert lds == {'match': 40, 'backproject': 8256}, found
    assert all(int(p) == 0 and int(ss) == 0 and int(vs) == 0 and int(w) == 64 for _, _, p, ss, vs, w in found), found
    source = open(os.path.join(CSRC, 'ssn_swd.hip')).read()
    assert 'asm' not in source and 'atomic' not in source.replace('no atomics', '')


# ---- 4. command lines -----------------------------------------------------------------------------------------------------

#: the option namespaces of the three older scripts with no argument, as they are on the parent commit
_COMMON = dict(truth_size=1000, truth_seed=42, dataset_provider='ssnode', contrasts=[20], include_inhibitory_neurons=False,
               unroll_scan=False, J0=0.01, D0=0.01, S0=0.01, ssn_type='default', gen_kernel='auto', z_device_seed=None,
               z_host_draw=False, iterations=100000, quiet=False, n_bandwidths=4, load_gen_param=None, datastore=None, load_config=None)
_GAN = dict(_COMMON, gen_learning_rate=0.01, gen_update_name='adam-wgan', disc_learning_rate=0.01, disc_update_name='adam-wgan',
            seqlen=1200, skip_steps=1000, gen_J_min=1e-3, gen_D_min=1e-3, gen_S_min=1e-3, gen_J_max=10, gen_D_max=10, gen_S_max=10,
            gen_dynamics_cost=1, disc_layers=[], disc_normalization='none', disc_nonlinearity='rectify', disc_precision='fp32',
            lipschitz_cost=10.0, critic_iters_init=50, critic_iters=5, quit_JDS_threshold=-1, disc_param_save_interval=5,
            disc_param_template='last.npz', disc_param_save_on_error=False, checkpoint_interval=-1, resume_from=None)
PARENT_NAMESPACES = {
    'w': dict(_GAN, batchsize=15, sample_sites=[0], datastore_template='logfiles/BPTT_WGAN_{layers_str}'),
    'c': dict(_GAN, num_models=15, probes_per_model=1, norm_probes=[0], tc_stats_record_interval=100,
              datastore_template='logfiles/BPTT_CWGAN_{layers_str}'),
    'm': dict(_COMMON, batchsize=15, sample_sites=[0], learning_rate=0.01, update_name='adam-wgan', seqlen=1200, skip_steps=1000,
              J_min=1e-3, D_min=1e-3, S_min=1e-3, J_max=10, D_max=10, S_max=10, dynamics_cost=1, lam=.1,
              moment_weights_regularization=1e-3, moment_weight_type='mean', gen_moments_record_interval=100,
              datastore_template='logfiles/BPTT_MM_{lam}'),
}


def test_the_older_scripts_parse_as_on_the_parent_commit():
    from tc_gan_amd.run import bptt_cwgan, bptt_moments, bptt_wgan
    for key, module in (('w', bptt_wgan), ('c', bptt_cwgan), ('m', bptt_moments)):
        got = vars(module.make_parser().parse_args([]))
        assert got == PARENT_NAMESPACES[key], (key, {k for k in set(got) | set(PARENT_NAMESPACES[key]) if got.get(k, key) != PARENT_NAMESPACES[key].get(k, key)})
        assert not [k for k in got if k.startswith('swd')]


def test_bptt_swd_command_line(capsys):
    from tc_gan_amd.run import bptt_moments, bptt_swd, options
    with pytest.raises(SystemExit) as err:
        bptt_swd.main(['--help'])
    assert err.value.code == 0
    text = capsys.readouterr().out
    assert '--swd-directions' in text and '--swd-power' in text and '--swd-direction-seed' in text
    got = vars(bptt_swd.make_parser().parse_args([]))
    assert (got['swd_directions'], got['swd_power'], got['swd_direction_seed']) == (128, 2, 0)
    assert got['datastore_template'] == 'logfiles/BPTT_SWD_{swd_directions}_{swd_power}'
    moments = vars(bptt_moments.make_parser().parse_args([]))
    dropped = {'lam', 'moment_weights_regularization', 'moment_weight_type', 'gen_moments_record_interval'}
    assert set(got) == (set(moments) - dropped) | {'swd_directions', 'swd_power', 'swd_direction_seed'}
    assert all(got[k] == moments[k] for k in set(moments) - dropped - {'datastore_template'})
    with pytest.raises(SystemExit):
        bptt_swd.make_parser().parse_args(['--swd-power', '3'])
    with pytest.raises(SystemExit):
        bptt_swd.make_parser().parse_args(['--lam', '1'])
    on = vars(bptt_swd.make_parser().parse_args(['--swd-power', '1', '--swd-directions', '16', '--swd-direction-seed', '4']))
    assert (on['swd_directions'], on['swd_power'], on['swd_direction_seed']) == (16, 1, 4)
    flags = [f for o in options.options_of('s') for f in o['flags']]
    assert len(flags) == len(set(flags))


def test_run_script_resolves_the_reference_module_path():
    import importlib
    module = 'tc_gan.run.bptt_swd'
    loaded = importlib.import_module('tc_gan_amd.' + module[len('tc_gan.'):])      # (run.py's mapping)
    assert hasattr(loaded, 'main') and hasattr(loaded, 'make_parser')
    assert "module.startswith('tc_gan.')" in open(os.path.join(ROOT, 'run.py')).read()


def test_learning_table_columns():
    from tc_gan_amd import recorders as r
    assert r.SWDLearningRecorder.tablename == 'learning'
    assert r.SWDLearningRecorder.dtype.names == ('step', 'loss', 'swd', 'dynamics_penalty', 'rate_penalty', 'train_time')
    assert r.MMLearningRecorder.dtype.names == ('step', 'loss', 'rate_penalty', 'dynamics_penalty', 'train_time')

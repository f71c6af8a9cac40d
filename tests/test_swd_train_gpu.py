"""The sliced Wasserstein trainer on the GPU (networks/sliced_wasserstein.py, drivers.SlicedWassersteinDriver, run/bptt_swd.py): one
update against fp64 autograd on the restatement's forward, the p = 1 gradient handed to the adjoint sweep bit for bit, the wiring's
known answer (the generator's own output as the truth), the command line, the refusal of several ranks, and a seeded run that
moves the generator toward the truth as the sliced W1 measures it."""
import json

import numpy as np
import pytest
import torch

import swd_cases as sc
from oracle import gan_torch as og
from oracle import ssn_numpy as on
from test_moments import JDS, MM_PARAMS, _load_tables

pytestmark = pytest.mark.gpu

SWD_PARAMS = dict({k: v for k, v in MM_PARAMS.items() if k not in ('lam', 'moment_weights_regularization')}, swd_directions=16)


def _make(power, **over):
    from tc_gan_amd.networks.sliced_wasserstein import make_sliced_wasserstein
    swd, rest = make_sliced_wasserstein(dict(SWD_PARAMS, swd_power=power, **over))
    assert rest == {}
    return swd


def _first_step_inputs(data, batch, directions, columns, seed=0):
    """What the trainer's first step takes: the first minibatch of `utils.random_minibatches` on RandomState(seed), the first
    direction draw of the same seed."""
    from tc_gan_amd.analyzers.distdiff import slice_directions
    idx = np.arange(len(data))
    np.random.RandomState(seed).shuffle(idx)
    return data[idx[:batch]].astype('float32'), slice_directions(directions, columns, seed)


def test_one_sliced_wasserstein_update_vs_oracle():
    """Same seed -> the moment matcher's zs; p = 2, sgd: the bare loss, the total, the penalties and the post-update (J, D, S)
    with the tolerances of test_one_moment_matching_update_vs_oracle."""
    swd = _make(2)
    assert swd.num_mom_conds == 6 * 4
    data = np.random.RandomState(5).rand(12, swd.num_mom_conds) * 8
    swd.set_dataset(data)
    info = next(swd.learning())
    assert info.step == 0

    N = 10
    zs = og.t64(np.random.RandomState(0).rand(6, 2 * N, 2 * N))
    y, theta = _first_step_inputs(data, 6, 16, swd.num_mom_conds)
    bw = np.tile(np.asarray(MM_PARAMS['bandwidths']), 2)[None].repeat(6, 0)
    con = np.repeat(np.asarray(MM_PARAMS['contrasts']), 3)[None].repeat(6, 0)
    J, D, S = (og.t64(JDS[k]).clone().requires_grad_(True) for k in 'JDS')
    # the forward oracle/gan_torch.moment_matching_loss is built on
    ta, dyn, rate = og.euler_ssn(og.make_W(zs, J, D, S, N), og.stimulus(bw, con, on.DEFAULT_PARAMS['smoothness'], N),
                                 'asym_tanh', 0.01, 2.2, 10., 1., 0.1, 40, 30, 5.0)
    tc = ta[:, :, torch.as_tensor(np.asarray(swd.gen.probes), dtype=torch.long)].reshape(6, -1)
    px, py = tc @ og.t64(theta).T, og.t64(y) @ og.t64(theta).T
    bare = ((torch.sort(px, dim=0).values - torch.sort(py, dim=0).values) ** 2).mean()
    loss = bare + 1.0 * dyn + 0.01 * rate
    gJ, gD, gS = torch.autograd.grad(loss, [J, D, S])
    print('swd', info.swd, float(bare.detach()), 'loss', info.loss, float(loss.detach()))
    np.testing.assert_allclose(info.swd, float(bare.detach()), rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(info.loss, float(loss.detach()), rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(info.dynamics_penalty, float(dyn.detach()), rtol=1e-3, atol=1e-7)
    np.testing.assert_allclose(info.rate_penalty, float(rate.detach()), rtol=1e-3, atol=1e-7)
    assert info.swd_per_direction.shape == (16,) and info.train_time > 0
    for name, g in (('J', gJ), ('D', gD), ('S', gS)):
        want = np.clip(JDS[name] - 0.01 * g.numpy(), 1e-3, 10)
        got = getattr(swd.gen, name)
        np.testing.assert_allclose(got - JDS[name], want - JDS[name], rtol=5e-3, atol=5e-3 * np.abs(want - JDS[name]).max())


def test_power_one_hands_the_restatements_gradient_to_the_adjoint_sweep():
    """The ranks of near-tied projections may differ between an fp32 and an fp64 forward and the p = 1 gradient jumps there: the
    gx of the step is compared with the restatement on the GPU's own tuning curves instead (backward given gx is pinned by
    tests of its own)."""
    swd = _make(1)
    data = np.random.RandomState(5).rand(12, swd.num_mom_conds) * 8
    swd.set_dataset(data)
    info = next(swd.learning())
    y, theta = _first_step_inputs(data, 6, 16, swd.num_mom_conds)
    want = sc.swd(swd.last_x.cpu().numpy(), y, theta, 1)
    np.testing.assert_array_equal(swd.last_gx.cpu().numpy(), want['gx'])
    assert np.abs(want['gx']).max() > 0
    np.testing.assert_allclose(info.swd, want['loss'], rtol=32 * 2.0 ** -52)
    np.testing.assert_allclose(info.loss, info.swd + info.dynamics_penalty + 0.01 * info.rate_penalty, rtol=1e-12)


@pytest.mark.parametrize('power', [1, 2])
def test_the_generators_own_output_as_truth_gives_zero(power):
    swd = _make(power)
    swd.set_dataset(np.zeros((6, swd.num_mom_conds)))
    swd.next_minibatch = lambda: swd.last_x.clone()
    before = swd.get_gen_param()
    swd.dynamics_cost = swd.rate_cost = 0.0
    info = next(swd.learning())
    assert info.swd == 0.0 and (info.swd_per_direction == 0).all()
    assert float(swd.last_gx.abs().max()) == 0.0
    for a, b in zip(before, swd.get_gen_param()):                # no loss gradient, no penalty gradient: sgd moves nothing
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-7)


@pytest.mark.parametrize('args', [
    [],
    ['--ssn-type', 'heteroin', '--dataset-provider', 'fixedtime'],
    ['--swd-power', '1'],
])
def test_cli_single_g_step(args, tmp_path, monkeypatch):
    from tc_gan_amd.run import bptt_swd
    monkeypatch.chdir(tmp_path)
    bptt_swd.main(['--iterations', '1', '--truth_size', '1', '--n_samples', '1', '--n_bandwidths', '1',
                   '--seqlen', '4', '--skip-steps', '2', '--swd-directions', '8', '--datastore', 'results', '--quiet'] + args)
    out = tmp_path / 'results'
    info = json.load(open(out / 'info.json'))
    assert info['extra_info']['script_file'] == bptt_swd.__file__
    assert info['run_config']['swd_power'] == (1 if '--swd-power' in args else 2) and info['run_config']['swd_directions'] == 8
    assert json.load(open(out / 'exit.json')) == dict(reason='end_of_iteration', good=True)
    assert np.load(out / 'truth.npy').shape[0] == 1
    tables = _load_tables(str(out), 'store')
    assert set(tables) == {'learning', 'generator'}
    assert tables['learning'].dtype.names == ('step', 'loss', 'swd', 'dynamics_penalty', 'rate_penalty', 'train_time')
    assert len(tables['learning']) == 1 and np.isfinite(tables['learning']['loss']).all()
    assert np.isfinite(tables['learning']['swd']).all() and (tables['learning']['swd'] >= 0).all()
    vnames = ('V_E', 'V_I') if '--ssn-type' in args else ()
    assert tables['generator'].dtype.names[:1 + len(vnames)] == ('gen_step',) + vnames


def test_several_ranks_are_refused(monkeypatch):
    from tc_gan_amd.networks.sliced_wasserstein import make_sliced_wasserstein
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='one GPU'):
        make_sliced_wasserstein(dict(SWD_PARAMS))


LEARN_STEPS = 100
LEARN_RATIO = 0.0239      # the geometric mean of 1 and the measured ratio (see the test's docstring)


def learning_run(steps, power=2):
    """(sliced W1 to the truth at the start parameters, at the end parameters): 2N = 40, 64 models, 8 bandwidths, 200 steps of
    dynamics, truth of 512 rows from the fixed-time provider at the default (J, D, S), start perturbed by +30 % / -25 %
    (tools/learn_probe.py's shape).  The W1 is the restatement's p = 1 loss of 256 draws on one fixed noise stream against 256
    truth rows on 64 fixed directions."""
    from tc_gan_amd.analyzers.distdiff import slice_directions
    from tc_gan_amd.networks.dataset import dataset_by_fixedtime
    from tc_gan_amd.networks.fixed_time_sampler import FixedTimeTuningCurveSampler, new_JDS
    from tc_gan_amd.networks.sliced_wasserstein import make_sliced_wasserstein
    true = {k: np.asarray(new_JDS[k], dtype=float) for k in 'JDS'}
    pert = np.array([[1.3, 0.75], [0.75, 1.3]])
    swd, rest = make_sliced_wasserstein(dict(
        num_sites=20, seqlen=200, skip_steps=150, batchsize=64, sample_sites=[0], include_inhibitory_neurons=False,
        bandwidths=[0, 0.0625, 0.125, 0.1875, 0.25, 0.5, 0.75, 1], contrasts=[20.],
        J0=true['J'] * pert, D0=true['D'] * pert, S0=true['S'] * pert, learning_rate=0.01, update_name='adam-wgan',
        swd_directions=64, swd_power=power))
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


def test_seeded_run_moves_the_generator_toward_the_truth():
    """Measured on MI355X (100 steps, p = 2, 0.2 s): the sliced W1 to the truth goes from 232.08 at the perturbed start -- whose
    rates run into the saturation of the transfer function -- to 0.1322, a ratio of 5.70e-4; r = sqrt(5.70e-4) = 0.0239.  Other
    run lengths and p = 1 gave ratios between 9.6e-4 and 3.3e-3 (50 and 200 steps, p = 2: 3.3e-3, 2.7e-3; p = 1 at 50, 100,
    200 steps: 1.2e-3, 3.3e-3, 9.6e-4): the minibatch loss of 64 draws is noisy at this distance, and all are 7 times below r."""
    start, end = learning_run(LEARN_STEPS)
    print('sliced W1 to the truth: start', start, 'end', end, 'ratio', end / start)
    assert np.isfinite(start) and np.isfinite(end) and end <= LEARN_RATIO * start

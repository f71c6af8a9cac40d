"""The conditional sliced Wasserstein trainer on the GPU (networks/conditional_sliced_wasserstein.py, run/bptt_cswd.py): one update
against fp64 autograd, the one-cell equivalence to the unconditional trainer on the whole truth, the wiring's known answer (the
generator's own output as every cell's truth), the command line with the scorer behind it, and a seeded conditional run against
the unconditional trainer as yardstick."""
import json
import os
from math import gcd

import numpy as np
import pytest
import torch

import swd_cases as sc
import swd_cells_cases as cc
from oracle import gan_torch as og
from oracle import ssn_numpy as on
from test_moments import JDS, MM_PARAMS, _load_tables
from test_swd_train_gpu import LEARN_RATIO

pytestmark = pytest.mark.gpu

BASE = {k: v for k, v in MM_PARAMS.items() if k not in ('lam', 'moment_weights_regularization', 'batchsize', 'sample_sites')}
CSWD_PARAMS = dict(BASE, num_models=8, probes_per_model=2, norm_probes=[0, 0.5], swd_directions=16)


def _make(power, **over):
    from tc_gan_amd.networks.conditional_sliced_wasserstein import make_conditional_sliced_wasserstein
    learner, rest = make_conditional_sliced_wasserstein(dict(CSWD_PARAMS, swd_power=power, **over))
    assert rest == {}
    return learner


def _truth(learner, rows, seed=5):
    """Random truth rows in the layout of the data set: (contrast, bandwidth, cell type, probe) columns."""
    columns = len(learner.contrasts) * len(learner.bandwidths) * (2 if learner.include_inhibitory_neurons else 1) * \
        len(learner.norm_probes)
    return np.random.RandomState(seed).rand(rows, columns) * 8


def test_one_conditional_update_vs_oracle():
    """p = 2, sgd, 2N = 20, E and I, two probes, two contrasts, 8 models x 2 probes against 12 truth rows per cell: the bare
    loss, the total, the penalties and the post-update (J, D, S) with the tolerances of
    tests/test_swd_train_gpu.py::test_one_sliced_wasserstein_update_vs_oracle.  The conditions are the sampler's on
    RandomState(swd_direction_seed), the noise RandomState(seed).rand, the directions the first draw of the direction seed.  The
    oracle's loss is sum_c (n_c / B) mean_l of the quantile coupling written with repeated rows."""
    from tc_gan_amd.analyzers.distdiff import slice_directions
    from tc_gan_amd.networks.conditional_sliced_wasserstein import cell_ids, truth_by_cell
    from tc_gan_amd.networks.cwgan import RandomChoiceSampler
    learner = _make(2)
    data = _truth(learner, 12)
    learner.set_dataset(data)
    assert learner.num_cells == 8 and tuple(learner.truth.shape) == (8, 12, 3)
    info = next(learner.learning())
    assert info.step == 0

    N, M, B = 10, 8, 16
    sampler = RandomChoiceSampler.from_grid_data(data, bandwidths=learner.bandwidths, contrasts=learner.contrasts,
                                                 norm_probes=learner.norm_probes, e_ratio=0.8, include_inhibitory_neurons=True,
                                                 seed=np.random.RandomState(0))
    batch = sampler.select_minibatch(M, 2)
    cells = cell_ids(batch.conditions, sampler.cond_values)
    np.testing.assert_array_equal(cells, learner.last_cells)
    y = truth_by_cell(sampler.nested).astype('float64')
    theta = og.t64(slice_directions(16, 3, 0))
    zs = og.t64(np.random.RandomState(0).rand(M, 2 * N, 2 * N))
    kw = batch.gen_kwargs
    J, Dp, S = (og.t64(JDS[k]).clone().requires_grad_(True) for k in 'JDS')
    ta, dyn, rate = og.euler_ssn(og.make_W(zs, J, Dp, S, N),
                                 og.stimulus(kw['stimulator_bandwidths'], kw['stimulator_contrasts'], on.DEFAULT_PARAMS['smoothness'], N),
                                 'asym_tanh', 0.01, 2.2, 10., 1., 0.1, 40, 30, 5.0)
    tc = og.conditional_probe(ta, kw['prober_model_ids'].astype(np.int64),
                              og.probes_from_norm(kw['prober_norm_probes'], kw['prober_cell_types'], N))
    assert tuple(tc.shape) == (B, 3)
    np.testing.assert_allclose(learner.last_x.cpu().numpy(), tc.detach().numpy(), rtol=1e-3, atol=1e-5)
    bare, per_cell, rows_per_cell = 0, np.zeros(8), np.zeros(8, dtype=int)
    for c in range(8):
        rows = np.nonzero(cells == c)[0]
        n, m = len(rows), y.shape[1]
        rows_per_cell[c] = n
        if n == 0:
            continue
        g = gcd(n, m)
        px, py = tc[torch.as_tensor(rows)] @ theta.T, og.t64(y[c]) @ theta.T
        d = torch.sort(px, dim=0).values.repeat_interleave(m // g, dim=0) - torch.sort(py, dim=0).values.repeat_interleave(n // g, dim=0)
        w = (d * d).mean()
        per_cell[c] = float(w.detach())
        bare = bare + (n / B) * w
    loss = bare + 1.0 * dyn + 0.01 * rate
    gJ, gD, gS = torch.autograd.grad(loss, [J, Dp, S])
    print('swd', info.swd, float(bare.detach()), 'loss', info.loss, float(loss.detach()), 'rows per cell', rows_per_cell)
    np.testing.assert_allclose(info.swd, float(bare.detach()), rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(info.loss, float(loss.detach()), rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(info.dynamics_penalty, float(dyn.detach()), rtol=1e-3, atol=1e-7)
    np.testing.assert_allclose(info.rate_penalty, float(rate.detach()), rtol=1e-3, atol=1e-7)
    np.testing.assert_array_equal(info.rows_per_cell, rows_per_cell)
    np.testing.assert_allclose(info.swd_per_cell, per_cell, rtol=1e-3, atol=1e-5)
    assert info.train_time > 0
    for name, g in (('J', gJ), ('D', gD), ('S', gS)):
        want = np.clip(JDS[name] - 0.01 * g.numpy(), 1e-3, 10)
        got = getattr(learner.gen, name)
        np.testing.assert_allclose(got - JDS[name], want - JDS[name], rtol=5e-3, atol=5e-3 * np.abs(want - JDS[name]).max())
    # the step's gradient is the restatement's on the GPU's own tuning curves
    want = cc.swd_cells(learner.last_x.cpu().numpy(), cells, y.astype('float32'), theta.numpy().astype('float32'), 2)
    np.testing.assert_array_equal(learner.last_gx.cpu().numpy(), want['gx'])
    np.testing.assert_allclose(info.swd, want['swd'], rtol=64 * 2.0 ** -52)


def test_one_cell_is_the_unconditional_trainer_on_the_whole_truth():
    """One probe, one contrast, E only, one probe per model: one cell, whose truth is the whole truth.  The first step's x, swd
    and gx are those of `BPTTSlicedWasserstein` with swd_truth_batch = -1 on the same seeds: x to the fp32 output tolerance 1e-4
    relative, swd and gx to the oracle tolerances of the test above (the probing kernels differ: no equality of bits)."""
    from tc_gan_amd.networks.sliced_wasserstein import make_sliced_wasserstein
    one = dict(BASE, include_inhibitory_neurons=False, contrasts=[20.], swd_directions=16, swd_power=2)
    cond = _make(2, include_inhibitory_neurons=False, contrasts=[20.], norm_probes=[0], probes_per_model=1, num_models=8)
    plain, rest = make_sliced_wasserstein(dict(one, batchsize=8, sample_sites=[0], swd_truth_batch=-1))
    assert rest == {}
    data = np.random.RandomState(5).rand(12, 3) * 8
    cond.set_dataset(data)
    plain.set_dataset(data)
    assert cond.num_cells == 1
    a, b = next(cond.learning()), next(plain.learning())
    assert list(a.rows_per_cell) == [8] and (cond.last_cells == 0).all()
    np.testing.assert_allclose(cond.last_x.cpu().numpy(), plain.last_x.cpu().numpy(), rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(a.swd, b.swd, rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(a.swd_per_cell, [b.swd], rtol=1e-3, atol=1e-5)
    gx = plain.last_gx.cpu().numpy()
    np.testing.assert_allclose(cond.last_gx.cpu().numpy(), gx, rtol=5e-3, atol=5e-3 * np.abs(gx).max())
    assert np.abs(gx).max() > 0
    np.testing.assert_allclose(a.loss, b.loss, rtol=1e-3, atol=1e-5)


def test_the_generators_own_output_as_every_cells_truth_gives_zero():
    """Every cell's truth is the cell's own generated rows, each repeated so that all cells have m rows (m a common multiple of
    the n_c): the quantile coupling pairs every value with copies of itself.  Both powers."""
    for power in (1, 2):
        _own_output_case(power)


def _own_output_case(power):
    learner = _make(power)
    learner.set_dataset(_truth(learner, 6))

    def own_output():
        x, cells = learner.last_x.cpu().numpy(), learner.last_cells
        counts = np.bincount(cells, minlength=learner.num_cells)
        m = int(np.lcm.reduce(counts[counts > 0]))
        y = np.zeros((learner.num_cells, m, x.shape[1]), dtype='float32')
        for c in np.nonzero(counts)[0]:
            y[c] = np.repeat(x[cells == c], m // counts[c], axis=0)
        return torch.as_tensor(y).to('cuda')
    learner.truth_of_step = own_output
    before = learner.get_gen_param()
    learner.dynamics_cost = learner.rate_cost = 0.0
    info = next(learner.learning())
    assert info.swd == 0.0 and (info.swd_per_cell == 0).all() and info.rows_per_cell.sum() == 16
    assert float(learner.last_gx.abs().max()) == 0.0
    for a, b in zip(before, learner.get_gen_param()):            # no loss gradient, no penalty gradient: sgd moves nothing
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-7)


def test_cli_one_step_writes_a_run_directory_the_scorer_reads(tmp_path, monkeypatch):
    import pandas
    from tc_gan_amd.analyzers import distdiff
    from tc_gan_amd.run import bptt_cswd
    monkeypatch.chdir(tmp_path)
    bptt_cswd.main(['--iterations', '1', '--truth_size', '8', '--num-models', '4', '--probes-per-model', '2', '--norm-probes', '0,0.5',
                    '--contrasts', '5,20', '--n_bandwidths', '4', '--seqlen', '40', '--skip-steps', '30', '--swd-directions', '8',
                    '--dataset-provider', 'fixedtime', '--datastore', 'results', '--quiet'])
    out = tmp_path / 'results'
    info = json.load(open(out / 'info.json'))
    assert info['extra_info']['script_file'] == bptt_cswd.__file__
    rc = info['run_config']
    assert rc['norm_probes'] == [0, 0.5] and rc['num_models'] == 4 and rc['probes_per_model'] == 2 and rc['swd_power'] == 2
    assert 'batchsize' not in rc and 'swd_truth_batch' not in rc
    assert json.load(open(out / 'exit.json')) == dict(reason='end_of_iteration', good=True)
    assert np.load(out / 'truth.npy').shape == (8, 2 * 4 * 1 * 2)
    tables = _load_tables(str(out), 'store')
    assert set(tables) == {'learning', 'generator'}
    assert tables['learning'].dtype.names == ('step', 'loss', 'swd', 'dynamics_penalty', 'rate_penalty', 'train_time')
    assert len(tables['learning']) == 1 and np.isfinite(tables['learning']['loss']).all()
    assert np.isfinite(tables['learning']['swd']).all() and (tables['learning']['swd'] >= 0).all()
    distdiff.main([str(out), '--wasserstein', '--draws', '64'])
    table = pandas.read_csv(os.path.join(str(out), 'wdist.csv'))
    sliced = table[table['stat'] == 'sliced_w1']
    assert len(sliced) >= 1 and np.isfinite(sliced['W1'].to_numpy()).all()


def test_several_ranks_are_refused(monkeypatch):
    from tc_gan_amd.networks.conditional_sliced_wasserstein import make_conditional_sliced_wasserstein
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='one GPU'):
        make_conditional_sliced_wasserstein(dict(CSWD_PARAMS))


# ---- a seeded run ------------------------------------------------------------------------------------------------------------

LEARN_STEPS = 100
LEARN_MODELS = 64


def _problem():
    from tc_gan_amd.networks.fixed_time_sampler import new_JDS
    true = {k: np.asarray(new_JDS[k], dtype=float) for k in 'JDS'}
    pert = np.array([[1.3, 0.75], [0.75, 1.3]])
    shared = dict(num_sites=20, seqlen=200, skip_steps=150, include_inhibitory_neurons=False,
                  bandwidths=[0, 0.0625, 0.125, 0.1875, 0.25, 0.5, 0.75, 1], contrasts=[5., 20.],
                  J0=true['J'] * pert, D0=true['D'] * pert, S0=true['S'] * pert, learning_rate=0.01, update_name='adam-wgan',
                  swd_directions=64, swd_power=2)
    return true, shared


def _run_and_score(learner, true, steps):
    """(mean over the four (probe, contrast) cells of the sliced W1 to the truth at the start parameters, at the end parameters):
    per cell the restatement's p = 1 loss of 256 draws on one fixed noise stream against 256 truth rows on 64 fixed directions."""
    from tc_gan_amd.analyzers.distdiff import slice_directions
    from tc_gan_amd.networks.dataset import dataset_by_fixedtime
    from tc_gan_amd.networks.fixed_time_sampler import FixedTimeTuningCurveSampler
    from tc_gan_amd.networks.utils import gridify_tc_samples
    truth = dataset_by_fixedtime(learner, truth_size=512, truth_seed=42, true_ssn_options={k: true[k] for k in 'JDS'})
    assert truth.shape == (512, 2 * 8 * 1 * 2)
    learner.set_dataset(truth)
    theta = slice_directions(64, 8, 11)

    def grid(rows):
        return gridify_tc_samples(np.asarray(rows), num_contrasts=2, num_bandwidths=8, num_cell_types=1, num_probes=2)[:, 0]

    def w1():
        jds = dict(zip('JDS', learner.get_gen_param()))
        x = FixedTimeTuningCurveSampler.from_learner(learner, batchsize=256, seed=7, **jds).forward().prober_tuning_curve
        gx, gy = grid(x.cpu().numpy()), grid(truth[:256])          # (256, probes, contrasts, bandwidths)
        return float(np.mean([sc.swd(gx[:, p, k].astype('float32'), gy[:, p, k].astype('float32'), theta, 1)['loss']
                              for p in range(2) for k in range(2)]))
    start = w1()
    updates = learner.learning()
    losses = [next(updates).swd for _ in range(steps)]
    assert np.isfinite(losses).all()
    return start, w1()


def test_seeded_conditional_run_ends_no_farther_from_the_truth_than_the_unconditional_one():
    """2N = 40, E only, two probes (both per model), two contrasts, 8 bandwidths, start perturbed by +30 % / -25 %, 100 steps.  The
    conditional run draws 64 models a step, each at one contrast: 512 stimulus solves.  The yardstick is the unconditional
    trainer on the same problem at batchsize 32 -- every draw at both contrasts: 512 solves -- which must itself meet the ratio
    bound of tests/test_swd_train_gpu.py; the conditional run must end no higher than twice the yardstick's end value, the margin
    tests/test_swd_sizes_gpu.py gives its second run: after 100 steps both sit at the sampling noise of their generated rows.
    Measured on MI355X: see DESIGN 3.11f."""
    from tc_gan_amd.networks.conditional_sliced_wasserstein import make_conditional_sliced_wasserstein
    from tc_gan_amd.networks.sliced_wasserstein import make_sliced_wasserstein
    true, shared = _problem()
    plain, rest = make_sliced_wasserstein(dict(shared, batchsize=32, sample_sites=[0, 0.5]))
    assert rest == {}
    start0, end0 = _run_and_score(plain, true, LEARN_STEPS)
    cond, rest = make_conditional_sliced_wasserstein(dict(shared, num_models=LEARN_MODELS, probes_per_model=2, norm_probes=[0, 0.5]))
    assert rest == {}
    start, end = _run_and_score(cond, true, LEARN_STEPS)
    print('mean sliced W1 of the four cells to the truth: start', start0, start, 'end unconditional:', end0, 'conditional:', end)
    np.testing.assert_allclose(start, start0, rtol=1e-6)          # (the same generator call at the same parameters)
    assert np.isfinite(end0) and end0 <= LEARN_RATIO * start0
    assert np.isfinite(end) and end <= 2 * end0

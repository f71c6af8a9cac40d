"""Scoring a run's checkpoints on the GPU (tc_gan_amd/analyzers/distdiff.py, csrc/ssn_score.hip): the W table against
ssn_build_w_f32, the KS kernel against the integer form restated in tests/test_distdiff.py (every (set, column), exactly), the
feature kernel against float64 numpy, the batched scorer against a loop over samplers, and the whole wiring on short runs of the
three trainers, where scoring the truth's own parameters on the truth's own noise must give distance zero."""
import json
import os

import numpy as np
import pytest
import torch

from tc_gan_amd import clib
from tc_gan_amd.analyzers import distdiff
from tc_gan_amd.clib import libssnode
from tc_gan_amd.networks.fixed_time_sampler import FixedTimeTuningCurveSampler, new_JDS
from test_distdiff import ks_numerators

pytestmark = pytest.mark.gpu


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype).contiguous()


def _thetas(count, seed, ssn_type='default', first=None):
    rs = np.random.RandomState(seed)
    out = []
    for i in range(count):
        th = {k: new_JDS[k] * (1 + 0.2 * (rs.rand(2, 2) - 0.5)) for k in 'JDS'}
        if ssn_type == 'heteroin':
            th['V'] = np.array([0.3, 0.1]) * (1 + 0.5 * (rs.rand(2) - 0.5))
        elif ssn_type == 'deg-heteroin':
            th['V'] = 0.5 * (1 + 0.5 * (rs.rand() - 0.5))
        out.append(th)
    if first is not None:
        out[2] = first
    return out


# ---- 5. W for a table of parameter sets ---------------------------------------------------------------------------------

@pytest.mark.parametrize('N', [10, 51, 101])
@pytest.mark.parametrize('B', [1, 7, 64])
def test_w_table_equals_build_w_per_set(N, B):
    from tc_gan_amd.weight_gen import generate_weight_batch
    S, M = 5, 2 * N
    thetas = _thetas(S, 100 + N + B)
    z = _dev(np.random.RandomState(N * 1000 + B).rand(B, M, M))
    table, _ = distdiff._theta_tables(thetas, 'default')
    W = torch.full((S, B, M, M), float('nan'), device='cuda')
    clib.check(libssnode.ssn_build_w_table_f32(z.data_ptr(), _dev(table).data_ptr(), W.data_ptr(), S, B, N, clib.stream_ptr()),
               'ssn_build_w_table_f32')
    for s, th in enumerate(thetas):
        want = generate_weight_batch(N, th['J'], th['D'], th['S'], z)
        np.testing.assert_array_equal(W[s].cpu().numpy(), want.cpu().numpy())


# ---- 6. the KS kernel ---------------------------------------------------------------------------------------------------

def _ks_device(x, t):
    """x (S, B, C), t (T, C) float32 numpy -> (num, n) (S, C) of ssn_ks_columns_f32 and m (C,)."""
    S, B, C = x.shape
    T = t.shape[0]
    finite = np.isfinite(t)
    srt = np.sort(np.where(finite, t, np.inf).astype('float32'), axis=0)
    m = finite.sum(axis=0).astype('int32')
    n = torch.full((S, C), -7, device='cuda', dtype=torch.int32)
    num = torch.full((S, C), -7, device='cuda', dtype=torch.int64)
    xd, td, md = _dev(x), _dev(srt.T), _dev(m, torch.int32)
    clib.check(libssnode.ssn_ks_columns_f32(xd.data_ptr(), td.data_ptr(), md.data_ptr(), S, B, C, T, n.data_ptr(), num.data_ptr(),
                                            clib.stream_ptr()), 'ssn_ks_columns_f32')
    return num.cpu().numpy(), n.cpu().numpy(), m.astype('int64')


def _ks_columns(rs, rows, C):
    """(rows, C) float32 with, by column mod 8: continuous values, one value everywhere, rectified values (many exact zeros),
    small integers, continuous with an Inf, no finite value at all, rectified with a -Inf, continuous."""
    x = rs.randn(rows, C)
    for c in range(C):
        k = c % 8
        if k == 1:
            x[:, c] = 1.25
        elif k == 2:
            x[:, c] = np.maximum(x[:, c], 0)
        elif k == 3:
            x[:, c] = rs.randint(0, 8, rows)
        elif k == 4:
            x[rs.randint(rows), c] = np.inf
        elif k == 5:
            x[:, c] = np.nan
        elif k == 6:
            x[:, c] = np.maximum(x[:, c], 0)
            x[rs.randint(rows), c] = -np.inf
    return x.astype('float32')


@pytest.mark.parametrize('T', [1, 32, 2048, 5000])
@pytest.mark.parametrize('B', [1, 2, 30, 128, 1000, 4096, 16384])
def test_ks_kernel_equals_the_integer_form(B, T):
    rs = np.random.RandomState(B * 7 + T)
    C = 16
    S = 80 if B <= 128 else (10 if B <= 4096 else 3)      # 1280 workgroups at the small sizes: several per compute unit
    x = _ks_columns(rs, S * B, C).reshape(S, B, C)
    if B > 1:
        x[:, B // 2, :] = np.nan                         # a NaN row in every set
    t = _ks_columns(rs, T, C)
    t[:, 5] = rs.randn(T)                                # (the truth keeps one column with missing values, none without any)
    t[0, 7] = np.nan
    num, n, m = _ks_device(x, t)
    for s in range(S):
        want_num, want_n, want_m = ks_numerators(x[s], t)
        np.testing.assert_array_equal(m, want_m)
        np.testing.assert_array_equal(n[s], want_n, err_msg='set {}'.format(s))
        np.testing.assert_array_equal(num[s], want_num, err_msg='set {}'.format(s))
    assert (n[:, 5] == 0).all() and (num[:, 5] == 0).all()


def test_ks_kernel_refuses_more_than_16384_values():
    x = torch.zeros(8, device='cuda')
    rc = libssnode.ssn_ks_columns_f32(x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 16385, 1, 1, x.data_ptr(), x.data_ptr(),
                                      clib.stream_ptr())
    assert rc != 0 and '16384' in clib.last_error()


# ---- 7. the feature kernel ----------------------------------------------------------------------------------------------

def test_features_against_float64_numpy_and_their_ks():
    rs = np.random.RandomState(11)
    NC, NB, CT, P = 2, 8, 2, 3
    Q, S, B = CT * P, 6, 500
    R, curves = S * B, NC * CT * P
    tc = (np.maximum(rs.randn(R, NC * NB * Q), 0) * rs.choice([0.0, 1e-3, 1.0, 50.0], size=(R, 1))).astype('float32')
    tc[::17] = 0                                          # whole rows of zeros: si and ipr are 0 / 0 there
    tcd = _dev(tc)
    feat = distdiff._features(tcd, NC, NB, Q).cpu().numpy()
    assert feat.shape == (R, 4 * curves)
    grid = tc.astype('float64').reshape(R, NC, NB, Q)                      # column (c NB + b) Q + q
    with np.errstate(invalid='ignore', divide='ignore'):
        maxrate = grid.max(axis=2)
        si = 1 - grid[:, :, NB - 1] / maxrate
        prefbw = grid.argmax(axis=2).astype('float64')
        ipr = grid.sum(axis=2) ** 2 / (NB * (grid ** 2).sum(axis=2))
    got = feat.reshape(R, 4, NC, Q)
    np.testing.assert_array_equal(got[:, 0], maxrate)
    np.testing.assert_array_equal(got[:, 2], prefbw)
    for name, g, w, tol, relative in (('si', got[:, 1], si, 2.0 ** -22, False), ('ipr', got[:, 3], ipr, (NB + 4) * 2.0 ** -23, True)):
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=name)
        ok = ~np.isnan(w)
        err = np.abs(g[ok].astype('float64') - w[ok]) / (np.abs(w[ok]) if relative else 1.0)
        print('{}: largest {} error {:.3g} = {:.3g} of the bound'.format(name, 'relative' if relative else 'absolute', err.max(),
                                                                        err.max() / tol))
        assert err.max() <= tol, name
    assert np.isnan(si).any() and (prefbw > 0).any()
    # the KS of the features, exactly, from the features the GPU returned
    truth = feat[rs.choice(R, 300, replace=False)]
    x = feat.reshape(S, B, 4 * curves)
    num, n, m = _ks_device(x, truth)
    for s in range(S):
        want_num, want_n, want_m = ks_numerators(x[s], truth)
        np.testing.assert_array_equal(num[s], want_num)
        np.testing.assert_array_equal(n[s], want_n)
        np.testing.assert_array_equal(m, want_m)


# ---- 8. batched equals looped -------------------------------------------------------------------------------------------

CFG = dict(num_sites=20, bandwidths=[0, 0.0625, 0.125, 0.1875, 0.25, 0.5, 0.75, 1], contrasts=[20.0], seqlen=40, skip_steps=30,
           norm_probes=[0, 0.5], include_inhibitory_neurons=True)


def _looped(cfg, thetas, truth, draws, seed):
    """One sampler per parameter set, the same model_zs / model_zs_in for all, curves read back, KS on the host."""
    M = 2 * cfg['num_sites']
    rng = np.random.RandomState(seed)
    zs = rng.rand(draws, M, M)
    zs_in = None
    if cfg.get('ssn_type', 'default') != 'default':
        zs_in = rng.choice(2, (draws, M)) * 2 - 1 if cfg.get('dist_in', 'bernoulli') == 'bernoulli' else rng.rand(draws, M) * 2 - 1
    curves, nums, ns = [], [], []
    for th in thetas:
        sampler = FixedTimeTuningCurveSampler.from_dict(dict(cfg, batchsize=draws, **th))
        kw = dict(model_zs_in=zs_in) if zs_in is not None else {}
        out = sampler.gen.forward(stimulator_bandwidths=sampler.stimulator_bandwidths,
                                  stimulator_contrasts=sampler.stimulator_contrasts, model_zs=zs, **kw)
        tc = out.prober_tuning_curve.cpu().numpy()
        curves.append(tc)
        num, n, m = ks_numerators(tc, truth)
        nums.append(num)
        ns.append(n)
    return np.stack(curves), np.stack(nums), np.stack(ns), m


@pytest.mark.parametrize('kernel,ssn_type,draws,budget', [
    ('tile', 'default', 7, 30), ('mfma-fp32', 'default', 7, 30), ('duo', 'default', 3, 15),
    ('tile', 'heteroin', 7, 30), ('tile', 'deg-heteroin', 7, 30)])
def test_batched_scoring_equals_a_loop_over_samplers(kernel, ssn_type, draws, budget):
    cfg = dict(CFG, gen_kernel=kernel, ssn_type=ssn_type)
    truth_theta = dict(new_JDS, **({'V': [0.3, 0.0]} if ssn_type == 'heteroin' else {'V': 0.5} if ssn_type == 'deg-heteroin' else {}))
    thetas = _thetas(6, 5, ssn_type, first=truth_theta)
    truth = FixedTimeTuningCurveSampler.from_dict(dict(cfg, batchsize=32, seed=42, **truth_theta)).sample()
    C = truth.shape[1]
    assert C == 8 * 2 * 2
    res = distdiff.score_parameter_sets(cfg, thetas, truth, draws=draws, seed=3, max_draws_per_launch=budget, return_samples=True)
    chunk = budget // draws
    assert res['gen_kernel'] == kernel and res['chunk'] == chunk and res['chunks'] == [chunk, 6 - chunk] and chunk not in (3, 6)
    if kernel == 'duo':
        assert all((c * draws) % 2 == 1 for c in res['chunks'])              # odd draw counts in both launches
    curves, num, n, m = _looped(cfg, thetas, truth, draws, 3)
    np.testing.assert_array_equal(res['tuning_curves'], curves)
    assert np.isfinite(curves).all() and curves.max() > 0
    np.testing.assert_array_equal(res['num'][:, :C], num)
    np.testing.assert_array_equal(res['n'][:, :C], n)
    np.testing.assert_array_equal(res['m'][:C], m)
    # features: KS recomputed on the host from the features the GPU returned, against the truth's features from the same kernel
    tfeat = distdiff._features(_dev(truth), 1, 8, 4).cpu().numpy()
    for s in range(6):
        want_num, want_n, want_m = ks_numerators(res['features'][s], tfeat)
        np.testing.assert_array_equal(res['num'][s, C:], want_num)
        np.testing.assert_array_equal(res['n'][s, C:], want_n)
        np.testing.assert_array_equal(res['m'][C:], want_m)
    assert len(res['stat']) == C + 4 * 4 and (res['KSD'] >= 0).all() and (res['KSD'] <= 1).all()


def test_duo_fused_runs_as_duo_and_says_so():
    cfg = dict(CFG, gen_kernel='duo-fused')
    truth = np.ones((4, 32), dtype='float32')
    res = distdiff.score_parameter_sets(cfg, _thetas(2, 9), truth, draws=3)
    assert res['gen_kernel'] == 'duo' and 'duo-fused' in res['note']


# ---- 9. a known answer for the whole wiring; 10. the command line ---------------------------------------------------------

RUN = ['--n_bandwidths', '8', '--seqlen', '40', '--skip-steps', '30', '--iterations', '4', '--quiet', '--truth_size', '32',
       '--dataset-provider', 'fixedtime', '--gen-kernel', 'tile']
GAN = ['--WGAN_n_critic0', '2', '--WGAN_n_critic', '1', '--disc-layers', '[8]']
TRUE_JDS = {k: (new_JDS[k] * 1.05).tolist() for k in 'JDS'}


def _run(tmp, module, args, config):
    d = tmp / 'run'
    cfg = tmp / 'config.json'
    cfg.write_text(json.dumps(dict(num_sites=20, **config)))
    module.main(RUN + args + ['--datastore', str(d), '--load-config', str(cfg)])
    assert json.load(open(str(d / 'exit.json')))['good']
    return str(d)


def _check_known_answer(rundir, columns, curves):
    info = json.load(open(os.path.join(rundir, 'info.json')))['run_config']
    opts = info['true_ssn_options']
    truth_theta = {k: opts[k] for k in ('J', 'D', 'S', 'V') if k in opts}
    res = distdiff.calc_distdiff(rundir, draws=info['truth_size'], seed=info['truth_seed'], extra_thetas=[truth_theta],
                                 max_draws_per_launch=96)
    S = 1 + 4
    assert res['gen_kernel'] == 'tile' and res['chunk'] == 3 and res['chunks'] == [3, 2]
    assert res['num'].shape == (S, columns + 4 * curves) and list(res['gen_step']) == [-1, 0, 1, 2, 3]
    np.testing.assert_array_equal(res['num'][0], 0)      # the truth's parameters on the truth's noise: the truth's curves
    assert (res['n'] == 32).all() and (res['m'] == 32).all()
    assert (res['KSD'] >= 0).all() and (res['KSD'] <= 1).all() and (res['KSD'][0] == 0).all()
    assert (res['KSD'][1:, :columns] > 0).any()          # J0 = D0 = S0 = 0.01 is not the truth
    return res


@pytest.fixture(scope='module')
def wgan_run(tmp_path_factory):
    from tc_gan_amd.run import bptt_wgan
    return _run(tmp_path_factory.mktemp('wgan'), bptt_wgan, GAN + ['--batchsize', '4', '--sample-sites', '0,0.5'],
                dict(true_ssn_options=TRUE_JDS))


def test_truth_parameters_score_zero_on_a_wgan_run(wgan_run):
    _check_known_answer(wgan_run, 8 * 2, 2)


def test_truth_parameters_score_zero_on_a_deg_heteroin_wgan_run(tmp_path):
    from tc_gan_amd.run import bptt_wgan
    d = _run(tmp_path, bptt_wgan, GAN + ['--batchsize', '4', '--sample-sites', '0,0.5', '--ssn-type', 'deg-heteroin',
                                         '--include-inhibitory-neurons'], dict(true_ssn_options=dict(TRUE_JDS, V=0.4)))
    _check_known_answer(d, 8 * 2 * 2, 4)


def test_truth_parameters_score_zero_on_a_cwgan_run(tmp_path):
    from tc_gan_amd.run import bptt_cwgan
    d = _run(tmp_path, bptt_cwgan, GAN + ['--num-models', '4', '--probes-per-model', '2', '--norm-probes', '0,0.5',
                                          '--contrasts', '5,20', '--include-inhibitory-neurons'], dict(true_ssn_options=TRUE_JDS))
    _check_known_answer(d, 2 * 8 * 2 * 2, 2 * 2 * 2)


def test_truth_parameters_score_zero_on_a_moments_run(tmp_path):
    from tc_gan_amd.run import bptt_moments
    d = _run(tmp_path, bptt_moments, ['--batchsize', '4', '--sample-sites', '0,0.5', '--gen-moments-record-interval', '1'],
             dict(true_ssn_options=TRUE_JDS))
    _check_known_answer(d, 8 * 2, 2)


def test_command_line_writes_the_tables(wgan_run, tmp_path):
    import pandas
    out = tmp_path / 'scores'
    res = distdiff.main([wgan_run, '--steps', '::2', '--draws', '8', '--max-draws-per-launch', '8', '--output', str(out),
                         '--save-tuning-curves'])
    C, curves = 16, 2
    table = pandas.read_csv(str(out / 'distdiff.csv'), float_precision='round_trip')
    assert len(table) == 2 * (C + 4 * curves) and list(table.columns) == ['gen_step', 'stat', 'KSD', 'n', 'm']
    again = distdiff.calc_distdiff(wgan_run, steps=slice(None, None, 2), draws=8, max_draws_per_launch=8)
    assert list(again['gen_step']) == [0, 2] and again['chunks'] == [1, 1]
    np.testing.assert_array_equal(table['gen_step'].to_numpy(), np.repeat(again['gen_step'], C + 4 * curves))
    assert list(table['stat']) == again['stat'] * 2
    np.testing.assert_array_equal(table['KSD'].to_numpy(), again['KSD'].reshape(-1))
    np.testing.assert_array_equal(table['n'].to_numpy(), again['n'].reshape(-1))
    np.testing.assert_array_equal(table['m'].to_numpy(), np.tile(again['m'], 2))
    np.testing.assert_array_equal(res['num'], again['num'])
    meta = json.load(open(str(out / 'distdiff.json')))
    assert meta['gen_kernel'] == 'tile' and meta['chunk'] == 1 and meta['gen_steps'] == [0, 2]
    assert meta['bandwidths'] == [0, 0.0625, 0.125, 0.1875, 0.25, 0.5, 0.75, 1] and meta['contrasts'] == [20.0] and len(meta['probes']) == 2
    assert sorted(os.listdir(str(out / 'tuning_curves'))) == ['0000000000.csv', '0000000001.csv']
    curves0 = np.loadtxt(str(out / 'tuning_curves' / '0000000000.csv'), delimiter=',')
    assert curves0.shape == (8, C)
    np.testing.assert_array_equal(curves0.astype('float32'), res['tuning_curves'][0])
    np.testing.assert_array_equal(np.loadtxt(str(out / 'bandwidths.csv'), delimiter=','), meta['bandwidths'])
    np.testing.assert_array_equal(np.loadtxt(str(out / 'sample_epochs.csv'), delimiter=','), [0, 2])

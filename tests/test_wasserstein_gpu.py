"""The Wasserstein distances of the scorer on the GPU (csrc/ssn_wdist.hip, tc_gan_amd/analyzers/distdiff.py with wasserstein=True):
the KS + W1 kernel against the exact restatement of tests/wasserstein_cases.py (equal on a lattice, within the derived bound on
generic values, the integers equal to ssn_ks_columns_f32's), the projection against the sequential fp64 sum bit for bit, the scorer
in both dynamics against the restatement applied to the samples it returns, and the wiring on short runs.

The shapes are the smallest that cover the paths: B = 1 (padded to 64), 64 (no padding), 65 (P = 128), 257 and 300 (more than one
sort element and more than one pooled point per thread), T = 1, 7, 50 (n + m below and above 256), three sets, five columns."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from tc_gan_amd import clib
from tc_gan_amd.analyzers import distdiff
from tc_gan_amd.clib import libssnode
from tc_gan_amd.networks.fixed_time_sampler import FixedTimeTuningCurveSampler, new_JDS
from test_distdiff import CFG as SMALL_CFG
from test_distdiff_gpu import GAN, TRUE_JDS, _ks_device, _run, _thetas
from wasserstein_cases import lattice, project_rows, w1_columns, w1_exact, wnum_bound, wnum_in_kernel_order

pytestmark = pytest.mark.gpu

SHAPES = [(B, T) for B in (1, 64, 65, 257, 300) for T in (1, 7, 50)]


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype).contiguous()


def _w1_device(x, t):
    """x (S, B, C), t (T, C) float32 numpy -> (num, n, wnum) (S, C) of ssn_ks_w1_columns_f32 and m (C,)."""
    S, B, C = x.shape
    T = t.shape[0]
    finite = np.isfinite(t)
    srt = np.sort(np.where(finite, t, np.inf).astype('float32'), axis=0)
    m = finite.sum(axis=0).astype('int32')
    n = torch.full((S, C), -7, device='cuda', dtype=torch.int32)
    num = torch.full((S, C), -7, device='cuda', dtype=torch.int64)
    wnum = torch.full((S, C), float('nan'), device='cuda', dtype=torch.float64)
    xd, td, md = _dev(x), _dev(srt.T), _dev(m, torch.int32)
    clib.check(libssnode.ssn_ks_w1_columns_f32(xd.data_ptr(), td.data_ptr(), md.data_ptr(), S, B, C, T, n.data_ptr(), num.data_ptr(),
                                               wnum.data_ptr(), clib.stream_ptr()), 'ssn_ks_w1_columns_f32')
    return num.cpu().numpy(), n.cpu().numpy(), wnum.cpu().numpy(), m.astype('int64')


def _plant(x, t):
    """The special columns: 1 of set 0 all NaN; 2 of set 1 with NaN, +inf and -inf mixed in (where there is room); the truth's
    column 3 without a finite value; 4 of set 2 the truth's column itself where B is a multiple of T.  Returns whether the last
    one could be planted."""
    S, B, C = x.shape
    T = t.shape[0]
    x[0, :, 1] = np.nan
    if B >= 4:
        x[1, [0, B // 2, B - 1], 2] = [np.nan, np.inf, -np.inf]
    else:
        x[1, 0, 2] = np.inf
    t[:, 3] = np.nan
    if B % T == 0:
        x[2, :, 4] = np.tile(t[:, 4], B // T)
    return B % T == 0


# ---- 1. the KS + W1 kernel -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('B,T', SHAPES)
def test_w1_kernel_is_exact_on_a_lattice(B, T):
    rs = np.random.RandomState(B * 100 + T)
    S, C = 3, 5
    x, t = lattice(rs, (S, B, C)), lattice(rs, (T, C))
    same = _plant(x, t)
    num, n, wnum, m = _w1_device(x, t)
    ks_num, ks_n, ks_m = _ks_device(x, t)
    np.testing.assert_array_equal(num, ks_num)
    np.testing.assert_array_equal(n, ks_n)
    np.testing.assert_array_equal(m, ks_m)
    for s in range(S):
        want, want_n, want_m = w1_columns(x[s], t)
        np.testing.assert_array_equal(n[s], want_n)
        np.testing.assert_array_equal(m, want_m)
        assert all(Fraction(float(w)) == w for w in want)                          # the lattice: representable
        np.testing.assert_array_equal(wnum[s], [float(w) for w in want], err_msg='set {}'.format(s))
    assert n[0, 1] == 0 and wnum[0, 1] == 0 and num[0, 1] == 0                     # all NaN
    assert n[1, 2] == (B - 3 if B >= 4 else 0)                                     # non-finite values left out
    assert m[3] == 0 and (wnum[:, 3] == 0).all() and (n[:, 3] == B).all()          # a truth column without a value
    if same:
        assert wnum[2, 4] == 0 and num[2, 4] == 0 and n[2, 4] == B                 # the truth's own distribution
    assert (wnum[:, 0] > 0).any()


@pytest.mark.parametrize('B,T', SHAPES)
def test_w1_kernel_holds_the_derived_bound_on_generic_values(B, T):
    rs = np.random.RandomState(B * 100 + T + 1)
    S, C = 3, 5
    x, t = (rs.rand(S, B, C) * 40).astype('float32'), (rs.rand(T, C) * 40).astype('float32')
    _plant(x, t)
    num, n, wnum, m = _w1_device(x, t)
    again = _w1_device(x, t)
    np.testing.assert_array_equal(wnum.view(np.uint64), again[2].view(np.uint64))  # the same bits every launch
    np.testing.assert_array_equal(num, again[0])
    ks_num, ks_n, _ = _ks_device(x, t)
    np.testing.assert_array_equal(num, ks_num)
    np.testing.assert_array_equal(n, ks_n)
    worst = Fraction(0)
    for s in range(S):
        want, want_n, want_m = w1_columns(x[s], t)
        np.testing.assert_array_equal(n[s], want_n)
        for c in range(C):
            err, bound = abs(Fraction(float(wnum[s, c])) - want[c]), wnum_bound(want[c], want_n[c], want_m[c])
            if bound:
                worst = max(worst, err / bound)
            assert err <= bound, (s, c, float(err), float(bound))
    print('largest error of wnum: {:.3g} of the bound'.format(float(worst)))
    # the order of the additions: wnum is the restatement of the thread, wave and block sums bit for bit
    ordered = np.array([[wnum_in_kernel_order(x[s, :, c], t[:, c]) for c in range(C)] for s in range(S)])
    np.testing.assert_array_equal(wnum.view(np.uint64), ordered.view(np.uint64))


def test_w1_kernel_refuses_more_than_16384_values():
    x = torch.zeros(8, device='cuda')
    out = torch.full((4,), -7, device='cuda', dtype=torch.int64)
    rc = libssnode.ssn_ks_w1_columns_f32(x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 16385, 1, 1, out.data_ptr(), out.data_ptr(),
                                         out.data_ptr(), clib.stream_ptr())
    assert rc != 0 and '16384' in clib.last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7).all()                                         # refused before any launch


# ---- 2. the projection -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('rows,C,L,ldx', [(7, 6, 5, 6), (7, 6, 5, 9), (300, 80, 128, 100)])
def test_projection_is_the_sequential_fp64_sum(rows, C, L, ldx):
    rs = np.random.RandomState(rows + ldx)
    x = np.full((rows, ldx), np.nan, dtype='float32')                              # (the padding of a row is never read)
    x[:, :C] = rs.randn(rows, C) * 30
    x[2, C // 2], x[5, C - 1] = np.nan, np.inf
    theta = distdiff.slice_directions(L, C, 4)
    out = distdiff.project_rows(_dev(x), _dev(theta), C).cpu().numpy()
    assert out.shape == (rows, L) and out.dtype == np.float32
    want = project_rows(x[:, :C], theta)
    finite = np.ones(rows, dtype=bool)
    finite[[2, 5]] = False
    assert np.isfinite(want[finite]).all() and (want[finite] != 0).all()
    np.testing.assert_array_equal(out[finite].view(np.uint32), want[finite].view(np.uint32))
    assert not np.isfinite(out[~finite]).any()


# ---- 3. the scorer ---------------------------------------------------------------------------------------------------------

def _check_result(res, off, truth32, tfeat, S, draws, C, L, direction_seed):
    """A wasserstein=True result against the result without the switch and against the restatement on the returned samples."""
    for key in ('num', 'n', 'm', 'KSD', 'tuning_curves', 'features'):
        np.testing.assert_array_equal(res[key], off[key], err_msg=key)
    assert not {'wnum', 'W1', 'SW1', 'sliced', 'projections'} & set(off)
    assert sorted(set(res) - set(off)) == ['SW1', 'W1', 'projections', 'sliced', 'wnum']
    Ct = C + tfeat.shape[1]
    assert res['wnum'].shape == (S, Ct) and res['wnum'].dtype == np.float64 and res['W1'].shape == (S, Ct)
    assert res['SW1'].shape == (S,) and res['projections'].shape == (S, draws, L)
    theta = distdiff.slice_directions(L, C, direction_seed)
    tproj = project_rows(truth32, theta)
    np.testing.assert_array_equal(distdiff.project_rows(_dev(truth32), _dev(theta)).cpu().numpy(), tproj)
    sl = res['sliced']
    assert sl['directions'] == L and sl['seed'] == direction_seed and sl['m'] == len(truth32) and sl['n'].shape == (S,)
    for s in range(S):
        samples = np.concatenate([res['tuning_curves'][s], res['features'][s]], axis=1)
        want, want_n, want_m = w1_columns(samples, np.concatenate([truth32, tfeat], axis=1))
        np.testing.assert_array_equal(res['n'][s], want_n)
        for c in range(Ct):
            assert abs(Fraction(float(res['wnum'][s, c])) - want[c]) <= wnum_bound(want[c], want_n[c], want_m[c]), (s, c)
            den = int(want_n[c] * want_m[c])
            if den:
                assert res['W1'][s, c] == res['wnum'][s, c] / den
            else:
                assert np.isnan(res['W1'][s, c])
        # the projections are the kernel's own arithmetic on the returned curves; a row that is not finite has none
        rows_ok = np.isfinite(res['tuning_curves'][s]).all(axis=1)
        np.testing.assert_array_equal(res['projections'][s][rows_ok], project_rows(res['tuning_curves'][s][rows_ok], theta))
        assert not np.isfinite(res['projections'][s][~rows_ok]).any() and sl['n'][s] == rows_ok.sum()
        # SW1: the mean of L distances, each within the bound of wnum and one division, summed with at most L more roundings
        pw, pn, pm = w1_columns(res['projections'][s], tproj)
        assert (pn == sl['n'][s]).all() and (pm == sl['m']).all()
        if sl['n'][s]:
            exact = sum(w / int(a * b) for w, a, b in zip(pw, pn, pm)) / L
            bound = (int(sl['n'][s]) + sl['m'] + 2 + L + 2) * Fraction(1, 2 ** 52) * exact
            assert abs(Fraction(float(res['SW1'][s])) - exact) <= bound, s
        else:
            assert np.isnan(res['SW1'][s])


def test_fixed_time_scores_with_wasserstein():
    cfg = dict(SMALL_CFG)                                                          # num_sites 10, 4 bandwidths, 'tile'
    thetas = _thetas(6, 5, first=new_JDS)
    truth = FixedTimeTuningCurveSampler.from_dict(dict(cfg, batchsize=16, seed=42, **new_JDS)).sample()
    C, S, draws, L = truth.shape[1], 6, 7, 9
    assert C == 4 * 2 * 2
    kw = dict(draws=draws, seed=3, max_draws_per_launch=30, return_samples=True)
    off = distdiff.score_parameter_sets(cfg, thetas, truth, **kw)
    res = distdiff.score_parameter_sets(cfg, thetas, truth, wasserstein=True, directions=L, direction_seed=2, **kw)
    assert res['chunks'] == [4, 2]                                                 # chunks of unequal size
    truth32 = np.ascontiguousarray(truth, dtype='float32')
    tfeat = distdiff._features(_dev(truth32), 1, 4, 4).cpu().numpy()
    _check_result(res, off, truth32, tfeat, S, draws, C, L, 2)
    assert (res['wnum'][:, :C] > 0).any() and (res['SW1'] > 0).all()
    for budget in (7, 4096):                                                       # one checkpoint per launch; all in one
        other = distdiff.score_parameter_sets(cfg, thetas, truth, wasserstein=True, directions=L, direction_seed=2,
                                              **dict(kw, max_draws_per_launch=budget))
        assert other['chunks'] != res['chunks']
        for key in ('num', 'n', 'wnum', 'W1', 'SW1', 'projections'):
            np.testing.assert_array_equal(other[key], res[key], err_msg='{} with max_draws_per_launch={}'.format(key, budget))
    # the default number of directions, and the seed matters
    dflt = distdiff.score_parameter_sets(cfg, thetas[:2], truth, wasserstein=True, draws=draws, seed=3)
    assert dflt['sliced']['directions'] == 128 and dflt['sliced']['seed'] == 0 and 'projections' not in dflt
    np.testing.assert_array_equal(dflt['wnum'], res['wnum'][:2])


def test_fixed_point_scores_with_wasserstein():
    import test_fixedpoint_score_gpu as fp
    from tc_gan_amd.networks.dataset import dataset_by_ssnode
    truth = dataset_by_ssnode(num_sites=fp.N, bandwidths=fp.BANDWIDTHS, contrasts=fp.CONTRAST, truth_size=fp.NZ, truth_seed=0,
                              sample_sites=fp.SITES, include_inhibitory_neurons=True,
                              true_ssn_options=dict(fp.THETAS[3], smoothness=fp.SMOOTHNESS, max_iter=fp.POWER['max_iter']))
    S, draws, C, L = 5, fp.NZ, 16, 6
    kw = dict(draws=draws, seed=0, return_samples=True, **fp.FP)
    off = distdiff.score_parameter_sets(fp.CFG, fp.THETAS, truth, **kw)
    res = distdiff.score_parameter_sets(fp.CFG, fp.THETAS, truth, wasserstein=True, directions=L, direction_seed=1, **kw)
    for key in ('accepted', 'used', 'rejections'):
        np.testing.assert_array_equal(res[key], off[key])
    truth32 = np.ascontiguousarray(truth, dtype='float32')
    tfeat = distdiff._features(_dev(truth32), 1, 4, 4).cpu().numpy()
    _check_result(res, off, truth32, tfeat, S, draws, C, L, 1)
    assert (res['accepted'] < draws).any()                                         # sets that come up short: rows of NaN
    np.testing.assert_array_equal(res['sliced']['n'], res['accepted'])
    # the truth's own parameters, seed and size: distance zero in every column and every direction
    assert (res['wnum'][3] == 0).all() and res['SW1'][3] == 0 and (res['wnum'][[0, 1, 2, 4], :C] > 0).any()
    other = distdiff.score_parameter_sets(fp.CFG, fp.THETAS, truth, wasserstein=True, directions=L, direction_seed=1,
                                          max_draws_per_launch=40, **kw)
    for key in ('num', 'n', 'wnum', 'SW1', 'projections'):
        np.testing.assert_array_equal(other[key], res[key], err_msg=key)


# ---- 4. a known answer for the whole wiring; the command line --------------------------------------------------------------

def test_truth_parameters_have_distance_zero_on_a_deg_heteroin_wgan_run(tmp_path):
    from tc_gan_amd.run import bptt_wgan
    rundir = _run(tmp_path, bptt_wgan, GAN + ['--batchsize', '4', '--sample-sites', '0,0.5', '--ssn-type', 'deg-heteroin',
                                              '--include-inhibitory-neurons'], dict(true_ssn_options=dict(TRUE_JDS, V=0.4)))
    info = json.load(open(os.path.join(rundir, 'info.json')))['run_config']
    opts = info['true_ssn_options']
    truth_theta = {k: opts[k] for k in ('J', 'D', 'S', 'V') if k in opts}
    res = distdiff.calc_distdiff(rundir, draws=info['truth_size'], seed=info['truth_seed'], extra_thetas=[truth_theta],
                                 max_draws_per_launch=96, wasserstein=True, directions=16)
    C = 8 * 2 * 2
    assert res['wnum'].shape == (5, C + 4 * 4) and list(res['gen_step']) == [-1, 0, 1, 2, 3] and res['chunks'] == [3, 2]
    np.testing.assert_array_equal(res['num'][0], 0)
    np.testing.assert_array_equal(res['wnum'][0], 0)      # the truth's parameters on the truth's noise: the truth's curves
    assert res['SW1'][0] == 0 and (res['W1'][0] == 0).all()
    assert (res['SW1'][1:] > 0).all() and (res['W1'][1:, :C] > 0).any()            # J0 = D0 = S0 = 0.01 is not the truth
    assert (res['sliced']['n'] == 32).all() and res['sliced']['m'] == 32


@pytest.fixture(scope='module')
def tiny_run(tmp_path_factory):
    from tc_gan_amd.run import bptt_moments
    tmp = tmp_path_factory.mktemp('moments')
    cfg = tmp / 'config.json'
    cfg.write_text(json.dumps(dict(num_sites=20, true_ssn_options={k: (new_JDS[k] * 1.05).tolist() for k in 'JDS'})))
    bptt_moments.main(['--n_bandwidths', '4', '--seqlen', '40', '--skip-steps', '30', '--iterations', '3', '--quiet', '--truth_size', '16',
                       '--dataset-provider', 'fixedtime', '--gen-kernel', 'tile', '--batchsize', '4', '--sample-sites', '0,0.5',
                       '--gen-moments-record-interval', '1', '--datastore', str(tmp / 'run'), '--load-config', str(cfg)])
    assert json.load(open(str(tmp / 'run' / 'exit.json')))['good']
    return str(tmp / 'run')


@pytest.mark.parametrize('mode', [[], ['--dynamics', 'fixed-point', '--max-candidates', '12']], ids=['fixed-time', 'fixed-point'])
def test_command_line_writes_wdist_and_leaves_distdiff_alone(tiny_run, tmp_path, monkeypatch, mode):
    """Two runs from two working directories with the same relative --output: the recorded arguments are then the same text."""
    import pandas
    args = [tiny_run, '--draws', '6', '--output', 'scores'] + mode
    (tmp_path / 'on').mkdir()
    (tmp_path / 'off').mkdir()
    monkeypatch.chdir(tmp_path / 'on')
    res = distdiff.main(args + ['--wasserstein', '--directions', '8', '--direction-seed', '5'])
    monkeypatch.chdir(tmp_path / 'off')
    distdiff.main(args)
    on, off = tmp_path / 'on' / 'scores', tmp_path / 'off' / 'scores'
    plain = ['distdiff.csv', 'distdiff.json'] + (['rejections.csv'] if mode else [])
    assert sorted(os.listdir(str(off))) == plain and sorted(os.listdir(str(on))) == sorted(plain + ['wdist.csv', 'wdist.json'])
    for name in plain:
        assert (on / name).read_bytes() == (off / name).read_bytes(), name
    table = pandas.read_csv(str(on / 'wdist.csv'), float_precision='round_trip')
    Ct = 4 * 2 + 4 * 2
    assert list(table.columns) == ['gen_step', 'stat', 'W1', 'n', 'm'] and len(table) == 3 * (Ct + 1)
    assert list(table['stat']) == (res['stat'] + ['sliced_w1']) * 3
    np.testing.assert_array_equal(table['gen_step'].to_numpy(), np.repeat(res['gen_step'], Ct + 1))
    np.testing.assert_array_equal(table['W1'].to_numpy().reshape(3, Ct + 1)[:, :Ct], res['W1'])
    np.testing.assert_array_equal(table['W1'].to_numpy().reshape(3, Ct + 1)[:, Ct], res['SW1'])
    np.testing.assert_array_equal(table['n'].to_numpy().reshape(3, Ct + 1)[:, Ct], res['sliced']['n'])
    np.testing.assert_array_equal(table['m'].to_numpy(), np.tile(np.concatenate([res['m'], [16]]), 3))
    meta = json.load(open(str(on / 'wdist.json')))
    assert meta['arguments'] == dict(wasserstein=True, directions=8, direction_seed=5) and meta['directions'] == 8
    assert meta['gen_steps'] == [int(s) for s in res['gen_step']]

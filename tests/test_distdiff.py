"""Scoring a run's checkpoints (tc_gan_amd/analyzers/distdiff.py), the parts that need no GPU: the integer form of the
two-sample KS statistic the device kernel computes (restated here in numpy and pinned to scipy's), the host logic of the
scorer (chunk planning, --steps, statistic names, the long-format table, the refusals) and the generated code of
csrc/ssn_score.hip (no spills, no scratch)."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tc_gan_amd', 'csrc')


def ks_numerators(x, t):
    """(num, n, m) per column of x (B, C) against t (T, C): n, m = finite counts, num = max over the pooled points v of
    |#{x <= v} m - #{t <= v} n|, so that the two-sample KS statistic is num / (n m).  Non-finite values are left out."""
    x, t = np.asarray(x), np.asarray(t)
    num, n, m = (np.zeros(x.shape[1], dtype=np.int64) for _ in range(3))
    for c in range(x.shape[1]):
        xs, ts = np.sort(x[np.isfinite(x[:, c]), c]), np.sort(t[np.isfinite(t[:, c]), c])
        n[c], m[c] = len(xs), len(ts)
        pooled = np.concatenate([xs, ts])
        if n[c] and m[c]:
            cx = np.searchsorted(xs, pooled, side='right').astype(np.int64)
            ct = np.searchsorted(ts, pooled, side='right').astype(np.int64)
            num[c] = np.abs(cx * m[c] - ct * n[c]).max()
    return num, n, m


def _ksd(x, t):
    num, n, m = ks_numerators(np.asarray(x)[:, None], np.asarray(t)[:, None])
    return num[0] / float(n[0] * m[0])


# ---- 1. the integer form is scipy's statistic ----------------------------------------------------------------------------

def test_integer_form_equals_scipy_on_seeded_pairs():
    ks_2samp = pytest.importorskip('scipy.stats').ks_2samp
    rs = np.random.RandomState(7)
    worst = 0.0
    for i in range(300):
        n, m = int(rs.choice([1, 2, 5, 30, 128, 400])), int(rs.choice([1, 3, 32, 257, 1000]))
        if i % 3 == 0:
            x, t = rs.randn(n), rs.randn(m)
        elif i % 3 == 1:
            x, t = np.maximum(rs.randn(n), 0), np.maximum(rs.randn(m), 0)          # rectified: heavy ties at zero
        else:
            x, t = rs.randint(0, 8, n).astype(float), rs.randint(0, 8, m).astype(float)
        worst = max(worst, abs(_ksd(x, t) - ks_2samp(x, t).statistic))
    print('largest difference to scipy:', worst)
    assert worst <= 1e-15


def test_integer_form_equals_committed_scipy_statistics():
    g = golden('ks_cases.npz')
    want = g['statistic']
    assert len(want) >= 40
    for i, w in enumerate(want):
        x, t = g['x{}'.format(i)], g['t{}'.format(i)]
        assert abs(_ksd(x, t) - w) <= 1e-15, i


def test_non_finite_values_are_left_out():
    x = np.array([[0.0, np.nan], [1.0, np.nan], [np.inf, np.nan], [np.nan, -np.inf]])
    t = np.array([[0.0, 1.0], [2.0, 2.0]])
    num, n, m = ks_numerators(x, t)
    assert list(n) == [2, 0] and list(m) == [2, 2] and num[1] == 0
    assert num[0] == 2                # F_x = 1 at 1, F_t = 1/2: |2 * 2 - 1 * 2|


# ---- 2. host logic ------------------------------------------------------------------------------------------------------

def test_chunk_planning():
    from tc_gan_amd.analyzers.distdiff import plan_chunks
    assert plan_chunks(6, 7, 30) == (4, [4, 2])
    assert plan_chunks(256, 30, 4096) == (136, [136, 120])
    assert plan_chunks(8, 128, 1024) == (8, [8])
    assert plan_chunks(3, 1024, 100) == (1, [1, 1, 1])          # a budget below one checkpoint: one checkpoint per launch
    assert plan_chunks(0, 30, 100) == (3, [])
    for S, draws, budget in [(17, 5, 23), (1, 16384, 16384), (100, 33, 1000)]:
        chunk, sizes = plan_chunks(S, draws, budget)
        assert chunk == max(1, budget // draws) and sum(sizes) == S and all(0 < s <= chunk for s in sizes)
        assert all(s == chunk for s in sizes[:-1])
    with pytest.raises(ValueError, match='16384'):
        plan_chunks(4, 16385, 1 << 20)
    with pytest.raises(ValueError, match='draws'):
        plan_chunks(4, 0, 10)


def test_steps_parsing():
    from tc_gan_amd.analyzers.distdiff import parse_steps
    assert parse_steps(':') == slice(None)
    assert parse_steps('::10') == slice(None, None, 10)
    assert parse_steps('5:') == slice(5, None)
    assert parse_steps('2:20:3') == slice(2, 20, 3)
    assert parse_steps('7') == [7]
    assert parse_steps('0, 5,-1') == [0, 5, -1]
    assert parse_steps(slice(1, 2)) == slice(1, 2)
    for bad in ('a:b', '1:2:3:4', 'x,y'):
        with pytest.raises(ValueError, match='--steps'):
            parse_steps(bad)


def test_stat_names_follow_gridify_order():
    from tc_gan_amd.analyzers.distdiff import FEATURES, stat_names
    from tc_gan_amd.networks.utils import gridify_tc_samples
    NC, NB, CT, P = 2, 3, 2, 4
    names = stat_names(NC, NB, CT, P)
    C, curves = NC * NB * CT * P, NC * CT * P
    assert len(names) == C + 4 * curves and len(set(names)) == len(names)
    grid = gridify_tc_samples(np.arange(C)[None, :], NC, NB, CT, P)[0]         # (cell_type, probe, contrast, bandwidth) -> column
    for t in range(CT):
        for p in range(P):
            for c in range(NC):
                for b in range(NB):
                    assert names[grid[t, p, c, b]] == 'tc_c{}_b{}_t{}_p{}'.format(c, b, t, p)
    for f, feat in enumerate(FEATURES):
        for c in range(NC):
            for t in range(CT):
                for p in range(P):
                    assert names[C + f * curves + (c * CT + t) * P + p] == '{}_c{}_t{}_p{}'.format(feat, c, t, p)


def test_long_format_writer_round_trips(tmp_path):
    import pandas
    from tc_gan_amd.analyzers.distdiff import ksd_from_counts, long_table, write_long_table
    num = np.array([[0, 3, 0], [6, 1, 0]], dtype=np.int64)
    n = np.array([[2, 3, 0], [2, 3, 3]], dtype=np.int64)
    m = np.array([3, 2, 0], dtype=np.int64)
    result = dict(gen_step=np.array([10, 20]), stat=['a', 'b', 'c'], num=num, n=n, m=m, KSD=ksd_from_counts(num, n, m[None, :]))
    np.testing.assert_array_equal(result['KSD'], [[0.0, 0.5, np.nan], [1.0, 1.0 / 6.0, np.nan]])
    path = tmp_path / 'distdiff.csv'
    write_long_table(str(path), result)
    back = pandas.read_csv(str(path), float_precision='round_trip')      # (the default parser may be one ulp off)
    assert list(back.columns) == ['gen_step', 'stat', 'KSD', 'n', 'm'] and len(back) == 6
    assert list(back['gen_step']) == [10, 10, 10, 20, 20, 20] and list(back['stat']) == ['a', 'b', 'c'] * 2
    np.testing.assert_array_equal(back['KSD'].to_numpy(), result['KSD'].reshape(-1))
    np.testing.assert_array_equal(back['n'].to_numpy(), n.reshape(-1))
    np.testing.assert_array_equal(back['m'].to_numpy(), np.tile(m, 2))
    pandas.testing.assert_frame_equal(back, long_table(result).astype({'stat': back['stat'].dtype}), check_dtype=False)


CFG = dict(num_sites=10, bandwidths=[0.0625, 0.125, 0.25, 0.75], contrasts=[20.0], seqlen=30, skip_steps=20, norm_probes=[0, 0.5],
           include_inhibitory_neurons=True, gen_kernel='tile')
THETA = dict(J=0.01, D=0.01, S=0.1)


def test_refusals_need_no_device():
    from tc_gan_amd.analyzers.distdiff import score_parameter_sets
    truth = np.zeros((8, 16))
    with pytest.raises(ValueError, match='16384'):
        score_parameter_sets(CFG, [THETA], truth, draws=16385)
    with pytest.raises(ValueError, match='float64'):
        score_parameter_sets(dict(CFG, dtype='float64'), [THETA], truth, draws=4)
    with pytest.raises(ValueError, match='16 columns'):
        score_parameter_sets(CFG, [THETA], np.zeros((8, 12)), draws=4)
    bad = truth.copy()
    bad[3, 5] = np.nan
    with pytest.raises(ValueError, match='non-finite'):
        score_parameter_sets(CFG, [THETA], bad, draws=4)
    with pytest.raises(ValueError, match='needs V'):
        score_parameter_sets(dict(CFG, ssn_type='heteroin'), [THETA], truth, draws=4)


def test_data_parallel_ranks_are_refused(monkeypatch):
    from tc_gan_amd.analyzers.distdiff import score_parameter_sets
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='data-parallel'):
        score_parameter_sets(CFG, [THETA], np.zeros((8, 16)), draws=4)


def test_directory_without_generator_table_is_refused(tmp_path):
    from tc_gan_amd.analyzers.distdiff import calc_distdiff
    (tmp_path / 'info.json').write_text(json.dumps(dict(run_config=CFG)))
    np.save(str(tmp_path / 'truth.npy'), np.zeros((8, 16)))
    with pytest.raises(ValueError, match='generator'):
        calc_distdiff(str(tmp_path))


def test_sampler_config_of_a_run():
    from tc_gan_amd.analyzers.distdiff import sampler_config_of_run
    w = sampler_config_of_run(dict(num_sites=20, bandwidths=[0.1, 0.2], contrasts=[5, 20], sample_sites=[0, 0.5], seqlen=40,
                                   skip_steps=30, include_inhibitory_neurons=True, ssn_type='deg-heteroin', gen_kernel='duo',
                                   batchsize=4, truth_size=32))
    assert w['norm_probes'] == [0, 0.5] and w['include_inhibitory_neurons'] and w['ssn_type'] == 'deg-heteroin'
    assert w['gen_kernel'] == 'duo' and w['seqlen'] == 40 and w['io_type'] == 'asym_tanh' and w['dist_in'] == 'bernoulli'
    c = sampler_config_of_run(dict(norm_probes=[0.25], bandwidths=[0.1], contrasts=[20]))
    assert c['norm_probes'] == [0.25] and c['gen_kernel'] == 'auto' and not c['include_inhibitory_neurons']


def test_cli_module_resolves_under_the_reference_name():
    import importlib
    name = 'tc_gan.analyzers.distdiff'
    mod = importlib.import_module('tc_gan_amd.' + name[len('tc_gan.'):])          # run.py's mapping
    assert callable(mod.main) and 'p-value' in mod.__doc__
    ns = mod.make_parser().parse_args(['somewhere', '--steps', '::4', '--draws', '64', '--save-tuning-curves'])
    assert ns.rundir == 'somewhere' and ns.draws == 64 and ns.save_tuning_curves and ns.seed == 0 and ns.output is None


def test_product_package_imports_no_scipy():
    pkg = os.path.join(ROOT, 'tc_gan_amd', 'analyzers')
    for f in os.listdir(pkg):
        if f.endswith('.py'):
            assert not re.search(r'^\s*(from|import)\s+(scipy|oracle)', open(os.path.join(pkg, f)).read(), flags=re.M), f


# ---- 4. the generated code of csrc/ssn_score.hip ------------------------------------------------------------------------

def test_no_kernel_of_the_scorer_spills_or_uses_scratch(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = tmp_path / 'ssn_score.s'
    flags = ['-O3', '-std=c++17', '--offload-arch=gfx950']                       # csrc/Makefile: CXXFLAGS
    subprocess.run([hipcc] + flags + ['-S', '--cuda-device-only', 'ssn_score.hip', '-o', str(out)], cwd=CSRC, check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(str(out)).read()
    found = re.findall(r'\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)', text, re.S)
    names = sorted(n for n, _, _ in found)
    assert len(names) == 4 and sum('build_w_table_kernel' in n for n in names) == 2
    assert any('ks_columns_kernel' in n for n in names) and any('tc_features_kernel' in n for n in names)
    assert all(int(p) == 0 and int(s) == 0 for _, p, s in found), found

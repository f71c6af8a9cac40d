"""Scoring checkpoints at their fixed points (ssnode.sample_tuning_curves_table, analyzers/distdiff.py with
dynamics='fixed-point', csrc/ssn_fpsample.hip), the parts that need no GPU: the planning of rounds and chunks, every refusal,
the command line's defaults and the generated code of the new kernels (no spills, no scratch)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tc_gan_amd', 'csrc')
THETA = dict(J=0.01, D=0.01, S=0.1)


# ---- host logic ---------------------------------------------------------------------------------------------------------

def test_default_max_candidates():
    from tc_gan_amd.ssnode import default_max_candidates
    assert default_max_candidates(30) == 120
    assert default_max_candidates(12) == 76
    assert default_max_candidates(1) == 65
    assert default_max_candidates(22) == 88 and default_max_candidates(21) == 85        # the two branches meet at 64 / 3


def test_round_planning():
    from tc_gan_amd import clib
    from tc_gan_amd.ssnode import plan_table_rounds
    assert plan_table_rounds(12, 5, 12) == [(0, 5), (5, 5), (10, 2)]
    assert plan_table_rounds(12, None, 40) == [(0, 12), (12, 12), (24, 12), (36, 4)]
    assert plan_table_rounds(30) == [(0, 30), (30, 30), (60, 30), (90, 30)]              # round = NZ, 120 candidates
    assert plan_table_rounds(12, 40, 40) == [(0, 40)]
    assert plan_table_rounds(3, 7, 2) == [(0, 2)]
    limit = clib.FP_SELECT_MAX_CANDIDATES
    assert limit == clib.libssnode.ssn_fp_select_max_candidates() and limit >= 4096
    assert plan_table_rounds(1, limit, limit + 1) == [(0, limit), (limit, 1)]
    for NZ, rd, mc in [(7, 3, 100), (30, 30, 31), (5, 64, 63)]:
        rounds = plan_table_rounds(NZ, rd, mc)
        assert rounds[0][0] == 0 and sum(c for _, c in rounds) == mc and all(0 < c <= rd for _, c in rounds)
        assert all(a[0] + a[1] == b[0] for a, b in zip(rounds, rounds[1:]))
    with pytest.raises(ValueError, match='NZ'):
        plan_table_rounds(0)
    for bad in (0, -1, limit + 1):
        with pytest.raises(ValueError, match='round_draws'):
            plan_table_rounds(4, bad)
    with pytest.raises(ValueError, match='max_candidates'):
        plan_table_rounds(4, 4, 0)


def test_chunk_planning():
    from tc_gan_amd.ssnode import plan_table_chunks
    assert plan_table_chunks(5, 12, 40) == [3, 2]
    assert plan_table_chunks(5, 40, 40) == [1] * 5
    assert plan_table_chunks(5, 41, 40) == [1] * 5               # a round above the budget: one set per launch
    assert plan_table_chunks(136, 30, 4096) == [136]
    assert plan_table_chunks(0, 30, 4096) == []
    for S, count, budget in [(17, 5, 23), (100, 33, 1000)]:
        sizes = plan_table_chunks(S, count, budget)
        assert sum(sizes) == S and all(0 < s * count <= max(budget, count) for s in sizes)
    with pytest.raises(ValueError):
        plan_table_chunks(3, 0, 10)


# ---- refusals, raised without a device -----------------------------------------------------------------------------------

def test_sampler_refusals_need_no_device(monkeypatch):
    from tc_gan_amd import clib
    from tc_gan_amd.ssnode import sample_tuning_curves_table
    kw = dict(N=13, bandwidths=[0, 1])
    with pytest.raises(ValueError, match='offset'):
        sample_tuning_curves_table([THETA], offset=[0, 0.1], **kw)
    with pytest.raises(ValueError, match='offset'):
        sample_tuning_curves_table([THETA], offset=[0.5], **kw)
    with pytest.raises(ValueError, match='NZ'):
        sample_tuning_curves_table([THETA], NZ=0, **kw)
    with pytest.raises(ValueError, match='round_draws'):
        sample_tuning_curves_table([THETA], NZ=4, round_draws=0, **kw)
    with pytest.raises(ValueError, match='round_draws'):
        sample_tuning_curves_table([THETA], NZ=4, round_draws=clib.FP_SELECT_MAX_CANDIDATES + 1, **kw)
    with pytest.raises(ValueError, match=r"unknown parameters \['V'\]"):
        sample_tuning_curves_table([THETA, dict(THETA, V=0.3)], **kw)
    with pytest.raises(ValueError, match='unknown parameters'):
        sample_tuning_curves_table([dict(THETA, K=1)], **kw)
    with pytest.raises(ValueError, match='dtype'):
        sample_tuning_curves_table([THETA], dtype='float16', **kw)
    with pytest.raises(ValueError, match='sample_sites'):
        sample_tuning_curves_table([THETA], sample_sites=[13], **kw)
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='data-parallel'):
        sample_tuning_curves_table([THETA], **kw)


CFG = dict(num_sites=10, bandwidths=[0.0625, 0.125, 0.25, 0.75], contrasts=[20.0], seqlen=30, skip_steps=20, norm_probes=[0, 0.5],
           include_inhibitory_neurons=True, gen_kernel='tile')


def test_scorer_refusals_need_no_device(monkeypatch):
    from tc_gan_amd.analyzers.distdiff import score_parameter_sets
    truth = np.zeros((8, 16))
    fp = dict(dynamics='fixed-point')
    with pytest.raises(ValueError, match='dynamics'):
        score_parameter_sets(CFG, [THETA], truth, draws=4, dynamics='steady')
    for ssn_type in ('heteroin', 'deg-heteroin'):
        with pytest.raises(NotImplementedError, match='heterogeneous input'):
            score_parameter_sets(dict(CFG, ssn_type=ssn_type), [dict(THETA, V=0.3)], truth, draws=4, **fp)
    with pytest.raises(ValueError, match='solver_dtype'):
        score_parameter_sets(CFG, [THETA], truth, draws=4, solver_dtype='float16', **fp)
    with pytest.raises(ValueError, match='16 columns'):
        score_parameter_sets(CFG, [THETA], np.zeros((8, 12)), draws=4, **fp)
    with pytest.raises(ValueError, match='16384'):
        score_parameter_sets(CFG, [THETA], truth, draws=16385, **fp)
    with pytest.raises(ValueError, match='unknown parameters'):
        score_parameter_sets(CFG, [dict(THETA, V=0.3)], truth, draws=4, **fp)
    with pytest.raises(ValueError, match='max_candidates'):
        score_parameter_sets(CFG, [THETA], truth, draws=4, max_candidates=0, **fp)
    with pytest.raises(ValueError, match=r"unknown options \['seqlen'\]"):
        score_parameter_sets(CFG, [THETA], truth, draws=4, solver_options=dict(seqlen=10), **fp)
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='data-parallel'):
        score_parameter_sets(CFG, [THETA], truth, draws=4, **fp)


def test_fixed_point_options_are_the_truths(monkeypatch):
    """The scorer starts from the very options `dataset_by_ssnode` hands to the sampler, and layers the recorded and the caller's
    options on them in that order; only solver keys pass."""
    from tc_gan_amd import ssnode
    from tc_gan_amd.analyzers.distdiff import (FIXED_POINT_OPTION_KEYS, FIXED_POINT_SOLVER_OPTIONS, fixed_point_options,
                                                sampler_config_of_run)
    from tc_gan_amd.networks import dataset
    assert FIXED_POINT_SOLVER_OPTIONS is dataset.SSNODE_TRUTH_OPTIONS
    seen = {}

    def fake(**kwargs):
        seen.update(kwargs)
        return np.zeros((4, 3)), (None, None, ssnode.null_FixedPointsInfo)
    monkeypatch.setattr(ssnode, 'sample_tuning_curves', fake)
    recorded = dict(J=[[1, 2], [3, 4]], dt=1e-3, max_iter=500)
    dataset.dataset_by_ssnode(13, [0, 1], [20], 3, 0, [0], False, true_ssn_options=recorded)
    truth_solver = {k: v for k, v in seen.items() if k in FIXED_POINT_OPTION_KEYS}
    assert truth_solver == dict(dt=1e-3, max_iter=500, io_type='asym_power', rate_stop_at=200)
    # a run of the fixed-time provider may have recorded options of its sampler: they are not the solver's
    cfg = sampler_config_of_run(dict(bandwidths=[0.1], contrasts=[20], k=0.02, true_ssn_options=dict(recorded, V=0.5, seqlen=100, N=7)))
    assert fixed_point_options(cfg) == truth_solver             # (k, n, smoothness: ssnode's defaults, as for the truth)
    opts = fixed_point_options(cfg, dict(max_iter=7, io_type='asym_tanh', k=0.03))
    assert opts == dict(truth_solver, max_iter=7, io_type='asym_tanh', k=0.03)
    assert fixed_point_options(sampler_config_of_run(dict(bandwidths=[0.1], contrasts=[20]))) == dict(dataset.SSNODE_TRUTH_OPTIONS)
    for bad in (dict(seqlen=3), dict(N=5), dict(bandwidths=[1]), dict(seed=1)):
        with pytest.raises(ValueError, match='solver_options: unknown options'):
            fixed_point_options(cfg, bad)


def test_parser_defaults_leave_the_fixed_time_mode():
    from tc_gan_amd.analyzers.distdiff import make_parser
    ns = make_parser().parse_args(['somewhere'])
    assert ns.dynamics == 'fixed-time' and ns.max_candidates is None and ns.solver_dtype == 'float64'
    ns = make_parser().parse_args(['somewhere', '--dynamics', 'fixed-point', '--max-candidates', '90', '--solver-dtype', 'float32'])
    assert ns.dynamics == 'fixed-point' and ns.max_candidates == 90 and ns.solver_dtype == 'float32'
    with pytest.raises(SystemExit):
        make_parser().parse_args(['somewhere', '--dynamics', 'steady'])


def test_new_symbols_are_declared():
    from tc_gan_amd import clib
    for name in ('ssn_build_w_table_f64', 'ssn_fp_select_f64', 'ssn_fp_select_f32', 'ssn_fp_select_max_candidates'):
        assert name in clib.DECLARED_SYMBOLS and getattr(clib.libssnode, name).argtypes is not None
    assert clib.libssnode.ssn_abi_version() == 1


def test_invalid_select_arguments_are_refused_on_the_host():
    """R over the limit, NZ < 1, null pointers and odd M return the invalid-value status with the error text set -- before any
    launch, so without a device; an empty batch is success."""
    from tc_gan_amd import clib
    lib, limit = clib.libssnode, clib.FP_SELECT_MAX_CANDIDATES
    buf = np.zeros(64, dtype=np.float64).ctypes.data         # never dereferenced: every call below returns before a launch
    for fn in (lib.ssn_fp_select_f64, lib.ssn_fp_select_f32):
        def call(A=1, R=1, NB=1, M=2, NZ=1, codes=buf, x=buf, out=buf):
            return fn(codes, x, A, R, NB, M, buf, 1, buf, 0, NZ, buf, out, buf, buf, buf, buf, None)
        assert call(A=0) == 0 and call(R=0) == 0 and call(A=0, codes=None, x=None, out=None) == 0
        ok_codes = {0}
        rc = call(R=limit + 1)
        assert rc not in ok_codes and str(limit) in clib.last_error()
        for kw in (dict(NZ=0), dict(M=3), dict(codes=None), dict(x=None), dict(out=None), dict(NB=0), dict(R=-1)):
            assert call(**kw) == rc, kw
            assert 'ssn_fp_select' in clib.last_error() and 'invalid argument' in clib.last_error()
    assert lib.ssn_build_w_table_f64(None, None, None, 0, 5, 3, None) == 0
    assert lib.ssn_build_w_table_f64(None, None, None, 2, 5, 3, None) == rc and 'ssn_build_w_table_f64' in clib.last_error()


# ---- the generated code of csrc/ssn_fpsample.hip -------------------------------------------------------------------------

def test_no_kernel_of_the_fixed_point_sampler_spills_or_uses_scratch(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    assert 'ssn_fpsample.hip' in open(os.path.join(CSRC, 'Makefile')).read()
    out = tmp_path / 'ssn_fpsample.s'
    flags = ['-O3', '-std=c++17', '--offload-arch=gfx950']                       # csrc/Makefile: CXXFLAGS
    subprocess.run([hipcc] + flags + ['-S', '--cuda-device-only', 'ssn_fpsample.hip', '-o', str(out)], cwd=CSRC, check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(str(out)).read()
    found = re.findall(r'\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)', text, re.S)
    names = sorted(n for n, _, _ in found)
    assert len(names) == 8, names
    assert sum('build_w_table_kernel' in n for n in names) == 2          # fp64: vectors of 4 and the scalar form
    assert sum('verdict_kernel' in n for n in names) == 4                # fp64 and fp32: 16-byte loads and the scalar form
    assert sum('select_kernel' in n for n in names) == 2
    assert all(int(p) == 0 and int(s) == 0 for _, p, s in found), found

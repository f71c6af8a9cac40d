"""Ensembles of sliced Wasserstein runs (networks/sliced_wasserstein_ensemble.py, run/bptt_swd_ensemble.py, csrc/ssn_ens_swd.hip),
the parts that need no GPU: member options, the datastore layout and the members' configs, the declarations of the new entry
points and their refusals from the arguments alone, and the generated code of the new kernels."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import pytest

from tc_gan_amd import clib, execution
from tc_gan_amd.networks import moment_matching_ensemble as mme
from tc_gan_amd.networks import sliced_wasserstein_ensemble as swe
from tc_gan_amd.run import bptt_swd, bptt_swd_ensemble as bse
from tc_gan_amd.run.bptt_wgan import preprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tc_gan_amd', 'csrc')

SHARED = dict(num_sites=20)
ARGS = ['--n_bandwidths', '8', '--seqlen', '40', '--skip-steps', '30', '--batchsize', '4', '--iterations', '6',
        '--gen-kernel', 'tile', '--sample-sites', '0,0.5', '--swd-directions', '33']
MEMBERS = [dict(seed=1, J0=0.02, learning_rate=0.01, swd_power=1, swd_direction_seed=3),
           dict(seed=2, S0=0.3, learning_rate=0.002, swd_power=2, rate_cost=3.0, truth_size=48)]
NEW_SYMBOLS = ('ssn_ens_swd_project_f32', 'ssn_ens_swd_match_f32', 'ssn_ens_swd_backproject_f32', 'ssn_ens_gen_grads_l0_f32')


# ---- member options ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('key', ['num_sites', 'batchsize', 'seqlen', 'gen_kernel', 'ssn_type', 'bandwidths', 'iterations',
                                 'swd_directions'])
def test_shared_key_refused_by_name(key):
    with pytest.raises(ValueError, match='{!r} is shared'.format(key)):
        swe.validate_member_overrides([dict(seed=1), {key: 1}])


@pytest.mark.parametrize('key', ['no_such_option', 'lam', 'moment_weight_type', 'moment_weights_regularization'])
def test_unknown_key_and_the_moment_loss_keys_refused_by_name(key):
    with pytest.raises(ValueError, match="unknown option {!r}".format(key)):
        swe.validate_member_overrides([{key: 1}])


def test_member_keys():
    assert swe.validate_member_overrides(MEMBERS) == MEMBERS
    assert swe.MEMBER_KEYS == (mme.MEMBER_KEYS - {'lam', 'moment_weight_type', 'moment_weights_regularization'}) | {
        'swd_power', 'swd_direction_seed'}
    assert swe.SHARED_KEYS == mme.SHARED_KEYS | {'swd_directions'}
    assert not (swe.MEMBER_KEYS & swe.SHARED_KEYS)
    swe.validate_member_overrides([dict(z_device_seed=1), dict(z_device_seed=2)])
    with pytest.raises(ValueError, match='z_device_seed'):
        swe.validate_member_overrides([dict(z_device_seed=1), dict(seed=2)])
    # the moment ensemble's own check is as it was
    assert mme.validate_member_overrides([dict(lam=0.5)]) == [dict(lam=0.5)]
    with pytest.raises(ValueError, match="unknown option 'swd_power'"):
        mme.validate_member_overrides([dict(swd_power=1)])


def test_factory_refusals_need_no_device(monkeypatch):
    with pytest.raises(ValueError, match='duo-fused'):
        swe.ensemble_from_member_configs([dict(gen_kernel='duo-fused')])
    with pytest.raises(ValueError, match='float32'):
        swe.ensemble_from_member_configs([dict(gen_kernel='tile', gen_dtype='float64')])
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='one GPU'):
        swe.ensemble_from_member_configs([dict(gen_kernel='tile')])


# ---- configs and the datastore layout -----------------------------------------------------------------------------------------

def _run_config(tmp_path, extra_args=()):
    members_file = tmp_path / 'members.json'
    members_file.write_text(json.dumps(MEMBERS))
    shared_file = tmp_path / 'shared.json'
    shared_file.write_text(json.dumps(SHARED))
    ns = bse.make_parser().parse_args(ARGS + list(extra_args) + ['--members', str(members_file), '--datastore', str(tmp_path / 'ens'),
                                                                 '--load-config', str(shared_file)])
    rc = vars(ns)
    rc.pop('members')
    return rc


def test_member_run_configs_resolve_one_kernel_for_all_draws(tmp_path):
    rc = _run_config(tmp_path)
    for key in ('load_config', 'datastore', 'datastore_template'):
        rc.pop(key)
    rc.update(SHARED, gen_kernel='auto', batchsize=32)
    want = swe.resolve_gen_kernel(dict(num_sites=20, bandwidths=[0] * 8, contrasts=[20], batchsize=32, seqlen=40, skip_steps=30), 3)
    assert want != swe.resolve_gen_kernel(dict(num_sites=20, bandwidths=[0] * 8, contrasts=[20], batchsize=32, seqlen=40,
                                               skip_steps=30), 1) == 'tile'
    overrides, configs = bse.member_run_configs(rc, MEMBERS + [dict(seed=5)])
    assert [c['gen_kernel'] for c in configs] == [want] * 3 and len(overrides) == 3
    assert [c['swd_power'] for c in configs] == [1, 2, 2] and [c['swd_direction_seed'] for c in configs] == [3, 0, 0]
    with pytest.raises(ValueError, match="unknown option 'lam'"):
        bse.member_run_configs(rc, [dict(lam=1.0)])
    with pytest.raises(ValueError, match="'swd_directions' is shared"):
        bse.member_run_configs(rc, [dict(swd_directions=8)])


def _solo_info(tmp_path, extra):
    """info.json of a single bptt_swd run with `extra` through --load-config (what pre_learn writes, no GPU)."""
    os.makedirs(str(tmp_path), exist_ok=True)
    cfg_file = tmp_path / 'solo.json'
    cfg_file.write_text(json.dumps(dict(SHARED, **extra)))
    rc = vars(bptt_swd.make_parser().parse_args(ARGS + ['--load-config', str(cfg_file)]))
    d = str(tmp_path / 'solo')
    execution.pre_learn(packages=[], datastore=d, datastore_template=rc.pop('datastore_template'), load_config=rc.pop('load_config'),
                        preprocess=preprocess, **{k: v for k, v in rc.items() if k != 'datastore'})
    return json.load(open(os.path.join(d, 'info.json')))['run_config']


def test_datastore_layout_and_member_configs(tmp_path):
    datastore, dirs, configs = bse.prepare_datastores(_run_config(tmp_path), MEMBERS)
    assert dirs == [os.path.join(str(tmp_path / 'ens'), str(i)) for i in range(2)]
    summary = json.load(open(os.path.join(datastore, 'members.json')))
    assert summary['num_members'] == 2 and summary['gen_kernel'] == 'tile' and summary['members'] == MEMBERS
    for i, over in enumerate(MEMBERS):
        info = json.load(open(os.path.join(dirs[i], 'info.json')))
        assert info['run_config'] == _solo_info(tmp_path / str(i), over)
        assert info['run_config']['gen_kernel'] == 'tile' and info['run_config']['swd_directions'] == 33
        assert info['extra_info']['learn'] == 'tc_gan_amd.run.bptt_swd_ensemble.learn'


def test_command_line():
    parser = bse.make_parser()
    with pytest.raises(SystemExit):
        parser.parse_args([])                                  # --members is required
    got = vars(parser.parse_args(['--members', 'm.json']))
    solo = vars(bptt_swd.make_parser().parse_args([]))
    assert set(got) == set(solo) | {'members'}
    assert got['datastore_template'] == 'logfiles/BPTT_SWD_ensemble_{swd_directions}'
    with pytest.raises(SystemExit):
        parser.parse_args(['--members', 'm.json', '--lam', '1'])


# ---- the library ------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_declared():
    header = open(os.path.join(ROOT, 'include', 'ssnode_mi355x.h')).read()
    for name in NEW_SYMBOLS:
        assert name in clib.DECLARED_SYMBOLS and getattr(clib.libssnode, name).argtypes is not None
        assert re.search(r'^int %s\(' % name, header, re.M)
    lib = clib.libssnode
    assert [len(getattr(lib, n).argtypes) for n in NEW_SYMBOLS] == [10, 11, 8, 3]
    for macro, value in (('SSN_ENS_SWD_MAX_MEMBERS', clib.ENS_SWD_MAX_MEMBERS), ('SSN_SWD_WAVE_MAX_BATCH', clib.SWD_WAVE_MAX_BATCH),
                         ('SSN_SWD_FORM_AUTO', clib.SWD_FORM_AUTO), ('SSN_SWD_FORM_GENERAL', clib.SWD_FORM_GENERAL),
                         ('SSN_SWD_FORM_WAVE', clib.SWD_FORM_WAVE)):
        assert int(re.search(r'#define %s (\d+)' % macro, header).group(1)) == value
    assert 'ssn_ens_swd.hip' in open(os.path.join(CSRC, 'Makefile')).read()
    import importlib.util
    spec = importlib.util.spec_from_file_location('gen_export_map', os.path.join(CSRC, 'gen_export_map.py'))
    gem = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gem)
    assert set(NEW_SYMBOLS) <= set(gem.declared(header))       # the export map is made from these
    nm = shutil.which('nm')
    if nm:
        exported = subprocess.run([nm, '-D', '--defined-only', lib._name], check=True, stdout=subprocess.PIPE,
                                  universal_newlines=True).stdout
        for name in NEW_SYMBOLS:
            assert ' T ' + name in exported


def test_c_entry_points_refuse_from_the_arguments_alone():
    """Host checks in front of any HIP call: no device needed."""
    lib = clib.libssnode
    invalid = clib.SSN_ERR_BASE + 1
    two = (ctypes.c_int * 2)(1, 2)
    assert lib.ssn_ens_swd_match_f32(None, None, two, 2, clib.SWD_MAX_BATCH + 1, 3, 0, None, None, None, None) == invalid
    assert '4096 rows' in clib.last_error()
    assert lib.ssn_ens_swd_project_f32(None, None, None, 2, 4, clib.W1_MAX_DIRECTIONS + 1, 3, None, None, None) == invalid
    assert '4096 directions' in clib.last_error()
    assert lib.ssn_ens_swd_backproject_f32(None, None, clib.ENS_SWD_MAX_MEMBERS + 1, 4, 3, 3, None, None) == invalid
    assert '2048 members' in clib.last_error()
    assert lib.ssn_ens_swd_match_f32(None, None, (ctypes.c_int * 2)(2, 3), 2, 4, 3, 0, None, None, None, None) == invalid
    assert 'power other than 1 or 2' in clib.last_error()
    assert lib.ssn_ens_swd_match_f32(None, None, two, 2, 65, 3, clib.SWD_FORM_WAVE, None, None, None, None) == invalid
    assert '64 rows' in clib.last_error()
    assert lib.ssn_ens_swd_match_f32(None, None, two, 2, 4, 3, 0, None, None, None, None) == invalid      # null pointers
    assert 'invalid argument' in clib.last_error()
    assert lib.ssn_ens_swd_project_f32(None, None, None, 2, -4, 3, 3, None, None, None) == invalid
    assert lib.ssn_ens_swd_backproject_f32(None, None, 2, 4, 3, -1, None, None) == invalid
    assert lib.ssn_ens_gen_grads_l0_f32(None, None, None) == invalid
    # empty problems succeed
    for k, b, l in ((0, 4, 3), (2, 0, 3), (2, 4, 0)):
        assert lib.ssn_ens_swd_project_f32(None, None, None, k, b, l, 3, None, None, None) == 0
        assert lib.ssn_ens_swd_match_f32(None, None, two, k, b, l, 0, None, None, None, None) == 0
    assert lib.ssn_ens_swd_backproject_f32(None, None, 0, 4, 3, 3, None, None) == 0
    assert lib.ssn_ens_swd_backproject_f32(None, None, 2, 4, 3, 0, None, None) == 0


def test_no_kernel_of_the_new_file_spills_or_uses_scratch(tmp_path):
    """Metadata only.  LDS: the projection's two tiles are 32 x 129 + 32 x 128 floats = 32896 bytes, the general
    match form's static part is 40 bytes (four doubles, one flag) beside the dynamic 12 P <= 48 KiB, the wave form and the l0 sum
    use none, the back-projection's two tiles are 16 x 65 + 64 x 16 floats = 8256 bytes."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = tmp_path / 'ssn_ens_swd.s'
    flags = ['-O3', '-std=c++17', '--offload-arch=gfx950']                       # csrc/Makefile: CXXFLAGS
    subprocess.run([hipcc] + flags + ['-S', '--cuda-device-only', 'ssn_ens_swd.hip', '-o', str(out)], cwd=CSRC, check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(str(out)).read()
    found = re.findall(r'\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)'
                       r'.*?\.sgpr_spill_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+).*?\.wavefront_size:\s+(\d+)', text, re.S)
    kernels = ('ens_swd_project_kernel', 'ens_swd_match_kernel', 'ens_swd_match_wave_kernel', 'ens_swd_l0_kernel',
               'ens_swd_backproject_kernel')
    lds = {next(k for k in kernels if re.search(r'\d%sE' % k, name)): int(g) for g, name, _, _, _, _ in found}
    assert lds == {'ens_swd_project_kernel': 32896, 'ens_swd_match_kernel': 40, 'ens_swd_match_wave_kernel': 0,
                   'ens_swd_l0_kernel': 0, 'ens_swd_backproject_kernel': 8256}, found
    assert all(int(p) == 0 and int(ss) == 0 and int(vs) == 0 and int(w) == 64 for _, _, p, ss, vs, w in found), found
    # the wave form sorts in registers: cross-lane moves, no LDS traffic but the moves' own, no barrier
    body = re.search(r'^_ZN\w*ens_swd_match_wave_kernel\w*:.*?^\.Lfunc_end', text, re.S | re.M).group(0)
    assert 'dpp' in body and 's_barrier' not in body and 'ds_read' not in body and 'ds_write' not in body
    for name in ('ssn_ens_swd.hip', 'ssn_swd_dev.h', 'ssn_sortcol_dev.h'):
        source = open(os.path.join(CSRC, name)).read()
        assert 'asm' not in source and 'atomic' not in source.lower().replace('no atomics', '')

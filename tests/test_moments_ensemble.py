"""Ensembles of moment-matching runs (tc_gan_amd.run.bptt_moments_ensemble): member options, datastore layout, configs.
CPU only: nothing here launches a kernel (the automatic kernel choice is host arithmetic of the library)."""
import json
import os

import pytest

from tc_gan_amd import execution
from tc_gan_amd.networks import moment_matching_ensemble as mme
from tc_gan_amd.run import bptt_moments, bptt_moments_ensemble as bme
from tc_gan_amd.run.bptt_wgan import preprocess

SHARED = dict(num_sites=20)
ARGS = ['--n_bandwidths', '8', '--seqlen', '40', '--skip-steps', '30', '--batchsize', '4',
        '--iterations', '6', '--gen-kernel', 'tile', '--sample-sites', '0,0.5']
MEMBERS = [dict(seed=1, J0=0.02, learning_rate=0.01, lam=0.1), dict(seed=2, S0=0.3, learning_rate=0.002, lam=1.0,
                                                                  moment_weight_type='ew_relative', rate_cost=3.0)]


@pytest.mark.parametrize('key', ['num_sites', 'batchsize', 'seqlen', 'gen_kernel', 'ssn_type', 'bandwidths', 'iterations'])
def test_shared_key_refused_by_name(key):
    with pytest.raises(ValueError, match=repr(key)):
        mme.validate_member_overrides([dict(seed=1), {key: 1}])


def test_unknown_key_refused():
    with pytest.raises(ValueError, match="unknown option 'no_such_option'"):
        mme.validate_member_overrides([dict(no_such_option=3)])


def test_member_keys_accepted_and_z_device_seed_all_or_none():
    assert mme.validate_member_overrides(MEMBERS) == MEMBERS
    mme.validate_member_overrides([dict(z_device_seed=1), dict(z_device_seed=2)])
    with pytest.raises(ValueError, match='z_device_seed'):
        mme.validate_member_overrides([dict(z_device_seed=1), dict(seed=2)])
    assert not (mme.MEMBER_KEYS & mme.SHARED_KEYS)


def test_auto_resolved_for_the_ensemble_batch():
    cfg = dict(num_sites=20, bandwidths=[0] * 8, contrasts=[20], batchsize=32, gen_kernel='auto', seqlen=40, skip_steps=30)
    assert mme.resolve_gen_kernel(cfg, 1) == 'tile'
    assert mme.resolve_gen_kernel(cfg, 3) in ('split-1g', 'mfma-fp32-1g')
    assert mme.resolve_gen_kernel(dict(cfg, gen_kernel='duo'), 1) == 'duo'
    with pytest.raises(ValueError):
        mme.resolve_gen_kernel(dict(cfg, gen_kernel='duo-fused'), 2)


def _solo_info(tmp_path, extra):
    """info.json of a single bptt_moments run with `extra` through --load-config (what pre_learn writes, no GPU)."""
    os.makedirs(str(tmp_path), exist_ok=True)
    cfg_file = tmp_path / 'solo.json'
    cfg_file.write_text(json.dumps(dict(SHARED, **extra)))
    ns = bptt_moments.make_parser().parse_args(ARGS + ['--load-config', str(cfg_file)])
    rc = vars(ns)
    d = str(tmp_path / 'solo')
    execution.pre_learn(packages=[], datastore=d, datastore_template=rc.pop('datastore_template'), load_config=rc.pop('load_config'),
                        preprocess=preprocess, **{k: v for k, v in rc.items() if k != 'datastore'})
    return json.load(open(os.path.join(d, 'info.json')))['run_config']


def test_datastore_layout_and_member_configs(tmp_path):
    members_file = tmp_path / 'members.json'
    members_file.write_text(json.dumps(MEMBERS))
    shared_file = tmp_path / 'shared.json'
    shared_file.write_text(json.dumps(SHARED))
    ns = bme.make_parser().parse_args(ARGS + ['--members', str(members_file), '--datastore', str(tmp_path / 'ens'),
                                              '--load-config', str(shared_file)])
    rc = vars(ns)
    rc.pop('members')
    datastore, dirs, configs = bme.prepare_datastores(rc, MEMBERS)
    assert dirs == [os.path.join(str(tmp_path / 'ens'), str(i)) for i in range(2)]
    summary = json.load(open(os.path.join(datastore, 'members.json')))
    assert summary['num_members'] == 2 and summary['gen_kernel'] == 'tile' and summary['members'] == MEMBERS
    for i, over in enumerate(MEMBERS):
        info = json.load(open(os.path.join(dirs[i], 'info.json')))
        assert info['run_config'] == _solo_info(tmp_path / str(i), over)
        assert info['run_config']['gen_kernel'] == 'tile'

"""Ensembles of moment-matching runs on the GPU: every member's tables are its single run's (run/bptt_moments.py with the
same config and the kernel the ensemble ran), and the segmented kernels of csrc/ssn_ensemble.hip agree member by member with
the single-run kernels -- a NaN in one member reaches no other."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tc_gan_amd import clib, execution
from tc_gan_amd.clib import libssnode
from tc_gan_amd.loaders import _read_table
from tc_gan_amd.run import bptt_moments, bptt_moments_ensemble as bme

pytestmark = pytest.mark.gpu

BASE = ['--n_bandwidths', '8', '--seqlen', '40', '--skip-steps', '30', '--batchsize', '4', '--iterations', '6', '--quiet',
        '--gen-moments-record-interval', '1', '--truth_size', '32', '--sample-sites', '0,0.5']
SHARED = dict(num_sites=20)
MEMBERS = [dict(seed=1, J0=0.02, learning_rate=0.01, lam=0.1, rate_cost=0.5),
           dict(seed=2, S0=0.3, learning_rate=0.002, lam=1.0, moment_weight_type='ew_relative', rate_cost=0.5),
           dict(seed=3, J0=0.015, S0=0.2, learning_rate=0.005, lam=0.3, moment_weight_type='ew_mean', rate_cost=3.0)]
MAXDIFF = {}


def _write(path, obj):
    path.write_text(json.dumps(obj))
    return str(path)


def _ensemble(tmp_path, args, members, shared=SHARED):
    d = tmp_path / 'ens'
    bme.main(args + ['--members', _write(tmp_path / 'members.json', members), '--datastore', str(d),
                     '--load-config', _write(tmp_path / 'shared.json', shared)])
    return [str(d / str(i)) for i in range(len(members))]


def _solo(tmp_path, args, shared, member, i, kernel):
    d = tmp_path / 'solo{}'.format(i)
    cfg = dict(shared, **member)
    argv = args + ['--datastore', str(d), '--load-config', _write(tmp_path / 'solo{}.json'.format(i), cfg)]
    if '--gen-kernel' in argv:
        argv[argv.index('--gen-kernel') + 1] = kernel
    else:
        argv += ['--gen-kernel', kernel]
    try:
        bptt_moments.main(argv)
    except execution.KnownError:
        pass
    return str(d)


def _compare(ens_dir, solo_dir, tag, rtol=1e-6):
    ea, eb = json.load(open(os.path.join(ens_dir, 'exit.json'))), json.load(open(os.path.join(solo_dir, 'exit.json')))
    assert ea == eb
    worst = 0.0
    for name in ('learning', 'generator', 'gen_moments'):
        ta, tb = _read_table(ens_dir, name), _read_table(solo_dir, name)
        assert list(ta.columns) == list(tb.columns) and len(ta) == len(tb), name
        cols = [c for c in ta.columns if c not in ('train_time',)]
        va, vb = ta[cols].to_numpy(dtype='float64'), tb[cols].to_numpy(dtype='float64')
        np.testing.assert_allclose(va, vb, rtol=rtol, atol=0, err_msg='{} {}'.format(tag, name))
        with np.errstate(invalid='ignore', divide='ignore'):
            rel = np.abs(va - vb) / np.maximum(np.abs(vb), 1e-300)
        worst = max(worst, float(np.nanmax(rel)) if rel.size else 0.0)
    # the first step's forward: the tuning-curve moments of step 0 are the same bits
    np.testing.assert_array_equal(_read_table(ens_dir, 'gen_moments').to_numpy()[0], _read_table(solo_dir, 'gen_moments').to_numpy()[0])
    MAXDIFF[tag] = max(MAXDIFF.get(tag, 0.0), worst)
    print('largest relative difference {}: {:.3g}'.format(tag, worst))


def _check(tmp_path, args, members, kernel, shared=SHARED, tag=None):
    ens = _ensemble(tmp_path, args + ['--gen-kernel', kernel], members, shared)
    for i, m in enumerate(members):
        info = json.load(open(os.path.join(ens[i], 'info.json')))
        assert info['run_config']['gen_kernel'] == kernel
        _compare(ens[i], _solo(tmp_path, args, shared, m, i, kernel), '{}/{}'.format(tag or kernel, i))


@pytest.mark.parametrize('kernel', ['tile', 'mfma-fp32'])
def test_three_members_match_solo(tmp_path, kernel):
    _check(tmp_path, BASE, MEMBERS, kernel)


def test_deg_heteroin_members_match_solo(tmp_path):
    shared = dict(SHARED, ssn_type='deg-heteroin', dataset_provider='fixedtime')
    members = [dict(m, V0=v) for m, v in zip(MEMBERS, (0.3, 0.5, 0.1))]
    _check(tmp_path, BASE, members, 'tile', shared, tag='deg-heteroin')


def test_philox_members_match_solo(tmp_path):
    members = [dict(m, z_device_seed=100 + i) for i, m in enumerate(MEMBERS)]
    _check(tmp_path, BASE, members, 'tile', tag='philox')


def test_duo_odd_batch_members_match_solo(tmp_path):
    args = [a if a != '4' else '3' for a in BASE]          # batchsize 3: a workgroup of two draws holds two members
    _check(tmp_path, args, MEMBERS, 'duo', tag='duo')


def test_single_member_matches_solo(tmp_path):
    _check(tmp_path, BASE, MEMBERS[:1], 'tile', tag='K=1')


def test_member_that_quits_leaves_the_others_unchanged(tmp_path):
    members = [MEMBERS[0], dict(MEMBERS[1], quit_JDS_threshold=1e-3), MEMBERS[2]]
    _check(tmp_path, BASE, members, 'tile', tag='quit')
    exit1 = json.load(open(str(tmp_path / 'ens' / '1' / 'exit.json')))
    assert exit1['reason'] == 'JDS_distance'
    assert json.load(open(str(tmp_path / 'ens' / '0' / 'exit.json')))['reason'] == 'end_of_iteration'


def test_auto_picks_the_ensemble_kernel(tmp_path):
    args = [a if a != '4' else '32' for a in BASE]
    args[args.index('--iterations') + 1] = '1'
    ens = _ensemble(tmp_path, args + ['--gen-kernel', 'auto'], MEMBERS, SHARED)
    want = bme.resolve_gen_kernel(dict(num_sites=20, bandwidths=[0] * 8, contrasts=[20], batchsize=32, seqlen=40, skip_steps=30), 3)
    assert want != bme.resolve_gen_kernel(dict(num_sites=20, bandwidths=[0] * 8, contrasts=[20], batchsize=32, seqlen=40,
                                               skip_steps=30), 1)
    for i, m in enumerate(MEMBERS):
        assert json.load(open(os.path.join(ens[i], 'info.json')))['run_config']['gen_kernel'] == want
        solo = _solo(tmp_path, args, SHARED, m, i, 'auto')
        np.testing.assert_allclose(_read_table(ens[i], 'gen_moments').to_numpy()[0, 1:],
                                   _read_table(solo, 'gen_moments').to_numpy()[0, 1:], rtol=1e-4, atol=1e-6)


# ---- the segmented kernels against the single-run kernels, member by member -------------------------------------------------
def _stream():
    return clib.stream_ptr()


def test_segmented_moments_match_single_run_kernels_and_isolate_nan():
    K, B, D = 4, 5, 7
    g = torch.Generator().manual_seed(0)
    x = torch.rand((K * B, D), generator=g).cuda()
    x[B + 2, 3] = float('nan')                              # member 1 poisoned
    dm = torch.rand((K, 2, D), generator=g, dtype=torch.float64).cuda()
    w = torch.rand((K, 2, D), generator=g, dtype=torch.float64).cuda()
    R = int(libssnode.ssn_ens_record_doubles(D, 12))
    rec = torch.zeros((K, R), device='cuda', dtype=torch.float64)
    sums = torch.empty((K, 2, D), device='cuda', dtype=torch.float64)
    gx = torch.empty_like(x)
    clib.check(libssnode.ssn_ens_moments_f32(x.data_ptr(), K, B, D, sums.data_ptr(), dm.data_ptr(), w.data_ptr(), gx.data_ptr(),
                                             rec.data_ptr(), R, _stream()), 'ssn_ens_moments_f32')
    for k in range(K):
        xs = x[k * B:(k + 1) * B].contiguous()
        s1 = torch.empty((2, D), device='cuda', dtype=torch.float64)
        clib.check(libssnode.ssn_moment_sums_f32(xs.data_ptr(), B, D, s1.data_ptr(), _stream()), 'sums')
        g1 = torch.empty_like(xs)
        out = torch.empty(1 + 2 * D, device='cuda', dtype=torch.float64)
        clib.check(libssnode.ssn_moment_loss_grad_f32(xs.data_ptr(), s1.data_ptr(), float(B), dm[k].contiguous().data_ptr(),
                                                      w[k].contiguous().data_ptr(), B, D, g1.data_ptr(), out.data_ptr(), _stream()),
                   'loss_grad')
        torch.testing.assert_close(sums[k], s1, rtol=0, atol=0, equal_nan=True)
        torch.testing.assert_close(gx[k * B:(k + 1) * B], g1, rtol=0, atol=0, equal_nan=True)
        torch.testing.assert_close(rec[k, 1:1 + 2 * D], out[1:], rtol=0, atol=0, equal_nan=True)
        assert torch.isfinite(gx[k * B:(k + 1) * B]).all() == (k != 1)


def test_segmented_grads_and_apply_isolate_nan():
    K, B, NB, M, D, nv = 3, 4, 2, 8, 3, 1
    P = nv + 12
    g = torch.Generator().manual_seed(1)
    f = dict(device='cuda', dtype=torch.float32)
    parts = torch.rand((K * B, 4, 3), generator=g, dtype=torch.float64).cuda()
    g_ext, ext_base = torch.rand((K * B, NB, M), generator=g).cuda(), torch.rand((K * B, NB, M), generator=g).cuda()
    zin = (torch.rand((K * B, M), generator=g) * 2 - 1).cuda()
    dyn, rate = torch.rand((K * B, NB, M), generator=g).cuda(), torch.rand((K * B, NB, M), generator=g).cuda()
    dyn[2 * B, 0, 1] = float('nan')                        # member 2 poisoned
    dm = torch.rand((K, 2, D), generator=g, dtype=torch.float64).cuda()
    w = torch.rand((K, 2, D), generator=g, dtype=torch.float64).cuda()
    costs = torch.tensor([[1.0, 0.5], [0.0, 2.0], [1.0, 1.0]], device='cuda', dtype=torch.float64)
    R = int(libssnode.ssn_ens_record_doubles(D, P))
    rec = torch.zeros((K, R), device='cuda', dtype=torch.float64)
    rec[:, 1:1 + 2 * D] = torch.rand((K, 2 * D), generator=g, dtype=torch.float64).cuda()
    grads = torch.empty((K, P), **f)
    n = B * NB * M
    a = clib.EnsGrads(K=K, B=B, nv=nv, NB=NB, M=M, D=D, part=parts.data_ptr(), g_ext=g_ext.data_ptr(), ext_base=ext_base.data_ptr(),
                      zin=zin.data_ptr(), dyn_row=dyn.data_ptr(), rate_row=rate.data_ptr(), scale_dyn=1.0 / n, scale_rate=1.0 / n,
                      data_moments=dm.data_ptr(), weights=w.data_ptr(), costs=costs.data_ptr(), grads=grads.data_ptr(),
                      rec=rec.data_ptr(), rstride=R)
    clib.check(libssnode.ssn_ens_gen_grads_f32(ctypes.byref(a), _stream()), 'ssn_ens_gen_grads_f32')
    for k in range(K):
        sl = slice(k * B, (k + 1) * B)
        gv = (g_ext[sl].double() * ext_base[sl].double() * zin[sl].double()[:, None, :]).sum()
        tot = parts[sl].sum(0)                                      # (4, 3)
        want = torch.cat([gv.reshape(1), tot[:, 0], tot[:, 1], tot[:, 2]]).float()
        torch.testing.assert_close(grads[k], want, rtol=1e-6, atol=1e-6)
        pd, pr = dyn[sl].double().mean(), rate[sl].double().mean()
        m = rec[k, 1:1 + 2 * D].reshape(2, D)
        L0 = (w[k] * (dm[k] - m) ** 2).mean()
        fd, fr = float(pd.float()), float(pr.float())
        assert rec[k, 0].item() == pytest.approx(L0.item(), rel=1e-12)
        if k == 2:
            assert np.isnan(rec[k, 1 + 2 * D].item()) and np.isnan(rec[k, 3 + 2 * D].item())
        else:
            assert rec[k, 1 + 2 * D].item() == fd and rec[k, 2 + 2 * D].item() == fr
            assert rec[k, 3 + 2 * D].item() == pytest.approx(L0.item() + costs[k, 0].item() * fd + costs[k, 1].item() * fr, rel=1e-12)
    # optimizer: against ssn_optimizer_step per member (Adam, member 0's gradient poisoned)
    grads[0, 5] = float('nan')
    p0 = torch.rand((K, P), generator=g).cuda()
    p, s1, s2 = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    lo, hi = torch.full((K, P), 0.05, **f), torch.full((K, P), 0.9, **f)
    lrs = [0.01, 0.003, 0.02]
    hyp = torch.zeros((K, 8), **f)
    for k, lr in enumerate(lrs):
        hyp[k, 0] = lr
        hyp[k, 1] = float(np.float32(lr * np.sqrt(1 - 0.9) / (1 - 0.5)))
    o = clib.EnsApply(K=K, P=P, kind=1, beta1=0.5, beta2=0.9, eps=1e-8, rho=0.9, hyp=hyp.data_ptr(), clip_lo=lo.data_ptr(),
                      clip_hi=hi.data_ptr(), p=p.data_ptr(), s1=s1.data_ptr(), s2=s2.data_ptr(), g=grads.data_ptr(),
                      rec=rec.data_ptr(), rstride=R, rec_off=4 + 2 * D)
    clib.check(libssnode.ssn_ens_apply_f32(ctypes.byref(o), _stream()), 'ssn_ens_apply_f32')
    for k, lr in enumerate(lrs):
        q, m1, m2 = p0[k].clone(), torch.zeros(P, **f), torch.zeros(P, **f)
        op = clib.OptParams(kind=1, step=1, clip=1, reserved=0, learning_rate=lr, beta1=0.5, beta2=0.9, epsilon=1e-8, rho=0.9,
                            reg_l2_penalty=0.0, reg_l1_penalty=0.0, reg_l2_decay=0.0, reg_l1_decay=0.0, clip_lo=0.05, clip_hi=0.9)
        gk = grads[k].contiguous()
        clib.check(libssnode.ssn_optimizer_step(q.data_ptr(), gk.data_ptr(), m1.data_ptr(), m2.data_ptr(), P, ctypes.byref(op),
                                                _stream()), 'ssn_optimizer_step')
        torch.testing.assert_close(p[k], q, rtol=0, atol=0, equal_nan=True)
        torch.testing.assert_close(rec[k, 4 + 2 * D:4 + 2 * D + P].float(), q, rtol=0, atol=0, equal_nan=True)
        assert torch.isfinite(p[k]).all() == (k != 0)


def test_segmented_stimulus_and_jds_grad_match_single_run_kernels():
    from tc_gan_amd import genops
    K, B, NB, N = 3, 2, 4, 10
    M = 2 * N
    g = torch.Generator().manual_seed(2)
    bw = torch.rand((K * B, NB), generator=g).cuda()
    con = torch.full((K * B, NB), 20.0).cuda()
    zin = (torch.randint(0, 2, (K * B, M), generator=g).float() * 2 - 1).cuda()
    v = torch.rand((K, 2), generator=g).cuda()
    ext = torch.empty((K * B, NB, M), device='cuda')
    clib.check(libssnode.ssn_ens_stimulus_hetero_f32(bw.data_ptr(), con.data_ptr(), 0.01, zin.data_ptr(), v.data_ptr(),
                                                     ext.data_ptr(), K, B, NB, N, _stream()), 'ssn_ens_stimulus_hetero_f32')
    for k in range(K):
        sl = slice(k * B, (k + 1) * B)
        one = torch.empty((B, NB, M), device='cuda')
        vk = v[k].contiguous()
        clib.check(libssnode.ssn_stimulus_hetero_f32(bw[sl].contiguous().data_ptr(), con[sl].contiguous().data_ptr(), 0.01,
                                                     zin[sl].contiguous().data_ptr(), vk.data_ptr(), 2, one.data_ptr(), B, NB, N,
                                                     _stream()), 'ssn_stimulus_hetero_f32')
        torch.testing.assert_close(ext[sl], one, rtol=0, atol=0)
    gW = torch.rand((K * B, M, M), generator=g).cuda()
    z = torch.rand((K * B, M, M), generator=g).cuda()
    gW[B, 3, 4] = float('nan')
    jds = [(np.full(4, 0.01 + k * 0.003), np.full(4, 0.2 + 0.1 * k), np.full(4, 0.1 + 0.05 * k)) for k in range(K)]
    from tc_gan_amd.networks.moment_matching_ensemble import _jds16
    p16 = torch.as_tensor(np.stack([_jds16(*t) for t in jds])).cuda()
    out = torch.empty((K * B, 4, 3), device='cuda', dtype=torch.float64)
    clib.check(libssnode.ssn_ens_jds_grad_f32(gW.data_ptr(), z.data_ptr(), p16.data_ptr(), out.data_ptr(), K, B, N, _stream()),
               'ssn_ens_jds_grad_f32')
    for k in range(K):
        sl = slice(k * B, (k + 1) * B)
        want = genops.jds_grad_parts(gW[sl].contiguous(), z[sl].contiguous(), *jds[k])
        torch.testing.assert_close(out[sl], want, rtol=0, atol=0, equal_nan=True)
        assert torch.isfinite(out[sl]).all() == (k != 1)

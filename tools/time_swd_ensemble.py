"""Time the sliced Wasserstein ensemble against the single-run loop at one shape (default: the sweep's -- num_sites 101,
batchsize 32, 8 stimuli, seqlen 240, skip_steps 200, deg-heteroin, 128 directions), warmed, in one process, the single loop
alternated with the ensembles.

    python tools/time_swd_ensemble.py [--members 1,2,4,8,16] [--steps 20] [--warmup 3] [--rounds 2] [--out FILE]
    python tools/time_swd_ensemble.py --match-only [--match-members 8,42] [--calls 50]

Prints one line per K and round: ms per ensemble step, member-steps per second and their ratio to the single loop of the same
round, the kernel that ran.  --match-only launches `ssn_ens_swd_match_f32` alone, --calls times in each form at B = 32, L = 128
(for a kernel trace: the kernel times are read from the profiler's statistics, the host times printed here include the launch)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tc_gan_amd import clib  # noqa: E402
from tc_gan_amd.networks.sliced_wasserstein import make_sliced_wasserstein  # noqa: E402
from tc_gan_amd.networks.sliced_wasserstein_ensemble import make_sliced_wasserstein_ensemble  # noqa: E402
from tc_gan_amd.run.bptt_wgan import preprocess  # noqa: E402
from tc_gan_amd.utils import Namespace, StopWatch  # noqa: E402

SHAPE = dict(num_sites=101, batchsize=32, n_bandwidths=8, contrasts=[20], seqlen=240, skip_steps=200, ssn_type='deg-heteroin',
             tau_E=2, dynamics_cost=0, rate_cost=1, sample_sites=[0, 0.125, 0.25, 0.5, 0.75], include_inhibitory_neurons=False,
             J0=0.01, D0=0.01, S0=0.01, load_gen_param=None, V0=0.1, swd_directions=128)


def shared_config(kernel):
    from tc_gan_amd.run import options
    cfg = vars(options.build_parser('s', '').parse_args([]))
    for key in ('datastore', 'datastore_template', 'load_config', 'iterations', 'quiet'):
        cfg.pop(key)
    cfg.update(SHAPE, gen_kernel=kernel)
    preprocess(cfg)
    return cfg


def fake_data(swd, n=64, seed=0):
    return np.random.RandomState(seed).rand(n, swd.num_mom_conds) + 0.5


def timed(step, steps, warmup, first):
    for s in range(first, first + warmup):
        step(s)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(first + warmup, first + warmup + steps):
        step(s)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def time_match(members, calls, B=32, L=128):
    rows = []
    g = torch.Generator().manual_seed(0)
    for K in members:
        px, py = torch.randn((K * B, L), generator=g).cuda(), torch.randn((K * B, L), generator=g).cuda()
        coef = torch.empty_like(px)
        loss_l = torch.empty((K, L), device='cuda', dtype=torch.float64)
        l0 = torch.empty((K,), device='cuda', dtype=torch.float64)
        power = (ctypes.c_int * K)(*[1 + k % 2 for k in range(K)])
        for form, name in ((clib.SWD_FORM_GENERAL, 'general'), (clib.SWD_FORM_WAVE, 'wave')) * 2:      # alternated
            def call():
                clib.check(clib.libssnode.ssn_ens_swd_match_f32(px.data_ptr(), py.data_ptr(), power, K, B, L, form, coef.data_ptr(),
                                                                loss_l.data_ptr(), l0.data_ptr(), clib.stream_ptr()), 'match')
            sec = timed(lambda s: call(), calls, 5, 0)
            rows.append(dict(K=K, B=B, L=L, form=name, host_us_per_call=1e6 * sec))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', default='1,2,4,8,16')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=2, help='times the whole list (single loop, then every K) is gone through')
    ap.add_argument('--gen-kernel', default='auto')
    ap.add_argument('--match-only', action='store_true')
    ap.add_argument('--match-members', default='8,42')
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--out', help='also write the rows to this JSON file')
    ns = ap.parse_args()
    if ns.match_only:
        rows = time_match([int(k) for k in ns.match_members.split(',')], ns.calls)
    else:
        rows = []
        swd, _ = make_sliced_wasserstein(shared_config(ns.gen_kernel))
        swd.set_dataset(fake_data(swd))
        swd.train_watch = StopWatch()
        kern = swd.gen.gen_kernel if swd.gen.gen_kernel != 'auto' else 'auto(variant {})'.format(swd.gen.forward_variant(save=True))
        members = [int(k) for k in ns.members.split(',')]
        ensembles = {}
        for K in members:
            ens = make_sliced_wasserstein_ensemble(shared_config(ns.gen_kernel),
                                                   [dict(seed=i, learning_rate=1e-3 * (1 + i), swd_power=1 + i % 2, swd_direction_seed=i)
                                                    for i in range(K)])
            for member in ens.members:
                member.set_dataset(fake_data(member))
            ensembles[K] = ens
        per = ns.steps + ns.warmup
        for r in range(ns.rounds):
            solo = timed(lambda s: swd.train_generator(Namespace(step=s)), ns.steps, ns.warmup, r * per)
            rows.append(dict(round=r, K='solo', ms_per_step=1e3 * solo, member_steps_per_s=1.0 / solo, vs_solo=1.0, kernel=kern))
            print(json.dumps(rows[-1]), flush=True)
            for K in members:
                sec = timed(ensembles[K].train_step, ns.steps, ns.warmup, r * per)
                rows.append(dict(round=r, K=K, ms_per_step=1e3 * sec, member_steps_per_s=K / sec, vs_solo=K * solo / sec,
                                 kernel=ensembles[K].gen_kernel))
                print(json.dumps(rows[-1]), flush=True)
    if ns.out:
        with open(ns.out, 'w') as f:
            json.dump(rows, f)


if __name__ == '__main__':
    main()

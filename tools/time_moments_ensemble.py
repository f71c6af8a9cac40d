"""Time the moment-matching ensemble against the single-run loop at one shape (default: a Fig. 6 MM run -- num_sites 101,
batchsize 32, 8 stimuli, seqlen 240, skip_steps 200, deg-heteroin).

    python tools/time_moments_ensemble.py [--members 1,2,4,8,16] [--steps 20] [--warmup 3] [--out FILE]

Prints one line per K: ms per ensemble step, member-steps per second, the kernel that ran; and the single run's loop first."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tc_gan_amd.networks.moment_matching import make_moment_matcher  # noqa: E402
from tc_gan_amd.networks.moment_matching_ensemble import make_moment_matcher_ensemble  # noqa: E402
from tc_gan_amd.run.bptt_wgan import preprocess  # noqa: E402
from tc_gan_amd.utils import Namespace, StopWatch  # noqa: E402

SHAPE = dict(num_sites=101, batchsize=32, n_bandwidths=8, contrasts=[20], seqlen=240, skip_steps=200, ssn_type='deg-heteroin',
             tau_E=2, dynamics_cost=0, rate_cost=1, lam=1.0, moment_weight_type='ew_relative', sample_sites=[0, 0.125, 0.25, 0.5, 0.75],
             include_inhibitory_neurons=False, J0=0.01, D0=0.01, S0=0.01, load_gen_param=None, V0=0.1)


def shared_config(kernel):
    from tc_gan_amd.run import options
    cfg = vars(options.build_parser('m', '').parse_args([]))
    for key in ('datastore', 'datastore_template', 'load_config', 'iterations', 'quiet', 'gen_moments_record_interval'):
        cfg.pop(key)
    cfg.update(SHAPE, gen_kernel=kernel)
    preprocess(cfg)
    return cfg


def fake_data(mm, n=64, seed=0):
    return np.random.RandomState(seed).rand(n, mm.num_mom_conds) + 0.5


def timed(step, steps, warmup):
    for s in range(warmup):
        step(s)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(warmup, warmup + steps):
        step(s)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', default='1,2,4,8,16')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--gen-kernel', default='auto')
    ap.add_argument('--out', help='also write the rows to this JSON file')
    ns = ap.parse_args()
    rows = []
    mm, _ = make_moment_matcher(shared_config(ns.gen_kernel))
    mm.set_dataset(fake_data(mm))
    mm.train_watch = StopWatch()
    sec = timed(lambda s: mm.train_generator(Namespace(step=s)), ns.steps, ns.warmup)
    kern = mm.gen.gen_kernel if mm.gen.gen_kernel != 'auto' else 'auto(variant {})'.format(mm.gen.forward_variant(save=True))
    rows.append(dict(K='solo', ms_per_step=1e3 * sec, member_steps_per_s=1.0 / sec, kernel=kern))
    print(json.dumps(rows[-1]), flush=True)
    for K in [int(k) for k in ns.members.split(',')]:
        ens = make_moment_matcher_ensemble(shared_config(ns.gen_kernel), [dict(seed=i, learning_rate=1e-3 * (1 + i)) for i in range(K)])
        for mmk in ens.members:
            mmk.set_dataset(fake_data(mmk))
        sec = timed(ens.train_step, ns.steps, ns.warmup)
        rows.append(dict(K=K, ms_per_step=1e3 * sec, member_steps_per_s=K / sec, kernel=ens.gen_kernel))
        print(json.dumps(rows[-1]), flush=True)
    if ns.out:
        with open(ns.out, 'w') as f:
            json.dump(rows, f)


if __name__ == '__main__':
    main()

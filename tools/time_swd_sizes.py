"""Time a sliced Wasserstein generator step at several sizes of the truth minibatch (--swd-truth-batch): one trainer per size in
one process, warmed, alternating, `--windows` timed windows each (a host clock around steps that end in a device synchronise).
The size 0 is the rank matching against `batchsize` truth rows, the path a run without the option takes.

    python tools/time_swd_sizes.py [--shape default|large] [--steps 20] [--warmup 3] [--windows 3] [--out FILE]
    python tools/time_swd_sizes.py --shape large --one-step        (one warmed step of each size, for a kernel trace)
    python tools/time_swd_sizes.py --spread                        (the loss's spread over truth minibatches at fixed x)

Shapes as tools/time_swd.py's: default -- the run scripts' defaults (2N = 204, batchsize 15), sizes 0, 960 and -1 (a truth of
1000 rows); large -- batchsize 1024, 2N = 200, 8 bandwidths, sizes 0, 4096 and 16384.  --spread: one batch of
tuning curves (B = 15, the generator shape of the seeded learning test) against 20 truth minibatches of B and of 64 B rows; the
standard deviation of the recorded swd over the minibatches.  Prints one JSON line per window and a summary line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from time_swd import config, window  # noqa: E402
from tc_gan_amd.networks.sliced_wasserstein import make_sliced_wasserstein, swd_loss_grad  # noqa: E402
from tc_gan_amd.utils import StopWatch  # noqa: E402

SIZES = {'default': (0, 960, -1), 'large': (0, 4096, 16384)}
TRUTH_ROWS = {'default': 1000, 'large': 16384}


def learners(shape):
    out = {}
    for size in SIZES[shape]:
        swd, rest = make_sliced_wasserstein(dict(config('s', shape), swd_truth_batch=size))
        assert not rest, rest
        swd.set_dataset(np.random.RandomState(0).rand(TRUTH_ROWS[shape], swd.num_mom_conds) + 0.5)
        swd.train_watch = StopWatch()
        out[size] = swd
    return out


def spread(minibatches=20, factor=64, B=15):
    """Standard deviation of swd over truth minibatches of B and of factor B rows, at fixed generated rows x.  Generator shape
    of the seeded learning test (2N = 40, 8 bandwidths, 200 steps of dynamics); the truth is minibatches x factor x B rows of the
    fixed-time provider at the default (J, D, S), x one batch of B draws at the same parameters on another noise stream."""
    from tc_gan_amd.networks.dataset import dataset_by_fixedtime
    from tc_gan_amd.networks.fixed_time_sampler import FixedTimeTuningCurveSampler, new_JDS
    true = {k: np.asarray(new_JDS[k], dtype=float) for k in 'JDS'}
    swd, _ = make_sliced_wasserstein(dict(
        num_sites=20, seqlen=200, skip_steps=150, batchsize=B, sample_sites=[0], include_inhibitory_neurons=False,
        bandwidths=[0, 0.0625, 0.125, 0.1875, 0.25, 0.5, 0.75, 1], contrasts=[20.], J0=true['J'], D0=true['D'], S0=true['S']))
    truth = dataset_by_fixedtime(swd, truth_size=minibatches * factor * B, truth_seed=42, truth_batchsize=factor * B, true_ssn_options=true)
    truth = torch.as_tensor(np.ascontiguousarray(truth, dtype='float32')).to('cuda')
    x = FixedTimeTuningCurveSampler.from_learner(swd, batchsize=B, seed=7, **true).forward().prober_tuning_curve
    x = x.to(torch.float32).contiguous()
    theta = swd.next_directions(x.shape[1])
    out = dict(batchsize=B, minibatches=minibatches, directions=int(theta.shape[0]), power=swd.swd_power)
    for name, M in (('M_equals_B', B), ('M_equals_{}_B'.format(factor), factor * B)):
        vals = [swd_loss_grad(x, truth[k * M:(k + 1) * M].contiguous(), theta, swd.swd_power, unequal=True)[1]
                for k in range(minibatches)]
        out[name] = dict(rows=M, mean=float(np.mean(vals)), std=float(np.std(vals, ddof=1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='default', choices=sorted(SIZES))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--one-step', action='store_true', help='warm up, then one step at each size and nothing else')
    ap.add_argument('--spread', action='store_true', help='the spread of the loss over truth minibatches instead of step times')
    ap.add_argument('--out', help='also write the rows to this JSON file')
    ns = ap.parse_args()
    if ns.spread:
        result = spread()
        print(json.dumps(result), flush=True)
        if ns.out:
            with open(ns.out, 'w') as f:
                json.dump(result, f)
        return
    every = learners(ns.shape)
    for swd in every.values():
        window(swd, 0, ns.warmup)
    if ns.one_step:
        for size, swd in every.items():
            print(json.dumps(dict(shape=ns.shape, swd_truth_batch=size, ms_per_step=1e3 * window(swd, ns.warmup, 1))), flush=True)
        return
    rows = []
    for w in range(ns.windows):
        for size, swd in every.items():
            sec = window(swd, ns.warmup + w * ns.steps, ns.steps)
            rows.append(dict(shape=ns.shape, swd_truth_batch=size, window=w, ms_per_step=1e3 * sec))
            print(json.dumps(rows[-1]), flush=True)
    summary = dict(shape=ns.shape, steps=ns.steps, truth_rows=TRUTH_ROWS[ns.shape])
    for size in every:
        ms = [r['ms_per_step'] for r in rows if r['swd_truth_batch'] == size]
        summary[str(size)] = dict(median_ms=float(np.median(ms)), min_ms=min(ms), max_ms=max(ms))
    print(json.dumps(summary), flush=True)
    if ns.out:
        with open(ns.out, 'w') as f:
            json.dump(dict(rows=rows, summary=summary), f)


if __name__ == '__main__':
    main()

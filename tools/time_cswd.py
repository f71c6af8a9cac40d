"""Time a conditional sliced Wasserstein generator step (tc_gan.run.bptt_cswd) against an unconditional one on the whole truth
(tc_gan.run.bptt_swd --swd-truth-batch -1) of equal stimulus solves: the two trainers alternate in one process, warmed,
`--windows` timed windows each (a host clock around steps that end in a device synchronise).

    python tools/time_cswd.py [--shape default|large] [--truth 1000] [--steps 20] [--warmup 3] [--windows 3] [--out FILE]
    python tools/time_cswd.py --shape large --truth 16384 --one-step      (one warmed step of each, for a kernel trace)

Shapes: default -- the run scripts' defaults (2N = 204, 15 models, 4 bandwidths, one contrast, one probe: one cell; the
unconditional trainer at batchsize 15); large -- 2N = 200, 8 bandwidths, two contrasts, two probes: 1024 models with both probes
each and one contrast each (2048 rows in 4 cells, 8192 solves) against batchsize 512 with both contrasts (512 rows of 32
columns, 8192 solves).  --truth: rows of the truth (per cell for the conditional trainer).  Prints one JSON line per window and
a summary line with the medians and the spread."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from time_swd import _DRIVER_KEYS, window  # noqa: E402
from tc_gan_amd.networks.conditional_sliced_wasserstein import make_conditional_sliced_wasserstein  # noqa: E402
from tc_gan_amd.networks.sliced_wasserstein import make_sliced_wasserstein  # noqa: E402
from tc_gan_amd.run import options  # noqa: E402
from tc_gan_amd.run.bptt_wgan import preprocess  # noqa: E402
from tc_gan_amd.utils import StopWatch  # noqa: E402

_LARGE = dict(num_sites=100, n_bandwidths=8, contrasts=[5., 20.])
SHAPES = {'default': dict(k=dict(), s=dict(swd_truth_batch=-1)),
          'large': dict(k=dict(_LARGE, num_models=1024, probes_per_model=2, norm_probes=[0, 0.5]),
                        s=dict(_LARGE, batchsize=512, sample_sites=[0, 0.5], swd_truth_batch=-1))}


def config(script, shape):
    cfg = vars(options.build_parser(script, '').parse_args([]))
    for key in _DRIVER_KEYS:
        cfg.pop(key, None)
    for key in ('J0', 'D0', 'S0'):                                # (preprocess then takes ssnode's default parameters)
        cfg.pop(key)
    cfg.update(SHAPES[shape][script])
    preprocess(cfg)
    cfg.pop('true_ssn_options')
    return cfg


def learners(shape, truth_rows):
    cond, rest = make_conditional_sliced_wasserstein(config('k', shape))
    assert not rest, rest
    plain, rest = make_sliced_wasserstein(config('s', shape))
    assert not rest, rest
    cells = (2 if cond.include_inhibitory_neurons else 1) * len(cond.norm_probes) * len(cond.contrasts)
    columns = cells * len(cond.bandwidths)
    assert columns == plain.num_mom_conds
    data = np.random.RandomState(0).rand(truth_rows, columns) + 0.5
    for learner in (cond, plain):
        learner.set_dataset(data)
        learner.train_watch = StopWatch()
    return dict(cswd=cond, swd=plain)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='default', choices=sorted(SHAPES))
    ap.add_argument('--truth', type=int, default=1000, help='rows of the truth')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--one-step', action='store_true', help='warm up, then one step of each trainer and nothing else')
    ap.add_argument('--out', help='also write the rows to this JSON file')
    ns = ap.parse_args()
    both = learners(ns.shape, ns.truth)
    for name in ('cswd', 'swd'):
        window(both[name], 0, ns.warmup)
    if ns.one_step:
        for name in ('cswd', 'swd'):
            print(json.dumps(dict(shape=ns.shape, truth=ns.truth, trainer=name,
                                  ms_per_step=1e3 * window(both[name], ns.warmup, 1))), flush=True)
        return
    rows = []
    for w in range(ns.windows):
        for name in ('cswd', 'swd'):
            sec = window(both[name], ns.warmup + w * ns.steps, ns.steps)
            rows.append(dict(shape=ns.shape, truth=ns.truth, trainer=name, window=w, ms_per_step=1e3 * sec))
            print(json.dumps(rows[-1]), flush=True)
    summary = dict(shape=ns.shape, truth=ns.truth, steps=ns.steps)
    for name in ('cswd', 'swd'):
        ms = [r['ms_per_step'] for r in rows if r['trainer'] == name]
        summary[name] = dict(median_ms=float(np.median(ms)), min_ms=min(ms), max_ms=max(ms))
    print(json.dumps(summary), flush=True)
    if ns.out:
        with open(ns.out, 'w') as f:
            json.dump(dict(rows=rows, summary=summary), f)


if __name__ == '__main__':
    main()

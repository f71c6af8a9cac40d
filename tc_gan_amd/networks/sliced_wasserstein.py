"""BPTT training of the SSN tuning-curve generator by the sliced Wasserstein distance: no critic.

Every step the minibatch of generated tuning curves x (B, D) and a minibatch y (B, D) of the truth are projected on L fresh
random unit directions (``ssn_project_rows_f32``); per direction the two columns are sorted and matched rank by rank
(``ssn_swd_match_f32``: the loss per direction and the coefficient of every projection), and the coefficients go back to the rows
(``ssn_swd_backproject_f32``: the gradient `gx` the adjoint sweep starts from).  With power 1 the recorded loss is the mean over
the directions of the W1 of the projections -- the unit of ``analyzers/distdiff.py --wasserstein``'s ``sliced_w1`` -- with power 2
the mean of their squared W2.  Forward, adjoint sweep, penalties and update are the moment matcher's
(`moment_matching.GeneratorStepTrainer`); the definitions are in include/ssnode_mi355x.h and DESIGN 3.11c.
"""
import os

import numpy as np
import torch

from .. import clib
from ..analyzers.distdiff import draw_slice_directions
from ..clib import libssnode
from ..utils import random_minibatches
from .moment_matching import DEFAULT_PARAMS as _MM_DEFAULTS, GeneratorStepTrainer, generator_step_parts

DEFAULT_PARAMS = dict(_MM_DEFAULTS, swd_directions=128, swd_power=2, swd_direction_seed=0)
del DEFAULT_PARAMS['moment_weight_type']

SWD_POWERS = (1, 2)


def swd_loss_grad(x, y, theta, power):
    """x, y (B, D), theta (L, D): device float32, contiguous -> (gx (B, D) device float32, loss, loss_l (L,) numpy fp64).
    Four launches (two projections, the match, the back-projection) and one read of the L doubles; the mean over the directions
    is formed on the host, in index order."""
    B, D = x.shape
    L = theta.shape[0]
    if tuple(y.shape) != (B, D) or theta.shape[1] != D or not (x.is_contiguous() and y.is_contiguous() and theta.is_contiguous()):
        raise ValueError('swd_loss_grad: x, y (B, D) and theta (L, D) must be contiguous, got {}, {} and {}'
                         .format(tuple(x.shape), tuple(y.shape), tuple(theta.shape)))
    stream = clib.stream_ptr()
    px = torch.empty((2, B, L), device=x.device, dtype=torch.float32)
    for src, dst in ((x, px[0]), (y, px[1])):
        clib.check(libssnode.ssn_project_rows_f32(src.data_ptr(), B, D, D, theta.data_ptr(), L, dst.data_ptr(), stream),
                   'ssn_project_rows_f32')
    coef = torch.empty((B, L), device=x.device, dtype=torch.float32)
    loss_l = torch.empty(L, device=x.device, dtype=torch.float64)
    clib.check(libssnode.ssn_swd_match_f32(px[0].data_ptr(), px[1].data_ptr(), B, L, int(power), coef.data_ptr(),
                                           loss_l.data_ptr(), stream), 'ssn_swd_match_f32')
    gx = torch.empty((B, D), device=x.device, dtype=torch.float32)
    clib.check(libssnode.ssn_swd_backproject_f32(coef.data_ptr(), theta.data_ptr(), B, L, D, gx.data_ptr(), stream),
               'ssn_swd_backproject_f32')
    host = loss_l.cpu().numpy()
    return gx, float(np.cumsum(host)[-1] / L), host           # (cumsum: the sequential sum)


class BPTTSlicedWasserstein(GeneratorStepTrainer):
    """The critic-free trainer: `set_dataset(data)`, then `learning()` yields one `info` per generator update -- step, loss
    (with the penalties), swd (the bare sliced loss), dynamics_penalty, rate_penalty, train_time."""

    def __init__(self, gen, gen_updaters, bandwidths, contrasts, swd_directions, swd_power, swd_direction_seed,
                 include_inhibitory_neurons, rate_penalty_threshold, dynamics_cost, rate_cost, param_bounds, seed=0):
        if swd_power not in SWD_POWERS:
            raise ValueError('swd_power must be 1 or 2, got {!r}'.format(swd_power))
        if not 1 <= int(swd_directions) <= clib.W1_MAX_DIRECTIONS:
            raise ValueError('swd_directions = {} is not in 1 .. {}'.format(swd_directions, clib.W1_MAX_DIRECTIONS))
        if gen.batchsize > clib.SWD_MAX_BATCH:
            raise ValueError('batchsize = {} is more than the {} rows the match kernel sorts'.format(gen.batchsize, clib.SWD_MAX_BATCH))
        self.swd_directions, self.swd_power = int(swd_directions), int(swd_power)
        # the directions and the minibatch shuffles have streams of their own, both seeded by `swd_direction_seed`: the
        # reference's noise stream on self.rng is not disturbed (the same seed gives the moment matcher's z)
        self.direction_rng = np.random.RandomState(swd_direction_seed)
        self.minibatch_rng = np.random.RandomState(swd_direction_seed)
        self.last_x = self.last_gx = None        # the tuning curves and the loss gradient of the last step, on the device
        self._init_generator_step(gen, gen_updaters, bandwidths, contrasts, include_inhibitory_neurons,
                                  rate_penalty_threshold, dynamics_cost, rate_cost, param_bounds, seed)

    def set_dataset(self, data, **kwargs):
        """The truth stays on the device; the minibatches are rows of it in the order of `utils.random_minibatches` (as
        `BPTTWassersteinGAN.set_dataset` takes them, but shuffled on `minibatch_rng`)."""
        kwargs.setdefault('seed', self.minibatch_rng)
        data = np.ascontiguousarray(data, dtype='float32')
        self.truth = torch.as_tensor(data).to('cuda')
        # (an ensemble takes the row indices themselves from `minibatch_rows`, one gather for all its members)
        self.minibatch_rows = rows = random_minibatches(self.gen.batchsize, np.arange(len(data)), **kwargs)
        self.dataset = (self.truth[torch.as_tensor(idx).to('cuda')] for idx in rows)

    def next_minibatch(self):
        return next(self.dataset)

    def next_directions(self, columns):
        return torch.as_tensor(draw_slice_directions(self.direction_rng, self.swd_directions, columns)).to('cuda')

    def swd_loss_grad(self, x, y, theta):
        """x, y (B, D), theta (L, D) device float32 -> (gx, loss, loss_l)."""
        return swd_loss_grad(x, y, theta, self.swd_power)

    def train_generator(self, info):
        def loss_grad(x):
            self.last_x = x = x.to(torch.float32).contiguous()
            y = self.next_minibatch()
            self.last_gx, info.swd, info.swd_per_direction = self.swd_loss_grad(x, y, self.next_directions(x.shape[1]))
            return self.last_gx, info.swd
        with self.train_watch:
            self.generator_step(info, loss_grad)
        info.train_time = self.train_watch.sum()
        return info


def make_sliced_wasserstein(config):
    """make_sliced_wasserstein(config: dict) -> (BPTTSlicedWasserstein, dict of unconsumed config)."""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world > 1:
        raise ValueError('the sliced Wasserstein trainer runs on one GPU: the match kernel needs whole columns of the projections, '
                         'and the all-gather that would give them to every rank is not built (WORLD_SIZE = {})'.format(world))
    kwargs = dict(DEFAULT_PARAMS, **config)
    parts = generator_step_parts(kwargs)
    swd = BPTTSlicedWasserstein(swd_directions=kwargs.pop('swd_directions'), swd_power=kwargs.pop('swd_power'),
                                swd_direction_seed=kwargs.pop('swd_direction_seed'), **parts)
    return swd, kwargs

"""BPTT training of the SSN tuning-curve generator by the sliced Wasserstein distance: no critic.

Every step the minibatch of generated tuning curves x (B, D) and a minibatch y (B, D) of the truth are projected on L fresh
random unit directions (``ssn_project_rows_f32``); per direction the two columns are sorted and matched rank by rank
(``ssn_swd_match_f32``: the loss per direction and the coefficient of every projection), and the coefficients go back to the rows
(``ssn_swd_backproject_f32``: the gradient `gx` the adjoint sweep starts from).  With ``swd_truth_batch`` the truth minibatch has
a size M of its own -- a generated row costs a forward and an adjoint sweep, a truth row one projection -- and the match is the
quantile coupling of ``ssnx_swd_match_sizes_f32`` (include/ssnode_mi355x_ext.h).  With power 1 the recorded loss is the mean over
the directions of the W1 of the projections -- the unit of ``analyzers/distdiff.py --wasserstein``'s ``sliced_w1`` -- with power 2
the mean of their squared W2.  Forward, adjoint sweep, penalties and update are the moment matcher's
(`moment_matching.GeneratorStepTrainer`); the definitions are in include/ssnode_mi355x.h and DESIGN 3.11c.
"""
import itertools
import os

import numpy as np
import torch

from .. import clib
from ..analyzers.distdiff import draw_slice_directions
from ..clib import libssnode
from ..utils import random_minibatches
from .moment_matching import DEFAULT_PARAMS as _MM_DEFAULTS, GeneratorStepTrainer, generator_step_parts

DEFAULT_PARAMS = dict(_MM_DEFAULTS, swd_directions=128, swd_power=2, swd_direction_seed=0, swd_truth_batch=0)
del DEFAULT_PARAMS['moment_weight_type']

SWD_POWERS = (1, 2)
#: `swd_truth_batch`: the truth minibatch is `batchsize` rows (the rank matching) / is the whole truth every step
SWD_TRUTH_BATCHSIZE, SWD_TRUTH_ALL = 0, -1


def swd_loss_grad(x, y, theta, power, unequal=False):
    """x (B, D), y (M, D), theta (L, D): device float32, contiguous -> (gx (B, D) device float32, loss, loss_l (L,) numpy fp64).
    Four launches (two projections, the match, the back-projection) and one read of the L doubles; the mean over the directions
    is formed on the host, in index order.  M == B: the rank matching of `ssn_swd_match_f32`.  M != B is taken only with
    `unequal=True` (a truth minibatch of another size is a decision, not a slip of shapes): the quantile coupling of
    `ssnx_swd_match_sizes_f32` in the companion library; projections and back-projection are the same calls."""
    B, D = x.shape
    L = theta.shape[0]
    M = y.shape[0] if y.dim() == 2 else -1
    if M < 0 or y.shape[1] != D or (M != B and not unequal) or theta.shape[1] != D or \
            not (x.is_contiguous() and y.is_contiguous() and theta.is_contiguous()):
        raise ValueError('swd_loss_grad: x, y (B, D) and theta (L, D) must be contiguous, got {}, {} and {}{}'
                         .format(tuple(x.shape), tuple(y.shape), tuple(theta.shape),
                                 '' if unequal else ' (y of another row count needs unequal=True)'))
    if M != B and not 1 <= M <= clib.SWD_MAX_TRUTH:
        raise ValueError('swd_loss_grad: {} truth rows are not in 1 .. {} (clib.SWD_MAX_TRUTH)'.format(M, clib.SWD_MAX_TRUTH))
    stream = clib.stream_ptr()
    px = torch.empty((B, L), device=x.device, dtype=torch.float32)
    py = torch.empty((M, L), device=x.device, dtype=torch.float32)
    for src, rows, dst in ((x, B, px), (y, M, py)):
        clib.check(libssnode.ssn_project_rows_f32(src.data_ptr(), rows, D, D, theta.data_ptr(), L, dst.data_ptr(), stream),
                   'ssn_project_rows_f32')
    coef = torch.empty((B, L), device=x.device, dtype=torch.float32)
    loss_l = torch.empty(L, device=x.device, dtype=torch.float64)
    if M == B:
        clib.check(libssnode.ssn_swd_match_f32(px.data_ptr(), py.data_ptr(), B, L, int(power), coef.data_ptr(),
                                               loss_l.data_ptr(), stream), 'ssn_swd_match_f32')
    else:
        clib.check_ext(clib.libssnode_ext.ssnx_swd_match_sizes_f32(px.data_ptr(), B, py.data_ptr(), M, L, int(power),
                                                                  coef.data_ptr(), loss_l.data_ptr(), stream),
                       'ssnx_swd_match_sizes_f32')
    gx = torch.empty((B, D), device=x.device, dtype=torch.float32)
    clib.check(libssnode.ssn_swd_backproject_f32(coef.data_ptr(), theta.data_ptr(), B, L, D, gx.data_ptr(), stream),
               'ssn_swd_backproject_f32')
    host = loss_l.cpu().numpy()
    return gx, float(np.cumsum(host)[-1] / L), host           # (cumsum: the sequential sum)


def checked_truth_batch(value):
    """`swd_truth_batch` as an int, or a ValueError that names it."""
    if isinstance(value, bool) or int(value) != value or not SWD_TRUTH_ALL <= value <= clib.SWD_MAX_TRUTH:
        raise ValueError('swd_truth_batch = {!r} is not 0 (batchsize rows), -1 (the whole truth) or a row count up to {} '
                         '(clib.SWD_MAX_TRUTH)'.format(value, clib.SWD_MAX_TRUTH))
    return int(value)


def truth_minibatch_rows(swd_truth_batch, batchsize, truth_rows, **kwargs):
    """The row indices of the truth minibatches, one array per step, by the three meanings of `swd_truth_batch`: 0 --
    `utils.random_minibatches(batchsize, ...)`, the stream of a run without the option; M > 0 -- the same with M rows; -1 --
    None: every minibatch is the whole truth, no shuffle is drawn, and `batchsize` may exceed the truth's rows."""
    if swd_truth_batch == SWD_TRUTH_ALL:
        if not 1 <= truth_rows <= clib.SWD_MAX_TRUTH:
            raise ValueError('swd_truth_batch = -1: the truth has {} rows, the match takes 1 .. {} (clib.SWD_MAX_TRUTH)'
                             .format(truth_rows, clib.SWD_MAX_TRUTH))
        return None
    if swd_truth_batch > truth_rows:
        raise ValueError('swd_truth_batch = {} > truth rows = {}; use -1 for the whole truth every step'
                         .format(swd_truth_batch, truth_rows))
    return random_minibatches(swd_truth_batch or batchsize, np.arange(truth_rows), **kwargs)


class BPTTSlicedWasserstein(GeneratorStepTrainer):
    """The critic-free trainer: `set_dataset(data)`, then `learning()` yields one `info` per generator update -- step, loss
    (with the penalties), swd (the bare sliced loss), dynamics_penalty, rate_penalty, train_time.  `swd_truth_batch` (set before
    `set_dataset`; `make_sliced_wasserstein` sets it from the config) is the size of the truth minibatch: 0 -- `batchsize` rows,
    -1 -- the whole truth every step, M -- M rows."""
    #: (an attribute and not a constructor argument: the constructor's call is recorded argument by argument)
    swd_truth_batch = SWD_TRUTH_BATCHSIZE

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
        """The truth stays on the device; the minibatches are rows of it in the order of `truth_minibatch_rows` (as
        `BPTTWassersteinGAN.set_dataset` takes them, but shuffled on `minibatch_rng`)."""
        kwargs.setdefault('seed', self.minibatch_rng)
        data = np.ascontiguousarray(data, dtype='float32')
        # (an ensemble takes the row indices themselves from `minibatch_rows`, one gather for all its members)
        self.minibatch_rows = rows = truth_minibatch_rows(self.swd_truth_batch, self.gen.batchsize, len(data), **kwargs)
        self.truth = torch.as_tensor(data).to('cuda')
        if rows is None:
            self.dataset = itertools.repeat(self.truth)
        else:
            self.dataset = (self.truth[torch.as_tensor(idx).to('cuda')] for idx in rows)

    def next_minibatch(self):
        return next(self.dataset)

    def next_directions(self, columns):
        return torch.as_tensor(draw_slice_directions(self.direction_rng, self.swd_directions, columns)).to('cuda')

    def swd_loss_grad(self, x, y, theta):
        """x (B, D), y (B, D) -- or (M, D) under `swd_truth_batch` --, theta (L, D) device float32 -> (gx, loss, loss_l)."""
        return swd_loss_grad(x, y, theta, self.swd_power, unequal=self.swd_truth_batch != SWD_TRUTH_BATCHSIZE)

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
    truth_batch = checked_truth_batch(kwargs.pop('swd_truth_batch'))      # (refused before the generator is built)
    parts = generator_step_parts(kwargs)
    swd = BPTTSlicedWasserstein(swd_directions=kwargs.pop('swd_directions'), swd_power=kwargs.pop('swd_power'),
                                swd_direction_seed=kwargs.pop('swd_direction_seed'), **parts)
    swd.swd_truth_batch = truth_batch
    return swd, kwargs

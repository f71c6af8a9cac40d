"""BPTT training of the CONDITIONAL SSN tuning-curve generator by the sliced Wasserstein distance: no critic.

A step draws `num_models` weight matrices, one contrast per model and `probes_per_model` (cell type, probe) pairs per model, as
the conditional WGAN does (`cwgan.RandomChoiceSampler`); every generated row x[b] (one tuning curve over the bandwidths) carries
its condition, and the conditions are a finite grid: (cell type, probe, contrast) -- a CELL, C = T P Cn of them.  The loss is the
mean over the generated rows' own conditions of the sliced distance under that condition,

    swd = sum_c (n_c / B) (1 / L) sum_l W_p^p(projections of the n_c rows of cell c, projections of the cell's WHOLE truth)[l],

with the quantile coupling of two samples of different sizes per (cell, direction): n_c is small and random, the truth of a cell
is all S rows of the truth table.  All cells and directions are matched by one launch (``ssnx2_swd_match_cells_f32``,
include/ssnode_mi355x_ext2.h); projections and back-projection are ``ssn_project_rows_f32`` and
``ssn_swd_backproject_f32``.  Forward, adjoint sweep, penalties and update are `moment_matching.GeneratorStepTrainer`'s.
"""
import ctypes
import os

import numpy as np
import torch

from .. import clib
from ..analyzers.distdiff import draw_slice_directions
from ..clib import libssnode
from ..gradient_expressions.utils import sample_sites_from_stim_space
from ._common import DEFAULT_PARAMS as _WGAN_DEFAULTS, build_generator, generator_trainer_parts
from .cwgan import ConditionalBPTTWassersteinGAN, RandomChoiceSampler
from .moment_matching import GeneratorStepTrainer
from .sliced_wasserstein import SWD_POWERS

DEFAULT_PARAMS = dict(_WGAN_DEFAULTS, num_models=15, probes_per_model=1, norm_probes=[0], e_ratio=0.8,
                      include_inhibitory_neurons=False, swd_directions=128, swd_power=2, swd_direction_seed=0,
                      **_WGAN_DEFAULTS['gen'])
for _key in ('gen', 'disc', 'batchsize', 'sample_sites'):
    del DEFAULT_PARAMS[_key]


def cell_layout(cells, C):
    """cells (B,) host ints in 0 .. C - 1 -> (cell_rows (B,) int32: the row indices grouped by cell, ascending within a cell;
    cell_start (C + 1,) int32): a stable argsort and a bincount."""
    cells = np.asarray(cells)
    if cells.ndim != 1 or not np.issubdtype(cells.dtype, np.integer):
        raise ValueError('cells must be a one-dimensional integer array, got {} of {}'.format(cells.shape, cells.dtype))
    if len(cells) and not (0 <= cells.min() and cells.max() < C):
        raise ValueError('cell ids must be in 0 .. {}, got {} .. {}'.format(C - 1, cells.min(), cells.max()))
    cell_rows = np.argsort(cells, kind='stable').astype(np.int32)
    cell_start = np.concatenate([[0], np.cumsum(np.bincount(cells, minlength=C))]).astype(np.int32)
    return cell_rows, cell_start


def cswd_loss_grad(x, cells, y, theta, power):
    """x (B, D) device float32, cells (B,) host ints in 0 .. C - 1, y (C, m, D) device float32 (the truth rows of every cell),
    theta (L, D) device float32, all contiguous -> (gx (B, D) device float32, swd, loss_cl (C, L) numpy fp64).
    Five launches (the upload of the row indices, two projections -- the truth as C m rows --, the match of all cells, the
    back-projection) and one read of the C L doubles.  `swd` is formed on the host in fp64: per cell the sequential sum over l
    divided by L, then the sequential sum over c ascending of (n_c / B) times that."""
    if x.dim() != 2 or y.dim() != 3 or theta.dim() != 2 or y.shape[2] != x.shape[1] or theta.shape[1] != x.shape[1] or \
            not (x.is_contiguous() and y.is_contiguous() and theta.is_contiguous()):
        raise ValueError('cswd_loss_grad: x (B, D), y (C, m, D) and theta (L, D) must be contiguous, got {}, {} and {}'
                         .format(tuple(x.shape), tuple(y.shape), tuple(theta.shape)))
    (B, D), (C, m), L = x.shape, y.shape[:2], theta.shape[0]
    if not 1 <= m <= clib.SWD_MAX_TRUTH:
        raise ValueError('cswd_loss_grad: {} truth rows per cell are not in 1 .. {} (clib.SWD_MAX_TRUTH)'.format(m, clib.SWD_MAX_TRUTH))
    if not 1 <= C <= clib.SWD_MAX_CELLS:
        raise ValueError('cswd_loss_grad: {} cells are not in 1 .. {} (clib.SWD_MAX_CELLS)'.format(C, clib.SWD_MAX_CELLS))
    if len(cells) != B:
        raise ValueError('cswd_loss_grad: {} cell ids for {} rows'.format(len(cells), B))
    cell_rows, cell_start = cell_layout(cells, C)
    stream = clib.stream_ptr()
    rows_dev = torch.as_tensor(cell_rows).to(x.device)
    px = torch.empty((B, L), device=x.device, dtype=torch.float32)
    py = torch.empty((C, m, L), device=x.device, dtype=torch.float32)
    for src, rows, dst in ((x, B, px), (y, C * m, py)):
        clib.check(libssnode.ssn_project_rows_f32(src.data_ptr(), rows, D, D, theta.data_ptr(), L, dst.data_ptr(), stream),
                   'ssn_project_rows_f32')
    coef = torch.empty((B, L), device=x.device, dtype=torch.float32)
    loss_cl = torch.empty((C, L), device=x.device, dtype=torch.float64)
    starts = np.ascontiguousarray(cell_start, dtype=np.int32)
    clib.check_ext2(clib.libssnode_ext2.ssnx2_swd_match_cells_f32(
        px.data_ptr(), B, rows_dev.data_ptr(), starts.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), C, py.data_ptr(), m, L,
        int(power), coef.data_ptr(), loss_cl.data_ptr(), stream), 'ssnx2_swd_match_cells_f32')
    gx = torch.empty((B, D), device=x.device, dtype=torch.float32)
    clib.check(libssnode.ssn_swd_backproject_f32(coef.data_ptr(), theta.data_ptr(), B, L, D, gx.data_ptr(), stream),
               'ssn_swd_backproject_f32')
    host = loss_cl.cpu().numpy()
    swd, _ = weighted_mean_over_cells(host, cell_start)
    return gx, swd, host


def weighted_mean_over_cells(loss_cl, cell_start):
    """loss_cl (C, L) fp64, cell_start (C + 1,) -> (swd, per_cell (C,)): per cell the sequential sum over l divided by L, then
    the sequential sum over c ascending of (n_c / B) times that (an empty cell adds +0)."""
    C, L = loss_cl.shape
    B = np.float64(cell_start[C])
    per_cell = np.array([np.cumsum(loss_cl[c])[-1] / np.float64(L) for c in range(C)])
    total = np.float64(0.0)
    for c in range(C):
        total = total + (np.float64(cell_start[c + 1] - cell_start[c]) / B) * per_cell[c]
    return float(total), per_cell


def cell_ids(conditions, cond_values):
    """conditions (B, 3): the rows' (contrast, norm_probe, cell_type) VALUES, as `ConditionalMinibatch.conditions` gives them;
    cond_values: the sampler's [cell_types, norm_probes, contrasts, bandwidths] -> (B,) int64 ids
    ((cell type index P) + probe index) Cn + contrast index.  Condition values that occur twice have no index: refused by
    name."""
    cell_types, norm_probes, contrasts = (np.asarray(v) for v in cond_values[:3])
    for name, values in (('cell_types', cell_types), ('norm_probes', norm_probes), ('contrasts', contrasts)):
        if len(np.unique(values)) != len(values):
            raise ValueError('{} = {} has duplicate values: the rows under them would be one condition with two cells'
                             .format(name, values.tolist()))
    conditions = np.asarray(conditions)

    def index_of(column, values, name):
        order = np.argsort(values, kind='stable')
        pos = np.clip(np.searchsorted(values[order], column), 0, len(values) - 1)
        idx = order[pos]
        if not (values[idx] == column).all():
            raise ValueError('a row has a value of {} that is not in {}'.format(name, values.tolist()))
        return idx.astype(np.int64)
    ic = index_of(conditions[:, 0], contrasts, 'contrasts')
    ip = index_of(conditions[:, 1], norm_probes, 'norm_probes')
    it = index_of(conditions[:, 2], cell_types, 'cell_types')
    return (it * len(norm_probes) + ip) * len(contrasts) + ic


def truth_by_cell(nested):
    """The sampler's table (S, T, P, Cn, D) -> (C = T P Cn, m = S, D) float32, contiguous: the truth rows of every cell."""
    nested = np.asarray(nested)
    S, T, P, Cn, D = nested.shape
    if not 1 <= S <= clib.SWD_MAX_TRUTH:
        raise ValueError('the truth has {} rows, the match takes 1 .. {} per cell (clib.SWD_MAX_TRUTH)'.format(S, clib.SWD_MAX_TRUTH))
    if T * P * Cn > clib.SWD_MAX_CELLS:
        raise ValueError('{} cell types x {} probes x {} contrasts = {} cells, the match takes {} (clib.SWD_MAX_CELLS)'
                         .format(T, P, Cn, T * P * Cn, clib.SWD_MAX_CELLS))
    return np.ascontiguousarray(nested.transpose((1, 2, 3, 0, 4)).reshape(T * P * Cn, S, D), dtype='float32')


class ConditionalBPTTSlicedWasserstein(GeneratorStepTrainer):
    """The critic-free conditional trainer: `set_dataset(data)`, then `learning()` yields one `info` per generator update --
    step, loss (with the penalties), swd (the bare loss), dynamics_penalty, rate_penalty, train_time, and per cell swd_per_cell
    (C,) and rows_per_cell (C,)."""

    def __init__(self, gen, gen_updaters, bandwidths, contrasts, norm_probes, e_ratio, num_models, probes_per_model,
                 swd_directions, swd_power, swd_direction_seed, include_inhibitory_neurons, rate_penalty_threshold,
                 dynamics_cost, rate_cost, param_bounds, seed=0):
        if swd_power not in SWD_POWERS:
            raise ValueError('swd_power must be 1 or 2, got {!r}'.format(swd_power))
        if not 1 <= int(swd_directions) <= clib.W1_MAX_DIRECTIONS:
            raise ValueError('swd_directions = {} is not in 1 .. {}'.format(swd_directions, clib.W1_MAX_DIRECTIONS))
        if not gen.conditional:
            raise ValueError('the conditional trainer needs a generator without fixed probes')
        assert gen.batchsize == num_models * probes_per_model and probes_per_model < gen.num_neurons
        self.swd_directions, self.swd_power = int(swd_directions), int(swd_power)
        self.norm_probes = np.asarray(norm_probes)
        self.e_ratio = e_ratio
        self.num_models, self.probes_per_model = int(num_models), int(probes_per_model)
        # the directions and the conditions have streams of their own, both seeded by `swd_direction_seed`: the reference's
        # noise stream on self.rng is not disturbed
        self.direction_rng = np.random.RandomState(swd_direction_seed)
        self.minibatch_rng = np.random.RandomState(swd_direction_seed)
        self._warned_host_noise = False
        self._predrawn = None
        self.last_x = self.last_gx = self.last_cells = None      # of the last step: tuning curves, loss gradient, cell ids
        self._init_generator_step(gen, gen_updaters, np.asarray(bandwidths), np.asarray(contrasts), include_inhibitory_neurons,
                                  rate_penalty_threshold, dynamics_cost, rate_cost, param_bounds, seed)

    @property
    def sample_sites(self):
        return sample_sites_from_stim_space(self.norm_probes, self.num_sites)

    def set_dataset(self, data, **kwargs):
        """The sampler of the conditional GAN on `minibatch_rng` draws the conditions; its table, by cell, is the truth and
        stays on the device.  Every step sees all of it."""
        kwargs.setdefault('seed', self.minibatch_rng)
        self.sampler = RandomChoiceSampler.from_grid_data(
            data, bandwidths=self.bandwidths, contrasts=self.contrasts, norm_probes=self.norm_probes, e_ratio=self.e_ratio,
            include_inhibitory_neurons=self.include_inhibitory_neurons, **kwargs)
        cell_ids(np.zeros((0, 3)), self.sampler.cond_values)      # (duplicate condition values are refused here)
        self._predrawn = None
        self.truth = torch.as_tensor(truth_by_cell(self.sampler.nested)).to('cuda')
        self.num_cells = int(self.truth.shape[0])

    def next_minibatch(self):
        """The conditions of a step (the sampler's drawn truth rows are not used): the batch drawn ahead, or a fresh one."""
        batch, self._predrawn = self._predrawn, None
        return batch if batch is not None else self.sampler.select_minibatch(self.num_models, self.probes_per_model)

    def _predraw_minibatch(self):
        """The NEXT step's conditions, drawn while this step's forward runs on the GPU: the sampler's per-model `rng.choice`
        loop costs 5 us a model on the host.  `minibatch_rng` serves the sampler alone, so the batches are the same ones in the
        same order whenever they are drawn."""
        if self._predrawn is None:
            self._predrawn = self.sampler.select_minibatch(self.num_models, self.probes_per_model)

    def next_directions(self, columns):
        return torch.as_tensor(draw_slice_directions(self.direction_rng, self.swd_directions, columns)).to('cuda')

    def truth_of_step(self):
        return self.truth

    def train_generator(self, info):
        def loss_grad(x):
            self._predraw_minibatch()                             # (the forward has been queued: the host is free)
            self.last_x = x = x.to(torch.float32).contiguous()
            gx, info.swd, loss_cl = cswd_loss_grad(x, cells, self.truth_of_step(), self.next_directions(x.shape[1]), self.swd_power)
            self.last_gx = gx
            _, start = cell_layout(cells, self.num_cells)
            info.swd_per_cell = weighted_mean_over_cells(loss_cl, start)[1]
            info.rows_per_cell = np.diff(start)
            return gx, info.swd
        with self.train_watch:
            batch = self.next_minibatch()
            self.last_cells = cells = cell_ids(batch.conditions, self.sampler.cond_values)
            noise = ConditionalBPTTWassersteinGAN._draw_noise(self, batch, keep_z=True)
            self.generator_step(info, loss_grad, forward_kwargs=batch.gen_kwargs, noise=noise)
        info.train_time = self.train_watch.sum()
        return info


def make_conditional_sliced_wasserstein(config):
    """make_conditional_sliced_wasserstein(config: dict) -> (ConditionalBPTTSlicedWasserstein, dict of unconsumed config)."""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world > 1:
        raise ValueError('the conditional sliced Wasserstein trainer runs on one GPU: the match kernel needs whole columns of the '
                         'projections, and the all-gather that would give them to every rank is not built (WORLD_SIZE = {})'
                         .format(world))
    kwargs = dict(DEFAULT_PARAMS, **config)
    take = kwargs.pop
    num_models, probes_per_model = take('num_models'), take('probes_per_model')
    bandwidths, contrasts = take('bandwidths'), take('contrasts')
    gen, ssn_type = build_generator(kwargs, take('gen_kernel', 'auto'), len(bandwidths), num_models * probes_per_model,
                                    include_rate_penalty=True)
    parts = generator_trainer_parts(kwargs, ssn_type)
    learner = ConditionalBPTTSlicedWasserstein(
        gen=gen, bandwidths=bandwidths, contrasts=contrasts, norm_probes=take('norm_probes'), e_ratio=take('e_ratio'),
        num_models=num_models, probes_per_model=probes_per_model, swd_directions=take('swd_directions'),
        swd_power=take('swd_power'), swd_direction_seed=take('swd_direction_seed'),
        include_inhibitory_neurons=take('include_inhibitory_neurons'), rate_penalty_threshold=take('rate_penalty_threshold'),
        seed=take('seed', 0), **parts)
    return learner, kwargs

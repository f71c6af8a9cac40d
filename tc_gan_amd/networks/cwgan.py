"""Conditional BPTT Wasserstein GAN on the GPU -- host-side mirror of ``tc_gan/networks/cwgan.py``.

Same components, names and schedule as the reference:

* `ConditionalMinibatch`, `RandomChoiceSampler` (cwgan.py:217-391) -- host index selection with the
  reference's RandomState consumption order (SURVEY.md section 8a gotcha 1);
* `ConditionalBPTTWassersteinGAN` (cwgan.py:410-552) -- ``learning()`` is a Python generator yielding a
  `Namespace` per critic step (``is_discriminator=True``) and per generator step, with the fields the
  driver/recorders read;
* `make_gan(config) -> (gan, rest)` (cwgan.py:555-614).

What differs is where the arithmetic runs: generator forward / BPTT in ``csrc/ssn_gen.hip``, critic
passes and optimizers in ``csrc/ssn_critic.hip``; tuning curves stay on the device between the
generator and the critic (the reference round-trips them through numpy, cwgan.py:478-505).

Data parallelism (new; the reference is single device): with ``torch.distributed`` initialised every
rank keeps a replica of the critic and of (J, D, S), works on its contiguous slice of the
``num_models`` weight draws, and ONE all-reduce per update (flat buffer: critic grads | 12 generator
grads | loss scalars) makes the replicas take identical optimizer steps.
"""
import ctypes
import itertools
import os
import pickle
import time
from logging import getLogger

import numpy as np
import torch

from .. import clib, genops
from ..critic import Critic
from ..execution import KnownError
from ..gradient_expressions.utils import sample_sites_from_stim_space
from ..utils import Namespace, StopWatch, as_randomstate, cartesian_product, to_device, to_device_packed
from .utils import gridify_tc_samples
from ._common import (DEFAULT_PARAMS as _WGAN_DEFAULTS, GradientAllReducer, _v_bounds,  # noqa: F401  (`_v_bounds` re-exported)
                      build_generator, generator_trainer_parts, updater_from)
from .gen_state import GeneratorParamState, HostRecord

# (A/B switch: TCGAN_PREQUEUE=0 queues the first critic forward of an iteration only after the generator step's record was read)
_PREQUEUE = os.environ.get('TCGAN_PREQUEUE', '1') != '0'
# (TCGAN_SUBSET_RETRY=0: a refused generator step is recomputed on the fp32 kernels for ALL draws, not only the refused ones)
_SUBSET_RETRY = os.environ.get('TCGAN_SUBSET_RETRY', '1') != '0'

logger = getLogger(__name__)

# cwgan.py:24-32
DEFAULT_PARAMS = dict(
    _WGAN_DEFAULTS,
    num_models=1,
    probes_per_model=1,
    e_ratio=0.8,
    hide_cell_type=False,
)
del DEFAULT_PARAMS['batchsize']
del DEFAULT_PARAMS['sample_sites']


class ConditionalMinibatch(object):
    """cwgan.py:217-274."""

    def __init__(self, tc_md, conditions_md, bandwidths, contrasts):
        self.tc_md = tc_md
        self.conditions_md = np.asarray(conditions_md)
        self.bandwidths = bandwidths
        self.contrasts = contrasts
        assert self.tc_md.shape[:-1] == self.conditions_md.shape[1:]
        assert self.tc_md.shape[-1] == len(bandwidths)

    num_models = property(lambda self: self.tc_md.shape[0])
    probes_per_model = property(lambda self: self.tc_md.shape[1])
    num_bandwidths = property(lambda self: self.tc_md.shape[2])

    @property
    def batchsize(self):
        return self.num_models * self.probes_per_model

    @property
    def gen_kwargs(self):
        contrasts, bandwidths = np.broadcast_arrays(self.contrasts.reshape((-1, 1)),
                                                    self.bandwidths.reshape((1, -1)))
        _, norm_probes, cell_types = self._conditions_T
        return dict(
            stimulator_bandwidths=bandwidths.astype('float32'),
            stimulator_contrasts=contrasts.astype('float32'),
            prober_norm_probes=norm_probes.astype('float32'),
            prober_cell_types=cell_types.astype('uint16'),
            prober_model_ids=self.model_ids.astype('uint16'))

    @property
    def tuning_curves(self):
        return self.tc_md.reshape((self.batchsize, self.num_bandwidths))

    @property
    def conditions(self):
        return self._conditions_T.T

    @property
    def _conditions_T(self):
        return self.conditions_md.reshape((-1, self.batchsize))

    @property
    def model_ids(self):
        ids = np.arange(self.num_models, dtype='uint16').reshape((-1, 1))
        return np.broadcast_to(ids, self.conditions_md.shape[1:]).flatten()

    def shard(self, rank, world):
        """The contiguous block of models of one data-parallel rank (same arrays, fewer rows)."""
        per = self.num_models // world
        sl = slice(rank * per, (rank + 1) * per)
        return ConditionalMinibatch(self.tc_md[sl], self.conditions_md[:, sl], self.bandwidths, self.contrasts[sl])


class RandomChoiceSampler(object):
    """Minibatch sampler based on random choice (cwgan.py:277-391)."""

    @classmethod
    def from_grid_data(cls, data, bandwidths, contrasts, norm_probes, include_inhibitory_neurons, **kwargs):
        cell_types = [0, 1] if include_inhibitory_neurons else [0]
        nested = gridify_tc_samples(data, num_contrasts=len(contrasts), num_bandwidths=len(bandwidths),
                                    num_cell_types=len(cell_types), num_probes=len(norm_probes))
        cond_values = [cell_types, norm_probes, contrasts, bandwidths]
        assert nested.shape == (len(data),) + tuple(map(len, cond_values))
        return cls(nested, cond_values, **kwargs)

    def __init__(self, nested, cond_values, e_ratio, seed=0):
        self.nested = np.asarray(nested)
        self.cond_values = cond_values = list(map(np.asarray, cond_values))
        self.e_ratio = e_ratio
        self.cell_types, self.norm_probes, self.contrasts, self.bandwidths = cond_values
        self.rng = as_randomstate(seed)
        assert tuple(self.cell_types) in [(0,), (0, 1)]

    def random_cells(self, num_models, probes_per_model):
        """Every (cell type, probe) pair at most once per model (cwgan.py:328-355)."""
        cellids = cartesian_product(np.arange(len(self.cell_types)), np.arange(len(self.norm_probes)), dtype=int).T
        if len(self.cell_types) == 2:
            probs = np.zeros(len(cellids))
            probs[:len(self.norm_probes)] = self.e_ratio
            probs[len(self.norm_probes):] = 1 - self.e_ratio
            probs /= probs.sum()
        else:
            probs = None
        if len(cellids) == 1:
            # one (cell type, probe) pair: `choice(1, 1, replace=False)` is permutation(1)[:1] = [0] and draws nothing
            # from the RandomState, so the per-model loop (5 us per model: 40 ms per critic step for the 8192 models
            # of an 8-GPU job, on every rank) can be skipped without changing the stream
            assert probes_per_model == 1
            ids = np.broadcast_to(cellids[0], (num_models, 1, 2))
        else:
            ids = np.asarray([cellids[self.rng.choice(len(cellids), probes_per_model, replace=False, p=probs)]
                              for _ in range(num_models)])
        ids_cell_type, ids_norm_probes = ids.transpose((2, 0, 1))
        return ids_cell_type, ids_norm_probes

    def select_minibatch(self, num_models, probes_per_model):
        """RandomState consumption order: samples, cells (per model), contrasts (cwgan.py:362-367)."""
        shape = (num_models, probes_per_model)
        ids_sample = self.rng.choice(len(self.nested), shape)
        ids_cell_type, ids_norm_probes = self.random_cells(*shape)
        ids_flat_contrast = self.rng.choice(len(self.contrasts), num_models)
        ids_contrast = np.broadcast_to(ids_flat_contrast.reshape((-1, 1)), shape)
        tc_md = self.nested[ids_sample, ids_cell_type, ids_norm_probes, ids_contrast]
        assert tc_md.shape == (num_models, probes_per_model, len(self.bandwidths))
        return ConditionalMinibatch(
            tc_md,
            [self.contrasts[ids_contrast], self.norm_probes[ids_norm_probes], self.cell_types[ids_cell_type]],
            self.bandwidths,
            self.contrasts[ids_flat_contrast])

    def random_minibatches(self, *args, **kwargs):
        while True:
            yield self.select_minibatch(*args, **kwargs)


# (the carried accuracy of data-parallel runs: see `_launch_disc`)
def _with_carry(tensors, carry):
    """`tensors` with the carried accuracy behind them, when there is one."""
    return tensors + [carry] if carry is not None else tensors


def _split_carry(host, carried):
    """(the accuracy that arrived as the last word of the host record, or None; the record without it)"""
    return (float(host[-1]), host[:-1]) if carried else (None, host)


class ConditionalBPTTWassersteinGAN(object):
    """cwgan.py:410-552."""

    loss_type = 'WD'

    def __init__(self, gen, disc, gen_updaters, disc_updater, bandwidths, contrasts, norm_probes,
                 e_ratio, include_inhibitory_neurons, rate_penalty_threshold,
                 num_models, probes_per_model, critic_iters_init, critic_iters, lipschitz_cost,
                 disc_rate_penalty_bound, dynamics_cost, rate_cost, param_bounds, seed=0):
        self.gen = gen
        self.disc = disc
        self.gen_updaters = gen_updaters          # {'J': Updater, 'D': ..., 'S': ...}
        self.disc_updater = disc_updater
        self.bandwidths = np.asarray(bandwidths)
        self.contrasts = np.asarray(contrasts)
        self.norm_probes = np.asarray(norm_probes)
        self.e_ratio = e_ratio
        self.include_inhibitory_neurons = include_inhibitory_neurons
        self.rate_penalty_threshold = rate_penalty_threshold
        self.num_models = num_models
        self.probes_per_model = probes_per_model
        self.critic_iters_init = critic_iters_init
        self.critic_iters = critic_iters
        self.lipschitz_cost = lipschitz_cost
        self.disc_rate_penalty_bound = disc_rate_penalty_bound
        self.dynamics_cost = dynamics_cost
        self.rate_cost = rate_cost
        self.param_bounds = param_bounds          # {'J': (min, max), ...}  (wgan.py:244-251)
        self._init_loop_state(seed)
        assert self.probes_per_model < gen.num_neurons
        assert num_models % self.reducer.world == 0, 'num_models must be divisible by the number of ranks'

    def _init_loop_state(self, seed):
        """What the update loop keeps between steps (shared with the unconditional GAN of networks/wgan.py)."""
        self.rng = as_randomstate(seed)
        self._predrawn = None          # host draws of the NEXT critic step, made early (see train_generator)
        self._next_ctx = None          # ... and that step itself, its forward queued behind the generator update (`_prequeue_next_disc`)
        self._rng_before_predraw = None
        self._acc_carry = None         # data-parallel runs: this rank's accuracy of the last critic step, waiting for a collective
        self._arrived_with_gen = None
        self._warned_host_noise = False
        self.host_draw_seconds = 0.0   # host time spent in the RNG draws of the critic steps (bench.py reads and resets it)
        self.reducer = GradientAllReducer()
        self.gen_state = GeneratorParamState(self.gen, self.param_bounds)    # the generator's parameters on the device
        self._pnames = self.gen_state.names                              # ['V',] 'J', 'D', 'S'
        self._disc_records = HostRecord(4)      # a step is read before the ring comes round: at most two steps are in flight
        self._gen_records = HostRecord(1)
        self.gen_forward_watch, self.gen_train_watch, self.disc_train_watch = StopWatch(), StopWatch(), StopWatch()

    batchsize = property(lambda self: self.num_models * self.probes_per_model)
    num_sites = property(lambda self: self.gen.num_sites)
    num_neurons = property(lambda self: self.gen.num_neurons)
    NZ = property(lambda self: self.batchsize)
    discriminator = property(lambda self: self.disc)

    @property
    def sample_sites(self):
        return sample_sites_from_stim_space(self.norm_probes, self.num_sites)

    def get_gen_param(self):
        return [self.gen.J.copy(), self.gen.D.copy(), self.gen.S.copy()]

    def set_gen_param(self, **params):
        self.gen.set_params(params)

    def set_dataset(self, data, **kwargs):
        kwargs.setdefault('seed', self.rng)       # the sampler SHARES the GAN's RandomState (cwgan.py:452)
        self.sampler = RandomChoiceSampler.from_grid_data(
            data, bandwidths=self.bandwidths, contrasts=self.contrasts, norm_probes=self.norm_probes,
            e_ratio=self.e_ratio, include_inhibitory_neurons=self.include_inhibitory_neurons, **kwargs)
        self.dataset = self.sampler.random_minibatches(self.num_models, self.probes_per_model)

    def next_minibatch(self):
        return next(self.dataset)

    def prepare(self):
        """Nothing to compile."""

    # ---------------------------------------------------------------------------------------
    def _local(self, batch):
        return batch.shard(self.reducer.rank, self.reducer.world) if self.reducer.on else batch

    def _draw_noise(self, batch, keep_z=None):
        """Noise in the reference's stream order (ssn.py:434-439, 764-767: zs, then zs_in): the GLOBAL draw is consumed from
        the shared RandomState, this rank's rows are returned -- a data-parallel run consumes the RandomState exactly like a
        single-GPU run.  z itself is generated on the device (`ssn.device_rand`: only this rank's rows; the host never sees
        it) unless the generator was built with `z_host_draw`.  Empty in Philox mode (`z_device_seed`)."""
        if self.gen._zgen is not None:
            return {}
        rows = None
        if self.reducer.on:
            per = batch.num_models // self.reducer.world
            rows = (self.reducer.rank * per, (self.reducer.rank + 1) * per)
            if self.gen.z_host_draw and not self._warned_host_noise:
                # host draw under data parallelism: EVERY rank draws the global (num_models, 2N, 2N) fp64 tensor on the host
                # and keeps 1/world of it, so the host cost per step grows with the job.  Meant for equivalence tests.
                self._warned_host_noise = True
                logger.warning('host-side noise with %d ranks: every rank draws all %d models\' z on the host each step',
                               self.reducer.world, batch.num_models)
        # keep_z given: the forward follows at once with the current parameters, so W is formed in the draw's own launch
        return self.gen.gen_noise(self.rng, stimulator_bandwidths=np.empty((batch.num_models, 1)), rows=rows, keep_z=keep_z)

    def gen_forward(self, batch, noise=None, save=False, params_dev=None):
        local = self._local(batch)
        kw = local.gen_kwargs
        kw.update(noise or {})
        return self.gen.forward(rng=self.rng, save=save, model_rate_penalty_threshold=self.rate_penalty_threshold,
                                params_dev=params_dev, **kw), local

    # A critic step is split in two so that the NEXT generator forward (which does not depend on the critic update)
    # is already queued on the stream when the host blocks on this step's scalars: `_prepare_disc` draws from the
    # host RNG (same order as the reference: minibatch, eps, zs) and launches the forward; `_finish_disc` runs the
    # critic update and reads loss / accuracy / penalties back with ONE device-to-host copy.
    def _draw_disc(self, early=False):
        """The RNG draws of one critic step, in the reference's order (minibatch, eps, zs).  `early`: the draws `train_generator`
        makes ahead of time, BEFORE its parameter update -- zs is drawn as numbers only (W is formed from them at the forward,
        with the updated parameters); otherwise the forward follows at once and W is formed in the draw's own launch."""
        t0 = time.perf_counter()
        batch = self.next_minibatch()
        eps_full = self.rng.rand(batch.batchsize, 1)
        noise = self._draw_noise(batch, keep_z=None if early else False)
        self.host_draw_seconds += time.perf_counter() - t0
        return batch, eps_full, noise

    def _prepare_disc(self, params_dev=None):
        drawn = self._predrawn
        if params_dev is None:
            # (the regular path uses the early draws up; a step prepared ahead from them is obsolete with that)
            self._predrawn = self._rng_before_predraw = self._next_ctx = None
        batch, eps_full, noise = drawn if drawn is not None else self._draw_disc()
        with self.gen_forward_watch:
            gen_out, local = self.gen_forward(batch, noise, params_dev=params_dev)
        return Namespace(batch=batch, eps_full=eps_full, gen_out=gen_out, local=local, pens64=self.gen.last_penalties,
                         gen_time=self.gen_forward_watch.times[-1])

    # The first critic step of the NEXT iteration needs nothing from the host but the updated generator parameters -- and those
    # are on the device the moment the optimizer launch is queued.  So its forward is queued right behind that launch, with W
    # formed from the device values (`ssn_build_w_devparams_f32`), BEFORE the host waits for the step's record: the GPU no
    # longer idles through the host's way from the record to the next launch (0.16 - 0.24 ms per iteration).  The draws were
    # made early anyway (`train_generator`); `_predrawn` stays set until the prepared step is taken up, so a checkpoint in
    # between still stores the RandomState from before them and a resumed run repeats them.
    def _prequeue_next_disc(self):
        pd = self.gen_state.jds_v_slices()
        if (self._predrawn is None or not _PREQUEUE or self.gen.dtype != 'float32' or pd is None
                or not self.gen.accepts_params_dev(self._predrawn[2].get('model_zs'))):
            return None
        ctx = self._prepare_disc(params_dev=pd)
        ctx.prequeued_time = self.gen_forward_watch.times.pop()       # (booked on the iteration that uses the step)
        return ctx

    def _take_prequeued(self):
        """The critic step `_prequeue_next_disc` prepared, unless the generator's attributes were changed from outside since
        the record of the update was read (then it is prepared again from the same draws, with the attributes' values)."""
        ctx, self._next_ctx = self._next_ctx, None
        if ctx is None or not self.gen_state.matches(self.gen):
            return None
        self._predrawn = self._rng_before_predraw = None
        self.gen_forward_watch.times.append(ctx.prequeued_time)
        return ctx

    def _launch_disc(self, ctx):
        """Queue the critic update of a prepared step (no host wait); the four scalars of the step go to pinned
        host memory with an asynchronous copy followed by an event."""
        gen_out, local = ctx.gen_out, ctx.local
        xg = gen_out.prober_tuning_curve
        per = local.batchsize
        r0 = self.reducer.rank * per if self.reducer.on else 0
        if local.conditions is None:              # the unconditional GAN of networks/wgan.py: no condition columns
            (xd, eps), cd = to_device_packed([local.tuning_curves, ctx.eps_full[r0:r0 + per]], torch.float32), None
        else:
            xd, cd, eps = to_device_packed([local.tuning_curves, local.conditions, ctx.eps_full[r0:r0 + per]], torch.float32)
        ctx.skipped = ctx.gated = ctx.acc_deferred = False
        ctx.snapshot = None
        if not self.reducer.on and xg.dtype == torch.float32 and self.disc.has_step:
            # single process: the whole step is one library call (same kernels, same order); the skip rule of cwgan.py:493-498
            # is honoured by the optimizer kernel itself, which reads the rate penalty where the forward left it
            ctx.gated = self.disc_rate_penalty_bound > 0
            with self.disc_train_watch:
                xp, tail = self.disc.step(self.disc_updater, xg, xd, cd, eps, self.lipschitz_cost, pens64=ctx.pens64,
                                          rate_penalty_bound=self.disc_rate_penalty_bound if ctx.gated else None)
        else:
            pens = ctx.pens64.to(torch.float32)      # [dynamics_penalty, rate_penalty] of this step's forward (averaged over ranks below)
            xp = self.disc.interpolate(eps, xd, xg)                               # cwgan.py:481
            # cwgan.py:493-498 skips the critic update when the rate penalty of the batch exceeds `disc_rate_penalty_bound`.
            # Waiting for that value here would stall the queue at every critic step, so the update is made
            # speculatively and rolled back in `_read_disc` (which learns the value before the next update is queued)
            # in the rare case that the bound was exceeded.
            ctx.snapshot = self.disc_updater.snapshot(self.disc.params) if self.disc_rate_penalty_bound > 0 else None
            # ONE collective per update: gradients, loss statistics, the two penalties -- and, riding along, the
            # accuracy of the critic as the PREVIOUS step left it.  That number (cwgan.py:505-507) is a recorded diagnostic
            # of the updated critic, so it only exists after this step's collective has gone; instead of its own one-float
            # all-reduce it travels in the next flat buffer (the next critic step's, or the generator's), and the step's
            # record is handed to the driver once it has arrived (`_single_gen_step`).
            carry = self._take_carry()
            with self.disc_train_watch:
                stats = self.disc.loss_grad(xg, cd, xd, cd, xp, cd, self.lipschitz_cost)
                self.reducer.mean_(*_with_carry([self.disc.grads, stats, pens], carry))
                self.disc_updater(self.disc.params, self.disc.grads)
            acc = self.disc.accuracy_device(xg, cd, xd, cd)
            arrived = None
            if self.reducer.on:
                self._acc_carry = acc            # this rank's share; averaged by the next collective
                ctx.acc_deferred = True
                arrived = carry if carry is not None else torch.full_like(acc, float('nan'))
            tail = torch.cat(_with_carry([pens, stats[3:4], acc, self.disc.param_sqnorms_device()], arrived))
        # `tail`: the four scalars of the step [dynamics penalty, rate penalty, loss, accuracy] + the per-tensor sums of squares
        # of the updated critic (disc_param_stats)
        ctx.xd, ctx.xg, ctx.xp, ctx.cd = xd, xg, xp, cd
        ctx.ticket = self._disc_records.post(tail)
        ctx.disc_time = self.disc_train_watch.times[-1]

    def _read_disc(self, info, ctx):
        """Wait for the scalars of a launched step (only for its own kernels: later launches are not waited for)."""
        # (deferred: the last word is the job-wide accuracy of the PREVIOUS critic step, which travelled in this step's collective)
        ctx.arrived_accuracy, host = _split_carry(ctx.ticket.wait(), ctx.acc_deferred)
        if (ctx.snapshot is not None or ctx.gated) and np.float32(host[1]) > np.float32(self.disc_rate_penalty_bound):
            if ctx.gated:
                self.disc_updater.uncommit_step()                                # (the kernel made no update: same test, same value)
            else:
                self.disc_updater.restore(self.disc.params, ctx.snapshot)        # the skipped step of cwgan.py:493-498
            ctx.skipped = True
            host = np.array([host[0], host[1], np.nan, np.nan], dtype='float32')
            info.param_sqnorms = None
        else:
            info.param_sqnorms = host[4:].copy()     # of the critic as THIS step left it; handed to the recorder when the record is
        self.disc.cache_param_nnorms(info.param_sqnorms)
        ctx.snapshot = None
        info.gen_out = ctx.gen_out
        info.xd, info.xg, info.xp = ctx.xd, ctx.xg, ctx.xp
        info.cd = info.cg = info.cp = ctx.cd
        info.batch = ctx.batch
        info.gen_time = ctx.gen_time
        info.dynamics_penalty, info.rate_penalty = float(host[0]), float(host[1])
        info.disc_loss, info.accuracy = float(host[2]), float(host[3])
        info.accuracy_pending = bool(ctx.acc_deferred and not ctx.skipped)   # (host[3] is this rank's share until the mean arrives)
        info.disc_time = np.nan if ctx.skipped else ctx.disc_time
        return info

    def _take_carry(self):
        """The accuracy waiting for a collective (data-parallel runs), handed to the caller whose collective takes it along."""
        carry, self._acc_carry = (self._acc_carry if self.reducer.on else None), None
        return carry

    def _flush_accuracy(self):
        """The job-wide mean of the accuracy still waiting for a collective, through one of its own (outside the loop's
        schedule: `train_discriminator` called by hand, the end of a run)."""
        carry, self._acc_carry = self._acc_carry, None
        if carry is None:
            return None
        self.reducer.mean_(carry)
        return float(carry[0])

    def _finish_disc(self, info, ctx):
        self._acc_carry = None
        self._launch_disc(ctx)
        info = self._read_disc(info, ctx)
        if info.accuracy_pending:
            info.accuracy, info.accuracy_pending = self._flush_accuracy(), False
        self._acc_carry = None
        return info

    def train_discriminator(self, info):
        return self._finish_disc(info, self._prepare_disc())

    def _prepare_gen(self, batch):
        """Noise draw + generator forward with the trajectory kept (independent of the critic: may be queued before
        the last critic step of the iteration has finished)."""
        noise = self._draw_noise(batch, keep_z=True)
        with self.gen_train_watch:
            gen_out, local = self.gen_forward(batch, noise, save=True)
        return gen_out, local

    def train_generator(self, info, batch, prepared=None):
        gen_out, local = prepared if prepared is not None else self._prepare_gen(batch)
        # The host draws of the NEXT critic step (per-model `rng.choice` loops: ~5 ms for 1024 models) are made now,
        # while the trajectory-saving forward is still running on the GPU -- after the parameter update the GPU would
        # sit idle for them.  Same RandomState order: nothing else draws between here and that step.  A checkpoint
        # taken in between stores the RandomState from BEFORE these draws (state_dict), so a resumed run repeats them.
        if self.critic_iters > 0 and self._predrawn is None:
            self._rng_before_predraw = self.rng.get_state()
            self._predrawn = self._draw_disc(early=True)
        st = self._gen_tail_fused()
        with self.gen_train_watch:
            cd = None if local.conditions is None else to_device(np.ascontiguousarray(local.conditions), torch.float32)
            xg = gen_out.prober_tuning_curve.to(torch.float32)
            gx, dmean = self.disc.input_grad(xg, cd, scale=-1.0 / xg.shape[0])           # d(-mean D)/d tuning curve
            # Everything up to the record is queued without a host wait; the device copies of the parameters are the working
            # values, and ONE device-to-host copy at the end returns the new values together with the loss.
            if st is None:
                host = self._gen_tail_by_parameter(gen_out, gx, dmean)
            else:
                host = self._gen_tail_one_launch(st, info, gx, dmean)
            self.gen_state.write_back(self.gen, host)
            info.gen_loss = float(host[-1])
            if not np.isfinite(host).all():
                self._report_poisoned(info, gen_out)
        info.gen_forward_time = self.gen_forward_watch.sum()
        info.gen_train_time = self.gen_train_watch.sum()
        info.gen_time = info.gen_train_time + info.gen_forward_time
        info.disc_time = self.disc_train_watch.sum()
        return info

    def _report_poisoned(self, info, gen_out):
        """(the drivers' NaN guards end the run; say why when it was the fp16 adjoint's range and not the model)"""
        bad = self.gen.poisoned_draws()
        if bad:
            logger.warning('generator step %s: %d of %d draws have an adjoint that grew by more than 2^8 within one '
                           'Euler step -- beyond the lagged scale of the fp16-split sweep, so their gradient is NaN; '
                           '--gen-kernel mfma-fp32 has no such limit', getattr(info, 'gen_step', '?'), bad,
                           gen_out.prober_tuning_curve.shape[0] // max(self.probes_per_model, 1))

    # -- the end of a generator step: both tails return the record on the host (new values in `_pnames` order, loss) -----------
    def _gen_tail_fused(self):
        """The flat device state of the generator's update (`GeneratorParamState`) with the updaters' moments bound to it, or
        None when the step has to go parameter by parameter: a generator in float64, or updaters that are not in step with
        each other."""
        st = self.gen_state
        if not st.in_step(self.gen_updaters, self.gen.dtype):
            return None
        st.bind_moments(self.gen_updaters)
        return st

    def _gen_tail_by_parameter(self, gen_out, gx, dmean):
        """Gradients and loss with torch, the job's all-reduce, one optimizer launch per parameter."""
        st = self.gen_state
        gdict = self.gen.backward(gx, self.dynamics_cost, self.rate_cost, as_tensor=True)
        loss = (-dmean.to(torch.float64) + self.dynamics_cost * gen_out.model_dynamics_penalty
                + self.rate_cost * gen_out.model_rate_penalty).reshape(1).to(torch.float32)
        grads = torch.cat([gdict[name].reshape(-1) for name in st.names]).to(torch.float32)
        carry = self._take_carry()
        self.reducer.mean_(*_with_carry([grads, loss], carry))
        st.upload_changed(self.gen)
        for name, (a, b) in zip(st.names, st.ranges()):                          # wgan.py:218-260
            self.gen_updaters[name](st.params[name], grads[a:b], clip=self.param_bounds[name])
        host = torch.cat(_with_carry([st.flat, loss], carry)).cpu().numpy()
        self._arrived_with_gen, host = _split_carry(host, carry is not None)
        return host

    def _gen_tail_one_launch(self, st, info, gx, dmean):
        """Adjoint sweep, dL/dW, chain rule; then gradient vector + loss in one launch (`ssn_gen_grads_f32`), the job's
        all-reduce, and the update of all parameters with their bounds + the record in one more (`ssn_gen_apply_f32`)."""
        pens = self.gen.last_penalties

        def grads_and_loss(pieces):
            return genops.gen_grads(pieces['parts'], dmean, pens, self.dynamics_cost, self.rate_cost, nv=pieces['nv'],
                                    g_ext=pieces.get('g_ext'), ext_base=pieces.get('ext_base'), zin=pieces.get('zin'))

        def apply(gl, gate):
            _, _, opt = self.gen_updaters[st.names[0]].begin_step(st.params[st.names[0]])
            opt.reserved = int(gate)          # bit 0: no update at all when a gradient element is not finite (record[n] = NaN)
            clib.check(clib.libssnode.ssn_gen_apply_f32(st.flat.data_ptr(), gl.data_ptr(), st.m.data_ptr(), st.v.data_ptr(),
                                                        st.n, ctypes.byref(opt), st.lo.data_ptr(), st.hi.data_ptr(),
                                                        st.record.data_ptr(), clib.stream_ptr()), 'ssn_gen_apply_f32')
            return opt

        pieces = self.gen.backward(gx, self.dynamics_cost, self.rate_cost, raw=True)
        gl = grads_and_loss(pieces)
        carry = self._take_carry()
        self.reducer.mean_(*_with_carry([gl], carry))
        st.upload_changed(self.gen)
        opt = apply(gl, gate=True)
        # the record's copy is queued BEFORE the next step's forward and waited for by its own event: a plain .cpu() behind the
        # forward would wait for the forward too
        ticket = self._gen_records.post(st.record if carry is None else torch.cat([st.record, carry]))
        self._next_ctx = self._prequeue_next_disc()
        self._arrived_with_gen, host = _split_carry(ticket.wait(), carry is not None)
        if np.isnan(host[-1]) and np.isfinite(host[:-1]).all() and self.gen.can_retry:
            # The update was withheld: the summed gradient is not finite.  With the fp16-split adjoint that is what a draw whose
            # adjoint grows by more than 2^8 within one Euler step gives (unstable dynamics: NaN by construction, never a
            # clamped value); the reference's fp32 arithmetic carries such a draw's large finite gradient.  So does the fp32
            # sweep: the refused draws are made again on it -- forward, adjoint, dL/dW; all draws when more than half were
            # refused -- and THAT gradient is applied, whatever it is.
            bad = self.gen.poisoned_draws()
            logger.warning('generator step %s: %d draws have an adjoint that grew by more than 2^8 within one Euler step, beyond '
                           'the lagged scale of the fp16-split sweep; they are recomputed on the fp32 kernels (gen_kernel '
                           'mfma-fp32 runs every step there)', getattr(info, 'gen_step', '?'), bad)
            self._next_ctx = None          # (prepared with the parameters the withheld update left: prepared again later)
            idx = self.gen.poisoned_draw_indices()
            nb = int(pieces['parts'].shape[0])
            if _SUBSET_RETRY and (0 < idx.numel() <= nb // 2 or (self.reducer.on and idx.numel() == 0)):
                # only the refused draws go through the fp32 kernels (a job-wide NaN may come from another rank's draws: then
                # this rank has nothing to redo); every other draw keeps the gradient pieces it has
                parts, g_ext = pieces['parts'], pieces.get('g_ext')
                if idx.numel():
                    sub = self.gen.backward(gx, self.dynamics_cost, self.rate_cost, raw=True, exact=True, subset=idx)
                    parts = parts.clone()
                    parts[idx] = sub['parts']
                    if g_ext is not None:
                        g_ext = g_ext.clone()
                        g_ext[idx] = sub['g_ext']
                pieces = dict(pieces, parts=parts, g_ext=g_ext)
            else:
                pieces = self.gen.backward(gx, self.dynamics_cost, self.rate_cost, raw=True, exact=True)
            gl = grads_and_loss(pieces)
            self.reducer.mean_(gl)
            opt = apply(gl, gate=False)
            host = st.record.cpu().numpy()
        for name in st.names:
            self.gen_updaters[name].commit_step(opt)
        return host

    def _single_gen_step(self, gen_step, critic_iters):
        self.gen_forward_watch, self.gen_train_watch, self.disc_train_watch = StopWatch(), StopWatch(), StopWatch()
        ctx = (self._take_prequeued() or self._prepare_disc()) if critic_iters > 0 else None
        prepared_gen = None
        self._acc_carry = None
        held = None            # data-parallel runs: the record of the step whose job-wide accuracy is still on its way
        for disc_step in range(critic_iters):
            last = disc_step + 1 == critic_iters
            # queue this step's critic update, THEN do the host work of the next step and queue its forward, and only
            # then wait for this step's scalars: the GPU always has the next forward queued (host RNG order unchanged)
            self._launch_disc(ctx)
            nxt = None if last else self._prepare_disc()
            if last:
                prepared_gen = self._prepare_gen(ctx.batch)    # reuses the LAST critic batch's conditions (cwgan.py:535-539)
            info = Namespace(is_discriminator=True, gen_step=gen_step, disc_step=disc_step)
            info = self._read_disc(info, ctx)
            if held is not None:
                if held.accuracy_pending:
                    held.accuracy, held.accuracy_pending = ctx.arrived_accuracy, False
                # (a held record is yielded after the NEXT step was read: the recorder must see its own norms, not that step's)
                self.disc.cache_param_nnorms(held.param_sqnorms)
                yield held
                held = None
            if info.accuracy_pending:
                held = info        # same order of records, one collective later
            else:
                if ctx.acc_deferred:
                    self._acc_carry = None      # (a skipped step has no accuracy: nothing to carry)
                self.disc.cache_param_nnorms(info.param_sqnorms)
                yield info
            ctx = nxt
        disc_info = info
        batch = info.batch
        info = Namespace(is_discriminator=False, gen_step=gen_step)
        info = self.train_generator(info, batch, prepared_gen)
        if held is not None:
            held.accuracy, held.accuracy_pending = self._arrived_with_gen, False
        logger.debug('[Loss] Acc: %-9.3g D: %-9.3g G: %-9.3g [Time] Fwd: %.3g D: %.3g G: %.3g',
                     disc_info.accuracy, disc_info.disc_loss, info.gen_loss, self.gen_forward_watch.mean(),
                     self.disc_train_watch.mean(), self.gen_train_watch.mean())
        if held is not None:
            self.disc.cache_param_nnorms(held.param_sqnorms)
            yield held
        yield info

    def learning(self, start_step=0):
        """wgan.py:439-444: `critic_iters_init` critic steps before generator step 0, then `critic_iters`.
        `start_step` > 0 continues a run restored with `load_state_dict` (no second initial critic phase)."""
        if start_step == 0:
            yield from self._single_gen_step(0, self.critic_iters_init)
        for gen_step in itertools.count(max(start_step, 1)):
            yield from self._single_gen_step(gen_step, self.critic_iters)

    # -- checkpoints (not in the reference: its runs cannot be resumed) -------------------------------------
    def state_dict(self):
        """Everything a bit-identical continuation needs: generator and critic parameters, the optimizer states,
        the host RandomState (shared with the minibatch sampler) and the device noise generator."""
        kind, keys, pos, has_gauss, cached = (self._rng_before_predraw if self._predrawn is not None
                                              else self.rng.get_state())
        d = dict(gen={name: np.array(value) for name, value in self.gen.get_all_params()},
                 disc=self.disc.get_flat(), disc_updater=self.disc_updater.state_dict(),
                 gen_updaters={name: self.gen_updaters[name].state_dict() for name in self._pnames},
                 rng=dict(kind=kind, keys=keys, pos=pos, has_gauss=has_gauss, cached=cached))
        if self.gen._zgen is not None:
            d['zgen'] = self.gen._zgen.get_state()
        # explicit state that changes what a continuation computes: the kernel family (operand precision) and the job size
        d['gen_kernel'] = self.gen.gen_kernel
        d['world'] = self.reducer.world
        return d

    def load_state_dict(self, d):
        self._predrawn = self._rng_before_predraw = self._next_ctx = None
        self.gen.set_params(d['gen'])
        self.disc.set_flat(np.asarray(d['disc']))
        self.disc_updater.load_state_dict(d['disc_updater'])
        for name in self._pnames:
            self.gen_updaters[name].load_state_dict(d['gen_updaters'][name])
        r = d['rng']
        self.rng.set_state((str(r['kind']), np.asarray(r['keys'], dtype='uint32'), int(r['pos']), int(r['has_gauss']),
                            float(r['cached'])))
        if self.gen._zgen is not None and 'zgen' in d:
            z = d['zgen']
            if not (isinstance(z, dict) and 'seed' in z and 'position' in z):
                # format 1 of round 1 kept a torch.Generator state (uint8 array) here; the stream is a different one now
                raise KnownError('this checkpoint holds the device-noise state of an earlier format (a torch.Generator state '
                                 'array, not a Philox seed/position pair); it cannot be continued with --z-device-seed',
                                 exit_code=5)
            self.gen._zgen.set_state(z)
        for key, mine in (('gen_kernel', self.gen.gen_kernel), ('world', self.reducer.world)):
            if key in d and d[key] != mine:
                logger.warning('checkpoint was written with %s = %r, this run has %r: the continuation will not reproduce the '
                               'uninterrupted run bit for bit%s', key, d[key], mine,
                               ' (each rank draws other rows of the noise stream)' if key == 'world' else '')

    CHECKPOINT_VERSION = 2          # 2: Philox (seed, position) device-noise state, gen_kernel and world recorded

    def save_checkpoint(self, path, gen_step):
        tmp = path + '.tmp'
        with open(tmp, 'wb') as f:
            pickle.dump(dict(version=self.CHECKPOINT_VERSION, gen_step=int(gen_step), state=self.state_dict()), f, protocol=4)
        os.replace(tmp, path)

    def load_checkpoint(self, path):
        """Restore a checkpoint (after `set_dataset`); returns the generator step to continue WITH."""
        with open(path, 'rb') as f:
            ck = pickle.load(f)
        if not isinstance(ck, dict) or ck.get('version') not in (1, self.CHECKPOINT_VERSION) or 'state' not in ck:
            raise KnownError('{} is not a checkpoint this version can read (format version {!r}; known: 1, {})'
                             .format(path, ck.get('version') if isinstance(ck, dict) else None, self.CHECKPOINT_VERSION),
                             exit_code=5)
        self.load_state_dict(ck['state'])
        return ck['gen_step'] + 1


def make_gan(config):
    """make_gan(config: dict) -> (GAN, dict): build the GAN and return the unconsumed part of `config`
    (cwgan.py:555-614).  ``config['gen']`` / ``config['disc']`` hold the trainer options with the reference's
    names (learning_rate, update_name, dynamics_cost, rate_cost, J_min..S_max, rate_penalty_threshold;
    layers, normalization, nonlinearity, rate_penalty_bound, ...)."""
    kwargs = dict(DEFAULT_PARAMS, **config)
    gen_cfg = dict(DEFAULT_PARAMS['gen'], **config.get('gen', {}))
    disc_cfg = dict(DEFAULT_PARAMS['disc'], **config.get('disc', {}))
    kwargs.pop('gen', None)
    kwargs.pop('disc', None)
    take = kwargs.pop

    num_models = take('num_models')
    probes_per_model = take('probes_per_model')
    bandwidths = take('bandwidths')
    contrasts = take('contrasts')
    # (the command line's --gen-kernel arrives as gen['kernel']: run scripts group their gen_* options; configs written
    # by hand may also say gen_kernel at the top level)
    gen_kernel = gen_cfg.pop('kernel', None) or take('gen_kernel', 'auto')
    kwargs.pop('gen_kernel', None)
    gen, ssn_type = build_generator(kwargs, gen_kernel, len(bandwidths),
                                    num_models // GradientAllReducer().world * probes_per_model)
    for key in ('V_min', 'V_max'):
        kwargs.pop(key, None)
    rate_penalty_threshold = gen_cfg.pop('rate_penalty_threshold')
    disc_rate_penalty_bound = disc_cfg.pop('rate_penalty_bound')
    seed = take('seed', 0)
    disc = Critic(nx=len(bandwidths), layers=disc_cfg.pop('layers', []),
                  normalization=disc_cfg.pop('normalization', 'none'),
                  nonlinearity=disc_cfg.pop('nonlinearity', 'rectify'),
                  hide_cell_type=take('hide_cell_type'),
                  precision=disc_cfg.pop('precision', 'fp32'),
                  seed=disc_cfg.pop('init_seed', seed), net_options=disc_cfg.pop('net_options', None))
    parts = generator_trainer_parts(gen_cfg, ssn_type)
    disc_updater = updater_from(disc_cfg)
    if gen_cfg or disc_cfg:
        raise ValueError('Unknown trainer options: gen={} disc={}'.format(sorted(gen_cfg), sorted(disc_cfg)))
    gan = ConditionalBPTTWassersteinGAN(
        gen=gen, disc=disc, disc_updater=disc_updater, bandwidths=bandwidths, contrasts=contrasts,
        norm_probes=take('norm_probes'), e_ratio=take('e_ratio'),
        include_inhibitory_neurons=take('include_inhibitory_neurons'),
        rate_penalty_threshold=rate_penalty_threshold,
        num_models=num_models, probes_per_model=probes_per_model,
        critic_iters_init=take('critic_iters_init'), critic_iters=take('critic_iters'),
        lipschitz_cost=take('lipschitz_cost'), disc_rate_penalty_bound=disc_rate_penalty_bound, seed=seed, **parts)
    return gan, kwargs

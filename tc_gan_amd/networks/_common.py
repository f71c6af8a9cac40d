"""What the BPTT trainers share outside their loops: the defaults and stimulus-grid helpers of ``tc_gan/networks/wgan.py``
(DEFAULT_PARAMS 39-63, grid_stimulator_inputs 293-296, probes_from_stim_space 447-451; `networks.wgan` re-exports them), the
all-reduce of a data-parallel job, and the one builder of a generator with its bounds, updaters and costs that
`cwgan.make_gan`, `wgan.make_gan` and `moment_matching.generator_step_parts` call."""
import os

import numpy as np
import torch
import torch.distributed as dist

from .. import ssnode
from ..critic import Updater
from ..gradient_expressions.utils import sample_sites_from_stim_space
from ..utils import cartesian_product
from .ssn import TuningCurveGenerator

# networks/wgan.py:39-63
DEFAULT_PARAMS = dict(
    bandwidths=ssnode.DEFAULT_PARAMS['bandwidths'],
    contrasts=ssnode.DEFAULT_PARAMS['contrast'],
    smoothness=ssnode.DEFAULT_PARAMS['smoothness'],
    sample_sites=[0],
    # Stimulator:
    num_sites=ssnode.DEFAULT_PARAMS['N'],
    # Model / SSN:
    k=ssnode.DEFAULT_PARAMS['k'],
    n=ssnode.DEFAULT_PARAMS['n'],
    io_type='asym_tanh',
    tau_E=10,
    tau_I=1,
    dt=0.1,
    seqlen=1200,
    batchsize=1,
    skip_steps=1000,
    gen=dict(
        rate_cost=0.01,
        rate_penalty_threshold=200.0,
    ),
    disc=dict(
        rate_penalty_bound=-1.0,
    ),
)


def grid_stimulator_inputs(contrasts, bandwidths, batchsize):
    """networks/wgan.py:293-296 -> (stimulator_contrasts, stimulator_bandwidths), each (batchsize, NC*NB)."""
    product = cartesian_product(contrasts, bandwidths)
    return np.tile(product.reshape((1,) + product.shape), (batchsize,) + (1,) * product.ndim).swapaxes(0, 1)


def probes_from_stim_space(stim_locs, num_sites, include_inhibitory_neurons):
    """networks/wgan.py:447-451."""
    probes = sample_sites_from_stim_space(stim_locs, num_sites)
    if include_inhibitory_neurons:
        probes.extend(np.array(probes) + num_sites)
    return probes


class GradientAllReducer(object):
    """One flat-buffer all-reduce (mean over ranks) per update; identity without torch.distributed."""

    def __init__(self):
        self.dist = dist
        # (TCGAN_DIST_SINGLE_RANK=1: run the collectives in a one-rank group as well -- the mean over one rank is the
        # identity; bench.py uses it to put the all-reduce path through RCCL on a one-GPU box)
        self.on = dist.is_available() and dist.is_initialized() and (
            dist.get_world_size() > 1 or os.environ.get('TCGAN_DIST_SINGLE_RANK') == '1')
        self.world = dist.get_world_size() if self.on else 1
        self.rank = dist.get_rank() if self.on else 0
        # per-phase timing for multi-GPU diagnosis (bench.py --gpus N): device time between two events around every
        # collective, summed on demand; off by default (two event records per update)
        self.timed = False
        self._events = []
        self.calls = 0                         # collectives issued so far
        self._flats = {}                       # flat buffers of `mean_`, one per total size

    def collective_ms(self):
        """Device milliseconds spent in the all-reduces since the last call (synchronises)."""
        if not self._events:
            return 0.0
        torch.cuda.synchronize()
        total = sum(a.elapsed_time(b) for a, b in self._events)
        self._events = []
        return total

    def _sum(self, t):
        """One all-reduce (sum) of `t`, in stream order; timed between two events when `self.timed`."""
        self.calls += 1
        if self.timed and t.is_cuda:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
            self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
            ev[1].record()
            self._events.append(ev)
        else:
            self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
        if self.world > 1:
            t /= self.world

    def mean_(self, *tensors):
        """In-place mean over ranks of several tensors through ONE collective.  A single contiguous fp32 tensor is reduced
        where it is; several go through a persistent flat fp32 buffer (one per total size: a step alternates between a
        few sizes, nothing is allocated per update)."""
        if not self.on:
            return
        if len(tensors) == 1 and tensors[0].dtype == torch.float32 and tensors[0].is_contiguous():
            self._sum(tensors[0])
            return
        n = sum(t.numel() for t in tensors)
        key = (n, tensors[0].device)
        flat = self._flats.get(key)
        if flat is None:
            flat = self._flats[key] = torch.empty(n, device=tensors[0].device, dtype=torch.float32)
        off = 0
        for t in tensors:
            flat[off:off + t.numel()].copy_(t.reshape(-1))
            off += t.numel()
        self._sum(flat)
        off = 0
        for t in tensors:
            t.copy_(flat[off:off + t.numel()].reshape(t.shape))
            off += t.numel()


def _v_bounds(v_min, v_max, ssn_type):
    """Clip bounds of the input-variability parameter V (wgan.py:244-251, 263-283): one (V_E, V_I) pair each for
    'heteroin' -- per element, like numpy's broadcasting clip in the reference -- a scalar each for 'deg-heteroin'."""
    if ssn_type == 'heteroin':
        return (np.broadcast_to(np.asarray(v_min, dtype='float64'), (2,)).copy(),
                np.broadcast_to(np.asarray(v_max, dtype='float64'), (2,)).copy())
    return float(np.min(v_min)), float(np.max(v_max))


UPDATER_KEYS = ('learning_rate', 'update_name', 'update_config', 'reg_l2_penalty', 'reg_l2_decay', 'reg_l1_penalty',
                'reg_l1_decay')


def updater_from(cfg):
    """An `Updater` from the updater options present in `cfg` (consumed)."""
    return Updater(**{k: cfg.pop(k) for k in UPDATER_KEYS if k in cfg})


def build_generator(kwargs, gen_kernel, num_tcdom, batchsize, probes=None, include_rate_penalty=None):
    """The `TuningCurveGenerator` of a trainer from the top level of its config (consumed in place): ssn_type / ssn_impl,
    V0 / V / dist_in, the model and solver options.  `batchsize` is this rank's share; `include_rate_penalty` None: the
    config's.  Returns (gen, ssn_type)."""
    take = kwargs.pop
    ssn_type = take('ssn_type', 'default')
    ssn_impl = take('ssn_impl', 'default')
    if ssn_impl not in ('default', 'mapclone'):     # 'mapclone' is the same arithmetic organised differently (ssn.py:25-30)
        raise ValueError('Unknown ssn_impl: {}'.format(ssn_impl))
    if 'V0' in kwargs:                              # cwgan.py:570-571, wgan.py:471-472
        kwargs['V'] = kwargs.pop('V0')
    V = kwargs.pop('V', 0)
    dist_in = kwargs.pop('dist_in', 'bernoulli')
    reducer = GradientAllReducer()
    gen = TuningCurveGenerator(
        num_sites=take('num_sites'), num_tcdom=num_tcdom, smoothness=take('smoothness'),
        J=take('J0'), D=take('D0'), S=take('S0'), k=take('k'), n=take('n'),
        tau_E=take('tau_E'), tau_I=take('tau_I'), dt=take('dt'), io_type=take('io_type'),
        seqlen=take('seqlen'), skip_steps=take('skip_steps'), batchsize=batchsize, probes=probes,
        include_rate_penalty=take('include_rate_penalty', True) if include_rate_penalty is None else include_rate_penalty,
        include_time_avg=take('include_time_avg', False), unroll_scan=take('unroll_scan', False),
        dtype=take('gen_dtype', 'float32'), z_device_seed=take('z_device_seed', None), shard=(reducer.rank, reducer.world),
        ssn_type=ssn_type, V=V, dist_in=dist_in, gen_kernel=gen_kernel, z_host_draw=take('z_host_draw', False))
    return gen, ssn_type


def generator_trainer_parts(cfg, ssn_type):
    """From the trainer options `cfg` (consumed): the costs, the clip bounds per parameter (wgan.py:244-251, 263-283) and one
    updater per parameter, as the keyword arguments the trainers' constructors take."""
    dynamics_cost = cfg.pop('dynamics_cost', 1.0)
    rate_cost = cfg.pop('rate_cost')
    bounds = {name: (cfg.pop(name + '_min', 1e-3), cfg.pop(name + '_max', 10.0)) for name in 'JDS'}
    bounds['V'] = _v_bounds(cfg.pop('V_min', 0), cfg.pop('V_max', 1), ssn_type)
    upd_cfg = {k: cfg.pop(k) for k in UPDATER_KEYS if k in cfg}
    return dict(gen_updaters={name: Updater(**upd_cfg) for name in 'VJDS'}, param_bounds=bounds,
                dynamics_cost=dynamics_cost, rate_cost=rate_cost)

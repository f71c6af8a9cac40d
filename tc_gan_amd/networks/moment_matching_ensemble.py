"""Several independent moment-matching runs trained together in one GPU loop.

K members, each a `BPTTMomentMatcher` of its own -- its own noise stream, parameters, hyper-parameters and data -- whose draws
share the launches of a generator step: member k owns the draws [k B, (k + 1) B) of one batch of K B.  Per step:

  * noise and W: one draw launch per member (its RandomState continued on the device, or its Philox stream), each writing the
    member's rows of one W buffer with the member's J, D, S;
  * the stimulus (heterogeneous input: `ssn_ens_stimulus_hetero_f32`, V of the draw's member), the forward, the adjoint sweep
    (one launch per run of adjacent members with equal dynamics / rate costs -- one when the costs are shared), dL/dW and the
    chain rule through make_W (`ssn_ens_jds_grad_f32`): one launch each over the K B draws;
  * the moment loss (`ssn_ens_moments_f32`), the gradient assembly (`ssn_ens_gen_grads_f32`) and the optimizer
    (`ssn_ens_apply_f32`): segmented kernels, one launch each, sums over each member's own rows;
  * ONE read of the record buffer (csrc/ssn_ensemble.hip) for all members.

The part of a step that does not depend on the loss is `EnsembleGeneratorStep`, which the ensemble of sliced Wasserstein runs
(networks/sliced_wasserstein_ensemble.py) shares; `EnsembleMomentMatcher` adds the moment loss and its gradient assembly.

With a fixed generator kernel every draw is computed independently of the rest of the batch, so a member's step is its single
run's step; the sums over a member's draws may add in another order (fp64).  `auto` is resolved once, for the ensemble's batch
of K B draws (`resolve_gen_kernel`), and every member records the kernel that ran.
"""
import copy
import ctypes
import itertools
import math

import numpy as np
import torch

from .. import clib, genops
from ..clib import libssnode
from ..stimuli import stimulus_batch
from ..utils import Namespace, StopWatch, to_device
from .gen_state import flat_bounds
from .moment_matching import DEFAULT_PARAMS, make_moment_matcher
from .ssn import TAIL_KINDS, _ticket_finisher

#: options a member may set for itself (run/options.py names; run_config keys)
MEMBER_KEYS = frozenset(
    ['seed', 'truth_seed', 'true_ssn_options', 'truth_size', 'J0', 'D0', 'S0', 'V0']
    + ['{}_{}'.format(p, b) for p in 'JDSV' for b in ('min', 'max')]
    + ['learning_rate', 'reg_l2_penalty', 'reg_l2_decay', 'reg_l1_penalty', 'reg_l1_decay', 'lam', 'moment_weight_type',
       'moment_weights_regularization', 'dynamics_cost', 'rate_cost', 'quit_JDS_threshold', 'z_device_seed'])

#: options every member shares: they fix the kernels' shapes or their launch parameters
SHARED_KEYS = frozenset([
    'num_sites', 'bandwidths', 'n_bandwidths', 'contrasts', 'sample_sites', 'include_inhibitory_neurons', 'batchsize', 'seqlen',
    'skip_steps', 'io_type', 'k', 'n', 'tau_E', 'tau_I', 'dt', 'ssn_type', 'dist_in', 'rate_penalty_threshold', 'update_name',
    'gen_kernel', 'iterations'])


class MemberOptionError(ValueError):
    pass


def validate_member_overrides(member_overrides, member_keys=MEMBER_KEYS, shared_keys=SHARED_KEYS):
    """A list of dicts, one per member: every key must be one a member may set (`member_keys`); a shared key or an unknown
    one is refused with an error that names it.  `z_device_seed` is given for all members or for none."""
    if not isinstance(member_overrides, (list, tuple)) or not member_overrides:
        raise MemberOptionError('members: a non-empty list of dicts of per-member options is needed')
    for i, over in enumerate(member_overrides):
        if not isinstance(over, dict):
            raise MemberOptionError('member {}: a dict of options is needed, got {!r}'.format(i, over))
        for key in over:
            if key in shared_keys:
                raise MemberOptionError('member {}: {!r} is shared by all members of an ensemble and may not be set per member'
                                        .format(i, key))
            if key not in member_keys:
                raise MemberOptionError('member {}: unknown option {!r}'.format(i, key))
    with_seed = [('z_device_seed' in over and over['z_device_seed'] is not None) for over in member_overrides]
    if any(with_seed) and not all(with_seed):
        raise MemberOptionError('z_device_seed must be given for all members or for none')
    return [dict(over) for over in member_overrides]


def resolve_gen_kernel(config, num_members):
    """The explicit kernel name the ensemble runs: `gen_kernel` as given, or for 'auto' the family the library picks for the
    ensemble's batch of num_members x batchsize draws (host arithmetic only, `ssn_gen_forward_variant`)."""
    name = config.get('gen_kernel', 'auto')
    if name == 'duo-fused':
        raise ValueError("gen_kernel 'duo-fused' is not available to ensembles; use 'duo'")
    if name != 'auto':
        clib.gen_kernel_code(name)
        return name
    if config.get('gen_dtype', 'float32') != 'float32':
        raise ValueError('ensembles run the float32 generator only')
    nb = len(config['bandwidths']) * len(config['contrasts'])
    return genops.resolve_kernel(int(config['batchsize']) * int(num_members), nb, 2 * int(config['num_sites']),
                                 genops.gen_params_of(dict(DEFAULT_PARAMS, **config)), save=True)


def member_config(shared_config, override):
    """The config of one member: the shared config with the member's options over it (J0 / D0 / S0 broadcast to 2 x 2)."""
    cfg = copy.deepcopy(dict(shared_config))
    cfg.update(copy.deepcopy(override))
    for key in ('J0', 'D0', 'S0'):
        if key in override:
            cfg[key] = np.broadcast_to(np.asarray(cfg[key], dtype='float64'), (2, 2)).tolist()
    return cfg


def _f32_ptrs(*arrays):
    return [(ctypes.c_float * 4)(*np.asarray(a, dtype='double').reshape(4)) for a in arrays]


def _jds16(J, D, S):
    """J, D, 1 / (2 S^2), 1 / S^3 in fp32, rounded as launch_jds_grad rounds them (ssn_ens_jds_grad_f32)."""
    s = np.asarray(S, dtype=np.float32).reshape(4)
    two, one = np.float32(2), np.float32(1)
    return np.concatenate([np.asarray(J, dtype=np.float32).reshape(4), np.asarray(D, dtype=np.float32).reshape(4),
                           one / (two * s * s), one / (s * s * s)]).astype(np.float32)


class EnsembleGeneratorStep(object):
    """What an ensemble of K critic-free BPTT trainers (`members`, each a `GeneratorStepTrainer`) does per step whatever its loss
    is: the draw, the stimulus, the forward over the K B draws, the scatter of the loss gradient `gx`, the adjoint sweep per run
    of equal costs, dL/dW, `ssn_ens_jds_grad_f32`, the update (`ssn_ens_apply_f32`), the ONE read of the record buffer, and
    `remove`.  A subclass gives two hooks -- `_loss` (tuning curves -> gx, and what it writes to the record) and `_assemble`
    (the gradient assembly that puts L0, the penalties and the loss into the record) -- and says what its record holds:
    `record_moments` (the D of `ssn_ens_record_doubles`), `_record_extra` (doubles appended to a row), `_member_state`
    (per-member device arrays rebuilt when a member leaves) and `_info_fields` (a member's row -> the fields of its `info`).
    `learning()` yields, per step, the list of one `Namespace` per ACTIVE member; `remove(i)` takes member i out of the later
    steps (its run has ended)."""

    def __init__(self, members, gen_kernel, dynamics_costs, rate_costs, rests=None):
        self.members = list(members)
        self.gen_kernel = gen_kernel
        self.dynamics_costs = [float(c) for c in dynamics_costs]
        self.rate_costs = [float(c) for c in rate_costs]
        self.rests = rests
        self.active = list(range(len(self.members)))
        g0 = self.members[0].gen
        self.B, self.N, self.M = g0.batchsize, g0.num_sites, g0.num_neurons
        self.NB = g0.num_tcdom
        self.heteroin = g0.heteroin
        self.nv = 0 if not self.heteroin else (2 if g0.ssn_type == 'heteroin' else 1)
        self.P = self.nv + 12
        self.D = self.record_moments()
        self.R0 = int(libssnode.ssn_ens_record_doubles(self.D, self.P))
        self.R = self.R0 + self._record_extra()
        self._state = None
        self._inputs = {}
        self.step_count = 0

    num_members = property(lambda self: len(self.members))

    # -- device state of the active members -------------------------------------------------------------------------------------
    def _build_state(self):
        mms = [self.members[i] for i in self.active]
        dev = dict(device='cuda')
        params = np.stack([np.asarray(mm.gen.get_flat_param_values(), dtype='float64') for mm in mms]).astype(np.float32)
        lo, hi = zip(*[flat_bounds([np.size(value) for _, value in mm.gen.get_all_params()],
                                   [mm.param_bounds[name] for name, _ in mm.gen.get_all_params()]) for mm in mms])
        st = dict(p=torch.as_tensor(params, **dev).contiguous(),
                  clip_lo=torch.as_tensor(np.asarray(lo, dtype=np.float32), **dev).contiguous(),
                  clip_hi=torch.as_tensor(np.asarray(hi, dtype=np.float32), **dev).contiguous(),
                  costs=torch.as_tensor(np.asarray([[self.dynamics_costs[i], self.rate_costs[i]] for i in self.active]),
                                        dtype=torch.float64, **dev).contiguous())
        if self._state is not None and self._state['index'] is not None:
            old = self._state
            keep = torch.as_tensor([old['index'].index(i) for i in self.active], device='cuda', dtype=torch.int64)
            st['s1'], st['s2'] = old['s1'].index_select(0, keep).contiguous(), old['s2'].index_select(0, keep).contiguous()
        else:
            st['s1'], st['s2'] = torch.zeros_like(st['p']), torch.zeros_like(st['p'])
        st['index'] = list(self.active)
        st.update(self._member_state(mms))
        self._state = st

    def remove(self, i):
        """Member i leaves the ensemble: the later steps run over the others."""
        if i in self.active:
            self.active.remove(i)
            if self.active:
                self._build_state()

    def _stimulus(self, K):
        """(bw, con, ext without amplification) of K members' draws, uploaded / formed once per K."""
        hit = self._inputs.get(K)
        if hit is None:
            mm = self.members[self.active[0]]
            bw = to_device(np.ascontiguousarray(np.tile(np.asarray(mm.stimulator_bandwidths), (K, 1))), torch.float32)
            con = to_device(np.ascontiguousarray(np.tile(np.asarray(mm.stimulator_contrasts), (K, 1))), torch.float32)
            ext = stimulus_batch(bw, con, mm.gen.smoothness, self.N, dtype='float32')
            hit = self._inputs[K] = (bw, con, ext)
        return hit

    # -- one step -----------------------------------------------------------------------------------------------------------
    def _draw(self, K):
        """z and W of every active member into its rows (and zs_in of the heterogeneous-input models)."""
        B, M, N = self.B, self.M, self.N
        W = torch.empty((K * B, M, M), device='cuda', dtype=torch.float32)
        z = torch.empty_like(W)
        zin = torch.empty((K * B, M), device='cuda', dtype=torch.float32) if self.heteroin else None
        amp = torch.empty((B, M), device='cuda', dtype=torch.float32) if self.heteroin else None
        row = B * M * M * 4
        stream = clib.stream_ptr()
        for j, i in enumerate(self.active):
            gen = self.members[i].gen
            J, D, S = _f32_ptrs(gen.J, gen.D, gen.S)
            Wp, zp = W.data_ptr() + j * row, z.data_ptr() + j * row
            zinp = zin.data_ptr() + j * B * M * 4 if self.heteroin else None
            if gen._zgen is not None:
                clib.check(libssnode.ssn_build_w_philox_f32(gen._zgen.seed, gen._zgen.take(B * M * M), J, D, S, Wp, zp, B, N, stream),
                           'ssn_build_w_philox_f32')
                if self.heteroin:
                    v = gen._input_variability()
                    clib.check(libssnode.ssn_philox_amp_f32(gen._zgen.seed, gen._zgen.take(B * M), v.data_ptr(), zinp, amp.data_ptr(),
                                                            B * M, M, int(gen.dist_in == 'bernoulli'), stream), 'ssn_philox_amp_f32')
                continue
            rng = self.members[i].rng
            kind, key, pos, has_gauss, cached = rng.get_state()
            key = np.ascontiguousarray(key, dtype=np.uint32)
            ticket = ctypes.c_int(-1)
            if self.heteroin:
                clib.check(libssnode.ssn_build_w_mt19937_tail_begin_f32(
                    key.ctypes.data, int(pos), B, 0, B, J, D, S, Wp, zp, N, TAIL_KINDS[gen.dist_in], zinp, stream,
                    ctypes.byref(ticket)), 'ssn_build_w_mt19937_tail_begin_f32')
            else:
                clib.check(libssnode.ssn_build_w_mt19937_begin_f32(key.ctypes.data, int(pos), B, 0, B, J, D, S, Wp, zp, N, stream,
                                                                   ctypes.byref(ticket)), 'ssn_build_w_mt19937_begin_f32')
            rng._defer(_ticket_finisher(ticket.value, key, kind, has_gauss, cached))
        return W, z, zin

    def _cost_runs(self):
        """(first, last + 1, dynamics_cost, rate_cost) of each run of adjacent active members with equal costs."""
        runs = []
        for j, i in enumerate(self.active):
            c = (self.dynamics_costs[i], self.rate_costs[i])
            if runs and runs[-1][2:] == c:
                runs[-1] = (runs[-1][0], j + 1) + c
            else:
                runs.append((j, j + 1) + c)
        return runs

    def train_step(self, step):
        if self._state is None or self._state['index'] != self.active:
            self._build_state()
        watch = StopWatch()
        with watch:
            infos = self._step(step)
        for info in infos:
            info.train_time = watch.sum()
        return infos

    def _step(self, step):
        K, B, M, N, NB, D, P, R = len(self.active), self.B, self.M, self.N, self.NB, self.D, self.P, self.R
        st = self._state
        mm0 = self.members[self.active[0]]
        gen0 = mm0.gen
        stream = clib.stream_ptr()
        f32 = dict(device='cuda', dtype=torch.float32)
        W, z, zin = self._draw(K)
        bw, con, ext_base = self._stimulus(K)
        if self.heteroin:
            vpop = np.stack([np.broadcast_to(np.asarray(self.members[i].gen.V, dtype='float64'), 2) for i in self.active])
            v = to_device(np.ascontiguousarray(vpop.astype(np.float32)), torch.float32)
            ext = torch.empty((K * B, NB, M), **f32)
            clib.check(libssnode.ssn_ens_stimulus_hetero_f32(bw.data_ptr(), con.data_ptr(), float(gen0.smoothness), zin.data_ptr(),
                                                             v.data_ptr(), ext.data_ptr(), K, B, NB, N, stream),
                       'ssn_ens_stimulus_hetero_f32')
        else:
            ext = ext_base
        # forward over the K B draws (the kernel the members record)
        gp = gen0.gen_params(mm0.rate_penalty_threshold)
        T, skip = gp.seqlen, gp.skip_steps
        ta3 = torch.empty((3, K * B, NB, M), **f32)
        traj = torch.empty((K * B, NB, T, M), **f32)
        df = torch.empty_like(traj)
        clib.check(libssnode.ssn_gen_forward_f32(W.data_ptr(), ext.data_ptr(), ta3[0].data_ptr(), ta3[1].data_ptr(), ta3[2].data_ptr(),
                                                 traj.data_ptr(), df.data_ptr(), K * B, NB, M, ctypes.byref(gp), stream),
                   'ssn_gen_forward_f32')
        self.last_time_avg = ta3[0]
        tc, _, probes = gen0._probe(ta3[0])
        tc = tc.contiguous()
        self.last_tuning_curves = tc
        # the loss and its gradient, member by member
        rec = torch.empty((K, R), device='cuda', dtype=torch.float64)
        gx = self._loss(tc, rec, K)
        g_ta = torch.zeros((K * B, NB, M), **f32)
        g_ta[:, :, probes] = gx.reshape(K * B, NB, -1)
        # adjoint sweep: one launch per run of adjacent members with equal costs
        n_dyn, n_rate = B * (T - skip - 1) * NB * M, B * (T - skip) * NB * M
        g_ext = torch.empty((K * B, NB, M), **f32) if self.heteroin else None
        dmax = torch.empty((K * B,), **f32)
        tracked = ctypes.c_int(0)
        big, small = NB * T * M * 4, NB * M * 4
        for j0, j1, dc, rc in self._cost_runs():
            o = j0 * B
            clib.check(libssnode.ssn_gen_backward_max_f32(
                W.data_ptr() + o * M * M * 4, traj.data_ptr() + o * big, df.data_ptr() + o * big, g_ta.data_ptr() + o * small,
                g_ext.data_ptr() + o * small if self.heteroin else None, dmax.data_ptr() + o * 4, ctypes.byref(tracked),
                dc / max(n_dyn, 1), rc / n_rate, (j1 - j0) * B, NB, M, ctypes.byref(gp), stream), 'ssn_gen_backward_max_f32')
        gW = genops.weight_grad(df, traj, dmax=dmax if tracked.value else None, xmax=genops.rate_bound(gp))
        p16 = to_device(np.ascontiguousarray(np.stack([_jds16(self.members[i].gen.J, self.members[i].gen.D, self.members[i].gen.S)
                                                       for i in self.active])), torch.float32)
        parts = torch.empty((K * B, 4, 3), device='cuda', dtype=torch.float64)
        clib.check(libssnode.ssn_ens_jds_grad_f32(gW.data_ptr(), z.data_ptr(), p16.data_ptr(), parts.data_ptr(), K, B, N, stream),
                   'ssn_ens_jds_grad_f32')
        grads = torch.empty((K, P), **f32)
        a = clib.EnsGrads(K=K, B=B, nv=self.nv, NB=NB, M=M, D=D, part=parts.data_ptr(),
                          g_ext=g_ext.data_ptr() if self.heteroin else None, ext_base=ext_base.data_ptr() if self.heteroin else None,
                          zin=zin.data_ptr() if self.heteroin else None, dyn_row=ta3[1].data_ptr(), rate_row=ta3[2].data_ptr(),
                          scale_dyn=(1.0 / n_dyn) if n_dyn > 0 else float('nan'), scale_rate=1.0 / n_rate,
                          costs=st['costs'].data_ptr(), grads=grads.data_ptr(), rec=rec.data_ptr(), rstride=R)
        self._assemble(a)
        # the optimizer over all members' parameter vectors
        t = step + 1
        hyp = np.zeros((K, 8), dtype=np.float32)
        upd0 = mm0.gen_updaters['J']
        for j, i in enumerate(self.active):
            u = self.members[i].gen_updaters['J']
            lr = float(u.learning_rate)
            a_t = lr * math.sqrt(1.0 - math.pow(u.cfg['beta2'], t)) / (1.0 - math.pow(u.cfg['beta1'], t))
            hyp[j, :6] = (lr, a_t) + tuple(u.reg)
        hyp_dev = to_device(hyp, torch.float32)
        o = clib.EnsApply(K=K, P=P, kind=upd0.kind, beta1=upd0.cfg['beta1'], beta2=upd0.cfg['beta2'], eps=upd0.cfg['epsilon'],
                          rho=upd0.cfg['rho'], hyp=hyp_dev.data_ptr(), clip_lo=st['clip_lo'].data_ptr(),
                          clip_hi=st['clip_hi'].data_ptr(), p=st['p'].data_ptr(), s1=st['s1'].data_ptr(), s2=st['s2'].data_ptr(),
                          g=grads.data_ptr(), rec=rec.data_ptr(), rstride=R, rec_off=4 + 2 * D)
        clib.check(libssnode.ssn_ens_apply_f32(ctypes.byref(o), stream), 'ssn_ens_apply_f32')
        host = rec.cpu().numpy()                               # the one host synchronisation of the step
        infos = []
        for j, i in enumerate(self.active):
            mm, row = self.members[i], host[j]
            off = 4 + 2 * D
            new = row[off:off + P]
            k0 = 0
            for name, value in mm.gen.get_all_params():
                size = int(np.size(value))
                setattr(mm.gen, name, np.array(new[k0:k0 + size], dtype='float64').reshape(np.shape(value)))
                k0 += size
            for u in mm.gen_updaters.values():
                u.step = t
            infos.append(Namespace(step=step, member=i, loss=float(row[3 + 2 * D]), dynamics_penalty=float(row[1 + 2 * D]),
                                   rate_penalty=float(row[2 + 2 * D]), gradients=row[off + P:off + 2 * P].copy(),
                                   **self._info_fields(row)))
        return infos

    def prepare(self):
        """Nothing to compile."""

    def learning(self):
        for step in itertools.count():
            if not self.active:
                return
            yield self.train_step(step)

    # -- what a loss gives -----------------------------------------------------------------------------------------------------
    def record_moments(self):
        """The D of `ssn_ens_record_doubles(D, P)`: the moments a record row holds between L0 and the penalties."""
        raise NotImplementedError

    def _record_extra(self):
        """Doubles a record row holds behind the `ssn_ens_record_doubles(D, P)` of the library."""
        return 0

    def _member_state(self, mms):
        """dict of device arrays over the active members `mms`, rebuilt whenever a member leaves (into `self._state`)."""
        return {}

    def _loss(self, tc, rec, K):
        """tc (K B, D) device float32, the tuning curves of the K active members -> gx of the same shape; may write to `rec`."""
        raise NotImplementedError

    def _assemble(self, a):
        """`a`: the `clib.EnsGrads` of the step without the loss's own fields.  Launches the gradient assembly."""
        raise NotImplementedError

    def _info_fields(self, row):
        """The loss's own fields of a member's `info` from its record row (numpy fp64)."""
        return {}


class EnsembleMomentMatcher(EnsembleGeneratorStep):
    """K `BPTTMomentMatcher`s (`members`) trained by one loop (`EnsembleGeneratorStep`).  The fields of a member's `info` are a
    single run's: step, loss, rate_penalty, dynamics_penalty, gen_moments, train_time, plus `member`, the member's index."""

    def record_moments(self):
        return self.members[0].num_mom_conds

    def _member_state(self, mms):
        return dict(dm=torch.stack([mm._dm for mm in mms]).contiguous(), w=torch.stack([mm._w for mm in mms]).contiguous())

    def _loss(self, tc, rec, K):
        st, B, D = self._state, self.B, self.D
        sums = torch.empty((K, 2, D), device='cuda', dtype=torch.float64)
        gx = torch.empty_like(tc)
        clib.check(libssnode.ssn_ens_moments_f32(tc.data_ptr(), K, B, D, sums.data_ptr(), st['dm'].data_ptr(), st['w'].data_ptr(),
                                                 gx.data_ptr(), rec.data_ptr(), self.R, clib.stream_ptr()), 'ssn_ens_moments_f32')
        return gx

    def _assemble(self, a):
        a.data_moments, a.weights = self._state['dm'].data_ptr(), self._state['w'].data_ptr()
        clib.check(libssnode.ssn_ens_gen_grads_f32(ctypes.byref(a), clib.stream_ptr()), 'ssn_ens_gen_grads_f32')

    def _info_fields(self, row):
        D = self.D
        return dict(gen_moments=row[1:1 + 2 * D].reshape(2, D).copy())


def members_from_configs(configs, make_member):
    """One trainer per fully resolved member config through `make_member(config) -> (trainer, unconsumed config)`, with what an
    ensemble refuses: several ranks, z drawn on the host, a generator that is not float32, members on different kernels or on
    none by name.  Returns (members, rests, dynamics costs, rate costs, the kernel)."""
    members, rests, dcosts, rcosts = [], [], [], []
    for cfg in configs:
        if cfg.get('gen_dtype', 'float32') != 'float32':
            raise ValueError('ensembles run the float32 generator only')
        mm, rest = make_member(dict(cfg))
        if mm.reducer.on:
            raise ValueError('ensembles run in one process (no data-parallel ranks)')
        if mm.gen.z_host_draw:
            raise ValueError('ensembles draw z on the device (z_host_draw is not available)')
        members.append(mm)
        rests.append(rest)
        dcosts.append(mm.dynamics_cost)
        rcosts.append(mm.rate_cost)
    kernels = set(mm.gen.gen_kernel for mm in members)
    if len(kernels) != 1 or 'auto' in kernels:
        raise ValueError('the members of an ensemble run one explicit generator kernel, got {}'.format(sorted(kernels)))
    return members, rests, dcosts, rcosts, kernels.pop()


def ensemble_from_member_configs(configs):
    """The `EnsembleMomentMatcher` of fully resolved member configs (each what `make_moment_matcher` takes, all naming the
    same explicit `gen_kernel`)."""
    members, rests, dcosts, rcosts, kernel = members_from_configs(configs, make_moment_matcher)
    return EnsembleMomentMatcher(members, kernel, dcosts, rcosts, rests=rests)


def make_moment_matcher_ensemble(shared_config, member_overrides):
    """One `BPTTMomentMatcher` per member from the shared config (what `make_moment_matcher` takes) with the member's options
    over it (`validate_member_overrides`), all on the kernel `resolve_gen_kernel` picks for the ensemble.  Returns the
    `EnsembleMomentMatcher`; its `rests` are the members' unconsumed configs (the data-set options)."""
    overrides = validate_member_overrides(member_overrides)
    kernel = resolve_gen_kernel(shared_config, len(overrides))
    configs = []
    for over in overrides:
        cfg = member_config(shared_config, over)
        cfg['gen_kernel'] = kernel
        configs.append(cfg)
    return ensemble_from_member_configs(configs)

"""Several independent sliced Wasserstein runs trained together in one GPU loop.

K members, each a `BPTTSlicedWasserstein` of its own -- its own noise stream, parameters, hyper-parameters, truth, power and
direction seed -- whose draws share the launches of a generator step (`moment_matching_ensemble.EnsembleGeneratorStep`: member k
owns the draws [k B, (k + 1) B) of one batch of K B).  The loss of a step:

  * every member draws its L directions on its own `direction_rng` (`draw_slice_directions`) and its minibatch rows on its own
    `minibatch_rng` (the order of `utils.random_minibatches`); the host stacks the directions into ONE upload theta[K][L][D] and
    the row indices, offset into the concatenated truths of all members on the device, into ONE upload; one gather makes y;
  * `ssn_ens_swd_project_f32`, `ssn_ens_swd_match_f32`, `ssn_ens_swd_backproject_f32` (csrc/ssn_ens_swd.hip): the single run's
    kernels over the members, a member's values the bits of its single run;
  * `ssn_ens_gen_grads_l0_f32`: the gradient assembly with L0 = l0[k] from the match.

The host still reads ONE buffer per step: the record rows with loss_l[K][L] appended.  `truth_size` may differ per member.
"""
import ctypes

import numpy as np
import torch

from .. import clib
from ..analyzers.distdiff import draw_slice_directions
from ..clib import libssnode
from ..utils import to_device
from . import moment_matching_ensemble as mme
from .moment_matching_ensemble import EnsembleGeneratorStep, MemberOptionError, member_config, resolve_gen_kernel  # noqa: F401
from .sliced_wasserstein import make_sliced_wasserstein

_MOMENT_ONLY = frozenset(['lam', 'moment_weight_type', 'moment_weights_regularization'])

#: options a member may set for itself: the moment ensemble's without the moment loss's, with the sliced loss's
MEMBER_KEYS = (mme.MEMBER_KEYS - _MOMENT_ONLY) | frozenset(['swd_power', 'swd_direction_seed'])

#: options every member shares: the moment ensemble's, and the number of directions (a shape of the loss kernels)
SHARED_KEYS = mme.SHARED_KEYS | frozenset(['swd_directions'])


def validate_member_overrides(member_overrides):
    """`moment_matching_ensemble.validate_member_overrides` with this ensemble's keys."""
    return mme.validate_member_overrides(member_overrides, MEMBER_KEYS, SHARED_KEYS)


class EnsembleSlicedWasserstein(EnsembleGeneratorStep):
    """K `BPTTSlicedWasserstein`s (`members`, each after `set_dataset`) trained by one loop.  The fields of a member's `info`
    are those `SlicedWassersteinDriver` takes -- step, loss, swd, dynamics_penalty, rate_penalty, train_time -- plus
    `swd_per_direction` and `member`.  `match_form`: the form of `ssn_ens_swd_match_f32` (clib.SWD_FORM_*)."""

    def __init__(self, members, gen_kernel, dynamics_costs, rate_costs, rests=None, match_form=clib.SWD_FORM_AUTO):
        members = list(members)
        directions = set(mm.swd_directions for mm in members)
        if len(directions) != 1:
            raise ValueError('the members of an ensemble share swd_directions, got {}'.format(sorted(directions)))
        if len(members) > clib.ENS_SWD_MAX_MEMBERS:
            raise ValueError('{} members are more than the {} the loss kernels take'.format(len(members), clib.ENS_SWD_MAX_MEMBERS))
        self.L = directions.pop()
        self.match_form = match_form
        self.last_x = self.last_gx = None        # the tuning curves and the loss gradient of the last step, on the device
        super(EnsembleSlicedWasserstein, self).__init__(members, gen_kernel, dynamics_costs, rate_costs, rests=rests)

    def record_moments(self):
        return 0

    def _record_extra(self):
        return self.L

    def _member_state(self, mms):
        columns = set(int(mm.truth.shape[1]) for mm in mms)
        if len(columns) != 1:
            raise ValueError('the truths of the members differ in their columns: {}'.format(sorted(columns)))
        sizes = [int(mm.truth.shape[0]) for mm in mms]
        return dict(truth=torch.cat([mm.truth for mm in mms]).contiguous(),
                    truth_offset=np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64),
                    power=(ctypes.c_int * len(mms))(*[mm.swd_power for mm in mms]))

    def _loss(self, tc, rec, K):
        st, B, L = self._state, self.B, self.L
        mms = [self.members[i] for i in self.active]
        D = int(tc.shape[1])
        stream = clib.stream_ptr()
        theta = to_device(np.ascontiguousarray(np.stack([draw_slice_directions(mm.direction_rng, L, D) for mm in mms])), torch.float32)
        rows = np.concatenate([np.asarray(next(mm.minibatch_rows), dtype=np.int64) + off
                               for mm, off in zip(mms, st['truth_offset'])])
        y = st['truth'].index_select(0, to_device(rows, torch.int64)).contiguous()
        self.last_x = x = tc.to(torch.float32).contiguous()
        f32 = dict(device='cuda', dtype=torch.float32)
        proj = torch.empty((2, K * B, L), **f32)
        clib.check(libssnode.ssn_ens_swd_project_f32(x.data_ptr(), y.data_ptr(), theta.data_ptr(), K, B, L, D, proj[0].data_ptr(),
                                                     proj[1].data_ptr(), stream), 'ssn_ens_swd_project_f32')
        coef = torch.empty((K * B, L), **f32)
        loss_l = torch.empty((K, L), device='cuda', dtype=torch.float64)
        self._l0 = torch.empty((K,), device='cuda', dtype=torch.float64)
        clib.check(libssnode.ssn_ens_swd_match_f32(proj[0].data_ptr(), proj[1].data_ptr(), st['power'], K, B, L, self.match_form,
                                                   coef.data_ptr(), loss_l.data_ptr(), self._l0.data_ptr(), stream),
                   'ssn_ens_swd_match_f32')
        rec[:, self.R0:] = loss_l                              # (rides with the record: one read per step)
        self.last_gx = gx = torch.empty((K * B, D), **f32)
        clib.check(libssnode.ssn_ens_swd_backproject_f32(coef.data_ptr(), theta.data_ptr(), K, B, L, D, gx.data_ptr(), stream),
                   'ssn_ens_swd_backproject_f32')
        return gx

    def _assemble(self, a):
        clib.check(libssnode.ssn_ens_gen_grads_l0_f32(ctypes.byref(a), self._l0.data_ptr(), clib.stream_ptr()),
                   'ssn_ens_gen_grads_l0_f32')

    def _info_fields(self, row):
        return dict(swd=float(row[0]), swd_per_direction=row[self.R0:self.R0 + self.L].copy())


def refuse_truth_batch(config):
    """The ensemble's match kernels take as many truth rows as generated ones: `swd_truth_batch` (an option of the single run,
    in neither key set here) may only be absent or 0."""
    if config.get('swd_truth_batch', 0) != 0:
        raise ValueError('swd_truth_batch = {!r}: an ensemble matches batchsize truth rows per member (its kernels know equal '
                         'sizes only); use 0 here, or tc_gan.run.bptt_swd for one run'.format(config['swd_truth_batch']))


def ensemble_from_member_configs(configs, match_form=clib.SWD_FORM_AUTO):
    """The `EnsembleSlicedWasserstein` of fully resolved member configs (each what `make_sliced_wasserstein` takes, all naming
    the same explicit `gen_kernel`)."""
    for cfg in configs:
        refuse_truth_batch(cfg)
        if cfg.get('gen_kernel') == 'duo-fused':
            raise ValueError("gen_kernel 'duo-fused' is not available to ensembles; use 'duo'")
    members, rests, dcosts, rcosts, kernel = mme.members_from_configs(configs, make_sliced_wasserstein)
    return EnsembleSlicedWasserstein(members, kernel, dcosts, rcosts, rests=rests, match_form=match_form)


def make_sliced_wasserstein_ensemble(shared_config, member_overrides, match_form=clib.SWD_FORM_AUTO):
    """One `BPTTSlicedWasserstein` per member from the shared config (what `make_sliced_wasserstein` takes) with the member's
    options over it (`validate_member_overrides`), all on the kernel `resolve_gen_kernel` picks for the ensemble's K B draws.
    Returns the `EnsembleSlicedWasserstein`; its `rests` are the members' unconsumed configs (the data-set options)."""
    overrides = validate_member_overrides(member_overrides)
    kernel = resolve_gen_kernel(shared_config, len(overrides))
    configs = []
    for over in overrides:
        cfg = member_config(shared_config, over)
        cfg['gen_kernel'] = kernel
        configs.append(cfg)
    return ensemble_from_member_configs(configs, match_form)

"""
Run several BPTT sliced Wasserstein runs together in one GPU loop (an ensemble).

Takes the options of ``tc_gan.run.bptt_swd`` for what the members share, and ``--members FILE``: a JSON list with one dict of
options per member (networks/sliced_wasserstein_ensemble.py: MEMBER_KEYS may differ -- seed, start values, learning rate,
``swd_power``, ``swd_direction_seed``, ``truth_size``, ... -- SHARED_KEYS may not).  Member i writes DATASTORE/<i>/ with the files
of a single run -- info.json (its fully resolved config, the generator kernel that ran included), the learning / generator
tables, truth.npy, exit.json: a run directory ``tc_gan.analyzers.distdiff --wasserstein`` scores -- and DATASTORE/members.json
records the ensemble.  A member whose run ends by the single run's rules (quit_JDS_threshold, an error) writes its exit.json and
leaves; the others go on.
"""
import contextlib
import os
from logging import getLogger

import numpy as np

from .. import execution
from ..drivers import SlicedWassersteinDriver
from ..networks.sliced_wasserstein_ensemble import ensemble_from_member_configs, refuse_truth_batch, validate_member_overrides
from . import bptt_moments_ensemble as bme
from .bptt_wgan import generate_dataset_and_save

logger = getLogger(__name__)

DATASTORE_TEMPLATE = 'logfiles/BPTT_SWD_ensemble_{swd_directions}'


def make_parser():
    from . import options
    parser = options.build_parser('s', __doc__)
    parser.add_argument('--members', required=True,
                        help='JSON file: a list with one dict of per-member options (seed, J0, learning_rate, swd_power, '
                             'swd_direction_seed, ...) per member')
    parser.set_defaults(datastore_template=DATASTORE_TEMPLATE)
    return parser


def member_run_configs(run_config, member_overrides):
    """The run_config of every member as a single ``bptt_swd`` run with the same options would write it to info.json
    (`bptt_moments_ensemble.member_run_configs` with this ensemble's keys): gen_kernel resolved once, for K x batchsize draws.
    But for one key: a single run always records `swd_truth_batch` (0 unless given); a member records it only where the ensemble's
    command line gave it, and then it is 0.
    A `swd_truth_batch` other than 0 is refused here, before anything is written or built."""
    refuse_truth_batch(run_config)
    return bme.member_run_configs(run_config, member_overrides, validate=validate_member_overrides)


def prepare_datastores(run_config, member_overrides, script_file=__file__):
    """`bptt_moments_ensemble.prepare_datastores` for this script: DATASTORE/members.json and DATASTORE/<i>/info.json."""
    return bme.prepare_datastores(run_config, member_overrides, script_file=script_file, template=DATASTORE_TEMPLATE,
                                  module=__name__, configs_of=member_run_configs)


def learn(datastores, configs):
    """Data set of every member (as `bptt_swd.learn` makes it), then the ensemble's loop with one driver per member."""
    driver_kw, model_cfgs = [], []
    for cfg in configs:
        cfg = dict(cfg)
        driver_kw.append(dict(iterations=cfg.pop('iterations'), quiet=cfg.pop('quiet'),
                              quit_JDS_threshold=cfg.pop('quit_JDS_threshold', -1)))
        model_cfgs.append(cfg)
    ens = ensemble_from_member_configs(model_cfgs)
    drivers = []
    for i, (swd, rest, ds) in enumerate(zip(ens.members, ens.rests, datastores)):
        np.random.seed(0)
        swd.prepare()
        swd.set_dataset(generate_dataset_and_save(ds, swd, **rest))
        drv = SlicedWassersteinDriver(swd, ds, **driver_kw[i])
        drv.pre_loop()
        drivers.append(drv)
    bme.run_ensemble(ens, drivers, iterations=driver_kw[0]['iterations'])
    return ens


def main(args=None):
    ns = make_parser().parse_args(args)
    run_config = vars(ns)
    members = execution.load_any_file(run_config.pop('members'))
    logger.info('PID: %d', os.getpid())
    datastore, dirs, configs = prepare_datastores(run_config, members)
    logger.info('Output directory: %s', datastore)
    with contextlib.ExitStack() as stack:
        stores = [stack.enter_context(execution.DataStore(d)) for d in dirs]
        learn(stores, configs)


if __name__ == '__main__':
    main()

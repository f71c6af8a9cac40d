"""
Run several BPTT moment-matching runs together in one GPU loop (an ensemble).

Takes the options of ``tc_gan.run.bptt_moments`` for what the members share, and ``--members FILE``: a JSON list with one dict
of options per member (networks/moment_matching_ensemble.py: MEMBER_KEYS may differ, SHARED_KEYS may not).  Member i writes
DATASTORE/<i>/ with the files of a single run -- info.json (its fully resolved config, the generator kernel that ran included),
the learning / generator / gen_moments tables, truth.npy, exit.json -- and DATASTORE/members.json records the ensemble.
A member whose run ends by the single run's rules (quit_JDS_threshold, an error) writes its exit.json and leaves; the others go on.
"""
import contextlib
import copy
import json
import os
from logging import getLogger

import numpy as np

from .. import execution
from ..drivers import MomentMatchingDriver
from ..networks.moment_matching_ensemble import ensemble_from_member_configs, resolve_gen_kernel, validate_member_overrides
from .bptt_wgan import generate_dataset_and_save, preprocess

logger = getLogger(__name__)

#: keys of a member's run_config the driver takes (init_driver of run/bptt_moments.py)
_DRIVER_KEYS = ('iterations', 'quiet', 'gen_moments_record_interval', 'quit_JDS_threshold')


def make_parser():
    from . import options
    parser = options.build_parser('m', __doc__)
    parser.add_argument('--members', required=True,
                        help='JSON file: a list with one dict of per-member options (seed, J0, learning_rate, lam, ...) per member')
    parser.set_defaults(datastore_template='logfiles/BPTT_MM_ensemble_{lam}')
    return parser


def member_run_configs(run_config, member_overrides, validate=validate_member_overrides):
    """The run_config of every member as a single ``bptt_moments`` run with the same options would write it to info.json: the
    shared options with the member's over them, pre-processed (bptt_wgan.preprocess), and gen_kernel resolved for the ensemble.
    `validate`: the ensemble's check of the members' keys."""
    overrides = validate(member_overrides)
    configs = []
    for over in overrides:
        cfg = copy.deepcopy(run_config)
        cfg.update(copy.deepcopy(over))
        preprocess(cfg)
        configs.append(cfg)
    kernel = resolve_gen_kernel(configs[0], len(configs))
    for cfg in configs:
        cfg['gen_kernel'] = kernel
    return overrides, configs


def prepare_datastores(run_config, member_overrides, script_file=__file__, template='logfiles/BPTT_MM_ensemble_{lam}',
                       module=__name__, configs_of=None):
    """Merge --load-config, resolve the members and write DATASTORE/members.json and DATASTORE/<i>/info.json (no GPU needed).
    Returns (datastore directory, member directories, member configs).  Another ensemble script gives its own default
    `template`, its `module` name and `configs_of`, its `member_run_configs`."""
    run_config = dict(run_config)
    load_config = run_config.pop('load_config', None)
    if load_config:
        run_config.update(execution.load_any_file(load_config))
    datastore = run_config.pop('datastore', None)
    template = run_config.pop('datastore_template', template)
    extra_info = dict(n_bandwidths=run_config['n_bandwidths'], load_gen_param=run_config['load_gen_param'], data_version=1,
                      script_file=script_file, learn='{}.{}'.format(module, 'learn'), init_driver='{}.{}'.format(module, 'learn'))
    overrides, configs = (configs_of or member_run_configs)(run_config, member_overrides)
    if not datastore:
        datastore = execution.format_datastore(template, configs[0])
    execution.makedirs_exist_ok(datastore)
    dirs = [os.path.join(datastore, str(i)) for i in range(len(configs))]
    meta = execution.get_meta_info(packages=_packages())
    for d, cfg in zip(dirs, configs):
        execution.makedirs_exist_ok(d)
        with open(os.path.join(d, 'info.json'), 'w') as fp:
            json.dump(execution._jsonable(dict(run_config=cfg, extra_info=extra_info, meta_info=meta)), fp)
    with open(os.path.join(datastore, 'members.json'), 'w') as fp:
        json.dump(execution._jsonable(dict(num_members=len(configs), gen_kernel=configs[0]['gen_kernel'], members=overrides,
                                           directories=[str(i) for i in range(len(configs))])), fp)
    return datastore, dirs, configs


def _packages():
    import torch
    return [np, torch]


def learn(datastores, configs):
    """Data set of every member (as `bptt_moments.learn` makes it), then the ensemble's loop with one driver per member."""
    driver_kw, model_cfgs = [], []
    for cfg in configs:
        cfg = dict(cfg)
        driver_kw.append(dict(iterations=cfg.pop('iterations'), quiet=cfg.pop('quiet'),
                              gen_moments_record_interval=cfg.pop('gen_moments_record_interval'),
                              quit_JDS_threshold=cfg.pop('quit_JDS_threshold', -1)))
        model_cfgs.append(cfg)
    ens = ensemble_from_member_configs(model_cfgs)
    drivers = []
    for i, (mm, rest, ds) in enumerate(zip(ens.members, ens.rests, datastores)):
        np.random.seed(0)
        mm.prepare()
        mm.set_dataset(generate_dataset_and_save(ds, mm, **rest))
        drv = MomentMatchingDriver(mm, ds, **driver_kw[i])
        drv.pre_loop()
        drivers.append(drv)
    run_ensemble(ens, drivers, iterations=driver_kw[0]['iterations'])
    return ens


def run_ensemble(ens, drivers, iterations):
    """The loop: one ensemble step per generator step, then every active member's `post_update` (its rows, its guards).  A
    member whose guard ends its run (a KnownError: exit.json already written) or whose recording fails leaves the ensemble."""
    logger.info('ensemble of %d members (gen_kernel %s): start iterations', len(drivers), ens.gen_kernel)
    try:
        for step in range(iterations):
            if not ens.active:
                break
            for info in ens.train_step(step):
                i = info.member
                try:
                    drivers[i].post_update(step, info)
                except execution.KnownError as err:
                    logger.info('member %d: %s', i, err)
                    ens.remove(i)
                except Exception as err:
                    drivers[i].datastore.save_exit_reason(reason='uncaught_exception', good=False, exception=str(err))
                    ens.remove(i)
    except KeyboardInterrupt:
        for i in ens.active:
            drivers[i].datastore.save_exit_reason(reason='keyboard_interrupt', good=False)
        raise
    except Exception as err:
        for i in ens.active:
            drivers[i].datastore.save_exit_reason(reason='uncaught_exception', good=False, exception=str(err))
        raise
    for i in ens.active:
        drivers[i].datastore.save_exit_reason(reason='end_of_iteration', good=True)
    logger.info('ensemble: maximum iterations reached')


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

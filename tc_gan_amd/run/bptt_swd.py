"""
Run BPTT training by the sliced Wasserstein distance on MI355X: no critic.

The generator options of ``tc_gan.run.bptt_moments`` (generator, dynamics, bounds, updater, data set) and the loss's own:
``--swd-directions``, ``--swd-power``, ``--swd-direction-seed``, ``--swd-truth-batch`` (truth rows per step: 0 = the batch size,
-1 = the whole truth, M = minibatches of M rows).  Outputs: the ``learning`` table (step, loss, swd,
dynamics_penalty, rate_penalty, train_time) and the ``generator`` table in the store, truth.npy -- a run directory that
``tc_gan.analyzers.distdiff --wasserstein`` scores; with ``--swd-power 1`` the ``swd`` column is in the unit of its sliced_w1.
"""
from logging import getLogger

import numpy as np

from ..drivers import SlicedWassersteinDriver
from ..networks.sliced_wasserstein import DEFAULT_PARAMS, make_sliced_wasserstein
from .bptt_wgan import do_learning, generate_dataset_and_save

logger = getLogger(__name__)


def learn(driver, **generate_dataset_kwargs):
    np.random.seed(0)
    learner = driver.mmatcher
    learner.prepare()
    data = generate_dataset_and_save(driver.datastore, learner, **generate_dataset_kwargs)
    learner.set_dataset(data)
    driver.run(learner)


def make_parser():
    """The option table lives in `run/options.py` (script 's')."""
    from . import options
    return options.build_parser('s', __doc__)


def init_driver(datastore, iterations, quiet, quit_JDS_threshold=-1, **run_config):
    learner, rest = make_sliced_wasserstein(run_config)
    driver = SlicedWassersteinDriver(learner, datastore, iterations=iterations, quiet=quiet, quit_JDS_threshold=quit_JDS_threshold)
    return dict(driver=driver, **rest)


def main(args=None):
    parser = make_parser()
    ns = parser.parse_args(args)
    run_config = vars(ns)
    run_config.setdefault('swd_truth_batch', DEFAULT_PARAMS['swd_truth_batch'])      # (recorded in info.json like the others)
    do_learning(learn, run_config, init_driver=init_driver, script_file=__file__)


if __name__ == '__main__':
    main()

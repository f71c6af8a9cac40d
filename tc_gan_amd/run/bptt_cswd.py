"""
Run BPTT training of the conditional SSN by the sliced Wasserstein distance on MI355X: no critic.

What a step samples is the conditional GAN's (``--num-models``, ``--probes-per-model``, ``--norm-probes``: one contrast per model,
a few (cell type, probe) pairs per model); the loss is ``tc_gan.run.bptt_swd``'s (``--swd-directions``, ``--swd-power``,
``--swd-direction-seed``) taken per condition: every generated tuning curve is compared with the WHOLE truth under its own
(cell type, probe, contrast).  Outputs: the ``learning`` table (step, loss, swd, dynamics_penalty, rate_penalty, train_time) and
the ``generator`` table in the store, truth.npy -- a run directory that ``tc_gan.analyzers.distdiff --wasserstein`` scores.
"""
from logging import getLogger

import numpy as np

from ..drivers import SlicedWassersteinDriver
from ..networks.conditional_sliced_wasserstein import make_conditional_sliced_wasserstein
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
    """The option table lives in `run/options.py` (script 'k')."""
    from . import options
    return options.build_parser('k', __doc__)


def init_driver(datastore, iterations, quiet, quit_JDS_threshold=-1, **run_config):
    learner, rest = make_conditional_sliced_wasserstein(run_config)
    driver = SlicedWassersteinDriver(learner, datastore, iterations=iterations, quiet=quiet, quit_JDS_threshold=quit_JDS_threshold)
    return dict(driver=driver, **rest)


def main(args=None):
    parser = make_parser()
    ns = parser.parse_args(args)
    do_learning(learn, vars(ns), init_driver=init_driver, script_file=__file__)


if __name__ == '__main__':
    main()

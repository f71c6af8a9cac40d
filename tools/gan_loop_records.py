#!/usr/bin/env python3
"""Frozen records of the GAN loop's host code: small runs of every path `networks/cwgan.py`, `networks/wgan.py` and the
critic-free trainers take, written as raw float64 / integer arrays into one .npz.  tests/test_gan_loop_frozen_gpu.py runs the
same cases through the same functions and compares bit for bit with tests/golden/gan_loop_records.npz.

usage: tools/gan_loop_records.py OUT.npz [case ...]

A change that alters arithmetic on purpose regenerates the golden file with this tool and says so."""
import os
import sys
import tempfile
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

FIELDS = ('disc_loss', 'accuracy', 'dynamics_penalty', 'rate_penalty', 'gen_loss', 'loss', 'gen_step', 'disc_step', 'step', 'swd')
RECORDS = 20


def _jds():
    from oracle import ssn_numpy as on          # parameters only
    return on.new_JDS()


def small_config(**over):
    """The shapes of `_small_run` in tests/test_cwgan_gpu.py: N = 10, 6 models x 2 probes, critic [16, 16]."""
    jds = _jds()
    cfg = dict(num_sites=10, seqlen=40, skip_steps=30, num_models=6, probes_per_model=2, norm_probes=[0, 0.5],
               include_inhibitory_neurons=True, bandwidths=[0.0625, 0.125, 0.25, 0.75], contrasts=[5., 20.],
               J0=jds['J'], D0=jds['D'], S0=jds['S'], critic_iters_init=3, critic_iters=2, lipschitz_cost=10.0,
               gen=dict(learning_rate=0.01, update_name='adam-wgan', dynamics_cost=1.0, rate_cost=0.01, rate_penalty_threshold=5.0),
               disc=dict(learning_rate=0.01, update_name='adam-wgan', layers=[16, 16], normalization='none',
                         nonlinearity='rectify', precision='fp32'))
    for key in ('gen', 'disc'):
        cfg[key] = dict(cfg[key], **over.pop(key, {}))
    cfg.update(over)
    return cfg


def cwgan_test_params(**over):
    """`TEST_PARAMS` of tests/test_cwgan_gpu.py: 4 models, both players on sgd, explicit bounds."""
    cfg = small_config(num_models=4)
    cfg['gen'] = dict(cfg['gen'], update_name='sgd', J_min=1e-3, J_max=10, D_min=1e-3, D_max=10, S_min=1e-3, S_max=10)
    cfg['disc'] = dict(cfg['disc'], update_name='sgd')
    for key in ('gen', 'disc'):
        cfg[key] = dict(cfg[key], **over.pop(key, {}))
    cfg.update(over)
    return cfg


DEG_HETEROIN = dict(ssn_type='deg-heteroin', V=0.4,
                    disc=dict(update_name='rmsprop', normalization=['none', 'layer'], reg_l2_decay=0.001))


def _f64(x):
    return np.ascontiguousarray(np.asarray(x, dtype='float64'))


def record_rows(infos):
    """(records, len(FIELDS)) float64, NaN where a record has no such field, and the critic norms of the records that have them."""
    def scalar(info, f):
        value = getattr(info, f, None)
        return np.nan if value is None else float(value)
    rows = np.array([[scalar(info, f) for f in FIELDS] for info in infos], dtype='float64').reshape(-1, len(FIELDS))
    with_norms = [i for i, info in enumerate(infos) if getattr(info, 'param_sqnorms', None) is not None]
    out = dict(records=rows, sqnorm_records=np.array(with_norms, dtype='int64'))
    if with_norms:
        out['param_sqnorms'] = np.stack([_f64(infos[i].param_sqnorms) for i in with_norms])
    if infos and hasattr(infos[0], 'gen_moments'):
        out['gen_moments'] = np.stack([_f64(info.gen_moments) for info in infos])
    return out


def final_state(trainer, rest):
    """Parameters, optimizer states, RandomState, collectives issued and what the builder left unconsumed."""
    out = dict(gen_param=np.concatenate([_f64(p).ravel() for p in trainer.get_gen_param()]),
               gen_all_params=np.concatenate([_f64(v).ravel() for _, v in trainer.gen.get_all_params()]),
               reducer_calls=np.array([trainer.reducer.calls], dtype='int64'),
               rest_keys=np.array(sorted(rest), dtype='U'))
    updaters = {'gen_' + name: u for name, u in trainer.gen_updaters.items()}
    if hasattr(trainer, 'disc'):
        out['disc_flat'] = _f64(trainer.disc.get_flat())
        updaters['disc'] = trainer.disc_updater
    for name, u in sorted(updaters.items()):
        sd = u.state_dict()
        out['updater_%s_step' % name] = np.array([sd['step']], dtype='int64')
        for k in ('m', 'v'):
            out['updater_%s_%s' % (name, k)] = _f64([] if sd[k] is None else sd[k]).ravel()
    st = trainer.rng.get_state()
    out['rng_keys'] = np.asarray(st[1], dtype='uint32').copy()
    out['rng_pos'] = np.array([st[2]], dtype='int64')
    return out


def _make_cgan(cfg):
    from tc_gan_amd.networks.cwgan import make_gan
    gan, rest = make_gan(cfg)
    ncols = len(gan.bandwidths) * len(gan.contrasts) * len(gan.norm_probes) * 2
    gan.set_dataset(np.random.RandomState(3).rand(9, ncols) * 10)
    return gan, rest


def run_cgan(cfg, records=RECORDS, tweak=None, poke=None):
    gan, rest = _make_cgan(cfg)
    if tweak is not None:
        tweak(gan)
    it = gan.learning()
    infos = []
    for _ in range(records):
        info = next(it)
        infos.append(info)
        if poke is not None and not info.is_discriminator and info.gen_step == poke:
            gan.gen.J = np.asarray(gan.gen.J) * 1.01          # (somebody changes the generator between two iterations)
    return dict(record_rows(infos), **final_state(gan, rest))


def _rate_bound_config(bound, **over):
    """The configuration of test_rate_bound_skips_exactly_the_steps_over_the_bound."""
    return cwgan_test_params(critic_iters_init=8, z_device_seed=5, gen=dict(rate_penalty_threshold=0.5),
                       disc=dict(update_name='adam-wgan', rate_penalty_bound=bound), **over)


def run_rate_bound(**over):
    """The bound lies between the two middle rate penalties of a free run's first eight critic steps, as in that test."""
    free = run_cgan(_rate_bound_config(-1.0, **over), records=8)
    pens = np.sort(free['records'][:, FIELDS.index('rate_penalty')])
    assert pens.min() < pens.max()
    bound = float(pens[len(pens) // 2 - 1] + pens[len(pens) // 2]) / 2
    out = run_cgan(_rate_bound_config(bound, **over))
    critic = ~np.isnan(out['records'][:, FIELDS.index('disc_step')])
    skipped = np.isnan(out['records'][critic, FIELDS.index('disc_loss')])
    assert skipped.any() and not skipped.all(), 'the bound must skip some critic steps and not others'
    return dict(out, bound=np.array([bound], dtype='float64'))


def run_resume():
    """deg-heteroin: checkpoint after generator step 1, a NEW GAN continues from it for two more steps; the continuation."""
    def until(it, n_gen_steps, infos):
        done = 0
        while done < n_gen_steps:
            infos.append(next(it))
            done += not infos[-1].is_discriminator
    first, _ = _make_cgan(small_config(**DEG_HETEROIN))
    until(first.learning(), 2, [])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'checkpoint.pkl')
        first.save_checkpoint(path, gen_step=1)
        second, rest = _make_cgan(small_config(**DEG_HETEROIN))
        start = second.load_checkpoint(path)
    infos = []
    until(second.learning(start), 2, infos)
    return dict(record_rows(infos), start=np.array([start], dtype='int64'), **final_state(second, rest))


def run_poisoned(subset):
    """One generator step with one draw's f' scaled by 1e5 (test_poisoned_generator_gradient_is_not_hidden_by_the_parameter_
    bounds, fused tail): the update is withheld and made again on the fp32 kernels, for the refused draws or for all."""
    from tc_gan_amd.networks import cwgan
    from tc_gan_amd.utils import Namespace
    cfg = cwgan_test_params(num_sites=60, num_models=4, probes_per_model=1, seqlen=60, skip_steps=40,
                      bandwidths=[0.0625, 0.125, 0.25, 0.5, 0.75, 1.0, 0.3, 0.4], contrasts=[20.], gen_kernel='duo',
                      critic_iters=0, gen=dict(update_name='adam-wgan'))
    before, cwgan._SUBSET_RETRY = cwgan._SUBSET_RETRY, subset
    try:
        gan, rest = cwgan.make_gan(cfg)
        ncols = len(gan.bandwidths) * len(gan.contrasts) * len(gan.norm_probes) * 2
        gan.set_dataset(np.random.RandomState(4).rand(9, ncols) * 10)
        batch = gan.next_minibatch()
        prepared = gan._prepare_gen(batch)
        assert gan._gen_tail_fused() is not None
        gan.gen._saved['fwd']['df'][1, :, 50, :] *= 1e5
        info = gan.train_generator(Namespace(is_discriminator=False, gen_step=0), batch, prepared)
        assert gan.gen.poisoned_draws() == 1
    finally:
        cwgan._SUBSET_RETRY = before
    return dict(record_rows([info]), **final_state(gan, rest))


def run_unconditional():
    """`_train_unconditional` of tests/test_dp_equivalence_gpu.py."""
    from tc_gan_amd.networks.wgan import make_gan
    cfg = cwgan_test_params()
    gen = dict(cfg['gen'], update_name='adam-wgan')
    disc = dict(cfg['disc'], update_name='adam-wgan')
    gan, rest = make_gan(dict(
        J0=cfg['J0'], D0=cfg['D0'], S0=cfg['S0'], gen=gen, disc=disc, critic_iters_init=2, critic_iters=2,
        include_inhibitory_neurons=True, lipschitz_cost=10.0, num_sites=10, seqlen=40, skip_steps=30, batchsize=4,
        bandwidths=[0.0625, 0.125, 0.25, 0.75], contrasts=[20.], z_device_seed=7, gen_kernel='auto'))
    ncols = len(gan.bandwidths) * len(gan.contrasts) * len(gan.sample_sites) * 2
    gan.set_dataset(np.random.RandomState(6).rand(9, ncols) * 10)
    it = gan.learning()
    return dict(record_rows([next(it) for _ in range(RECORDS)]), **final_state(gan, rest))


def _mm_params(**over):
    """`MM_PARAMS` of tests/test_moments.py."""
    jds = _jds()
    return dict(dict(num_sites=10, seqlen=40, skip_steps=30, batchsize=6, sample_sites=[0, 0.5],
                     include_inhibitory_neurons=True, bandwidths=[0.0625, 0.25, 0.75], contrasts=[5., 20.],
                     J0=jds['J'], D0=jds['D'], S0=jds['S'], learning_rate=0.01, update_name='sgd', dynamics_cost=1.0,
                     rate_cost=0.01, rate_penalty_threshold=5.0, J_min=1e-3, J_max=10, D_min=1e-3, D_max=10, S_min=1e-3,
                     S_max=10), **over)


def run_critic_free(kind):
    if kind == 'moments':
        from tc_gan_amd.networks.moment_matching import make_moment_matcher
        trainer, rest = make_moment_matcher(_mm_params(lam=0.1, moment_weights_regularization=1e-3, moment_weight_type='mean',
                                                       truth_size=3))
        trainer.set_dataset(np.random.RandomState(5).rand(3, trainer.num_mom_conds) * 8)
    else:
        from tc_gan_amd.networks.sliced_wasserstein import make_sliced_wasserstein
        trainer, rest = make_sliced_wasserstein(_mm_params(swd_directions=16, swd_power=2))
        trainer.set_dataset(np.random.RandomState(5).rand(12, trainer.num_mom_conds) * 8)
    it = trainer.learning()
    return dict(record_rows([next(it) for _ in range(3)]), **final_state(trainer, rest))


def _one_rank_child(port, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ['TCGAN_DIST_SINGLE_RANK'] = '1'
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=0, world_size=1)
    res = run_cgan(small_config())
    out.put(res)
    dist.barrier()
    dist.destroy_process_group()


def run_one_rank_group(timeout=240):
    """The default case in a fresh child with a one-rank gloo group: the collectives run, the accuracy is deferred."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    out = ctx.Queue()
    proc = ctx.Process(target=_one_rank_child, args=(24700 + (os.getpid() % 1000), out))
    proc.start()
    try:
        res = out.get(timeout=timeout)
        proc.join(timeout=60)
    finally:
        if proc.is_alive():
            proc.kill()
            proc.join()
    assert proc.exitcode == 0, proc.exitcode
    assert res['reducer_calls'][0] > 0
    return res


def _updaters_out_of_step(gan):
    gan.gen_updaters['J'].learning_rate *= 2


CASES = dict(
    default=lambda: run_cgan(small_config()),
    deg_heteroin=lambda: run_cgan(small_config(**DEG_HETEROIN)),
    heteroin=lambda: run_cgan(small_config(ssn_type='heteroin', V=[0.3, 0.1], gen=dict(V_min=[0, 0], V_max=[1, 0]))),
    rate_bound_fused=run_rate_bound,
    rate_bound_fp64=lambda: run_rate_bound(gen_dtype='float64'),
    updaters_out_of_step=lambda: run_cgan(small_config(), tweak=_updaters_out_of_step),
    host_noise=lambda: run_cgan(small_config(z_host_draw=True)),
    device_noise=lambda: run_cgan(small_config(z_device_seed=123)),
    poked=lambda: run_cgan(small_config(), poke=2),
    resume=run_resume,
    poisoned_subset=lambda: run_poisoned(True),
    poisoned_all=lambda: run_poisoned(False),
    unconditional=run_unconditional,
    moment_matcher=lambda: run_critic_free('moments'),
    sliced_wasserstein=lambda: run_critic_free('swd'),
    one_rank_group=run_one_rank_group,
)


def load(path):
    """{case: {field: array}} of a file this tool wrote."""
    out = {}
    with np.load(path) as z:
        for key in z.files:
            case, field = key.split('/', 1)
            out.setdefault(case, {})[field] = z[key]
    return out


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def main(argv):
    path, names = argv[0], argv[1:] or list(CASES)
    flat, failed = {}, []
    for name in names:
        try:
            res = CASES[name]()
        except Exception:
            traceback.print_exc()
            failed.append(name)
            continue
        print('%-22s %3d records, %d fields' % (name, len(res['records']), len(res)), flush=True)
        flat.update({'%s/%s' % (name, k): v for k, v in res.items()})
    np.savez_compressed(path, **flat)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))
    if failed:
        sys.exit('failed: ' + ' '.join(failed))


if __name__ == '__main__':
    main(sys.argv[1:])

"""
Score the checkpoints of a run: KS distances between the truth's tuning curves and generated ones.

Counterpart of ``tc_gan/analyzers/distdiff.py`` (KS per tuning-curve column), ``csv_tuning_curves.py`` (the sampled curves
per checkpoint as CSV) and the per-curve features of ``Fig4analysis.py``, for the fixed-time generator.  For every selected
row of the run's ``generator`` table, `draws` tuning curves are generated at that row's parameters and compared with
``truth.npy``: the two-sample Kolmogorov-Smirnov statistic of every tuning-curve column and of four features of every curve
over its bandwidths (``maxrate``, suppression index ``si``, preferred bandwidth ``prefbw``, inverse participation ratio
``ipr``).

All checkpoints see the SAME noise, drawn once from ``numpy.random.RandomState(seed)`` in the reference's order
(``rand(draws, 2N, 2N)``, then the input signs of the heterogeneous-input models), as the reference's
``sample_tuning_curves(seed=0)`` per checkpoint does: the KS curve is smooth in the step.  That also makes the checkpoints one
batch: a chunk of them is ONE launch that forms W for a table of parameter sets from the shared z (``ssn_build_w_table_f32``),
one stimulus launch, ONE generator forward over chunk x draws draws, the probe gather, one feature launch
(``ssn_tc_features_f32``) and one KS launch (``ssn_ks_columns_f32``: a workgroup per (checkpoint, column) sorts its values in
LDS and walks the pooled points), then one small copy of the integer results to the host.

The statistic is kept as integers: ``num = max_v |#{x <= v} m - #{t <= v} n|`` with ``n``, ``m`` the finite counts of the
generated and the truth column, ``KSD = num / (n m)`` -- exactly ``scipy.stats.ks_2samp(...).statistic``, ties included.
There is no p-value here: scipy's default for these sample sizes is its exact method, host arithmetic on (KSD, n, m), and the
table carries all three for whoever wants it.  (Nothing here imports scipy.)

``dynamics='fixed-point'`` (``--dynamics fixed-point``) scores with the reference's own definition instead, for runs whose truth
is a sample of fixed points (``--dataset-provider ssnode``, the default): the curves of a checkpoint are those of the first
`draws` candidate draws, in stream order, whose fixed points converge for every stimulus
(`ssnode.sample_tuning_curves_table`: the draws, W, the solves, the rejection step and the gather of the probed rates all stay
on the device), with the truth's solver options.  A checkpoint that rejects draws is short of rows -- its ``n`` is the accepted
count -- and the counts of rejected draws per error code are part of the result (``rejections.csv``): the rejection rate is
the diagnostic for a generator that has left the stable regime.

``wasserstein=True`` (``--wasserstein``) adds the distance the training loop minimises, in the unit of the column (Hz for a raw
column), where KS saturates at 1 for every sample that lies on one side of the truth's.  The KS launch is replaced by one
``ssn_ks_w1_columns_f32`` launch over the same columns: the same integers ``num`` and ``n``, and beside them
``wnum = sum_k (p_{k+1} - p_k) |#{x <= p_k} m - #{t <= p_k} n|`` over the distinct pooled values ``p_0 < ... < p_K`` in fp64, so
that ``W1 = wnum / (n m)`` -- ``scipy.stats.wasserstein_distance``.  The sliced distance ``SW1`` of a checkpoint is the mean over
`directions` unit vectors (`slice_directions`: seeded, shared by all checkpoints and by the truth) of the W1 between the
projections of the generated rows and of the truth's rows onto the vector: the raw columns of a chunk are projected by
``ssn_project_rows_f32`` (a sequential fp64 sum per (row, direction), rounded to float32) and a second
``ssn_ks_w1_columns_f32`` launch treats the directions as columns.  A row that is not finite drops out of every direction.
The command line then writes ``wdist.csv`` (gen_step, stat, W1, n, m; one ``sliced_w1`` row per checkpoint) and ``wdist.json``;
``distdiff.csv`` and ``distdiff.json`` are what they are without the option.

    ./run tc_gan.analyzers.distdiff -- RUNDIR [--steps ::10] [--draws 30] [--seed 0] [--gen-kernel K]
                                       [--max-draws-per-launch D] [--output DIR] [--save-tuning-curves]
                                       [--dynamics {fixed-time,fixed-point}] [--max-candidates N]
                                       [--solver-dtype {float64,float32}]
                                       [--wasserstein] [--directions 128] [--direction-seed 0]
"""
import ctypes
import json
import os

import numpy as np

from .. import clib
from ..clib import libssnode
from ..networks.dataset import SSNODE_TRUTH_OPTIONS

FEATURES = ('maxrate', 'si', 'prefbw', 'ipr')
DEFAULT_DRAWS = 30                      # the reference's NZ per checkpoint
DEFAULT_MAX_DRAWS_PER_LAUNCH = 4096
DYNAMICS = ('fixed-time', 'fixed-point')
#: solver options of a fixed-point score: the very ones `networks.dataset.dataset_by_ssnode` makes the truth with
FIXED_POINT_SOLVER_OPTIONS = SSNODE_TRUTH_OPTIONS
#: what `fixed_point_options` hands to `ssnode.sample_tuning_curves_table` besides the stimuli and the probes
FIXED_POINT_OPTION_KEYS = ('io_type', 'k', 'n', 'smoothness', 'dt', 'max_iter', 'atol', 'tau', 'rate_stop_at', 'rate_soft_bound',
                           'rate_hard_bound', 'solver')
#: the command-line arguments distdiff.json records in the fixed-time mode: the file keeps the keys it always had
#: the command-line arguments of the Wasserstein distances: wdist.json records them, distdiff.json never does
_WASSERSTEIN_ARGUMENTS = ('wasserstein', 'directions', 'direction_seed')
DEFAULT_DIRECTIONS = 128
SLICED_STAT = 'sliced_w1'
_FIXED_TIME_ARGUMENTS = ('rundir', 'steps', 'draws', 'seed', 'gen_kernel', 'max_draws_per_launch', 'output', 'save_tuning_curves')
_SAMPLER_KEYS = ('num_sites', 'bandwidths', 'contrasts', 'smoothness', 'k', 'n', 'tau_E', 'tau_I', 'dt', 'io_type', 'seqlen',
                 'skip_steps')


# ---- host logic (no device) ---------------------------------------------------------------------------------------------

def plan_chunks(num_sets, draws, max_draws_per_launch):
    """(chunk, sizes): checkpoints per launch = max(1, max_draws_per_launch // draws), and the sizes of the chunks that cover
    `num_sets` (all `chunk` but possibly the last).

    >>> plan_chunks(6, 7, 30)
    (4, [4, 2])
    """
    num_sets, draws, budget = int(num_sets), int(draws), int(max_draws_per_launch)
    if draws < 1:
        raise ValueError('draws must be at least 1, got {}'.format(draws))
    if draws > clib.KS_MAX_DRAWS:
        raise ValueError('draws = {} is more than the {} values per column the KS kernel sorts in LDS'
                         .format(draws, clib.KS_MAX_DRAWS))
    if num_sets < 0 or budget < 1:
        raise ValueError('need num_sets >= 0 and max_draws_per_launch >= 1')
    chunk = max(1, budget // draws)
    sizes = [chunk] * (num_sets // chunk) + ([num_sets % chunk] if num_sets % chunk else [])
    return chunk, sizes


def parse_steps(text):
    """``--steps``: 'START:STOP:STEP' (any part may be empty) -> slice, '3' or '0,5,9' -> list of row positions; rows of the
    ``generator`` table, negative positions from the end.

    >>> parse_steps('::10'), parse_steps('0,5,-1'), parse_steps('7')
    (slice(None, None, 10), [0, 5, -1], [7])
    """
    if isinstance(text, (slice, list, tuple)):
        return text
    text = str(text).strip()
    try:
        if ':' in text:
            parts = text.split(':')
            if len(parts) > 3:
                raise ValueError
            parts += [''] * (3 - len(parts))
            return slice(*[int(p) if p.strip() else None for p in parts])
        return [int(p) for p in text.split(',') if p.strip()]
    except ValueError:
        raise ValueError('--steps: expected START:STOP:STEP or a comma separated list of row positions, got {!r}'.format(text))


def stat_names(num_contrasts, num_bandwidths, num_cell_types, num_probes):
    """Names of the statistics in column order: the raw columns ``tc_c{c}_b{b}_t{t}_p{p}`` in the order of a sampled tuning-curve
    row (contrast, bandwidth, cell type, probe: what `networks.utils.gridify_tc_samples` reshapes), then for each feature the
    curves ``{feature}_c{c}_t{t}_p{p}``."""
    raw = ['tc_c{}_b{}_t{}_p{}'.format(c, b, t, p) for c in range(num_contrasts) for b in range(num_bandwidths)
           for t in range(num_cell_types) for p in range(num_probes)]
    feats = ['{}_c{}_t{}_p{}'.format(f, c, t, p) for f in FEATURES for c in range(num_contrasts)
             for t in range(num_cell_types) for p in range(num_probes)]
    return raw + feats


def ksd_from_counts(num, n, m):
    """KSD = num / (n m); NaN where a side has no finite value."""
    num, n, m = np.asarray(num, dtype='float64'), np.asarray(n, dtype='float64'), np.asarray(m, dtype='float64')
    den = n * m
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.nan)


def long_table(result):
    """The long-format table of a result: one row per (checkpoint, statistic) -- gen_step, stat, KSD, n, m."""
    import pandas
    S, C = result['num'].shape
    return pandas.DataFrame(dict(
        gen_step=np.repeat(np.asarray(result['gen_step']), C), stat=np.tile(np.asarray(result['stat'], dtype=object), S),
        KSD=result['KSD'].reshape(-1), n=result['n'].reshape(-1), m=np.tile(result['m'], S)),
        columns=['gen_step', 'stat', 'KSD', 'n', 'm'])


def write_long_table(path, result):
    """`long_table` as CSV.  KSD is written with the digits that give the double back (``pandas.read_csv(path,
    float_precision='round_trip')``; pandas' default parser may be one ulp off -- n and m are exact either way)."""
    long_table(result).to_csv(path, index=False)


def slice_directions(directions, columns, seed=0):
    """The directions of the sliced distance, float32 (directions, columns): the rows of
    ``numpy.random.RandomState(seed).randn(directions, columns)``, each divided by its float64 norm, then rounded to float32."""
    return draw_slice_directions(np.random.RandomState(seed), directions, columns)


def draw_slice_directions(rng, directions, columns):
    """`slice_directions` from the next ``rng.randn(directions, columns)`` of a RandomState that is continued: a trainer that
    draws fresh directions every step calls this on one stream (the first call gives ``slice_directions(..., seed)``)."""
    directions, columns = int(directions), int(columns)
    if directions < 1:
        raise ValueError('directions must be at least 1, got {}'.format(directions))
    if directions > clib.W1_MAX_DIRECTIONS:
        raise ValueError('directions = {} is more than the {} the projection kernel takes'.format(directions, clib.W1_MAX_DIRECTIONS))
    if columns < 1:
        raise ValueError('directions need at least one column, got {}'.format(columns))
    g = rng.randn(directions, columns)
    return np.ascontiguousarray(g / np.sqrt((g * g).sum(axis=1, keepdims=True)), dtype='float32')


def w1_from_sums(wnum, n, m):
    """W1 = wnum / (n m); NaN where a side has no finite value."""
    wnum, n, m = np.asarray(wnum, dtype='float64'), np.asarray(n, dtype='float64'), np.asarray(m, dtype='float64')
    den = n * m
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(den > 0, wnum / np.where(den > 0, den, 1.0), np.nan)


def wdist_table(result):
    """The long-format table of the Wasserstein distances of a result: per checkpoint one row per statistic of ``stat`` and one
    `SLICED_STAT` row -- gen_step, stat, W1, n, m."""
    import pandas
    S, C = result['wnum'].shape
    sl = result['sliced']
    stat = np.asarray(list(result['stat']) + [SLICED_STAT], dtype=object)
    return pandas.DataFrame(dict(
        gen_step=np.repeat(np.asarray(result['gen_step']), C + 1), stat=np.tile(stat, S),
        W1=np.concatenate([result['W1'], np.asarray(result['SW1'])[:, None]], axis=1).reshape(-1),
        n=np.concatenate([result['n'], np.asarray(sl['n'])[:, None]], axis=1).reshape(-1),
        m=np.tile(np.concatenate([result['m'], [sl['m']]]), S)), columns=['gen_step', 'stat', 'W1', 'n', 'm'])


def write_wdist_table(path, result):
    """`wdist_table` as CSV, W1 with the digits that give the double back (see `write_long_table`)."""
    wdist_table(result).to_csv(path, index=False)


def _shape_of(cfg):
    """(num_contrasts, num_bandwidths, num_cell_types, num_probes, probes) of a sampler config."""
    from ..networks._common import probes_from_stim_space
    num_sites = int(cfg['num_sites'])
    if cfg.get('probes') is not None:
        probes = [int(p) for p in cfg['probes']]
        inhibitory = any(p >= num_sites for p in probes)
        if inhibitory and (len(probes) % 2 or [p + num_sites for p in probes[:len(probes) // 2]] != probes[len(probes) // 2:]):
            raise ValueError('probes: the inhibitory half must repeat the excitatory sites')
    else:
        inhibitory = bool(cfg.get('include_inhibitory_neurons', False))
        probes = [int(p) for p in probes_from_stim_space(list(cfg.get('norm_probes', [0])), num_sites, inhibitory)]
    ct = 2 if inhibitory else 1
    return len(cfg['contrasts']), len(cfg['bandwidths']), ct, len(probes) // ct, probes


def _check_config(cfg, draws, truth):
    """Everything that can be refused without a device; returns (config with defaults, shape, truth as float32)."""
    from ..networks._common import DEFAULT_PARAMS
    cfg = dict({k: DEFAULT_PARAMS[k] for k in _SAMPLER_KEYS}, **cfg)
    dtype = str(cfg.get('dtype', cfg.get('gen_dtype', 'float32')))
    if dtype != 'float32':
        raise ValueError('the scorer runs the float32 generator only, got dtype {!r} (float64 is not supported)'.format(dtype))
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise ValueError('the scorer runs on one GPU: data-parallel ranks (WORLD_SIZE = {}) are not supported'
                         .format(os.environ['WORLD_SIZE']))
    ssn_type = cfg.get('ssn_type', 'default')
    if ssn_type not in ('default', 'heteroin', 'deg-heteroin'):
        raise ValueError('Unknown ssn_type: {}'.format(ssn_type))
    if int(draws) > clib.KS_MAX_DRAWS:
        raise ValueError('draws = {} is more than the {} values per column the KS kernel sorts in LDS'
                         .format(draws, clib.KS_MAX_DRAWS))
    shape = _shape_of(cfg)
    columns = shape[0] * shape[1] * shape[2] * shape[3]
    truth = np.asarray(truth)
    if truth.ndim != 2 or truth.shape[1] != columns:
        raise ValueError('truth has shape {}: the sampler gives {} columns ({} contrasts x {} bandwidths x {} cell types x {} '
                         'probes)'.format(truth.shape, columns, *shape[:4]))
    if not np.isfinite(truth).all():
        raise ValueError('truth holds {} non-finite values'.format(int((~np.isfinite(truth)).sum())))
    return cfg, shape, np.ascontiguousarray(truth, dtype='float32')


def sampler_config_of_run(run_config):
    """The fixed-prober sampler of a run of bptt_wgan, bptt_cwgan or bptt_moments from the ``run_config`` of its info.json:
    same probes, cell types, contrasts, bandwidths, ssn_type, dist_in, I/O function, seqlen / skip_steps and gen_kernel."""
    from ..networks._common import DEFAULT_PARAMS
    rc = dict(run_config)
    cfg = {k: rc.get(k, DEFAULT_PARAMS[k]) for k in _SAMPLER_KEYS}
    cfg['norm_probes'] = list(rc['norm_probes'] if 'norm_probes' in rc else rc.get('sample_sites', [0]))
    cfg['include_inhibitory_neurons'] = bool(rc.get('include_inhibitory_neurons', False))
    cfg['ssn_type'] = rc.get('ssn_type', 'default')
    cfg['dist_in'] = rc.get('dist_in', 'bernoulli')
    cfg['gen_kernel'] = rc.get('gen_kernel', 'auto')
    cfg['dtype'] = rc.get('gen_dtype', 'float32')
    cfg['true_ssn_options'] = dict(rc.get('true_ssn_options') or {})
    return cfg


def fixed_point_options(cfg, solver_options=None):
    """Keyword arguments of `ssnode.sample_tuning_curves_table` for a sampler config, as the truth of `dataset_by_ssnode` gets
    them: `FIXED_POINT_SOLVER_OPTIONS`, overridden by the config's ``true_ssn_options`` and then by `solver_options`; what
    neither names (k, n, smoothness among them) is ssnode's default, not the generator's.  Of the recorded options only the
    `FIXED_POINT_OPTION_KEYS` are taken -- the truth's own J, D, S, V and whatever a fixed-time truth recorded (seqlen, ...)
    are not the solver's; a key of `solver_options` outside them is refused by name."""
    unknown = sorted(set(solver_options or {}) - set(FIXED_POINT_OPTION_KEYS))
    if unknown:
        raise ValueError('solver_options: unknown options {} (known: {})'.format(unknown, ', '.join(FIXED_POINT_OPTION_KEYS)))
    recorded = {k: v for k, v in dict(cfg.get('true_ssn_options') or {}).items() if k in FIXED_POINT_OPTION_KEYS}
    return dict(dict(FIXED_POINT_SOLVER_OPTIONS, **recorded), **(solver_options or {}))


def _check_dynamics(dynamics, cfg, solver_dtype):
    if dynamics not in DYNAMICS:
        raise ValueError('dynamics must be one of {}, got {!r}'.format(DYNAMICS, dynamics))
    if dynamics == 'fixed-point':
        if cfg.get('ssn_type', 'default') != 'default':
            raise NotImplementedError('fixed-point scoring does not support SSN with heterogeneous input (ssn_type {!r}): the '
                                      'fixed-point sampler has none'.format(cfg.get('ssn_type')))
        if solver_dtype not in ('float64', 'float32'):
            raise ValueError("solver_dtype must be 'float64' or 'float32', got {!r}".format(solver_dtype))


# ---- the core -----------------------------------------------------------------------------------------------------------

def _resolve_kernel(name, rows, nb, M, cfg):
    """(explicit kernel name, note): 'auto' is what the library picks for `rows` draws; 'duo-fused' runs as 'duo'."""
    from .. import genops
    note = None
    if name == 'duo-fused':
        name, note = 'duo', "gen_kernel 'duo-fused' differs from 'duo' only in the backward: the forward ran as 'duo'"
    return genops.resolve_kernel(rows, nb, M, genops.gen_params_of(cfg, clib.gen_kernel_code(name))), note


def shared_noise(cfg, draws, seed):
    """(z (draws, 2N, 2N), z_in (draws, 2N) or None), float32 CUDA tensors: ``rand(draws, 2N, 2N)`` of
    ``numpy.random.RandomState(seed)`` (generated on the device, bit for bit, rounded to float32), then the input noise of the
    heterogeneous-input models from the same stream (ssn.py:707-720)."""
    import torch
    from ..networks.ssn import device_rand
    from ..utils import to_device
    M = 2 * int(cfg['num_sites'])
    rng = np.random.RandomState(seed)
    z = device_rand(rng, (int(draws), M, M), torch.float32)
    zin = None
    if cfg.get('ssn_type', 'default') != 'default':
        shape = (int(draws), M)
        host = rng.choice(2, shape) * 2 - 1 if cfg.get('dist_in', 'bernoulli') == 'bernoulli' else rng.rand(*shape) * 2 - 1
        zin = to_device(host, torch.float32).contiguous()
    return z, zin


def _theta_tables(thetas, ssn_type):
    """(float32 [S][12] of J, D, S; float32 [S][2] of (V_E, V_I) or None)."""
    table = np.empty((len(thetas), 12), dtype='float32')
    v = None if ssn_type == 'default' else np.empty((len(thetas), 2), dtype='float32')
    for i, th in enumerate(thetas):
        unknown = set(th) - {'J', 'D', 'S', 'V'}
        if unknown:
            raise ValueError('parameter set {}: unknown parameters {}'.format(i, sorted(unknown)))
        for j, name in enumerate('JDS'):
            table[i, 4 * j:4 * j + 4] = np.broadcast_to(np.asarray(th[name], dtype='float64'), (2, 2)).reshape(4)
        if v is not None:
            if 'V' not in th:
                raise ValueError('parameter set {}: ssn_type {!r} needs V'.format(i, ssn_type))
            # ('deg-heteroin' has one V for both populations)
            v[i] = np.broadcast_to(np.asarray(th['V'], dtype='float64').reshape(-1), 2)
    return table, v


def _truth_on_device(truth32, shape):
    """The truth's raw and feature columns, each sorted ascending with its finite values first: (device float32 [C'][T],
    device int32 [C'], host int64 [C'])."""
    import torch
    nc, nb, ct, npr = shape[:4]
    T = truth32.shape[0]
    t = torch.as_tensor(truth32).to('cuda')
    return _sorted_columns(torch.cat([t, _features(t, nc, nb, ct * npr)], dim=1))


def _sorted_columns(allcols):
    """The columns of a device (T, C') array as the KS kernels take a truth: (float32 [C'][T] ascending with the finite values
    first, device int32 [C'] of their counts, the counts as host int64)."""
    import torch
    T = allcols.shape[0]
    finite = torch.isfinite(allcols)
    srt = torch.sort(torch.where(finite, allcols, torch.full_like(allcols, float('inf'))), dim=0).values
    m = finite.sum(dim=0).to(torch.int32).contiguous()
    return srt.t().contiguous().reshape(-1, T), m, m.cpu().numpy().astype('int64')


def _features(tc, nc, nb, q):
    import torch
    rows = tc.shape[0]
    feat = torch.empty((rows, 4 * nc * q), device=tc.device, dtype=torch.float32)
    clib.check(libssnode.ssn_tc_features_f32(tc.data_ptr(), feat.data_ptr(), rows, nc, nb, q, clib.stream_ptr()),
               'ssn_tc_features_f32')
    return feat


def project_rows(x, theta, columns=None):
    """Device float32 (rows, L): the first `columns` (default: all) values of every row of the device float32 matrix x (rows, ldx)
    projected on the rows of theta (L, columns) by ``ssn_project_rows_f32``."""
    import torch
    rows, ldx = x.shape
    C = ldx if columns is None else int(columns)
    L = theta.shape[0]
    if theta.shape[1] != C or not x.is_contiguous() or not theta.is_contiguous():
        raise ValueError('project_rows: x (rows, ldx >= {0}) and theta (L, {0}) must be contiguous, got {1} and {2}'
                         .format(C, tuple(x.shape), tuple(theta.shape)))
    out = torch.empty((rows, L), device=x.device, dtype=torch.float32)
    clib.check(libssnode.ssn_project_rows_f32(x.data_ptr(), rows, ldx, C, theta.data_ptr(), L, out.data_ptr(), clib.stream_ptr()),
               'ssn_project_rows_f32')
    return out


def _sliced_on_device(truth32, directions, direction_seed):
    """What a Wasserstein score carries from chunk to chunk: the directions on the device and the truth's projections, sorted per
    direction as `_truth_on_device` sorts the truth's columns."""
    import torch
    theta = torch.as_tensor(slice_directions(directions, truth32.shape[1], direction_seed)).to('cuda')
    tsorted, m_dev, m_host = _sorted_columns(project_rows(torch.as_tensor(truth32).to('cuda'), theta))
    return dict(theta=theta, tsorted=tsorted, m_dev=m_dev, m_host=m_host, L=theta.shape[0], C=truth32.shape[1])


def _reduce_columns(x, S, draws, truth, sliced=None):
    """The statistics of x, device float32 (S draws, C'), against truth = (sorted columns, counts, T): (num, n) as host int64
    (S, C') from one ``ssn_ks_columns_f32`` launch and one copy to the host.  With `sliced` (`_sliced_on_device`) the launch is
    ``ssn_ks_w1_columns_f32`` instead, the raw columns are projected and the projections go through a second such launch:
    (num, n, wnum, n of the projections, wnum of the projections, the projections on the device), still one copy."""
    import torch
    tsorted, m_dev, T = truth
    Ct = x.shape[1]
    out_n = torch.empty((S, Ct), device='cuda', dtype=torch.int32)
    out_num = torch.empty((S, Ct), device='cuda', dtype=torch.int64)
    if sliced is None:
        clib.check(libssnode.ssn_ks_columns_f32(x.data_ptr(), tsorted.data_ptr(), m_dev.data_ptr(), S, draws, Ct, T,
                                                out_n.data_ptr(), out_num.data_ptr(), clib.stream_ptr()), 'ssn_ks_columns_f32')
        got = torch.stack([out_num, out_n.to(torch.int64)]).cpu().numpy() if S else np.zeros((2, 0, Ct), dtype='int64')
        return got[0], got[1]
    L = sliced['L']
    out_w = torch.empty((S, Ct), device='cuda', dtype=torch.float64)
    clib.check(libssnode.ssn_ks_w1_columns_f32(x.data_ptr(), tsorted.data_ptr(), m_dev.data_ptr(), S, draws, Ct, T, out_n.data_ptr(),
                                               out_num.data_ptr(), out_w.data_ptr(), clib.stream_ptr()), 'ssn_ks_w1_columns_f32')
    proj = project_rows(x, sliced['theta'], sliced['C'])
    p_n = torch.empty((S, L), device='cuda', dtype=torch.int32)
    p_num = torch.empty((S, L), device='cuda', dtype=torch.int64)
    p_w = torch.empty((S, L), device='cuda', dtype=torch.float64)
    clib.check(libssnode.ssn_ks_w1_columns_f32(proj.data_ptr(), sliced['tsorted'].data_ptr(), sliced['m_dev'].data_ptr(), S, draws, L,
                                               sliced['tsorted'].shape[1], p_n.data_ptr(), p_num.data_ptr(), p_w.data_ptr(),
                                               clib.stream_ptr()), 'ssn_ks_w1_columns_f32')
    # (the doubles travel as their bits: one copy for everything)
    got = torch.cat([out_num.reshape(-1), out_n.to(torch.int64).reshape(-1), out_w.view(torch.int64).reshape(-1),
                     p_n.to(torch.int64).reshape(-1), p_w.view(torch.int64).reshape(-1)]).cpu().numpy()
    a, b = S * Ct, S * L
    return (got[:a].reshape(S, Ct), got[a:2 * a].reshape(S, Ct), got[2 * a:3 * a].view('float64').reshape(S, Ct),
            got[3 * a:3 * a + b].reshape(S, L), got[3 * a + b:].view('float64').reshape(S, L), proj)


def _wasserstein_keys(result, wnum, p_n, p_w, sliced, directions, direction_seed):
    """The result keys of wasserstein=True from the sums of all chunks."""
    result['wnum'] = wnum
    result['W1'] = w1_from_sums(wnum, result['n'], result['m'][None, :])
    per_direction = w1_from_sums(p_w, p_n, sliced['m_host'][None, :])
    result['SW1'] = per_direction.mean(axis=1) if per_direction.shape[0] else np.zeros(0)
    # (a row is finite in every direction or in none, and the truth is finite: one count per checkpoint, one for the truth)
    result['sliced'] = dict(directions=int(directions), seed=direction_seed, n=p_n[:, 0].copy(), m=int(sliced['m_host'][0]))


def _score_fixed_points(sampler_config, thetas, truth, draws, seed, max_draws_per_launch, return_samples, solver_options,
                        max_candidates, solver_dtype, wasserstein=False, directions=DEFAULT_DIRECTIONS, direction_seed=0):
    """`score_parameter_sets` with dynamics='fixed-point'."""
    _check_dynamics('fixed-point', sampler_config, solver_dtype)
    cfg, shape, truth32 = _check_config(dict(sampler_config, dtype='float32'), draws, truth)
    if wasserstein:
        slice_directions(directions, truth32.shape[1], direction_seed)   # (refuses before the device is touched)
    nc, nb, ct, npr, probes = shape
    draws = int(draws)
    N = int(cfg['num_sites'])
    opts = fixed_point_options(cfg, solver_options)
    from .. import ssnode
    rounds = ssnode.plan_table_rounds(draws, None, max_candidates)
    ssnode._theta_table(list(thetas))                                    # (refuses V and other keys before the device is touched)
    chunk, sizes = plan_chunks(len(thetas), rounds[0][1], max_draws_per_launch)

    import torch
    clib.require_gpu()
    tab = ssnode.sample_tuning_curves_table(
        list(thetas), NZ=draws, seed=seed, N=N, bandwidths=list(cfg['bandwidths']), contrast=list(cfg['contrasts']),
        sample_sites=probes[:npr], include_inhibitory_neurons=ct == 2, dtype=solver_dtype, max_candidates=max_candidates,
        max_draws_per_launch=max_draws_per_launch, return_torch=True, **opts)
    S, Q = len(thetas), ct * npr
    C = nc * nb * Q
    stat = stat_names(nc, nb, ct, npr)
    Ct = len(stat)
    tsorted, m_dev, m_host = _truth_on_device(truth32, shape)
    tc = tab.tunings.to(torch.float32).reshape(S * draws, C)
    feat = _features(tc, nc, nb, Q)
    # (a row that was not accepted is NaN in every raw column; the feature kernel gives such a curve a finite prefbw)
    feat = torch.where(torch.isnan(tc[:, :1]), torch.full_like(feat, float('nan')), feat)
    x = torch.cat([tc, feat], dim=1).contiguous()
    sliced = _sliced_on_device(truth32, directions, direction_seed) if wasserstein else None
    got = _reduce_columns(x, S, draws, (tsorted, m_dev, truth32.shape[0]), sliced)
    num, n = got[0], got[1]
    result = dict(stat=stat, num=num, n=n, m=m_host, KSD=ksd_from_counts(num, n, m_host[None, :]), gen_kernel=None, chunk=chunk,
                  chunks=sizes, note=None, draws=draws, seed=seed, bandwidths=[float(b) for b in cfg['bandwidths']],
                  contrasts=[float(c) for c in cfg['contrasts']], probes=probes, gen_step=np.arange(S), dynamics='fixed-point',
                  accepted=tab.accepted, used=tab.used, rejections=tab.rejections, candidates=tab.candidates,
                  solver_variant=tab.variant, solver_options={k: (v if isinstance(v, (int, float, str)) else list(v))
                                                              for k, v in opts.items()}, solver_dtype=solver_dtype)
    if wasserstein:
        _wasserstein_keys(result, got[2], got[3], got[4], sliced, directions, direction_seed)
    if return_samples:
        xh = x.cpu().numpy().reshape(S, draws, Ct)
        result['tuning_curves'], result['features'] = xh[:, :, :C], xh[:, :, C:]
        if wasserstein:
            result['projections'] = got[5].cpu().numpy().reshape(S, draws, sliced['L'])
    return result


def score_parameter_sets(sampler_config, thetas, truth, draws=DEFAULT_DRAWS, seed=0, gen_kernel=None,
                         max_draws_per_launch=DEFAULT_MAX_DRAWS_PER_LAUNCH, return_samples=False, dynamics='fixed-time',
                         solver_options=None, max_candidates=None, solver_dtype='float64', wasserstein=False,
                         directions=DEFAULT_DIRECTIONS, direction_seed=0):
    """KS statistics of `draws` tuning curves per parameter set against `truth`, all sets on the same noise.

    sampler_config: the fixed-time sampler -- num_sites, bandwidths, contrasts, smoothness, k, n, tau_E, tau_I, dt, io_type,
      seqlen, skip_steps (defaults: networks.wgan.DEFAULT_PARAMS), norm_probes + include_inhibitory_neurons (or probes),
      ssn_type, dist_in, gen_kernel.
    dynamics: 'fixed-time' (the generator above) or 'fixed-point': the curves of a set are those of the first `draws` candidate
      draws whose fixed points converge for every stimulus (`ssnode.sample_tuning_curves_table` in `solver_dtype`, at most
      `max_candidates` candidates; solver options: `fixed_point_options`); sets with heterogeneous input are refused
      (NotImplementedError).  The result then has accepted, used (S,), rejections (S, 2), candidates and solver_variant too, and
      ``n`` is the accepted count.
    thetas: list of dicts J, D, S (2 x 2 or scalars) and V where the ssn_type has it.
    truth: (T, columns) array in the sampler's column order.
    wasserstein: also the Wasserstein distances (both dynamics): wnum (S, C') float64, the weighted sums of
      ``ssn_ks_w1_columns_f32`` that replaces the KS launch (num, n, KSD are the same arrays as without), W1 = wnum / (n m)
      (NaN where n m = 0), SW1 (S,), the mean over `directions` directions (`slice_directions` with `direction_seed`) of the W1
      of the projected raw columns, and sliced = dict(directions, seed, n (S,): finite rows per checkpoint, m); with
      `return_samples` also projections (S, draws, directions).

    Returns a dict: stat (names, `stat_names`), num / n (S, C') and m (C',) integers, KSD (S, C'), gen_kernel (the kernel that
    ran), chunk, chunks, note; with `return_samples` also tuning_curves (S, draws, C) and features (S, draws, 4 curves)."""
    if dynamics != 'fixed-time':
        _check_dynamics(dynamics, sampler_config, solver_dtype)
        return _score_fixed_points(sampler_config, thetas, truth, draws, seed, max_draws_per_launch, return_samples,
                                   solver_options, max_candidates, solver_dtype, wasserstein, directions, direction_seed)
    kernel_name = gen_kernel or sampler_config.get('gen_kernel') or 'auto'
    cfg, shape, truth32 = _check_config(sampler_config, draws, truth)
    if wasserstein:
        slice_directions(directions, truth32.shape[1], direction_seed)   # (refuses before the device is touched)
    nc, nb, ct, npr, probes = shape
    draws = int(draws)
    chunk, sizes = plan_chunks(len(thetas), draws, max_draws_per_launch)
    ssn_type = cfg.get('ssn_type', 'default')
    table, vtab = _theta_tables(thetas, ssn_type)
    N = int(cfg['num_sites'])
    M, NBT, Q = 2 * N, nc * nb, ct * npr
    C = NBT * Q
    kernel, note = _resolve_kernel(kernel_name, chunk * draws, NBT, M, cfg)

    import torch
    from .. import genops
    gp = genops.gen_params_of(cfg, clib.gen_kernel_code(kernel))
    from ..networks._common import grid_stimulator_inputs
    from ..stimuli import stimulus_batch
    from ..utils import to_device
    clib.require_gpu()
    stat = stat_names(nc, nb, ct, npr)
    tsorted, m_dev, m_host = _truth_on_device(truth32, shape)
    T = truth32.shape[0]
    z, zin = shared_noise(cfg, draws, seed)
    con_h, bw_h = grid_stimulator_inputs(np.asarray(cfg['contrasts'], dtype='float64'), np.asarray(cfg['bandwidths'], dtype='float64'),
                                         chunk * draws)
    bw, con = to_device(bw_h, torch.float32).contiguous(), to_device(con_h, torch.float32).contiguous()
    pr = to_device(np.asarray(probes, dtype=np.int64))
    zin_tiled = zin.repeat(chunk, 1).contiguous() if zin is not None else None
    table_dev = to_device(table, torch.float32).contiguous()
    v_dev = to_device(vtab, torch.float32).contiguous() if vtab is not None else None
    S, Ct = len(thetas), len(stat)
    num, n = np.zeros((S, Ct), dtype='int64'), np.zeros((S, Ct), dtype='int64')
    samples = ([], [], []) if return_samples else None
    sliced = _sliced_on_device(truth32, directions, direction_seed) if wasserstein else None
    if wasserstein:
        wnum, p_n, p_w = np.zeros((S, Ct)), np.zeros((S, sliced['L']), dtype='int64'), np.zeros((S, sliced['L']))
    s0 = 0
    for ns in sizes:
        rows = ns * draws
        W = torch.empty((rows, M, M), device='cuda', dtype=torch.float32)
        clib.check(libssnode.ssn_build_w_table_f32(z.data_ptr(), table_dev[s0:s0 + ns].data_ptr(), W.data_ptr(), ns, draws, N,
                                                   clib.stream_ptr()), 'ssn_build_w_table_f32')
        if zin is None:
            ext = stimulus_batch(bw[:rows], con[:rows], cfg['smoothness'], N)
        else:
            ext = torch.empty((rows, NBT, M), device='cuda', dtype=torch.float32)
            clib.check(libssnode.ssn_ens_stimulus_hetero_f32(
                bw.data_ptr(), con.data_ptr(), ctypes.c_float(cfg['smoothness']), zin_tiled.data_ptr(),
                v_dev[s0:s0 + ns].data_ptr(), ext.data_ptr(), ns, draws, NBT, N, clib.stream_ptr()), 'ssn_ens_stimulus_hetero_f32')
        ta = genops.gen_forward(W, ext, gp)['time_avg']
        tc = ta[:, :, pr].reshape(rows, C)                                  # ssn.py:846-848
        x = torch.cat([tc, _features(tc, nc, nb, Q)], dim=1)               # (ns draws, C + 4 curves)
        got = _reduce_columns(x, ns, draws, (tsorted, m_dev, T), sliced)   # the chunk's one copy to the host
        num[s0:s0 + ns], n[s0:s0 + ns] = got[0], got[1]
        if wasserstein:
            wnum[s0:s0 + ns], p_n[s0:s0 + ns], p_w[s0:s0 + ns] = got[2], got[3], got[4]
        if return_samples:
            xh = x.cpu().numpy().reshape(ns, draws, Ct)
            samples[0].append(xh[:, :, :C])
            samples[1].append(xh[:, :, C:])
            if wasserstein:
                samples[2].append(got[5].cpu().numpy().reshape(ns, draws, sliced['L']))
        s0 += ns
    result = dict(stat=stat, num=num, n=n, m=m_host, KSD=ksd_from_counts(num, n, m_host[None, :]), gen_kernel=kernel, chunk=chunk,
                  chunks=sizes, note=note, draws=draws, seed=seed, bandwidths=[float(b) for b in cfg['bandwidths']],
                  contrasts=[float(c) for c in cfg['contrasts']], probes=probes, gen_step=np.arange(S))
    if wasserstein:
        _wasserstein_keys(result, wnum, p_n, p_w, sliced, directions, direction_seed)
    if return_samples:
        result['tuning_curves'] = np.concatenate(samples[0]) if samples[0] else np.zeros((0, draws, C), dtype='float32')
        result['features'] = np.concatenate(samples[1]) if samples[1] else np.zeros((0, draws, Ct - C), dtype='float32')
        if wasserstein:
            result['projections'] = (np.concatenate(samples[2]) if samples[2]
                                     else np.zeros((0, draws, sliced['L']), dtype='float32'))
    return result


# ---- runs ---------------------------------------------------------------------------------------------------------------

def _records(records_or_path):
    from ..loaders import Records, load_records
    return records_or_path if isinstance(records_or_path, Records) else load_records(records_or_path)


def calc_distdiff(records_or_path, steps=slice(None), draws=DEFAULT_DRAWS, seed=0, gen_kernel=None,
                  max_draws_per_launch=DEFAULT_MAX_DRAWS_PER_LAUNCH, return_samples=False, extra_thetas=(),
                  dynamics='fixed-time', solver_options=None, max_candidates=None, solver_dtype='float64', wasserstein=False,
                  directions=DEFAULT_DIRECTIONS, direction_seed=0):
    """`score_parameter_sets` for the rows `steps` (a slice or a list of row positions) of a run's ``generator`` table, with the
    run's own sampler and ``truth.npy``.  `extra_thetas`: parameter sets scored in front of the rows (gen_step -1, -2, ...),
    e.g. the truth's own.  The result carries the rows' ``gen_step``.  `dynamics`, `solver_options`, `max_candidates`,
    `solver_dtype`, `wasserstein`, `directions`, `direction_seed`: see `score_parameter_sets` (the run's recorded
    ``true_ssn_options`` come before `solver_options`)."""
    rec = _records(records_or_path)
    try:
        table = rec.generator
    except RuntimeError as err:
        raise ValueError('{} is not a run directory with a generator table: {}'.format(rec.directory, err))
    cfg = sampler_config_of_run(rec.run_config)
    steps = parse_steps(steps)
    positions = list(range(len(table)))[steps] if isinstance(steps, slice) else [range(len(table))[int(i)] for i in steps]
    thetas = list(extra_thetas) + [rec.gen_params_at(i) for i in positions]
    gen_step = np.concatenate([-1 - np.arange(len(extra_thetas)), np.asarray(table['gen_step'], dtype='int64')[positions]]).astype('int64')
    result = score_parameter_sets(cfg, thetas, rec.truth, draws=draws, seed=seed, gen_kernel=gen_kernel,
                                  max_draws_per_launch=max_draws_per_launch, return_samples=return_samples, dynamics=dynamics,
                                  solver_options=solver_options, max_candidates=max_candidates, solver_dtype=solver_dtype,
                                  wasserstein=wasserstein, directions=directions, direction_seed=direction_seed)
    result['gen_step'] = gen_step
    return result


def make_parser():
    import argparse
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('rundir', help='Run directory (info.json, generator table, truth.npy).')
    parser.add_argument('--steps', default=':', help="Rows of the generator table: START:STOP:STEP or a comma separated list.")
    parser.add_argument('--draws', default=DEFAULT_DRAWS, type=int, help='Tuning curves per checkpoint (at most {}).'.format(clib.KS_MAX_DRAWS))
    parser.add_argument('--seed', default=0, type=int, help='Seed of the noise every checkpoint shares.')
    parser.add_argument('--gen-kernel', default=None, choices=tuple(clib.GEN_KERNELS), help='Default: the kernel the run recorded.')
    parser.add_argument('--max-draws-per-launch', default=DEFAULT_MAX_DRAWS_PER_LAUNCH, type=int,
                        help='Draws of one generator launch: checkpoints per chunk = this // draws.')
    parser.add_argument('--output', default=None, help='Output directory (default: the run directory).')
    parser.add_argument('--save-tuning-curves', action='store_true',
                        help='Also write tuning_curves/{:010d}.csv, bandwidths.csv and sample_epochs.csv.')
    parser.add_argument('--dynamics', default='fixed-time', choices=DYNAMICS,
                        help="'fixed-point': score the first --draws candidate draws whose fixed points converge (the truth of "
                             "--dataset-provider ssnode) and write rejections.csv.")
    parser.add_argument('--max-candidates', default=None, type=int,
                        help='fixed-point: candidate draws per checkpoint at most (default: max(4 draws, draws + 64)).')
    parser.add_argument('--solver-dtype', default='float64', choices=('float64', 'float32'), help='fixed-point: solver arithmetic.')
    parser.add_argument('--wasserstein', action='store_true',
                        help='Also the Wasserstein distances: W1 per statistic and the sliced W1 of the raw columns, written to '
                             'wdist.csv and wdist.json.')
    parser.add_argument('--directions', default=DEFAULT_DIRECTIONS, type=int,
                        help='--wasserstein: directions of the sliced distance (at most {}).'.format(clib.W1_MAX_DIRECTIONS))
    parser.add_argument('--direction-seed', default=0, type=int, help='--wasserstein: seed of the directions.')
    return parser


def recorded_arguments(ns):
    """The ``arguments`` of distdiff.json for parsed options: the keys the file always had in its mode, never the options of
    --wasserstein (those are wdist.json's)."""
    fixed_point = ns.dynamics == 'fixed-point'
    return {k: v for k, v in vars(ns).items()
            if (fixed_point and k not in _WASSERSTEIN_ARGUMENTS) or k in _FIXED_TIME_ARGUMENTS}


def write_rejections(path, result):
    """rejections.csv of a fixed-point result: gen_step, accepted, used, code1, code2 per checkpoint."""
    import pandas
    pandas.DataFrame(dict(gen_step=np.asarray(result['gen_step']), accepted=result['accepted'], used=result['used'],
                          code1=result['rejections'][:, 0], code2=result['rejections'][:, 1]),
                     columns=['gen_step', 'accepted', 'used', 'code1', 'code2']).to_csv(path, index=False)


def main(args=None):
    ns = make_parser().parse_args(args)
    output = ns.output or ns.rundir
    result = calc_distdiff(ns.rundir, steps=parse_steps(ns.steps), draws=ns.draws, seed=ns.seed, gen_kernel=ns.gen_kernel,
                           max_draws_per_launch=ns.max_draws_per_launch, return_samples=ns.save_tuning_curves,
                           dynamics=ns.dynamics, max_candidates=ns.max_candidates, solver_dtype=ns.solver_dtype,
                           wasserstein=ns.wasserstein, directions=ns.directions, direction_seed=ns.direction_seed)
    os.makedirs(output, exist_ok=True)
    write_long_table(os.path.join(output, 'distdiff.csv'), result)
    fixed_point = ns.dynamics == 'fixed-point'
    arguments = recorded_arguments(ns)
    extra = {}
    if fixed_point:
        write_rejections(os.path.join(output, 'rejections.csv'), result)
        extra = dict(dynamics='fixed-point', accepted=[int(v) for v in result['accepted']], used=[int(v) for v in result['used']],
                     rejections=[[int(v) for v in row] for row in result['rejections']], candidates=int(result['candidates']),
                     solver_variant=int(result['solver_variant']), solver_options=result['solver_options'],
                     solver_dtype=result['solver_dtype'])
    with open(os.path.join(output, 'distdiff.json'), 'w') as f:
        json.dump(dict(arguments=arguments, gen_kernel=result['gen_kernel'], note=result['note'], chunk=result['chunk'],
                       chunks=result['chunks'], draws=result['draws'], bandwidths=result['bandwidths'],
                       contrasts=result['contrasts'], probes=result['probes'], features=list(FEATURES),
                       gen_steps=[int(s) for s in result['gen_step']], **extra), f, indent=1)
    if ns.wasserstein:
        write_wdist_table(os.path.join(output, 'wdist.csv'), result)
        with open(os.path.join(output, 'wdist.json'), 'w') as f:
            json.dump(dict(arguments={k: getattr(ns, k) for k in _WASSERSTEIN_ARGUMENTS}, directions=result['sliced']['directions'],
                           gen_steps=[int(s) for s in result['gen_step']]), f, indent=1)
    if ns.save_tuning_curves:
        tcdir = os.path.join(output, 'tuning_curves')
        os.makedirs(tcdir, exist_ok=True)
        for i, curves in enumerate(result['tuning_curves']):
            np.savetxt(os.path.join(tcdir, '{:010d}.csv'.format(i)), curves, delimiter=',')
        np.savetxt(os.path.join(output, 'bandwidths.csv'), result['bandwidths'], delimiter=',')
        np.savetxt(os.path.join(output, 'sample_epochs.csv'), result['gen_step'], delimiter=',')
    return result


if __name__ == '__main__':
    main()

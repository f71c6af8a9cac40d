"""ORACLE -- TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Nothing under tc_gan_amd/ imports this module.

The cases, inputs, fp64 results, error measures and tolerances that hold the fp32 critic (`--disc-precision fp32`, the default
of every GAN run) to `gan_torch.critic_forward` + torch autograd at the edges of every kernel path
(tests/test_critic_edges_gpu.py), and that tests/test_critic_cases.py checks without a GPU.

Why its own inputs.  A net made the way tests/test_critic_gpu.py makes it (Glorot weights, biases ~ N(0, 0.01), contrast
column 20) has rectify units that are inactive on every row: the oracle's dL/dW_l then has a column that is exactly zero and
dL/dW_{l+1} a row that is exactly zero, and a kernel that drops exactly such a unit -- the last one of a ragged tile, say --
passes (tests/test_critic_cases.py::test_the_gap_dead_units_hide_a_lost_edge records that).  And a unit whose pre-activation
rounds to the other side of zero in fp32 moves one row's share of a whole gradient column, which is why those tests sit at
1e-3.  Here, by construction and asserted by `conditions`:

  * every unit is alive: unit j's bias is minus the q_j quantile of its (normalised) pre-activation over a 4096-row probe
    batch, q_j in [0.25, 0.75] ([0.4, 0.6] where a batch has fewer than 200 rows, so that a batch of 33 stays inside 10 ... 90 %);
  * no row of xg, xd, xp (or of the extra forward batch) has a pre-activation of any layer within 1e-3 of that layer's rms
    pre-activation: such rows are redrawn (rows are independent in the critic), so the device's masks are the oracle's;
  * no bias / w_out gradient hides an end element: first and last element >= 0.05 of the vector's largest, at most 1 % of its
    elements below 100 x the tolerance -- by the reseed table below.

Measures.  Weight-gradient matrices: |got - want|_ij / min(max_j' |want_ij'|, max_i' |want_i'j|), every element on the scale of
its own row and column (a lost row or column measures >= 1 whatever the contrast row of W_0 holds).  Vectors, D values, the
input gradient: relative to the tensor's largest element.  Loss and the three statistics (and the mean D of `input_grad`):
relative.  The accuracy mean D(xg) - mean D(xd): relative to the larger of the two means it is the difference of.

Tolerance: four times the deviation of the same oracle run in float32 on the CPU, in the same measure,
per case and tensor kind (`tolerances`); never above 1e-3, never taken from a kernel.  One deliberate exception to the plain rule:
for the two scalar kinds (statistics, accuracy) a deviation below float32's unit roundoff 2^-24 counts as that roundoff.

Measured (largest over the cases; float32 oracle on two CPUs / one MI355X, default setting / SSN_CRITIC_FUSED=0):
    weight matrices (row-and-column scale)   5.0e-6, 7.0e-6  /  6.3e-6 / 2.7e-6      tolerances 1.5e-6 ... 2.8e-5
    bias and w_out gradients / largest       2.3e-6, 3.2e-6  /  1.4e-6 / 1.4e-6                 1.1e-6 ... 1.3e-5
    D values / largest                       3.4e-6, 3.3e-6  /  3.3e-6 / 3.3e-6                 8.5e-7 ... 1.3e-5
    input gradient / largest                 8.0e-6, 4.8e-6  /  8.0e-6 / 8.0e-6                 4.9e-7 ... 1.9e-5
    loss, statistics (relative)              6.2e-7, 1.4e-6  /  5.4e-7 / 5.4e-7                 2.4e-7 ... 5.5e-6
    accuracy / larger mean                   5.3e-7, 4.3e-7  /  6.0e-7 / 6.0e-7                 2.4e-7 ... 1.7e-6
D values, input gradient, statistics and accuracy have their largest figures in 'ragged-ln' (LayerNorm over 6 and 5 units);
without it the device is within 9.7e-7, 1.2e-6, 3.6e-7 and 5.0e-7.  No case missed its tolerance on either setting and no
kernel had to change; the device used at most 0.92 of a tolerance (the input gradient of 'ln-wide-unsplit', whose dot products
run over K = 512; 0.78 elsewhere).

The unsplit fall-back of the split-K GEMM (ssn_critic.hip `gemm`: "a 5th split GEMM into one C", or scratch exhausted).  The
first is unreachable: the plain chain issues two weight-gradient GEMMs per weight, the LayerNorm chain three.  The plain chain
cannot exhaust the scratch either: it is sized 2 x choose_splits(K = ng + nd + np) slabs per weight and choose_splits does not
fall with K.  The LayerNorm chain CAN: its three GEMMs per weight take choose_splits(ng + nd) + 2 choose_splits(np) slabs, which
exceeds 2 x choose_splits(ng + nd + np) once the tile count and not K limits the splits -- wide layers, np >= 1024 (512 x 512:
8 + 8 + 8 against 16).  The case 'ln-wide-unsplit' is there for that.
"""
import collections
import functools

import numpy as np
import torch

from . import gan_torch as og

LMD = 10.0
MARGIN = 1e-3                # rows with a pre-activation within MARGIN x the layer's rms pre-activation are redrawn
PROBE_ROWS = 4096
LN_EPS = 1e-4
LEAK = {'rectify': 0.0, 'leaky_rectify': 0.01}
TAIL_ROWS = 6                # the rows of the last short K slice's tail in 'chain-first' (70 = 4 x 16 + 6)

Case = collections.namedtuple('Case', 'name batches nx layers norm nonlinearity conditional path rb reaches')

_LN3 = ('none', 'layer', 'layer')
_LN4 = ('none', 'layer', 'layer', 'layer')
_PAPER = (128, 128, 128, 128)


def _case(name, batches, nx, layers, path, rb=None, norm='none', nonlinearity='rectify', conditional=True, reaches=''):
    norm = tuple(norm) if isinstance(norm, (list, tuple)) else (norm,) * len(layers)
    return Case(name, tuple(batches), nx, tuple(layers), norm, nonlinearity, conditional, path, rb, reaches)


# path / rb: the path of `loss_grad` in the default environment ('fused': ssn_critic_fused.hip with `rb` rows per workgroup,
# 'plain': the GEMM chain of ssn_critic.hip, 'general': the LayerNorm chain of ssn_critic_ln.hip).  With SSN_CRITIC_FUSED=0 a
# fused case runs on 'plain' (no normalisation) or 'general'; the others stay where they are.
CASES = [
    _case('ragged', (7, 5, 6), 4, (9, 6, 5), 'fused', 4, reaches='fused, RB = 4, everything ragged'),
    _case('ragged-ln', (7, 5, 6), 4, (9, 6, 5), 'fused', 4, norm=_LN3, reaches='the same with LayerNorm on layers 2, 3'),
    _case('rb4-last', (342, 341, 341), 5, (128, 100, 17), 'fused', 4, reaches='fused, last size of RB = 4 (1024 rows)'),
    _case('rb8-first', (342, 342, 341), 5, (128, 100, 17), 'fused', 8,
          reaches='fused, first size of RB = 8 (1025 rows): ragged last block of the [xg; xd] rows (684 = 85 x 8 + 4) and of the '
                  'penalty rows (341 = 42 x 8 + 5)'),
    _case('fused-last', (683, 683, 682), 8, _PAPER, 'fused', 8, reaches="fused, last size (2048 rows), the paper's critic"),
    _case('fused-last-ln', (683, 683, 682), 8, _PAPER, 'fused', 8, norm=_LN4, reaches='the same with LayerNorm on layers 2-4'),
    _case('chain-first', (683, 683, 683), 8, _PAPER, 'plain',
          reaches='2049 rows: GEMM chain; split-K with K = 1366 -> 10 slices of 144, last 70 (= 4 x 16 + 6); K = 683 -> 5 slices, last 107'),
    _case('chain-first-ln', (683, 683, 683), 8, _PAPER, 'general', norm=_LN4, reaches='2049 rows: LayerNorm chain, same slices'),
    _case('odd-129', (700, 650, 600), 8, (129, 65, 33), 'plain',
          reaches='widths just past 128, every M N odd (1419, 8385, 2145, 33): the scalar branch of splitk_reduce_kernel through M N % 4'),
    _case('odd-129-ln', (700, 650, 600), 8, (129, 65, 33), 'general', norm='layer', reaches='the same on the LayerNorm chain'),
    _case('wide-nosplit', (130, 97, 64), 5, (132, 200), 'plain', reaches='wide, K below 512 (no split), ragged M, N, K tiles'),
    _case('leaky', (77, 50, 33), 4, (72, 100, 36), 'plain', nonlinearity='leaky_rectify',
          reaches='leaky slope on the GEMM chain at fused sizes'),
    _case('nocond', (64, 40, 50), 5, (40, 24), 'plain', conditional=False, reaches='unconditional critic (no condition columns: GEMM chain)'),
    # fewer slices than chosen; a slab with M N % 4 == 0 behind odd-sized ones; the unsplit fall-back of `gemm`
    _case('resliced', (650, 645, 520), 5, (130, 41), 'plain',
          reaches='K = 1295: 10 splits chosen, kchunk 130 -> 144, 9 slices after rounding (last 143); K = 520: 4 slices of 144, last 88; '
                  'the slabs of dW_1 (M N = 8 x 130 = 1040, a multiple of 4) lie behind 9 x 41 + 9 x 5330 floats of earlier slabs, off '
                  '16-byte alignment: the scalar branch of splitk_reduce_kernel through the alignment test'),
    _case('ln-wide-unsplit', (512, 512, 1024), 5, (512, 512), 'general', norm='layer',
          reaches='LayerNorm chain, scratch exhausted: the 512 x 512 weight-gradient GEMM of layer 2 in sweep 2 (the second to last '
                  'issued) runs unsplit and adds into the gradient before the slabs of the earlier ones'),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# Seed offsets of the cases whose first draw misses a condition of `conditions` (an end element of a bias or w_out gradient
# below 0.05 of the vector's largest, or more than 1 % of a vector below 100 x the tolerance).
RESEED = {'ragged-ln': 1, 'rb4-last': 1, 'fused-last': 5, 'fused-last-ln': 1, 'chain-first': 17, 'chain-first-ln': 14,
          'odd-129-ln': 4, 'wide-nosplit': 2, 'nocond': 2, 'resliced': 3, 'ln-wide-unsplit': 16}


def case_id(c):
    return c.name


def dims(c):
    return [c.nx + (3 if c.conditional else 0)] + list(c.layers)


def rows(c):
    return sum(c.batches)


def has_extra(c):
    """Nets up to 128 wide also run forward / input_grad / accuracy on 1030 rows (fused forward with RB = 8) and on 2049 (chain)."""
    return max(c.layers) <= 128


EXTRA = (1030, 2049)


# ------------------------------------------------------------------ the dispatch rule, restated (ssn_capi.hip `critic_path`)
FUSED_MAX_WIDTH, FUSED_MAX_LAYERS, FUSED_MAX_ROWS = 128, 8, 2048


def fused_supported(c):
    d = dims(c)
    return len(c.layers) <= FUSED_MAX_LAYERS and all(1 <= w <= FUSED_MAX_WIDTH for w in d) and d[0] > 3


def critic_path(c, nrows, fused_enabled=True):
    """'fused' / 'plain' / 'general' for a pass over `nrows` stacked rows (loss_grad: ng + nd + np; forward, input_grad: the batch)."""
    norm, leak = any(n == 'layer' for n in c.norm), LEAK[c.nonlinearity]
    if norm and leak:
        return 'general'
    if leak:
        return 'plain'
    if c.conditional and fused_enabled and nrows <= FUSED_MAX_ROWS and fused_supported(c):
        return 'fused'
    return 'general' if norm else 'plain'


def fused_rb(nrows):
    """Rows per workgroup of the fused kernels (ssn_critic_fused.hip `fused_rb`)."""
    return 4 if nrows <= 1024 else 8 if nrows <= 2048 else 16


def choose_splits(M, N, K):
    """ssn_critic.hip `choose_splits`."""
    tiles = ((N + 63) // 64) * ((M + 63) // 64)
    if K < 512 or tiles >= 256:
        return 1
    return max(1, min((512 + tiles - 1) // tiles, K // 128))


def k_slices(M, N, K):
    """(slices, kchunk, length of the last slice) of an fp32 weight-gradient GEMM with room in the scratch (`gemm`: 16-deep tiles)."""
    s = choose_splits(M, N, K)
    kchunk = ((K + s - 1) // s + 15) // 16 * 16
    s = (K + kchunk - 1) // kchunk
    return s, kchunk, K - (s - 1) * kchunk


def splitk_scratch_floats(c):
    d = dims(c)
    n = sum(2 * choose_splits(a, b, rows(c)) * a * b for a, b in zip(d[:-1], d[1:]))
    return n + 2 * choose_splits(d[-1], 1, rows(c)) * d[-1] + 64


def plain_chain_slabs(c):
    """The weight-gradient GEMMs of the plain chain in the order it issues them (w_out, the [xg; xd] chain from the last layer
    down, the penalty chain from the first layer up): [(M, N, K, slices, offset)] -- offset: where the GEMM's slabs start, in
    floats from the start of the workspace (whose base is aligned), None without a split."""
    d, (ng, nd, npn) = dims(c), c.batches
    L, bgd, per_row = len(c.layers), ng + nd, sum(dims(c))
    order = [(d[L], 1, bgd)] + [(d[l], d[l + 1], bgd) for l in range(L - 1, -1, -1)] + [(d[l], d[l + 1], npn) for l in range(L)]
    used, out = 2 * bgd * per_row + bgd + 3 * npn * per_row + npn + d[L], []         # (critic_loss_grad: h, v, up; hp, vp, ep, dp; tmp)
    for M, N, K in order:
        s = k_slices(M, N, K)[0]
        out.append((M, N, K, s, used if s > 1 else None))
        used += s * M * N if s > 1 else 0
    return out


def general_chain_slabs(c):
    """The weight-gradient GEMMs of the LayerNorm chain in the order it issues them: [(M, N, K, slices actually taken)] -- 1 where
    the scratch (or K) leaves no split."""
    d, (ng, nd, npn) = dims(c), c.batches
    L = len(c.layers)
    order = [(d[L], 1, ng + nd)] + [(d[l - 1], d[l], ng + nd) for l in range(1, L + 1)]
    order += [(d[l - 1], d[l], npn) for l in range(1, L + 1)] + [(d[l - 1], d[l], npn) for l in range(L, 0, -1)]
    cap, used, out = splitk_scratch_floats(c), 0, []
    for M, N, K in order:
        s = choose_splits(M, N, K)
        if used + s * M * N > cap:
            s = 1
        else:
            s = k_slices(M, N, K)[0]
        if s > 1:
            used += s * M * N
        out.append((M, N, K, s))
    return out


# ------------------------------------------------------------------ inputs
def _f32(a):
    return np.asarray(a, dtype='float64').astype('float32').astype('float64')


SCALE = {'g': (1.0, 1.0), 'd': (0.85, 0.85), 'p': (0.85, 1.0), 'e': (0.85, 1.0)}


def _draw_rows(rs, n, c, which='p'):
    """Rows of batch `which`: tuning curves uniform in [0, 5 s) with s = 1 for xg, 0.85 for xd (the two batches differ in
    distribution, so mean D(xg) - mean D(xd) and the last bias gradient w_j (frac_g - frac_d) are no near-ties) and s uniform
    in [0.85, 1] per row for xp, the extra rows and the probe batch."""
    lo, hi = SCALE[which]
    x = _f32(rs.rand(n, c.nx) * 5 * rs.uniform(lo, hi, (n, 1)))
    if not c.conditional:
        return x, None
    cond = np.stack([rs.choice([5.0, 10.0, 20.0], n), _f32(rs.rand(n) * 2 - 1), rs.randint(0, 2, n).astype('float64')], axis=1)
    return x, cond


def pre_activations(c, params, x, cond):
    """numpy fp64 restatement of the forward: ([pre_l (n, width_l): after normalisation and bias, in front of the nonlinearity], D)."""
    h = x if cond is None else np.concatenate([x, cond[:, :1], np.abs(cond[:, 1:2]), cond[:, 2:3]], axis=1)
    leak, pres = LEAK[c.nonlinearity], []
    for l in range(len(c.layers)):
        a = h @ params[2 * l]
        if c.norm[l] == 'layer':
            a = (a - a.mean(axis=1, keepdims=True)) / np.sqrt(a.var(axis=1, keepdims=True) + LN_EPS)
        pre = a + params[2 * l + 1]
        pres.append(pre)
        h = np.where(pre > 0, pre, leak * pre)
    return pres, (h @ params[-1])[:, 0]


def _kink_free(rs, n, c, params, rms, which):
    """n rows none of which has a pre-activation of any layer within MARGIN x that layer's rms; (x, cond, redraw rounds)."""
    x, cond = _draw_rows(rs, n, c, which)
    todo, rounds = np.arange(n), 0
    while True:
        pres, _ = pre_activations(c, params, x[todo], None if cond is None else cond[todo])
        bad = np.zeros(len(todo), dtype=bool)
        for pre, r in zip(pres, rms):
            bad |= (np.abs(pre) < MARGIN * r).any(axis=1)
        if not bad.any():
            return x, cond, rounds
        todo = todo[bad]
        xr, cr = _draw_rows(rs, len(todo), c, which)
        x[todo] = xr
        if cond is not None:
            cond[todo] = cr
        rounds += 1
        assert rounds < 200


@functools.lru_cache(maxsize=None)
def inputs(c):
    """fp64 arrays of fp32-representable numbers: params (W_1, b_1, ..., W_L, b_L, W_out), xg, cg, xd, cd, xp, cp (cond None for the
    unconditional critic), xe, ce (2049 further rows, `has_extra` cases), rms (per layer), rounds (redraws of the worst batch)."""
    rs = np.random.RandomState(1000003 * RESEED.get(c.name, 0) + 7919 * CASES.index(c) + 17)
    d = dims(c)
    span = 0.25 if min(c.batches) >= 200 else 0.1
    xs, cs = _draw_rows(rs, PROBE_ROWS, c)
    h = xs if cs is None else np.concatenate([xs, cs[:, :1], np.abs(cs[:, 1:2]), cs[:, 2:3]], axis=1)
    leak, params, rms = LEAK[c.nonlinearity], [], []
    for l in range(len(c.layers)):
        W = _f32(og.glorot_uniform(rs, d[l], d[l + 1]))
        a = h @ W
        if c.norm[l] == 'layer':
            a = (a - a.mean(axis=1, keepdims=True)) / np.sqrt(a.var(axis=1, keepdims=True) + LN_EPS)
        q = rs.uniform(0.5 - span, 0.5 + span, d[l + 1])
        b = _f32([-np.quantile(a[:, j], q[j]) for j in range(d[l + 1])])
        pre = a + b
        rms.append(float(np.sqrt((pre ** 2).mean())))
        h = np.where(pre > 0, pre, leak * pre)
        params += [W, b]
    params.append(_f32(og.glorot_uniform(rs, d[-1], 1)))
    res = dict(params=params, rms=rms, rounds=0)
    for key, n in zip('gdp', c.batches):
        res['x' + key], res['c' + key], r = _kink_free(rs, n, c, params, rms, key)
        res['rounds'] = max(res['rounds'], r)
    if has_extra(c):
        res['xe'], res['ce'], _ = _kink_free(rs, EXTRA[1], c, params, rms, 'e')
    return res


def flat_params(c):
    return np.concatenate([p.ravel() for p in inputs(c)['params']])


# ------------------------------------------------------------------ the oracle (torch, fp64 or fp32)
def _kw(c):
    return dict(normalization=list(c.norm), nonlinearity=c.nonlinearity, use_scale=False)


def _t(a, dt):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dt)


def _forward_and_input_grad(c, P, x, cond, dt):
    """D (n,), gx = d(-mean D)/dx (n, nx), mean D -- what `forward` and `input_grad(scale=-1/n)` return."""
    x = _t(x, dt).clone().requires_grad_(True)
    D = og.critic_forward(P, x, _t(cond, dt), **_kw(c))[:, 0]
    gx, = torch.autograd.grad(-D.mean(), x)
    return D.detach().double().numpy(), gx.double().numpy(), float(D.detach().double().mean())


@functools.lru_cache(maxsize=None)
def oracle(c, dtype='float64'):
    """Everything the GPU module compares, numpy fp64 whatever `dtype` the oracle ran in:
    grads (list, parameter order), stats [mean D(xg), mean D(xd), penalty, loss], dvals (ng + nd), pen_rows (np), fwd_p = D(xp),
    gx, gx_mean (input_grad of xg, scale -1 / ng), acc; `has_extra` cases: fwd_<n>, gx_<n>, gxmean_<n> for n in EXTRA, acc_1030 =
    accuracy(xe[:1030], xe[1030:]), acc_2049 = accuracy(xe, xd).  fp64 only: tail_grads, the share of the last TAIL_ROWS rows of
    [xg; xd] in every gradient."""
    dt = getattr(torch, dtype)
    x = inputs(c)
    ng, nd, npn = c.batches
    P = [torch.tensor(p, dtype=dt, requires_grad=True) for p in x['params']]
    kw = _kw(c)
    dg = og.critic_forward(P, _t(x['xg'], dt), _t(x['cg'], dt), **kw)[:, 0]
    dd = og.critic_forward(P, _t(x['xd'], dt), _t(x['cd'], dt), **kw)[:, 0]
    xp = _t(x['xp'], dt).clone().requires_grad_(True)
    dp = og.critic_forward(P, xp, _t(x['cp'], dt), **kw)[:, 0]
    g, = torch.autograd.grad(dp.sum(), xp, create_graph=True)
    pen_rows = (g.norm(2, dim=1) - 1) ** 2
    pen = pen_rows.mean()
    loss = dg.mean() - dd.mean() + LMD * pen
    grads = torch.autograd.grad(loss, P, retain_graph=True)
    res = dict(grads=[t.double().numpy() for t in grads],
               stats=np.array([float(t.detach()) for t in (dg.mean(), dd.mean(), pen, loss)], dtype='float64'),
               dvals=torch.cat([dg, dd]).detach().double().numpy(), pen_rows=pen_rows.detach().double().numpy(),
               fwd_p=dp.detach().double().numpy())
    if dtype == 'float64':
        up = torch.cat([torch.full((ng,), 1.0 / ng, dtype=dt), torch.full((nd,), -1.0 / nd, dtype=dt)])
        tail = (up * torch.cat([dg, dd]))[-TAIL_ROWS:].sum()
        res['tail_grads'] = [t.numpy() for t in torch.autograd.grad(tail, P)]
    P = [p.detach() for p in P]
    _, res['gx'], res['gx_mean'] = _forward_and_input_grad(c, P, x['xg'], x['cg'], dt)
    res['acc'] = res['stats'][0] - res['stats'][1]
    if has_extra(c):
        for n in EXTRA:
            res['fwd_%d' % n], res['gx_%d' % n], res['gxmean_%d' % n] = _forward_and_input_grad(
                c, P, x['xe'][:n], None if x['ce'] is None else x['ce'][:n], dt)
        full = res['fwd_%d' % EXTRA[1]]
        res['acc_1030'] = float(full[:1030].mean()) - float(full[1030:].mean())
        res['means_1030'] = (float(full[:1030].mean()), float(full[1030:].mean()))
        res['acc_2049'] = float(full.mean()) - float(res['stats'][1])
        res['means_2049'] = (float(full.mean()), float(res['stats'][1]))
        if dtype != 'float64':          # (the means of a float32 run are float32 means)
            f = torch.as_tensor(full, dtype=dt)
            a, b, m = float(f[:1030].mean()), float(f[1030:].mean()), float(f.mean())
            res['acc_1030'], res['acc_2049'] = a - b, m - float(res['stats'][1])
    return res


# ------------------------------------------------------------------ measures
# (each returns the largest error and the flat index of the element that has it)
def err_matrix(got, want):
    """|got - want|_ij / min(largest |want| of row i, largest |want| of column j)."""
    got, want = np.asarray(got, dtype='float64'), np.asarray(want, dtype='float64')
    assert got.shape == want.shape and want.ndim == 2, (got.shape, want.shape)
    scale = np.minimum(np.abs(want).max(axis=1, keepdims=True), np.abs(want).max(axis=0, keepdims=True))
    assert (scale > 0).all(), 'a row or a column of the oracle is all zero'
    ratio = np.nan_to_num(np.abs(got - want) / scale, nan=np.inf)
    return float(ratio.max()), int(ratio.argmax())


def err_max(got, want):
    """|got - want| relative to the tensor's largest element."""
    got, want = np.asarray(got, dtype='float64'), np.asarray(want, dtype='float64')
    assert got.shape == want.shape, (got.shape, want.shape)
    dev = np.nan_to_num(np.abs(got - want), nan=np.inf)
    return float(dev.max() / np.abs(want).max()), int(dev.argmax())


def err_rel(got, want):
    got, want = np.atleast_1d(np.asarray(got, dtype='float64')), np.atleast_1d(np.asarray(want, dtype='float64'))
    assert got.shape == want.shape and (want != 0).all()
    dev = np.nan_to_num(np.abs(got - want) / np.abs(want), nan=np.inf)
    return float(dev.max()), int(dev.argmax())


def is_matrix(c, i):
    """Parameter i (lasagne order) is a hidden layer's weight matrix; biases and the one-column W_out are vectors."""
    return i < 2 * len(c.layers) and i % 2 == 0


def split_flat(c, flat):
    out, off = [], 0
    for p in inputs(c)['params']:
        out.append(np.asarray(flat[off:off + p.size], dtype='float64').reshape(p.shape))
        off += p.size
    assert off == len(flat)
    return out


KINDS = ('W', 'vec', 'D', 'gx', 'stats', 'acc')


def errors(c, got, want=None):
    """{kind: {tensor: (error, flat index of the worst element)}} of a result `got` (keys as `oracle`'s; grads a list or a flat vector) against the fp64 oracle."""
    want = oracle(c) if want is None else want
    grads = got['grads'] if isinstance(got['grads'], (list, tuple)) else split_flat(c, got['grads'])
    e = {k: {} for k in KINDS}
    for i, (g, w) in enumerate(zip(grads, want['grads'])):
        layer = i // 2 + 1
        if is_matrix(c, i):
            e['W']['dW%d' % layer] = err_matrix(g, w)
        else:
            e['vec']['db%d' % layer if i < 2 * len(c.layers) else 'dw_out'] = err_max(np.ravel(g), np.ravel(w))
    e['D']['dvals'] = err_max(got['dvals'], want['dvals'])
    e['D']['fwd_p'] = err_max(got['fwd_p'], want['fwd_p'])
    e['gx']['gx'] = err_max(got['gx'], want['gx'])
    e['stats']['stats'] = err_rel(got['stats'], want['stats'])
    e['stats']['gx_mean'] = err_rel(got['gx_mean'], want['gx_mean'])
    e['acc']['acc'] = (float(abs(float(np.ravel(got['acc'])[0]) - want['acc']) / np.abs(want['stats'][:2]).max()), 0)
    if has_extra(c):
        for n in EXTRA:
            e['D']['fwd_%d' % n] = err_max(got['fwd_%d' % n], want['fwd_%d' % n])
            e['gx']['gx_%d' % n] = err_max(got['gx_%d' % n], want['gx_%d' % n])
            e['stats']['gxmean_%d' % n] = err_rel(got['gxmean_%d' % n], want['gxmean_%d' % n])
            e['acc']['acc_%d' % n] = (float(abs(float(np.ravel(got['acc_%d' % n])[0]) - want['acc_%d' % n]) / np.abs(want['means_%d' % n]).max()), 0)
    return e


def worst(e):
    """{kind: largest error of the kind}."""
    return {k: max(err for err, _ in v.values()) for k, v in e.items()}


@functools.lru_cache(maxsize=None)
def fp32_oracle_deviation(c):
    """{kind: deviation of the oracle run in float32 from the fp64 one}, in the measures above."""
    return worst(errors(c, oracle(c, 'float32')))


TOLERANCE_MULTIPLE = 4.0
TOLERANCE_CAP = 1e-3
SCALAR_KINDS = ('stats', 'acc')
UNIT_ROUNDOFF = 2.0 ** -24      # of float32: what storing a result in the device's format costs, whatever computed it


def tolerances(c):
    """{kind: 4 x the float32 oracle's deviation}.  Above TOLERANCE_CAP the case's inputs are at fault, not the bound.
    The deviation of a kind that is a handful of scalars (the accuracy: one to three numbers) is one draw of a rounding error
    and can come out at 1e-8 by luck, below what rounding the result to float32 costs; it counts as at least UNIT_ROUNDOFF
    (measured: that lifts the accuracy's figure in about a third of the cases -- from 1e-8 at the least -- and now and then the
    statistics')."""
    tol = {k: TOLERANCE_MULTIPLE * (max(v, UNIT_ROUNDOFF) if k in SCALAR_KINDS else v) for k, v in fp32_oracle_deviation(c).items()}
    assert all(0 < t <= TOLERANCE_CAP for t in tol.values()), (c.name, tol)
    return tol


# ------------------------------------------------------------------ the conditions of a case
def active_fractions(c):
    """[per layer: (3, width) -- the fraction of the rows of xg, xd, xp on which each unit is active]."""
    x = inputs(c)
    per_batch = [pre_activations(c, x['params'], x['x' + k], x['c' + k])[0] for k in 'gdp']
    return [np.stack([(pres[l] > 0).mean(axis=0) for pres in per_batch]) for l in range(len(c.layers))]


def kink_distance(c):
    """Smallest |pre-activation| / (layer rms) over every row of every batch (the extra rows included) and every layer."""
    x = inputs(c)
    keys = [('xg', 'cg'), ('xd', 'cd'), ('xp', 'cp')] + ([('xe', 'ce')] if has_extra(c) else [])
    return min(float(np.abs(pre).min() / r) for kx, kc in keys
               for pre, r in zip(pre_activations(c, x['params'], x[kx], x[kc])[0], x['rms']))


def vector_conditions(c):
    """[(tensor, smaller end / largest, fraction of the elements below 100 x the tolerance)] of every bias and w_out gradient."""
    tol, o, out = tolerances(c)['vec'], oracle(c), []
    for i, g in enumerate(o['grads']):
        if not is_matrix(c, i):
            v = np.abs(np.ravel(g)) / np.abs(g).max()
            out.append(('param%d' % i, float(min(v[0], v[-1])), float((v < 100 * tol).mean())))
    return out


def conditions(c):
    """Asserts the three conditions of the module docstring; returns the figures."""
    x = inputs(c)
    for key in ('xg', 'xd', 'xp', 'cg', 'cd', 'cp', 'xe', 'ce'):
        if x.get(key) is not None:
            assert np.array_equal(x[key], _f32(x[key])), key
    assert all(np.array_equal(p, _f32(p)) for p in x['params'])
    fr = active_fractions(c)
    if min(c.batches) >= 20:
        assert all(0.1 <= f.min() and f.max() <= 0.9 for f in fr), [(f.min(), f.max()) for f in fr]
    else:           # a unit may be fully on or off on one batch of 5 ... 7 rows: alive and not saturated over the three together
        n = np.asarray(c.batches, dtype='float64')[:, None]
        assert all(((f * n).sum(axis=0) >= 1).all() and ((f * n).sum(axis=0) <= n.sum() - 1).all() for f in fr)
    kink = kink_distance(c)
    assert kink >= MARGIN, kink
    vec = vector_conditions(c)
    for name, end, small in vec:
        assert end >= 0.05, (c.name, name, end)
        assert small <= 0.01, (c.name, name, small)
    return dict(active=(min(f.min() for f in fr), max(f.max() for f in fr)), kink=kink, rounds=x['rounds'],
                ends=min(v[1] for v in vec), small=max(v[2] for v in vec))

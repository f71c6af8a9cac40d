"""ORACLE -- TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

The cases, inputs, fp64 results and error measures that hold the BPTT backward of the fixed-time generator (adjoint sweep,
dL/dW, dL/d ext, the per-draw chain to J, D, S) to `gan_torch.euler_ssn_adjoint` ELEMENT BY ELEMENT
(tests/test_adjoint_elementwise_gpu.py), and that tests/test_adjoint_oracle.py checks without a GPU.

Why its own inputs: with the stimulus of the other generator tests (centred on the ring, sparse G) the neurons at the ends of
the ring are nearly silent, and they are the tail rows and columns of every tile grid -- the smallest row maximum of dL/dW is
1e-13 ... 3e-16 of the draw's largest element, so neither "relative to the largest element" nor the twelve sums dL/d(J, D, S)
see a tail row that is dropped (tests/test_adjoint_oracle.py records that).  Here every neuron is driven (ext uniform per
draw, stimulus and neuron, dense G), with asym_tanh the last draw is driven into the saturating branch, and every error is
measured on a scale of its own element or block.
"""
import collections

import numpy as np
import torch

from . import gan_torch as og
from . import ssn_numpy as on

GEN = dict(k=0.01, n=2.2, tau_E=10., tau_I=1., dt=0.1)
B, T, THETA = 3, 24, 1.0            # an odd number of draws: the two-draw kernel is left with a lone one
# window -> (skip_steps, dynamics_cost, rate_cost); 'last' is one step wide, where the dynamics penalty has no terms
WINDOWS = {'mid': (14, 1.0, 0.01), 'from0': (0, 1.0, 0.01), 'last': (T - 1, 0.0, 0.01)}

Case = collections.namedtuple('Case', 'dtype io_type M NB window')

# fp32: 2N = 66 partly fills the first tile grid (2N <= 104); 104 / 106 top of the first grid and first size of the second
# (<= 152); 152 / 154 the same for the third (<= 208); 198 the half-real tail tile of the two-draw form; 202 an odd N; 208
# the top; 210 the first streaming size; 258 streaming with M > 224 (dL/dW in its plain form only).  Stimuli: 1 and 3 (tile /
# streaming kernels only), 4, 5 (the second group of four holds one), 8, 9 (three groups); each at a partly filled 2N.
_SIZES32 = [(66, (1, 4, 9)), (104, (5, 8)), (106, (3, 5)), (152, (4, 8)), (154, (1, 8)), (198, (4, 9)), (202, (3, 5, 8)),
            (208, (4, 9)), (210, (1, 4)), (258, (3, 8))]
_SIZES64 = [(20, (1, 5)), (104, (4, 9)), (106, (3, 8))]      # 104: top of the resident fp64 kernels, 106: first streaming size
_WINDOW_SIZES = [(66, 5), (106, 8), (202, 4)]                # one size per tile grid for the two other windows

CASES = ([Case('float32', io, M, NB, 'mid') for M, nbs in _SIZES32 for NB in nbs for io in ('asym_tanh', 'asym_power')]
         + [Case('float32', io, M, NB, w) for M, NB in _WINDOW_SIZES for w in ('from0', 'last') for io in ('asym_tanh', 'asym_power')]
         + [Case('float64', io, M, NB, 'mid') for M, nbs in _SIZES64 for NB in nbs for io in ('asym_tanh', 'asym_power')]
         + [Case('float64', io, 20, 4, w) for w in ('from0', 'last') for io in ('asym_tanh', 'asym_power')])


def case_id(c):
    return '%s-%s-M%d-NB%d-%s' % (c.dtype, c.io_type, c.M, c.NB, c.window)


def tile_grid(c):
    """The size class of the resident kernels a case falls in (0, 1, 2: 2N <= 104, 152, 208 in fp32; fp64 has one, <= 104)
    or 'stream'."""
    if c.dtype == 'float64':
        return 0 if c.M <= 104 else 'stream'
    return 0 if c.M <= 104 else 1 if c.M <= 152 else 2 if c.M <= 208 else 'stream'


def _rounded(a, dtype):
    return np.asarray(a, dtype='float64').astype(dtype).astype('float64')


_INPUTS, _ORACLE = {}, {}
# Seed offsets of the cases whose first draw misses one of the conditions tests/test_adjoint_oracle.py asserts for every case
# (a row of dL/dW that cancels to below 0.2 of its scale, or more than 60 % of the saturated draw above v0).
RESEED = {'float32-asym_tanh-M66-NB1-mid': 1, 'float64-asym_tanh-M20-NB1-mid': 1, 'float64-asym_tanh-M20-NB5-mid': 3,
          'float64-asym_tanh-M20-NB4-last': 1}


def inputs(c):
    """fp64 arrays that are exactly representable in the case's dtype: z, W = make_W(z; new_JDS) (B, M, M), ext, G (B, NB, M)."""
    if c in _INPUTS:
        return _INPUTS[c]
    _INPUTS.clear()                         # (one case at a time: the tests walk the cases in order)
    rs = np.random.RandomState(100000 * RESEED.get(case_id(c), 0) + 1000 * c.M + 10 * c.NB + list(WINDOWS).index(c.window))
    N = c.M // 2
    jds = on.new_JDS()
    z = _rounded(rs.rand(B, c.M, c.M), c.dtype)
    W = _rounded(og.make_W(og.t64(z), *(og.t64(jds[k]) for k in 'JDS'), N).numpy(), c.dtype)
    ext = rs.uniform(2.0, 20.0, (B, c.NB, c.M))
    if c.io_type == 'asym_tanh':            # the last draw runs into the saturating branch of f (rates of a few hundred)
        ext[B - 1] = rs.uniform(60.0, 160.0, (c.NB, c.M))
    G = rs.randn(B, c.NB, c.M)
    res = _INPUTS[c] = dict(jds=jds, z=z, W=W, ext=_rounded(ext, c.dtype), G=_rounded(G, c.dtype))
    return res


def gen_kwargs(c):
    skip, dyn_cost, rate_cost = WINDOWS[c.window]
    return dict(GEN, io_type=c.io_type, seqlen=T, skip_steps=skip, rate_penalty_threshold=THETA), dyn_cost, rate_cost


def oracle(c, dtype='float64'):
    """`euler_ssn_adjoint` of a case in the KERNELS' layout, numpy fp64 whatever `dtype` it ran in (cached):
    traj, df, u, delta (B, NB, T, M); dsh = the shifted stream (dsh[:, :, t] = delta[:, :, t + 1], last slot zero);
    gW (B, M, M), scale = sum_k |dsh_ki| |traj_kj| (B, M, M); g_ext, time_avg (B, NB, M); parts (B, 4, 3) = this draw's share
    of dL/dJ_pq, dL/dD_pq, dL/dS_pq through make_W (fp64 only).  The cache holds the last case per dtype: the tests walk the
    cases in order, kernel by kernel."""
    if _ORACLE.get(dtype, (None,))[0] == c:
        return _ORACLE[dtype][1]
    x = inputs(c)
    gen, dyn_cost, rate_cost = gen_kwargs(c)
    o = og.euler_ssn_adjoint(og.t64(x['W']), og.t64(x['ext']), og.t64(x['G']), dyn_cost, rate_cost, dtype=getattr(torch, dtype), **gen)
    res = {k: o[k].double().permute(0, 2, 1, 3).contiguous().numpy() for k in ('traj', 'df', 'u', 'delta')}
    res.update({k: o[k].double().numpy() for k in ('gW', 'g_ext', 'time_avg')})
    res['dsh'] = shifted(res['delta'])
    res['scale'] = weight_grad_of(np.abs(res['dsh']), np.abs(res['traj']))
    if dtype == 'float64':
        J, D, S = (og.t64(x['jds'][k]).clone().requires_grad_(True) for k in 'JDS')
        Wz = og.make_W(og.t64(x['z']), J, D, S, c.M // 2)
        parts = [torch.stack(torch.autograd.grad((o['gW'][b] * Wz[b]).sum(), [J, D, S], retain_graph=True), dim=-1) for b in range(B)]
        res['parts'] = torch.stack(parts).reshape(B, 4, 3).numpy()
    _ORACLE[dtype] = (c, res)
    return res


def shifted(delta):
    """The stream the sweeps leave: slot t holds delta_{t+1}, the last slot zero (include/ssnode_mi355x.h, section 3)."""
    out = np.zeros_like(delta)
    out[:, :, :-1] = delta[:, :, 1:]
    return out


def weight_grad_of(dsh, traj):
    """dL/dW[b] = dsh[b].reshape(NB T, M)^T @ traj[b].reshape(NB T, M) in fp64."""
    nb, K, M = dsh.shape[0], dsh.shape[1] * dsh.shape[2], dsh.shape[3]
    return np.einsum('bki,bkj->bij', dsh.reshape(nb, K, M), traj.reshape(nb, K, M))


# ------------------------------------------------------------------ the three measures (each a scale per element or block)
# Every measure returns one figure per draw: the draw that asym_tanh drives into saturation is worse conditioned than the
# others (the fp32 oracle itself deviates several times as much there), so it has tolerances of its own.
def saturated_draws(c):
    """(B,) bool: the draws whose inputs reach the saturating branch of f (the last one of the asym_tanh cases)."""
    return np.arange(B) == (B - 1 if c.io_type == 'asym_tanh' else -1)


def _per_block(err, want):
    """max |err| / max |want|, both maxima over the neurons of one population: arrays (B, ..., M) -> the largest ratio per draw."""
    sh = want.shape[:-1] + (2, want.shape[-1] // 2)
    top = np.abs(want).reshape(sh).max(axis=-1)
    assert (top > 0).all(), 'a block of the oracle is all zero'
    return (np.abs(err).reshape(sh).max(axis=-1) / top).reshape(want.shape[0], -1).max(axis=1)


def err_delta(got_dsh, o):
    """The shifted stream against the oracle's: |got - want| / max |want| over the (draw, stimulus, step, population) block.
    (The last slot is zero on both sides; the caller asserts that exactly.)"""
    return _per_block(got_dsh[:, :, :-1] - o['dsh'][:, :, :-1], o['dsh'][:, :, :-1])


def err_g_ext(got, o):
    """dL/d ext against the oracle's, per (draw, stimulus, population) block."""
    return _per_block(got - o['g_ext'], o['g_ext'])


def err_df(got, o, plain_from, rtol, atol):
    """f'(u) against the oracle's, two figures per draw.  (i) |got - want| / max |want| over the (draw, stimulus, step,
    population) block, every element.  (ii) The plain comparison |got - want| <= atol + rtol |want| on the elements that reach
    `plain_from[b]` of their block's maximum, as rtol times the largest ratio of the two sides: it holds where (ii) <= rtol."""
    want = o['df']
    sh = want.shape[:-1] + (2, want.shape[-1] // 2)
    top = np.broadcast_to(want.reshape(sh).max(axis=-1, keepdims=True), sh).reshape(want.shape)
    err = np.abs(got - want)
    held = want >= np.asarray(plain_from).reshape(-1, 1, 1, 1) * top
    plain = rtol * np.where(held, err / (atol + rtol * want), 0.0).reshape(want.shape[0], -1).max(axis=1)
    return _per_block(got - want, want), plain


def err_weight_grad(got, o, want=None, scale=None):
    """|got - want|_ij / scale_ij with scale_ij = sum_k |dsh_ki| |traj_kj|: what every dot product is measured against."""
    want, scale = o['gW'] if want is None else want, o['scale'] if scale is None else scale
    assert (scale > 0).all()
    return (np.abs(got - want) / scale).reshape(got.shape[0], -1).max(axis=1)

"""ORACLE -- TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Nothing under tc_gan_amd/ imports this module.

The cases, inputs, fp64 restatements, error measures and tolerances that hold the six segmented kernels of an ensemble step
(tc_gan_amd/csrc/ssn_ensemble.hip) ONE BY ONE (tests/test_ens_step_gpu.py), and that tests/test_ens_step_cases.py checks without
a GPU:

  moments      ssn_ens_moments_f32                  ens_moment_sums_kernel, ens_moment_loss_grad_kernel
  jds_grad     ssn_ens_jds_grad_f32                 ens_jds_grad_kernel
  gen_grads    ssn_ens_gen_grads_f32 / _l0_f32      ens_gen_grads_kernel
  apply        ssn_ens_apply_f32                    ens_apply_kernel
  stimulus     ssn_ens_stimulus_hetero_f32          ens_stimulus_hetero_kernel

Every case has K = 3 members whose values differ (one K = 1 case per kernel), at the smallest shapes that enter each strided
loop a second time: B, B NB M, N N and D on both sides of the 256 threads of a workgroup, K P above the 64 x 256 threads of the
optimizer's capped grid, K B NB 2N above the 2048 x 256 of the stimulus's.  The restatements reuse oracle/gen_step_cases.py
(`tree256`, `strided_partials`, `jds_grad`, `stimulus`, `hetero_gain`, `_lattice`); the one new primitive is the sum of ONE
workgroup, `block_sum` = tree256(strided_partials(x, 1)): what ens_block_sum and both moment kernels compute.

Measures and tolerances (u = 2^-24, e = 2^-53; TOLERANCE_MULTIPLE, TOLERANCE_CAP, SENSITIVITY of oracle/ff_cases.py).  Every
check is |got - want| <= allowed per element, or equality where the order of the fp64 operations is pinned and a contraction
into an fma cannot move the result.

  moments   sums: bit for bit `moment_sums_in_order` (the square of a float32 number is exact in fp64).  m, s, gx against fp64
      from math.fsum sums, with a first-order error propagation in which every rounding of the kernel AND of the oracle is
      counted once (with or without a contraction of s2 / B - m m and of c0 + c1 (x - m), a contraction only drops one):
          d_m = e (h sum |x| / B + 3 |m|),  h = ceil(B / 256) + 8 the additions one element passes through
          d_q = e (h sum x^2 / B + 3 q),    q = s2 / B
          d_s = d_q + 2 |m| d_m + d_m^2 + 2 e m^2 + 2 e |s|               (the cancellation: ~ e m^2 / s relative)
          d_em = d_m + 2 e |em|, d_es = d_s + 2 e |es|, d_c0 = |w0| d_em / (B D) + 4 e |c0|, d_c1 = 2 |w1| d_es / (B D) + 4 e |c1|
          d_t = d_m + 2 e |t|, t = x - m;  d_g = d_c0 + |c1| d_t + |t| d_c1 + d_c1 d_t + 2 e |c1 t| + 2 e |g|
      allowed(m) = d_m, allowed(s) = d_s, allowed(gx) = u |g| + d_g + 2^-149 (one float32 rounding).  The figure held under
      TOLERANCE_CAP is allowed(gx) / (|c0| + |c1 t|).
  jds_grad   gen_step_cases' measure and tolerance per member: |delta| / sum |terms|, 4 x the float32 restatement's deviation
      plus the derived term of `jds_grad(with_bound=True)`; bit-equal to the single-run kernel per member.
  gen_grads   on lattice inputs (every product exact, a + b of two exact products rounds once whether or not one of them is
      fused) bit for bit `gen_grads_in_order`; the penalties bit for bit on any input (sums of converted float32 numbers
      in a pinned order, one product).  On free inputs: grads within one float32 ulp of the math.fsum value plus
      (n + 1) e sum |terms|; L0 within (h(D) + 14) e L0 (all terms >= 0: em, es one rounding each and squared 4 e, four
      products 4 e, the inner addition 2 e, the division 2 e, 2 e spare, in kernel and oracle together, and the summation);
      loss within 8 e (|L0| + |c_dyn dyn| + |c_rate rate|) of the value formed from the record's own L0 and ROUNDED penalties.
  apply   gen_step_cases' rtol 2e-5, atol 2e-6 against oracle/gan_torch's fp64 rules with the regularisation terms of
      optimizer_kernel and critic.Updater around them (`apply_step_reg`); a clipped element equals its bound; record words
      are bits.
  stimulus   gen_step_cases' allowed = rel |ext| + 2^-149 with the gain 1 + fl(v z) of the draw's member; bit-equal to the
      single-run kernel per member (the check that fails if the product is contracted).

Nothing is fitted to a kernel; a relative tolerance above TOLERANCE_CAP means the inputs are at fault.
"""
import collections
import math

import numpy as np

from . import ff_cases as _fc
from . import gen_step_cases as gc
from .gen_step_cases import _cached, _f32, _lattice, hetero_gain, onehot_places, strided_partials, tree256

U = _fc.U
E = 2.0 ** -53
TOLERANCE_MULTIPLE = _fc.TOLERANCE_MULTIPLE
TOLERANCE_CAP = _fc.TOLERANCE_CAP
SENSITIVITY = _fc.SENSITIVITY
APPLY_MARGIN = gc.APPLY_MARGIN
RULES = gc.RULES
BLOCK = 256
APPLY_SWEEP = 64 * 256                # threads of one sweep of ens_apply_kernel's capped grid
STIM_SWEEP = 2048 * 256               # ... of ens_stimulus_hetero_kernel's

ENTRIES = ('ssn_ens_moments_f32', 'ssn_ens_jds_grad_f32', 'ssn_ens_gen_grads_f32', 'ssn_ens_gen_grads_l0_f32', 'ssn_ens_apply_f32',
           'ssn_ens_stimulus_hetero_f32')


def block_sum(x):
    """The sum ONE workgroup of 256 threads forms: thread t adds x[t], x[t + 256], ... in that order, then the 128 ... 1 tree."""
    return float(tree256(strided_partials(x, 1))[0])


def depth(n):
    """The additions one of n elements passes through in `block_sum`."""
    return -(-n // BLOCK) + 8


def _rows(K, B):
    return [slice(k * B, (k + 1) * B) for k in range(K)]


# ------------------------------------------------------------------ moments
Mom = collections.namedtuple('Mom', 'K B D kind')
MOM_B, MOM_D = (1, 255, 256, 257, 513), (1, 7, 24)
MOM_CASES = [Mom(3, B, D, 'free') for B in MOM_B for D in MOM_D] + [Mom(3, 257, 7, 'offset'), Mom(1, 257, 7, 'free')]


def mom_inputs(c):
    """x (K B, D) float32, data moments and weights (K, 2, D).  'offset': mean 100, spread 0.01 -- s2 / B - m m cancels eight
    digits.  The data moments keep em and es away from 0 (at least a fifth of the spread, about half of s)."""
    def make():
        rs = np.random.RandomState(7000 + 31 * c.B + c.D + 1000 * c.K + (c.kind == 'offset'))
        member = np.repeat(np.arange(c.K), c.B)[:, None]
        if c.kind == 'offset':
            x = 100.0 + 0.01 * (1 + member) * rs.randn(c.K * c.B, c.D)
        else:
            x = rs.randn(c.K * c.B, c.D) * 10.0 ** rs.uniform(-1, 1, (1, c.D)) + rs.uniform(-2, 2, (c.K, 1))[member[:, 0]]
        x = _f32(x)
        xm = x.reshape(c.K, c.B, c.D)
        m, s = xm.mean(axis=1), xm.var(axis=1)
        dm0 = m + (np.sqrt(s) + 0.01) * rs.uniform(0.2, 1.0, m.shape) * rs.choice([-1.0, 1.0], m.shape)
        dm1 = s * rs.uniform(0.3, 0.7, s.shape) + 1e-5
        return dict(x=x, dm=np.stack([dm0, dm1], axis=1), w=rs.uniform(0.5, 2.0, (c.K, 2, c.D)))
    return _cached(('em-in', c), make)


def moment_sums_in_order(x, K, B, D, rows=None):
    """sums[k][2][D] of ens_moment_sums_kernel; rows: only the first `rows` rows of a member are added (a defect)."""
    xm = np.asarray(x, dtype='float64').reshape(K, B, D)[:, :rows]
    out = np.zeros((K, 2, D))
    for k in range(K):
        for d in range(D):
            col = xm[k, :, d]
            out[k, 0, d], out[k, 1, d] = block_sum(col), block_sum(col * col)
    return out


def moment_loss(x, dm, w):
    """L0 of one member in plain fp64: mean over the 2 D moments of w (moment - data moment)^2."""
    m = x.mean(axis=0)
    s = (x * x).mean(axis=0) - m * m
    return float((w[0] * (m - dm[0]) ** 2 + w[1] * (s - dm[1]) ** 2).sum() / (2.0 * x.shape[1]))


def mom_oracle(c, rows=None):
    """dict(m, s (K, D), gx (K B, D), their allowed errors, scale of gx): the docstring's propagation from math.fsum sums."""
    x = mom_inputs(c)
    K, B, D = c.K, c.B, c.D
    xm = x['x'].reshape(K, B, D)
    used = xm[:, :rows]
    s1 = np.array([[math.fsum(used[k, :, d]) for d in range(D)] for k in range(K)])
    s2 = np.array([[math.fsum(used[k, :, d] * used[k, :, d]) for d in range(D)] for k in range(K)])
    a1 = np.abs(used).sum(axis=1)
    Bg, h = float(B), depth(B)
    m, q = s1 / Bg, s2 / Bg
    s = q - m * m
    d_m = E * (h * a1 / Bg + 3 * np.abs(m))
    d_q = E * (h * q + 3 * q)
    d_s = d_q + 2 * np.abs(m) * d_m + d_m * d_m + 2 * E * m * m + 2 * E * np.abs(s)
    em, es = m - x['dm'][:, 0], s - x['dm'][:, 1]
    w0, w1 = x['w'][:, 0], x['w'][:, 1]
    c0, c1 = w0 * em / (Bg * D), 2.0 * w1 * es / (Bg * D)
    d_c0 = np.abs(w0) * (d_m + 2 * E * np.abs(em)) / (Bg * D) + 4 * E * np.abs(c0)
    d_c1 = 2 * np.abs(w1) * (d_s + 2 * E * np.abs(es)) / (Bg * D) + 4 * E * np.abs(c1)
    t = xm - m[:, None, :]
    d_t = d_m[:, None, :] + 2 * E * np.abs(t)
    g = c0[:, None, :] + c1[:, None, :] * t
    d_g = (d_c0[:, None, :] + np.abs(c1)[:, None, :] * d_t + np.abs(t) * d_c1[:, None, :] + d_c1[:, None, :] * d_t
           + 2 * E * np.abs(c1[:, None, :] * t) + 2 * E * np.abs(g))
    scale = np.abs(c0)[:, None, :] + np.abs(c1[:, None, :] * t)
    return dict(m=m, s=s, gx=g.reshape(K * B, D), allowed_m=d_m, allowed_s=d_s,
                allowed_gx=(U * np.abs(g) + d_g + 2.0 ** -149).reshape(K * B, D), scale_gx=scale.reshape(K * B, D))


# ------------------------------------------------------------------ jds_grad
EnsJds = collections.namedtuple('EnsJds', 'K N B gw')
JDS_N, JDS_B = (1, 16, 17, 52), (1, 3)
JDS_CASES = [EnsJds(3, N, B, gw) for N in JDS_N for B in JDS_B for gw in ('free', 'onehot')] + [EnsJds(1, 17, 3, 'free')]


def member_jds(k):
    """J, D, S (2, 2) float32 numbers of member k: four distinct entries each, distinct across members."""
    J, D, S = gc.jds_set('four')
    return _f32(J * (1 + 0.25 * k)), _f32(D * (1 - 0.125 * k)), _f32(S * (1 + 0.375 * k))


def jds16(J, D, S):
    """p16 of one member: J[4], D[4], 1 / (2 S^2)[4], 1 / S^3[4] in float32, each S term rounded as launch_jds_grad rounds it."""
    s = np.asarray(S, dtype='float32').reshape(4)
    one, two = np.float32(1), np.float32(2)
    return np.concatenate([np.asarray(J, dtype='float32').reshape(4), np.asarray(D, dtype='float32').reshape(4),
                           one / ((two * s) * s), one / ((s * s) * s)]).astype('float32')


def ens_jds_inputs(c):
    """z (K B, M, M) and the list of gW: one free draw, or one gW per place of `onehot_places` with its one element in draw
    (place index) % (K B) -- over the twelve places every member is fed."""
    def make():
        rs = np.random.RandomState(8000 + 13 * c.N + c.B + 100 * c.K)
        M, nb = 2 * c.N, c.K * c.B
        z = _f32(rs.rand(nb, M, M))
        if c.gw == 'free':
            gWs = [_f32(rs.randn(nb, M, M))]
        else:
            gWs = []
            for k, (_, p, q, i, j) in enumerate(onehot_places(c.N)):
                g = np.zeros((nb, M, M))
                g[k % nb, p * c.N + i, q * c.N + j] = rs.uniform(0.5, 2.0) * (-1) ** k
                gWs.append(_f32(g))
        return dict(z=z, gW=gWs, jds=[member_jds(k) for k in range(c.K)])
    return _cached(('ej-in', c), make)


def ens_jds_oracle(c, params=None):
    """One dict(want, allowed, tol, scale) (K B, 4, 3) per gW: gen_step_cases.jds_oracle's arithmetic with the parameters of the
    draw's member; `params` replaces the members' own (the defects)."""
    x = ens_jds_inputs(c)
    params = x['jds'] if params is None else params
    tiny = 2.0 ** -126
    res = []
    for gW in x['gW']:
        per = []
        for k, sl in enumerate(_rows(c.K, c.B)):
            J, D, S = params[k]
            want, scale, derived, xarg, coef = gc.jds_grad(gW[sl], x['z'][sl], J, D, S, c.N, with_bound=True)
            sub = np.broadcast_to(np.exp(-xarg) < tiny, coef[0].shape)
            floor = np.stack([(np.where(sub, t, 0.0) * tiny).sum(axis=(2, 4)).reshape(-1, 4) for t in coef], axis=-1)
            o32 = gc.jds_grad(gW[sl], x['z'][sl], J, D, S, c.N, 'float32')
            with np.errstate(divide='ignore', invalid='ignore'):
                dev = np.nan_to_num(np.maximum(np.abs(o32 - want) - floor, 0.0) / scale)
            rel = TOLERANCE_MULTIPLE * dev.max(axis=(0, 1))[None, None, :] + derived
            per.append((want, rel * scale + floor, rel, scale))
        want, allowed, rel, scale = (np.concatenate([p[i] for p in per]) for i in range(4))
        res.append(dict(want=want, allowed=allowed, tol=float(rel.max()), scale=scale))
    return res


# ------------------------------------------------------------------ gen_grads
EnsGG = collections.namedtuple('EnsGG', 'entry K nv B NB M D')
GG_SHAPES = ((1, 3, 10), (2, 8, 16), (3, 5, 18), (257, 1, 6))       # B NB M = 30; 256 exactly; 270 (M does not divide 256); 1542
GG_D = (1, 24, 257)


def _gg_cases():
    cases = []
    for nv in (0, 1, 2):
        for i, (B, NB, M) in enumerate(GG_SHAPES):
            cases.append(EnsGG(ENTRIES[2], 3, nv, B, NB, M, GG_D[(i + nv) % 3]))
            cases.append(EnsGG(ENTRIES[3], 3, nv, B, NB, M, 0))
    return cases + [EnsGG(ENTRIES[2], 1, 2, 3, 5, 18, 24), EnsGG(ENTRIES[3], 1, 1, 3, 5, 18, 0)]


GG_CASES = _gg_cases()


def gg_inputs(c, kind):
    """kind 'exact': every product the kernel forms is exact -- g_ext, ext_base with 12 significant bits and zin = +-1; em, es
    multiples of 2^-8 below 8 (12 bits) and weights with 8 bits (32 in w em em), costs with few bits against the 24 of a rounded
    penalty -- and exponents spread so that the order of the additions counts.  'free': plain draws.  Costs, moments, weights
    and l0 differ between members."""
    def make():
        rs = np.random.RandomState(9000 + 17 * c.B + c.M + 3 * c.nv + 7 * c.D + 100 * c.K + (kind == 'free') * 50)
        K, B, NB, M, D = c.K, c.B, c.NB, c.M, c.D
        sh = (K * B, NB, M)
        member = np.repeat(np.arange(K), B)
        x = dict(scale_dyn=1.0 / (B * NB * M), scale_rate=1.0 / (B * NB * M + 3))
        x['dyn'] = _f32(rs.rand(*sh) * (1 + member)[:, None, None])
        x['rate'] = _f32(rs.rand(*sh) * 10.0 ** rs.uniform(-3, 3, sh))
        if kind == 'exact':
            x['parts'] = _lattice(rs, (K * B, 4, 3), 20, 40)
            x['costs'] = np.array([[(3.0 + k) / 4, (5.0 + 2 * k) / 8] for k in range(K)])
            if c.nv:
                x['g_ext'], x['ext_base'] = _lattice(rs, sh, 12, 15), _lattice(rs, sh, 12, 5)
                x['zin'] = rs.choice([-1.0, 1.0], (K * B, M))
            if D:
                x['dm'] = rs.randint(-2 ** 12, 2 ** 12, (K, 2, D)) / 64.0
                x['mom'] = (x['dm'] + rs.randint(-2 ** 11, 2 ** 11, (K, 2, D)) / 256.0).reshape(K, 2 * D)
                x['w'] = np.abs(_lattice(rs, (K, 2, D), 8, 10))
            else:
                x['l0'] = _lattice(rs, (K,), 20, 5)
        else:
            x['parts'] = rs.randn(K * B, 4, 3) * 10.0 ** rs.uniform(-2, 2, (K * B, 4, 3))
            x['costs'] = rs.uniform(0.2, 2.0, (K, 2))
            if c.nv:
                x['g_ext'], x['ext_base'], x['zin'] = _f32(rs.randn(*sh)), _f32(rs.uniform(0, 20, sh)), _f32(rs.uniform(-1, 1, (K * B, M)))
            if D:
                x['dm'], x['mom'], x['w'] = rs.rand(K, 2, D), rs.rand(K, 2 * D) + np.arange(K)[:, None], rs.uniform(0.5, 2.0, (K, 2, D))
            else:
                x['l0'] = rs.rand(K) + np.arange(K)
        return x
    return _cached(('eg-in', c, kind), make)


def _l0_terms(x, k, D):
    em, es = x['mom'][k, :D] - x['dm'][k, 0], x['mom'][k, D:] - x['dm'][k, 1]
    return x['w'][k, 0] * em * em + x['w'][k, 1] * es * es


def gen_grads_in_order(c, x, rows=None):
    """dict(grads (K, nv + 12) float32, L0, dyn, rate (the float32 roundings, as doubles), loss (K,)) of ens_gen_grads_kernel in
    its order, member by member; rows: only the first `rows` elements / draws of a member enter its strided sums (a defect)."""
    K, B, NB, M, D, nv = c.K, c.B, c.NB, c.M, c.D, c.nv
    P = nv + 12
    out = dict(grads=np.zeros((K, P), dtype='float32'), L0=np.zeros(K), dyn=np.zeros(K), rate=np.zeros(K), loss=np.zeros(K))
    for k, sl in enumerate(_rows(K, B)):
        L0 = float(x['l0'][k]) if D == 0 else block_sum(_l0_terms(x, k, D)[:rows]) / (2.0 * D)
        fd = float(np.float32(block_sum(x['dyn'][sl].reshape(-1)[:rows]) * x['scale_dyn']))
        fr = float(np.float32(block_sum(x['rate'][sl].reshape(-1)[:rows]) * x['scale_rate']))
        if nv:
            t = (x['g_ext'][sl] * x['ext_base'][sl] * x['zin'][sl][:, None, :]).reshape(-1)
            pop_i = (np.arange(t.size) % M) >= M // 2
            tE, tI = block_sum(np.where(pop_i, 0.0, t)[:rows]), block_sum(np.where(pop_i, t, 0.0)[:rows])
            if nv == 1:
                out['grads'][k, 0] = np.float32(tE + tI)
            else:
                out['grads'][k, :2] = np.float32(tE), np.float32(tI)
        parts = x['parts'][sl].reshape(B, 12)[:rows]
        for col in range(12):
            out['grads'][k, nv + (col % 3) * 4 + col // 3] = np.float32(block_sum(parts[:, col]))
        out['L0'][k], out['dyn'][k], out['rate'][k] = L0, fd, fr
        out['loss'][k] = L0 + x['costs'][k, 0] * fd + x['costs'][k, 1] * fr
    return out


def gen_grads_exact(c, x):
    """The math.fsum values and the docstring's allowances: grads (K, P), L0, dyn, rate (K,) each as (want, allowed)."""
    K, B, M, D, nv = c.K, c.B, c.M, c.D, c.nv
    P = nv + 12
    want, allowed = np.zeros((K, P)), np.zeros((K, P))
    o = dict(L0=np.zeros(K), L0_allowed=np.zeros(K), dyn=np.zeros(K), rate=np.zeros(K))

    def put(k, i, terms):
        terms = np.asarray(terms, dtype='float64').reshape(-1)
        want[k, i] += math.fsum(terms)
        allowed[k, i] += (terms.size + 1) * E * math.fsum(np.abs(terms))
    for k, sl in enumerate(_rows(K, B)):
        if nv:
            t = x['g_ext'][sl] * x['ext_base'][sl] * x['zin'][sl][:, None, :]
            for pop in range(2):
                put(k, 0 if nv == 1 else pop, t[..., pop * (M // 2):(pop + 1) * (M // 2)])
        for q in range(4):
            for tt in range(3):
                put(k, nv + tt * 4 + q, x['parts'][sl][:, q, tt])
        if D:
            o['L0'][k] = math.fsum(_l0_terms(x, k, D)) / (2.0 * D)
            o['L0_allowed'][k] = (depth(D) + 14) * E * o['L0'][k]
        else:
            o['L0'][k] = x['l0'][k]
        o['dyn'][k] = math.fsum(x['dyn'][sl].reshape(-1)) * x['scale_dyn']
        o['rate'][k] = math.fsum(x['rate'][sl].reshape(-1)) * x['scale_rate']
    allowed += np.spacing(np.abs(want).astype('float32')).astype('float64')
    o.update(grads=want, grads_allowed=allowed)
    return o


def loss_allowed(L0, costs, fd, fr):
    return 8 * E * (np.abs(L0) + np.abs(costs[:, 0] * fd) + np.abs(costs[:, 1] * fr))


# ------------------------------------------------------------------ apply
EnsApply = collections.namedtuple('EnsApply', 'K P rule')
APPLY_CASES = [EnsApply(K, P, rule) for rule in RULES for P in (12, 13, 14) for K in (1, 3)] + [EnsApply(1300, 13, 'adam')]
APPLY_HYPER = gc.APPLY_HYPER
REG_NAMES = ('l2_penalty', 'l1_penalty', 'l2_decay', 'l1_decay')


def apply_hyper(K):
    """(K, 5) float32 numbers by formula: lr (distinct for every member), l2_penalty, l1_penalty, l2_decay, l1_decay (nonzero)."""
    k = np.arange(K)
    return _f32(np.stack([0.02 + 0.0007 * (k % 97) + 1e-6 * k, 0.05 * (1 + k % 3), 0.03 * (1 + k % 4), 0.3 * (1 + k % 2),
                          0.1 * (1 + k % 5)], axis=1))


def adam_a_t(lr, t):
    """Adam's a_t the way the caller of ssn_ens_apply_f32 forms it (fp64; the kernel reads its float32 rounding)."""
    return lr * math.sqrt(1.0 - math.pow(APPLY_HYPER['beta2'], t)) / (1.0 - math.pow(APPLY_HYPER['beta1'], t))


def apply_step_reg(rule, p0, g, state, lr, reg, lo=None, hi=None, defect=None):
    """One fp64 update with regularisation, as optimizer_kernel and critic.Updater order it: the penalties enter the gradient
    before the rule (2 l2_penalty p0 + l1_penalty sign(p0)), the decoupled decays act on the OLD value after it
    (lr l2_decay p0 + lr l1_decay sign(p0)), then numpy's clip.  lr and the four weights: scalars or per element.  Returns
    (unclipped, clipped, the regularised gradient).  `defect`: one of DEFECTS[4:7]."""
    from . import gan_torch as og
    h = APPLY_HYPER
    l2p, l1p, l2d, l1d = reg
    sign = (lambda v: (v > 0).astype('float64')) if defect == 'sign-dropped-below-zero' else np.sign
    with np.errstate(invalid='ignore', over='ignore'):
        g2 = g + 2 * l2p * p0 + l1p * sign(p0)
        if rule == 'adam':
            u = og.adam_step(p0, g2, state, lr, beta1=h['beta1'], beta2=h['beta2'], eps=h['epsilon_adam'])
        elif rule == 'rmsprop':
            u = og.rmsprop_step(p0, g2, state, lr, rho=h['rho'], eps=h['epsilon_rmsprop'])
        else:
            u = og.sgd_step(p0, g2, state, lr)
        base = u if defect == 'decay-from-new-value' else p0
        u = u - (lr * l2d * base + lr * l1d * sign(base))
        return u, (u if lo is None else np.clip(u, lo, hi)), g2


def _per_element(c, hyp):
    return [np.repeat(hyp[:, i], c.P) for i in range(5)]


def apply_trace(c, x, defect=None, hyp=None, rule=None, scalar_clip=False):
    """The two steps in fp64 over the K P elements: per step dict(u, p, g2, where, m, v), and per element the smallest distance of
    an update from a bound it is not clipped to or beyond (the lo == hi element left out)."""
    hyp = x['hyp'] if hyp is None else hyp
    lr, reg = _per_element(c, hyp)[0], _per_element(c, hyp)[1:]
    n = c.K * c.P
    lo, hi = (np.full(n, x['lo'].min()), np.full(n, x['hi'].max())) if scalar_clip else (x['lo'], x['hi'])
    state, p, steps, margin = {}, x['p0'], [], np.full(n, np.inf)
    for g in x['g']:
        u, p, g2 = apply_step_reg(rule or c.rule, p, g, state, lr, reg, lo, hi, defect)
        where = np.where(u < lo, -1, np.where(u > hi, 1, 0))
        d = np.minimum(np.abs(u - lo), np.abs(u - hi))
        d[2] = np.inf
        margin = np.minimum(margin, d)
        steps.append(dict(u=u, p=p, g2=g2, where=where, m=state.get('m', state.get('a')), v=state.get('v')))
    return dict(steps=steps, margin=margin)


def apply_inputs(c):
    """p0 (negative, exactly 0 in element 1 of every member, positive), two gradients, per-element bounds built as
    gen_step_cases.apply_inputs builds them: element e is meant to land inside (e % 4 in {0, 3}), below lo (1) or above hi (2)
    in step 1, element 2 has lo == hi.  The second gradient is redrawn, element by element (the update is element-wise), until
    every update of both steps lies APPLY_MARGIN or more from both of its bounds."""
    def make():
        rs = np.random.RandomState(10000 + 3 * c.P + c.K + 100 * RULES.index(c.rule))
        n = c.K * c.P
        hyp = apply_hyper(c.K)
        p0 = rs.uniform(0.1, 1.0, n) * rs.choice([-1.0, 1.0], n)
        p0[0], p0[2] = -0.5, 0.5
        p0[1::c.P] = 0.0
        p0 = _f32(p0)
        g1 = _f32(rs.randn(n))
        u1, _, _ = apply_step_reg(c.rule, p0, g1, {}, _per_element(c, hyp)[0], _per_element(c, hyp)[1:])
        kind = np.arange(n) % 4
        off, width = rs.uniform(0.2, 0.4, n), rs.uniform(0.5, 1.0, n)
        lo = np.where(kind == 1, u1 + off, np.where(kind == 2, u1 - off - width, u1 - off))
        hi = lo + width + np.where((kind == 0) | (kind == 3), off, 0.0)
        lo[2] = hi[2] = 0.25
        x = dict(p0=p0, hyp=hyp, lo=_f32(lo), hi=_f32(hi), g=[g1, _f32(rs.randn(n))])
        for rounds in range(200):
            near = apply_trace(c, x)['margin'] < APPLY_MARGIN
            if not near.any():
                x['rounds'] = rounds
                return x
            x['g'][1][near] = _f32(rs.randn(int(near.sum())))
        raise AssertionError('no draw clear of the bounds: %r' % (c,))
    return _cached(('ea-in', c), make)


def apply_tol(want):
    return gc.apply_tol(want)


# ------------------------------------------------------------------ stimulus
EnsStim = collections.namedtuple('EnsStim', 'K B NB N smooth')
STIM_CASES = [EnsStim(3, 2, 4, 1, gc.SMOOTH[0]), EnsStim(3, 2, 4, 10, gc.SMOOTH[1]), EnsStim(8, 33, 8, 125, gc.SMOOTH[0]),
              EnsStim(1, 2, 4, 10, gc.SMOOTH[0])]


def ens_gain(v, zin, K, B, N):
    """(K B, 2N) float32: 1 + fl(v z) with (V_E, V_I) of the draw's member."""
    return np.concatenate([hetero_gain(v[k], zin[sl], N) for k, sl in enumerate(_rows(K, B))])


def ens_stim_inputs(c):
    def make():
        rs = np.random.RandomState(11000 + 11 * c.N + 3 * c.NB + c.B + 100 * c.K)
        nb, M = c.K * c.B, 2 * c.N
        bw = rs.choice([0.0625, 0.125, 0.1875, 0.25, 0.5, 0.75], (nb, c.NB))
        bw.flat[0], bw.flat[1] = 0.0, 1.0
        x = dict(bw=bw, con=_f32(rs.uniform(1, 40, (nb, c.NB))), smooth=float(np.float32(c.smooth)),
                 v=_f32(rs.uniform(0.1, 0.5, (c.K, 2)) + 0.5 * np.arange(c.K)[:, None] / c.K), zin=_f32(rs.uniform(-1, 1, (nb, M))))
        x['gain'] = ens_gain(x['v'], x['zin'], c.K, c.B, c.N).astype('float64')
        return x
    return _cached(('es-in', c), make)


def ens_stim_oracle(c, gain=None):
    """dict(want (K B, NB, 2N), allowed, tol): gen_step_cases.stim_oracle's arithmetic; `gain` replaces the case's (the defects)."""
    x = ens_stim_inputs(c)
    g = x['gain'] if gain is None else gain
    want, bound = gc.stimulus(x['bw'], x['con'], x['smooth'], c.N, g, with_bound=True)
    e32 = gc.stimulus(x['bw'], x['con'], x['smooth'], c.N, g, 'float32').astype('float64')
    dev32 = float((np.abs(e32 - want) / np.abs(want)).max())
    rel = TOLERANCE_MULTIPLE * dev32 + np.broadcast_to(bound, want.shape)
    return dict(want=want, allowed=rel * np.abs(want) + 2.0 ** -149, tol=float(rel.max()), dev32=dev32)


def fused_gain(v, zin, K, B, N):
    """The gain with the product contracted into the addition: fl(1 + v z), ONE rounding."""
    vm = np.repeat(np.repeat(np.asarray(v, dtype='float64'), N, axis=1), B, axis=0)
    return (1.0 + vm * np.asarray(zin, dtype='float64')).astype('float32')


# ------------------------------------------------------------------ defects, for the sensitivity of the checks
DEFECTS = ('rows-past-256-dropped', 'member-reads-the-member-before', 'pq-of-block-01-in-block-10', 'V_E-and-V_I-swapped',
           'sign-dropped-below-zero', 'decay-from-new-value', 'regularised-gradient-recorded', 'rule-2-run-as-rule-0',
           'second-sweep-skipped', 'product-contracted')


def _worst(pairs):
    """The largest |bad - good| / allowed over (bad, good, allowed) triples; 0 / 0 counts as 0."""
    worst = 0.0
    for bad, good, allowed in pairs:
        with np.errstate(divide='ignore', invalid='ignore'):
            r = np.abs(np.asarray(bad, dtype='float64') - good) / allowed
        worst = max(worst, float(np.nan_to_num(r, nan=0.0, posinf=np.inf).max()))
    return worst


def defect_ratio(kind, c):
    """The largest |defective - oracle| / allowed over the checked elements of case `c` (True / False for the bit test of the
    last defect), or None where the defect does not apply."""
    if kind == DEFECTS[0]:
        if isinstance(c, Mom) and c.B > BLOCK:
            o, bad = mom_oracle(c), mom_oracle(c, rows=BLOCK)
            return min(_worst([(bad[k], o[k], o['allowed_' + k])]) for k in ('m', 's', 'gx'))
        if isinstance(c, EnsGG):
            x = gg_inputs(c, 'free')
            o, bad = gen_grads_exact(c, x), gen_grads_in_order(c, x, rows=BLOCK)
            r = []
            if c.B * c.NB * c.M > BLOCK:
                r += [_worst([(bad['dyn'], o['dyn'], U * np.abs(o['dyn']))]), _worst([(bad['rate'], o['rate'], U * np.abs(o['rate']))])]
                if c.nv:
                    r.append(_worst([(bad['grads'][:, :c.nv], o['grads'][:, :c.nv], o['grads_allowed'][:, :c.nv])]))
            if c.B > BLOCK:
                r.append(_worst([(bad['grads'][:, c.nv:], o['grads'][:, c.nv:], o['grads_allowed'][:, c.nv:])]))
            if c.D > BLOCK:
                r.append(_worst([(bad['L0'], o['L0'], o['L0_allowed'])]))
            return min(r) if r else None
        return None
    if kind == DEFECTS[1]:
        if getattr(c, 'K', 1) < 2:
            return None
        if isinstance(c, EnsJds) and c.N > 1:
            good, bad = ens_jds_oracle(c), ens_jds_oracle(c, params=[member_jds((k - 1) % c.K) for k in range(c.K)])
            r = [_worst([(b['want'], g['want'], g['allowed'])]) for g, b in zip(good, bad)]
            if c.gw == 'onehot':       # (on the diagonal dx = 0: no parameter enters)
                r = [r[k] for k, (name, p, q, i, j) in enumerate(onehot_places(c.N)) if i != j]
            return min(r)
        if isinstance(c, EnsStim):
            x, o = ens_stim_inputs(c), ens_stim_oracle(c)
            bad = ens_stim_oracle(c, gain=ens_gain(np.roll(x['v'], 1, axis=0), x['zin'], c.K, c.B, c.N).astype('float64'))
            return _worst([(bad['want'], o['want'], o['allowed'])])
        if isinstance(c, EnsApply):
            x = apply_inputs(c)
            good, bad = apply_trace(c, x), apply_trace(c, x, hyp=np.roll(x['hyp'], 1, axis=0))
            return max(_worst([(b['p'], g['p'], apply_tol(g['p']))]) for g, b in zip(good['steps'], bad['steps']))
        if isinstance(c, EnsGG):
            x = gg_inputs(c, 'free')
            o = gen_grads_in_order(c, x)
            bad = gen_grads_in_order(c, dict(x, costs=np.roll(x['costs'], 1, axis=0)))
            return _worst([(bad['loss'], o['loss'], loss_allowed(o['L0'], x['costs'], o['dyn'], o['rate']))])
        return None
    if kind == DEFECTS[2] and isinstance(c, EnsJds) and c.N > 1:
        def swap(a):
            a = a.copy()
            a[1, 0] = a[0, 1]
            return a
        good, bad = ens_jds_oracle(c), ens_jds_oracle(c, params=[tuple(swap(a) for a in member_jds(k)) for k in range(c.K)])
        r = [_worst([(b['want'], g['want'], g['allowed'])]) for g, b in zip(good, bad)]
        if c.gw == 'onehot':           # the defect shows where block (1, 0) is fed off its diagonal
            r = [r[k] for k, (name, p, q, i, j) in enumerate(onehot_places(c.N)) if (p, q) == (1, 0) and i != j]
        return min(r)
    if kind == DEFECTS[3] and isinstance(c, EnsStim):
        x, o = ens_stim_inputs(c), ens_stim_oracle(c)
        bad = ens_stim_oracle(c, gain=ens_gain(x['v'][:, ::-1], x['zin'], c.K, c.B, c.N).astype('float64'))
        return _worst([(bad['want'], o['want'], o['allowed'])])
    if kind in DEFECTS[4:8] and isinstance(c, EnsApply):
        x = apply_inputs(c)
        good = apply_trace(c, x)
        if kind == DEFECTS[6]:         # rec[P + i] is held to the bits of the gradient handed in
            return _worst([(s['g2'], g, U * np.abs(g)) for s, g in zip(good['steps'], x['g'])])
        if kind == DEFECTS[7]:
            if c.rule != 'rmsprop':
                return None
            bad = apply_trace(c, x, rule='sgd')
        else:
            bad = apply_trace(c, x, defect=kind)
        return max(_worst([(b['p'], g['p'], apply_tol(g['p']))]) for g, b in zip(good['steps'], bad['steps']))
    if kind == DEFECTS[8]:
        if isinstance(c, EnsApply) and c.K * c.P > APPLY_SWEEP:
            x, s = apply_inputs(c), apply_trace(c, apply_inputs(c))['steps'][0]
            return _worst([(x['p0'][APPLY_SWEEP:], s['p'][APPLY_SWEEP:], apply_tol(s['p'][APPLY_SWEEP:]))])
        if isinstance(c, EnsStim) and c.K * c.B * c.NB * 2 * c.N > STIM_SWEEP:
            o = ens_stim_oracle(c)
            w, a = o['want'].reshape(-1)[STIM_SWEEP:], o['allowed'].reshape(-1)[STIM_SWEEP:]
            return _worst([(np.zeros_like(w), w, a)])
        return None
    if kind == DEFECTS[9] and isinstance(c, EnsStim):
        x = ens_stim_inputs(c)
        return bool((fused_gain(x['v'], x['zin'], c.K, c.B, c.N) != x['gain'].astype('float32')).any())
    return None

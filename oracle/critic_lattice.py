"""ORACLE -- TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  numpy only.

The WGAN-GP critic (networks/cwgan.py:123-214, simple_discriminator.py:139-165) on inputs for which there is nothing to
round: every operand of every GEMM of an update is a bf16 number and every partial sum of every GEMM is an fp32 number, in any
summation order.  On such a case the fp64 evaluation below is THE answer of any arithmetic with bf16 (or wider) operands and
fp32 (or wider) accumulation: precision and order cannot matter, no pre-activation is close to zero without being zero, and
the GPU's bf16 paths have to give these bits (tests/test_critic_lattice_gpu.py).  That a case is of this kind is not assumed:
`check_lattice` asserts it GEMM by GEMM, and tests/test_critic_lattice.py pins the hand-written chains below to torch autograd
on oracle/gan_torch.py.

The chains are written by hand (no autograd) in the form of csrc/ssn_critic.hip's header comment, so that every operand site
is visible and can be hooked:

    h_0 = [x, c_0, |c_1|, c_2 (0 with hide_cell_type)],  u_l = h_{l-1} W_l + b_l,  h_l = f(u_l),  D = h_L w_out
    Wasserstein half on [xg; xd], upstream up = [1/ng ..., -1/nd ...]:
        v_L = f'(u_L) * w_out^T * up,  v_{l-1} = f'(u_{l-1}) * (v_l W_l^T),  dW_l = h_{l-1}^T v_l,  db_l = colsum v_l
    penalty half on xp (upstream 1): the same chain gives g = v_1 W_1^T, taken over the x columns only;
        ghat = 2 (||g|| - 1) / ||g|| / np * g,  e_0 = ghat,  dW_l += lmd e_{l-1}^T v_l,  e_l = f'(u_l) * (e_{l-1} W_l),
        dw_out += lmd colsum e_L

`site` is applied to both operands of every GEMM (x, cond, every W_l in both orientations, w_out, h_l, v_l, ghat, e_l): the
identity, or `round_bf16` -- on a lattice case the two agree bit for bit.
"""
import numpy as np

LEAK = {'rectify': 0.0, 'linear': 1.0}          # the dyadic slopes (0.01 and 1/3 are not: they stay with tests/test_critic_gpu.py)

# name -> shape of the case (tests/test_critic_lattice_gpu.py runs all of them; nx = 8)
CASES = {
    'c3': dict(layers=[512, 512, 512], ng=256, nd=512, np=32),
    'ragged': dict(layers=[512, 64], ng=16, nd=64, np=8),
    'odd': dict(layers=[96, 160, 32], ng=64, nd=32, np=16),
    'one': dict(layers=[32], ng=8, nd=32, np=4),
    'tails': dict(layers=[72, 100, 132], ng=128, nd=64, np=32),
    'linear': dict(layers=[256, 128], ng=128, nd=128, np=64, nonlinearity='linear'),
    'nocond': dict(layers=[256, 128], ng=128, nd=128, np=64, conditional=False),
    'hide': dict(layers=[96, 160, 32], ng=64, nd=32, np=16, hide_cell_type=True),
    # every weight-gradient GEMM of both halves contracts over >= 512 rows, as in the benchmark's critic step: the only kind of
    # shape whose weight gradients go through gemm_bf16_pipe_batch_kernel (row-block path) or the three streams (layer path);
    # 'c3', with 32 penalty rows, issues them one by one
    'c3par': dict(layers=[512, 512, 512], ng=512, nd=512, np=512),
}
NX = 8


# ------------------------------------------------------------------------------------------------------------------
# number formats
# ------------------------------------------------------------------------------------------------------------------
def round_bf16(a, mode='rne'):
    """fp32 -> bf16 -> fp32 by bit operations (finite values).  'rne': to nearest, ties to even (what the kernels do);
    'trunc': towards zero; 'away': away from zero whenever inexact -- the last two only for the mutation checks."""
    a32 = np.ascontiguousarray(a, dtype=np.float32)
    u = a32.view(np.uint32).astype(np.uint64)
    if mode == 'rne':
        u = u + 0x7fff + ((u >> 16) & 1)
    elif mode == 'away':
        u = u + 0xffff
    elif mode != 'trunc':
        raise ValueError(mode)
    return (u & 0xffff0000).astype(np.uint32).view(np.float32).reshape(a32.shape)


def is_bf16(a):
    """Every element is an fp32 number whose low 16 bits are zero."""
    a64 = np.asarray(a, dtype=np.float64)
    a32 = a64.astype(np.float32)
    return bool(np.array_equal(a32.astype(np.float64), a64) and ((np.ascontiguousarray(a32).view(np.uint32) & 0xffff) == 0).all())


def is_bf16_tie(a):
    """Elementwise: an fp32 number exactly half way between two neighbouring bf16 numbers."""
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) & 0xffff) == 0x8000


def lsb(a):
    """The largest power of two that divides every non-zero element (1 for an all-zero array)."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    a = a[a > 0]
    if a.size == 0:
        return 1.0
    m, e = np.frexp(a)                       # a = m 2^e, m in [.5, 1)
    x = (m * 2.0 ** 53).astype(np.int64)
    tz = np.zeros(a.shape, dtype=np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        z = (x & ((1 << s) - 1)) == 0
        tz += z * s
        x = np.where(z, x >> s, x)
    return 2.0 ** int((e - 53 + tz).min())


# ------------------------------------------------------------------------------------------------------------------
# the evaluation
# ------------------------------------------------------------------------------------------------------------------
class Eval(object):
    """One evaluation of a case: the rounding hook, the mutation, and what `check_lattice` and the tests read afterwards.

    rounding: None (hooks off) or a mode of `round_bf16`.
    mutate:   None or (kind, where): ('drop_tail', gemm name) zeroes the last 16 k of that GEMM; ('mask_shift', l) takes the
              slopes of hidden layer l from the row above in the backward chains; ('swap_n', None) swaps 1/ng and 1/nd;
              ('transpose', l) reads W_l (square) the wrong way round in the backward chain of the Wasserstein half.
    """

    def __init__(self, rounding=None, mutate=None, record=False):
        self.rounding, self.mutate = rounding, mutate or (None, None)
        self.gemms = [] if record else None          # (name, A, B) as the MFMA would see them
        self.ties = {}                               # site kind -> (ties, elements) of its operands before rounding

    def site(self, a, kind=None):
        if kind is not None:
            t = self.ties.setdefault(kind, [0, 0])
            t[0] += int(is_bf16_tie(a).sum())
            t[1] += int(np.size(a))
        if self.rounding is None:
            return np.asarray(a, dtype=np.float64)
        return round_bf16(a, self.rounding).astype(np.float64)

    def gemm(self, A, B, name, kinds=(None, None)):
        A, B = self.site(A, kinds[0]), self.site(B, kinds[1])
        if self.mutate == ('drop_tail', name):
            A = A.copy()
            A[:, -16:] = 0.0
        if self.gemms is not None:
            self.gemms.append((name, A, B))
        return A @ B


def input_block(x, cond, hide_cell_type):
    """h_0 of cwgan.py:164-170; cond None: the unconditional critic's h_0 = x."""
    x = np.asarray(x, dtype=np.float64)
    if cond is None:
        return x
    c = np.asarray(cond, dtype=np.float64)
    c2 = np.zeros(len(c)) if hide_cell_type else c[:, 2]
    return np.concatenate([x, np.stack([c[:, 0], np.abs(c[:, 1]), c2], axis=1)], axis=1)


def _split(params):
    L = (len(params) - 1) // 2
    W = [np.asarray(params[2 * l], dtype=np.float64) for l in range(L)]
    b = [np.asarray(params[2 * l + 1], dtype=np.float64) for l in range(L)]
    return W, b, np.asarray(params[-1], dtype=np.float64).reshape(-1, 1)


def forward(ev, params, h0, leak, tag):
    """hs[l] = h_l (l = 0..L), sl[l] = f'(u_l) (l = 1..L; sl[0] unused), D (rows,)."""
    W, b, wout = _split(params)
    hs, sl = [h0], [None]
    for l in range(len(W)):
        u = ev.gemm(hs[-1], W[l], 'fwd%d%s' % (l + 1, tag), ('x' if l == 0 else 'h', 'W')) + b[l]
        pos = u > 0
        hs.append(np.where(pos, u, leak * u))
        sl.append(np.where(pos, 1.0, leak))
    D = ev.gemm(hs[-1], wout, 'out' + tag, ('h', None))[:, 0]
    return hs, sl, D


def backward_chain(ev, params, sl, up, tag, to_input):
    """v[l], l = L..1 (and v[0] = v_1 W_1^T with `to_input`): v_L = f'(u_L) * w_out^T * up, v_{l-1} = f'(u_{l-1}) * (v_l W_l^T)."""
    W, b, wout = _split(params)
    L = len(W)

    def slopes(l):
        return np.roll(sl[l], 1, axis=0) if ev.mutate == ('mask_shift', l) else sl[l]
    v = [None] * (L + 1)
    v[L] = slopes(L) * wout.T * up[:, None] if L else wout.T * up[:, None]
    for l in range(L, 0, -1):
        if l == 1 and not to_input:
            break
        Wl = W[l - 1].T
        if ev.mutate == ('transpose', l) and tag == 'w':
            Wl = W[l - 1]
        t = ev.gemm(v[l], Wl, 'bwd%d%s' % (l, tag))
        v[l - 1] = t if l == 1 else slopes(l - 1) * t
    return v


def evaluate(case, rounding=None, mutate=None, record=False):
    """Everything the GPU entry points return for the case, in fp64: see the keys at the end."""
    ev = Eval(rounding, mutate, record)
    params, lmd, leak = case['params'], float(case['lmd']), LEAK[case['nonlinearity']]
    W, b, wout = _split(params)
    L = len(W)
    hide = case['hide_cell_type']
    ng, nd, npn = len(case['xg']), len(case['xd']), len(case['xp'])
    nx = np.asarray(case['xg']).shape[1]
    # ---- Wasserstein half on the stacked batch
    h0 = np.concatenate([input_block(case['xg'], case['cg'], hide), input_block(case['xd'], case['cd'], hide)])
    a, c = (1.0 / nd, 1.0 / ng) if ev.mutate[0] == 'swap_n' else (1.0 / ng, 1.0 / nd)
    up = np.concatenate([np.full(ng, a), np.full(nd, -c)])
    hs, sl, D = forward(ev, params, h0, leak, 'w')
    v = backward_chain(ev, params, sl, up, 'w', False)
    gW = [None] * L
    gb = [None] * L
    gwout = ev.gemm(hs[L].T, up[:, None], 'gout')
    sW = [None] * L                                      # sum of |terms| of every gradient element (for derived bounds)
    swout = np.abs(hs[L]).T @ np.abs(up[:, None])
    for l in range(L):
        gW[l] = ev.gemm(hs[l].T, v[l + 1], 'gW%dw' % (l + 1))
        gb[l] = v[l + 1].sum(axis=0)
        sW[l] = np.abs(hs[l]).T @ np.abs(v[l + 1])
    # ---- penalty half
    hp0 = input_block(case['xp'], case['cp'], hide)
    hp, slp, _ = forward(ev, params, hp0, leak, 'p')
    vp = backward_chain(ev, params, slp, np.ones(npn), 'p', True)
    g = vp[0][:, :nx] if L else np.broadcast_to(wout.T, (npn, len(wout)))[:, :nx]
    nrm = np.sqrt((g * g).sum(axis=1))
    d = nrm - 1.0
    with np.errstate(invalid='ignore', divide='ignore'):
        coef = np.where(nrm > 0, 2.0 * d / nrm / npn, 0.0)
    ghat = np.zeros_like(hp0)
    ghat[:, :nx] = coef[:, None] * g
    # (lmd = 0: the second chain is multiplied by zero as a whole -- its operands are finite, not lattice numbers, and it is
    # left out here; the kernels compute it and add 0 * sum)
    es, ea = [ghat], np.abs(ghat)
    for l in range(L if lmd != 0 else 0):
        gW[l] = gW[l] + lmd * ev.gemm(es[l].T, vp[l + 1], 'gW%dp' % (l + 1), ('ghat' if l == 0 else None, None))
        sW[l] = sW[l] + lmd * (ea.T @ np.abs(vp[l + 1]))
        es.append(slp[l + 1] * ev.gemm(es[l], W[l], 'e%d' % (l + 1)))
        ea = slp[l + 1] * (ea @ np.abs(W[l]))
    if lmd != 0:
        gwout = gwout + lmd * es[L].sum(axis=0)[:, None]
        swout = swout + lmd * ea.sum(axis=0)[:, None]
    pen = float((d * d).mean())
    dg, dd = float(D[:ng].mean()), float(D[ng:].mean())
    flat, sflat = [], []
    for l in range(L):
        flat += [gW[l].ravel(), gb[l].ravel()]
        sflat += [sW[l].ravel(), np.zeros(gb[l].size)]
    # ---- generator side: scale * dD/dx of the xg rows, scale = -1 / ng
    hg, slg, Dg = forward(ev, params, h0[:ng], leak, 'g')
    vg = backward_chain(ev, params, slg, np.ones(ng), 'g', True)
    gx = (-1.0 / ng) * (vg[0][:, :nx] if L else np.broadcast_to(wout.T, (ng, len(wout)))[:, :nx])
    return dict(
        D=D, stats=np.array([dg, dd, pen, dg - dd + lmd * pen]), flat=np.concatenate(flat + [gwout.ravel()]),
        flat_abs=np.concatenate(sflat + [swout.ravel()]), gx=gx, gx_mean=float(Dg.mean()), accuracy=dg - dd,
        # intermediates (tests of the oracle itself)
        active=[float((s == 1.0).mean()) for s in sl[1:]], norms=nrm, e=es[1:], h=hs, hp=hp, ev=ev)


def tensor_slices(case):
    """(kind, slice into the flat vector) per parameter tensor, in `Critic.get_param_values()` order."""
    out, off = [], 0
    for i, p in enumerate(case['params']):
        n = int(np.size(p))
        out.append(('W' if i % 2 == 0 else 'b', slice(off, off + n)))
        off += n
    return out


def check_lattice(case):
    """Asserts that the case is what the module docstring says: for every GEMM of the update, the forward and the input
    gradient both operands are bf16 numbers, and the largest sum of |a||b| of any output element, in units of the product of
    the operands' last places, stays below 2^24 -- so every partial sum in any order is an fp32 number; no penalty row has
    norm 0 and every norm is an integer when the penalty counts (lmd != 0).  Returns the largest such sum (log2) and the names."""
    out = evaluate(case, record=True)
    worst = 0.0
    names = []
    for name, A, B in out['ev'].gemms:
        assert is_bf16(A), name + ': left operand is no bf16 number'
        assert is_bf16(B), name + ': right operand is no bf16 number'
        bound = float((np.abs(A) @ np.abs(B)).max()) / (lsb(A) * lsb(B))
        assert bound < 2.0 ** 24, (name, np.log2(max(bound, 1.0)))
        worst = max(worst, bound)
        names.append(name)
    for p in case['params'][1::2]:
        assert np.array_equal(p, np.round(p)) and np.abs(p).max() < 2 ** 10, 'biases are small integers'
    if case['lmd'] != 0:
        nrm = out['norms']
        assert (nrm > 0).all(), 'a penalty row with norm 0'
        assert np.array_equal(nrm, np.round(nrm)), 'a norm that is no integer'
    return np.log2(max(worst, 1.0)), names


# ------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------
def _ternary(rs, shape, density):
    return np.where(rs.rand(*shape) < density, rs.choice([-1.0, 1.0], shape), 0.0)


def _signed_perm_sum(rs, nin, nout, terms=2):
    """A sum of `terms` signed permutation matrices, wrapped round the shorter side: `terms` entries in every line of the longer
    side, terms * max / min in every line of the shorter one (a rectangular layer with empty rows or columns would leave most of
    the gradient of the layer in front of it exactly zero)."""
    W = np.zeros((nin, nout))
    n = max(nin, nout)
    for _ in range(terms):
        np.add.at(W, (rs.permutation(n) % nin, np.arange(n) % nout), rs.choice([-1.0, 1.0], n))
    return W


def _inputs(rs, n, conditional):
    x = rs.randint(0, 4, (n, NX)).astype(np.float64)
    if not conditional:
        return x, None
    # contrast in {1, 2, 4}, norm_probe in {-1, 0, 1} (the critic sees its absolute value), cell type in {0, 1}
    c = np.stack([rs.choice([1.0, 2.0, 4.0], n), rs.randint(0, 2, n) * rs.choice([-1.0, 1.0], n), rs.randint(0, 2, n).astype(np.float64)], axis=1)
    return x, c


def make_case(name, family, seed=0):
    """Parameters in `Critic.get_param_values()` order, inputs and lmd of a lattice case.

    Both families: x integer in 0..3, condition columns [{1, 2, 4}, {-1, 0, 1}, {0, 1}]; W_1 ternary with density 0.5, W_l
    (l >= 2) a sum of two signed permutation matrices, biases integer in -2..2, w_out ternary with one zero in ten, upstreams
    +-1/ng, +-1/nd, 1/np with powers of two.  (A constant contrast that outweighs everything else in its unit, a w_out with a
    third of zeros and rectangular layers with empty rows were tried first: most units were then always on or always off and
    5-24 % of a deep tensor's gradient was non-zero; with these choices it is 27 % or more in every tensor of every case.)
    family 'A': lmd = 0, W_1 dense ternary in all its rows.
    family 'B': lmd = 8; the first four x rows of W_1 are +-w0 for ONE ternary w0 (density 0.5) and the other four are zero, so every
    coordinate of a row's input gradient has the same magnitude |g0|, ||g|| = 2 |g0| is an integer and the row's upstream
    2 (||g|| - 1) / ||g|| / np * g_i = +-(2 |g0| - 1) / np is a bf16 number; penalty rows are the first np of 8 np seeded
    candidates with |g0| >= 1.  (A parameter draw that leaves fewer such rows -- a linear critic's g0 is the same for every
    row -- is drawn again from the next sub-seed.)"""
    spec = dict(nonlinearity='rectify', conditional=True, hide_cell_type=False)
    spec.update(CASES[name])
    layers, ng, nd, npn = spec['layers'], spec['ng'], spec['nd'], spec['np']
    assert family in ('A', 'B')
    for sub in range(64):
        rs = np.random.RandomState([sum(ord(ch) for ch in name), ord(family), seed, sub])
        dims = [NX + (3 if spec['conditional'] else 0)] + list(layers)
        W = [_ternary(rs, (dims[0], dims[1]), 0.5)]
        if family == 'B':
            w0 = _ternary(rs, (dims[1],), 0.5)
            W[0][4:NX] = 0.0
            for i in range(4):
                W[0][i] = rs.choice([-1.0, 1.0]) * w0
        for l in range(1, len(layers)):
            W.append(_signed_perm_sum(rs, dims[l], dims[l + 1]))
        b = [rs.randint(-2, 3, n).astype(np.float64) for n in layers]
        wout = _ternary(rs, (layers[-1], 1), 0.9)
        params = []
        for l in range(len(layers)):
            params += [W[l], b[l]]
        params.append(wout)
        xg, cg = _inputs(rs, ng, spec['conditional'])
        xd, cd = _inputs(rs, nd, spec['conditional'])
        case = dict(name=name, family=family, seed=seed, layers=list(layers), nx=NX, params=params, xg=xg, cg=cg, xd=xd, cd=cd,
                    lmd=8.0 if family == 'B' else 0.0, nonlinearity=spec['nonlinearity'], conditional=spec['conditional'],
                    hide_cell_type=spec['hide_cell_type'])
        xc, cc = _inputs(rs, 8 * npn, spec['conditional'])
        if family == 'A':
            case['xp'], case['cp'] = xc[:npn], (None if cc is None else cc[:npn])
            return case
        ev = Eval()
        _, sl, _ = forward(ev, params, input_block(xc, cc, spec['hide_cell_type']), LEAK[spec['nonlinearity']], 'c')
        g0 = backward_chain(ev, params, sl, np.ones(len(xc)), 'c', True)[0][:, 0]
        keep = np.where(np.abs(g0) >= 1)[0][:npn]
        if len(keep) == npn:
            case['xp'], case['cp'] = xc[keep], (None if cc is None else cc[keep])
            return case
    raise AssertionError('no parameter draw with enough penalty rows: ' + name)


def make_tie_case(seed=0):
    """One hidden layer of 32 units, no condition columns, forward only: the operands at the three rounding sites of the
    forward -- x, W_1, h_1 -- are exact ties between neighbouring bf16 numbers, so the rounding MODE decides D.

    x in {1 + 2^-8, 1 + 3 2^-8} (to nearest even: 1 and 1 + 2^-6; truncated: 1 and 1 + 2^-7; away: 1 + 2^-7 and 1 + 2^-6);
    W_1 has one non-zero per column, +-(1 + 2^-8) or +-(1 + 3 2^-8); b = 2 + 2^-7 (added in fp32, no rounding site), so that
    with nearest-even operands u = x w + b is 3 + 2^-7 or 3 + 2^-6 + 2^-7 wherever x w is 1 or 1 + 2^-6: half way between
    two bf16 numbers of [2, 4).  Whatever the mode, the rounded operands have few bits: products and sums are exact."""
    rs = np.random.RandomState(1000 + seed)
    n, width = 40, 32
    t = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])
    x = rs.choice(t, (n, NX))
    W1 = np.zeros((NX, width))
    W1[np.arange(width) % NX, np.arange(width)] = rs.choice(t, width) * rs.choice([-1.0, 1.0], width, p=[0.25, 0.75])
    b = np.full(width, 2.0 + 2.0 ** -7)
    wout = rs.choice([-1.0, 1.0], (width, 1))
    return dict(name='tie', family='T', seed=seed, layers=[width], nx=NX, params=[W1, b, wout], x=x, nonlinearity='rectify',
                conditional=False, hide_cell_type=False)


def tie_forward(case, rounding):
    """D of the tie case under a rounding mode, and the share of exact ties among the operands of each site."""
    ev = Eval(rounding)
    _, _, D = forward(ev, case['params'], input_block(case['x'], None, False), 0.0, 't')
    return D, {k: t[0] / float(t[1]) for k, t in ev.ties.items()}

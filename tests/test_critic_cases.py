"""What makes tests/test_critic_edges_gpu.py meaningful, without a GPU: for every case of oracle/critic_cases.py the three
conditions on its inputs (every unit alive, no row near a kink, no end element of a vector gradient hidden), the path table
against the dispatch rule, the float32 oracle's deviation in every measure -- the number the tolerance is four times of -- with
its cap, and the sensitivity of the measures: what a kernel that loses an edge would return measures at least ten times the
tolerance.  And the reason the cases exist: with the biases of tests/test_critic_gpu.py::_setup a net has dead units, whose
gradient rows are exactly zero (`test_the_gap_dead_units_hide_a_lost_edge`)."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import critic_cases as cc
from oracle import gan_torch as og

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c.name for c in cc.CASES]


# ------------------------------------------------------------------ the conditions
@pytest.mark.parametrize('c', cc.CASES, ids=IDS)
def test_case_conditions(c):
    """`critic_cases.conditions`: inputs and parameters are fp32 numbers; in the fp64 oracle every unit of every layer is active
    on 10 ... 90 % of the rows of each batch (batches under 20 rows: on some row and not on some row of the three together); no
    pre-activation of any row of any batch within 1e-3 of its layer's rms; first and last element of every bias / w_out gradient
    >= 0.05 of the vector's largest and at most 1 % of a vector below 100 x the tolerance.  The numpy forward those are read
    from is the oracle's: same D values."""
    fig = cc.conditions(c)
    print('%s: active on %.2f ... %.2f of a batch, nearest pre-activation %.2e of its rms after %d redraws, smaller end of a vector '
          '%.3f of its largest, %.3f of a vector below 100 x tol' % (c.name, fig['active'][0], fig['active'][1], fig['kink'],
                                                                     fig['rounds'], fig['ends'], fig['small']))
    x, o = cc.inputs(c), cc.oracle(c)
    D = np.concatenate([cc.pre_activations(c, x['params'], x['x' + k], x['c' + k])[1] for k in 'gd'])
    np.testing.assert_allclose(D, o['dvals'], rtol=1e-11, atol=1e-13)


def test_batches_are_unequal_somewhere_in_every_family():
    """Gap 3: ng != nd != np.  Cases with three different batches exist on every path."""
    for path in ('fused', 'plain', 'general'):
        assert any(len(set(c.batches)) == 3 for c in cc.CASES if c.path == path), path


# ------------------------------------------------------------------ the path table
@pytest.mark.parametrize('c', cc.CASES, ids=IDS)
def test_path_table_against_the_dispatch_rule(c):
    n = cc.rows(c)
    norm = 'layer' in c.norm
    assert cc.critic_path(c, n) == c.path
    assert c.rb == (cc.fused_rb(n) if c.path == 'fused' else None)
    assert cc.critic_path(c, n, fused_enabled=False) == ('general' if norm else 'plain')
    if cc.has_extra(c) and c.conditional and c.nonlinearity == 'rectify':     # 1030 rows: fused forward with RB = 8; 2049: a chain
        assert cc.critic_path(c, 1030) == 'fused' and cc.fused_rb(1030) == 8
        assert cc.critic_path(c, 2049) == ('general' if norm else 'plain')
    if c.path == 'fused':           # a ragged last block of both row ranges, or an exact fit at the last size of a blocking
        bgd, npn = c.batches[0] + c.batches[1], c.batches[2]
        print('%s: %d rows, RB = %d, [xg; xd] blocks %d (last holds %d), penalty blocks %d (last holds %d)' % (
            c.name, n, c.rb, -(-bgd // c.rb), (bgd - 1) % c.rb + 1, -(-npn // c.rb), (npn - 1) % c.rb + 1))


def test_what_the_table_says_each_case_reaches():
    by = cc.BY_NAME
    assert cc.rows(by['rb4-last']) == 1024 and cc.rows(by['rb8-first']) == 1025
    assert cc.rows(by['fused-last']) == 2048 and cc.rows(by['chain-first']) == 2049
    b = by['rb8-first'].batches
    assert (b[0] + b[1]) % 8 == 4 and b[2] % 8 == 5               # ragged last block of both row ranges
    # 2049 rows: K = 1366 -> 10 slices of 144, last 70 = 4 x 16 + 6; K = 683 -> 5 slices, last 107
    assert cc.k_slices(128, 128, 1366) == (10, 144, 70) and 70 == 4 * 16 + cc.TAIL_ROWS
    assert cc.k_slices(128, 128, 683) == (5, 144, 107)
    # the same nets one row down, on the chains with SSN_CRITIC_FUSED=0: K = 682 -> 5 slices, last 106 (a K tail of 10)
    assert cc.k_slices(128, 128, 682) == (5, 144, 106)
    # widths just past 128: M N = 11 x 129 = 1419 is odd, so its slabs and every later one are off 16-byte alignment and
    # splitk_reduce_kernel takes its scalar branch
    d = cc.dims(by['odd-129'])
    assert d[0] * d[1] == 1419 and cc.k_slices(d[0], d[1], 1350) == (10, 144, 54) and cc.k_slices(d[0], d[1], 600) == (4, 160, 120)
    assert (129 * 65) % 4 == 1 and (65 * 33) % 4 == 1 and 33 % 4 == 1          # every M N odd: the scalar branch through `mn & 3` only
    # no split: K < 512
    c = by['wide-nosplit']
    assert all(cc.choose_splits(m, n, k) == 1 for m, n in zip(cc.dims(c)[:-1], cc.dims(c)[1:]) for k in (227, 64))
    assert 227 % 16 == 3 and 132 % 64 == 4 and 200 % 64 == 8
    # splits recomputed after rounding kchunk: 10 chosen, 9 taken
    d = cc.dims(by['resliced'])
    assert cc.choose_splits(d[0], d[1], 1295) == 10 and cc.k_slices(d[0], d[1], 1295) == (9, 144, 143)
    assert cc.k_slices(d[0], d[1], 520) == (4, 144, 88)
    # ... and the other way into the scalar branch of splitk_reduce_kernel: M N = 8 x 130 is a multiple of 4, but both GEMMs into
    # that gradient write their slabs behind odd-sized ones (9 x 41 of w_out, 9 x 130 x 41 of dW_2), off 16-byte alignment
    w1 = [(s, off) for M, N, K, s, off in cc.plain_chain_slabs(by['resliced']) if (M, N) == (8, 130)]
    assert len(w1) == 2 and (8 * 130) % 4 == 0 and all(s > 1 and off % 4 != 0 for s, off in w1), w1
    assert all(M * N % 4 for M, N, K, s, off in cc.plain_chain_slabs(by['odd-129']))
    # no other case of the table takes fewer slices than it chose
    for c in cc.CASES:
        if c.name != 'resliced':
            dd = cc.dims(c)
            for K in (c.batches[0] + c.batches[1], c.batches[2]):
                assert all(cc.k_slices(m, n, K)[0] == cc.choose_splits(m, n, K) for m, n in zip(dd[:-1], dd[1:]))


def test_the_unsplit_fallback_is_reached_by_one_case_only():
    """`gemm` runs a weight-gradient GEMM unsplit when the scratch is exhausted (module docstring of critic_cases): on the
    LayerNorm chain with wide layers and np >= 1024 -- 'ln-wide-unsplit', where the 512 x 512 GEMM of layer 2 in sweep 2 (the second to
    last issued) finds no room, while the 8 x 512 one of layer 1 behind it still fits and is split -- and by no other case on either chain (the fused-size LayerNorm cases run that chain with
    SSN_CRITIC_FUSED=0)."""
    for c in cc.CASES:
        if 'layer' not in c.norm:
            continue
        slabs = cc.general_chain_slabs(c)
        unsplit = [(M, N, K) for M, N, K, s in slabs if s == 1 and cc.choose_splits(M, N, K) > 1]
        print(c.name, 'scratch', cc.splitk_scratch_floats(c), 'unsplit for want of room:', unsplit)
        assert bool(unsplit) == (c.name == 'ln-wide-unsplit'), (c.name, unsplit)
        if unsplit:
            assert unsplit == [(512, 512, 1024)] and slabs[-2] == (512, 512, 1024, 1) and slabs[-1][3] > 1
        assert len(slabs) == 3 * len(c.layers) + 1                # three per weight (one for w_out): never a 5th into one C
    # the plain chain: two GEMMs per weight, K = ng + nd and np, into room for 2 x choose_splits(rows)
    for c in cc.CASES:
        d, (ng, nd, npn) = cc.dims(c), c.batches
        for m, n in list(zip(d[:-1], d[1:])) + [(d[-1], 1)]:
            assert cc.choose_splits(m, n, ng + nd) + cc.choose_splits(m, n, npn) <= 2 * cc.choose_splits(m, n, cc.rows(c))


def test_the_restated_rule_is_the_one_in_the_source():
    """The constants of `critic_cases.critic_path`, `fused_rb`, `choose_splits` as the library's source states them."""
    src = {f: open(os.path.join(ROOT, 'tc_gan_amd', 'csrc', f)).read() for f in ('ssn_capi.hip', 'ssn_critic_fused.hip', 'ssn_critic.hip')}
    assert re.search(r'return enabled && rows <= %d && ssn::critic_fused_supported' % cc.FUSED_MAX_ROWS, src['ssn_capi.hip'])
    assert re.search(r'constexpr int FMAXW = %d;' % cc.FUSED_MAX_WIDTH, src['ssn_critic_fused.hip'])
    assert re.search(r'constexpr int FMAXL = %d;' % cc.FUSED_MAX_LAYERS, src['ssn_critic_fused.hip'])
    assert 'return rows <= 1024 ? 4 : (rows <= 2048 ? 8 : 16);' in src['ssn_critic_fused.hip']
    assert 'if (K < 512 || tiles >= 256) return 1;' in src['ssn_critic.hip'] and 'const int maxs = K / 128;' in src['ssn_critic.hip']
    assert 'int splits = (512 + tiles - 1) / tiles;' in src['ssn_critic.hip']


# ------------------------------------------------------------------ the float32 oracle: what the tolerance is built from
@pytest.mark.parametrize('c', cc.CASES, ids=IDS)
def test_fp32_oracle_deviation_and_tolerance_cap(c):
    """The tolerance of a case and tensor kind is four times the deviation of the oracle itself run in float32 (DESIGN.md
    section 1) and may not exceed 1e-3 -- above that the inputs are at fault.  Measured (largest over the cases): weight matrices
    5.0e-6, vectors 2.3e-6, D values 3.4e-6, input gradient 8.0e-6 (both in 'ragged-ln'; 9.3e-7 / 6.9e-7 elsewhere), loss and
    statistics 6.2e-7, accuracy 5.3e-7.  A float32 run depends on the order its BLAS adds in, so no figure is pinned tighter
    than by a ceiling: each is at most 2.5e-5 (the tolerance at most 1e-4); for the two scalar kinds a figure below float32's unit
    roundoff 2^-24 counts as that (`critic_cases.tolerances`)."""
    dev = cc.fp32_oracle_deviation(c)
    tol = cc.tolerances(c)
    print('%s: fp32 oracle %s' % (c.name, ' '.join('%s %.2e' % (k, dev[k]) for k in cc.KINDS)))
    assert set(dev) == set(cc.KINDS)
    for k in cc.KINDS:
        floor = 2.0 ** -24 if k in ('stats', 'acc') else 0.0          # (the scalar kinds only: `critic_cases.tolerances`)
        assert tol[k] == 4 * max(dev[k], floor) and tol[k] <= cc.TOLERANCE_CAP == 1e-3
        assert 0 <= dev[k] <= 2.5e-5, (k, dev[k])


# ------------------------------------------------------------------ sensitivity
def _mutated(o, **kw):
    m = dict(o)
    m.update(kw)
    return m


@pytest.mark.parametrize('c', cc.CASES, ids=IDS)
def test_a_lost_edge_measures_ten_times_the_tolerance(c):
    """Mutations of the fp64 oracle's own result, each measured as the GPU module measures a kernel: the last row, the last
    column, the last unit's row and column of every weight gradient zero; the last element of every vector gradient zero; the
    share of the last TAIL_ROWS rows of [xg; xd] (the tail of the last short K slice in 'chain-first') taken out of the weight
    gradients; the D values of the last row block zero; the penalty mean taken over np - 1 rows."""
    o, tol = cc.oracle(c), cc.tolerances(c)
    L = len(c.layers)
    found = {}

    def factor(kind, tensor, **kw):
        return cc.errors(c, _mutated(o, **kw))[kind][tensor][0] / tol[kind]

    def with_grad(changes):
        g = [a.copy() for a in o['grads']]
        for i, sl in changes:
            g[i][sl] = 0
        return g

    for l in range(1, L + 1):
        iW, ib = 2 * (l - 1), 2 * (l - 1) + 1
        found['last row of dW%d' % l] = factor('W', 'dW%d' % l, grads=with_grad([(iW, np.s_[-1, :])]))
        found['last column of dW%d' % l] = factor('W', 'dW%d' % l, grads=with_grad([(iW, np.s_[:, -1])]))
        found['last element of db%d' % l] = factor('vec', 'db%d' % l, grads=with_grad([(ib, np.s_[-1])]))
        # the last unit of layer l: its column of dW_l, its bias gradient, its row of dW_{l+1} (or its element of dw_out)
        unit = with_grad([(iW, np.s_[:, -1]), (ib, np.s_[-1]), (iW + 2, np.s_[-1, :])])
        e = cc.errors(c, _mutated(o, grads=unit))
        nxt = ('W', 'dW%d' % (l + 1)) if l < L else ('vec', 'dw_out')
        found['last unit of layer %d' % l] = min(e['W']['dW%d' % l][0] / tol['W'], e['vec']['db%d' % l][0] / tol['vec'],
                                                 e[nxt[0]][nxt[1]][0] / tol[nxt[0]])
    found['last element of dw_out'] = factor('vec', 'dw_out', grads=with_grad([(2 * L, np.s_[-1, :])]))
    e = cc.errors(c, _mutated(o, grads=[g - t for g, t in zip(o['grads'], o['tail_grads'])]))
    found['without the last %d rows of [xg; xd]' % cc.TAIL_ROWS] = min(err for err, _ in e['W'].values()) / tol['W']
    rb = c.rb or 4
    d = o['dvals'].copy()
    d[-rb:] = 0
    found['D of the last row block zero'] = factor('D', 'dvals', dvals=d)
    pen = o['pen_rows'][:-1].mean()
    stats = o['stats'].copy()
    stats[3] += cc.LMD * (pen - stats[2])
    stats[2] = pen
    found['penalty mean over np - 1 rows'] = factor('stats', 'stats', stats=stats)
    for name, f in found.items():
        print('%s, %s: %.3g x the tolerance' % (c.name, name, f))
    assert all(f >= 10 for f in found.values()), {k: v for k, v in found.items() if not v >= 10}
    assert all(f >= 1 / tol['W'] * 0.999 for k, f in found.items() if k.startswith('last row') or k.startswith('last column'))


# ------------------------------------------------------------------ the reason these cases exist
def _setup_of_test_critic_gpu(batch, nx, layers, seed):
    """tests/test_critic_gpu.py::_setup without the device: `Critic.init_params` (Glorot weights, biases ~ N(0, 0.01), W_out
    last; one RandomState(seed)) and that function's inputs (contrast column 20)."""
    rng = np.random.RandomState(seed)
    d = [nx + 3] + list(layers)
    params = []
    for nin, nout in zip(d[:-1], d[1:]):
        a = np.sqrt(6.0 / (nin + nout))
        params += [rng.uniform(-a, a, size=(nin, nout)), rng.normal(0.0, 0.01, size=(nout,))]
    a = np.sqrt(6.0 / (d[-1] + 1))
    params.append(rng.uniform(-a, a, size=(d[-1], 1)))
    params = [og.t64(p.astype('float32')) for p in params]
    rs = np.random.RandomState(seed)
    xg, xd = rs.rand(batch, nx) * 5, rs.rand(batch, nx) * 5
    eps = rs.rand(batch, 1)
    xp = eps * xd + (1 - eps) * xg
    cond = np.stack([np.full(batch, 20.), rs.rand(batch) * 2 - 1, rs.randint(0, 2, batch)], axis=1)
    return params, xg, xd, xp, cond


@pytest.mark.parametrize('batch,layers', [(130, [100, 128, 72]), (130, [128, 128, 128, 128]), (256, [512, 512, 512])])
def test_the_gap_dead_units_hide_a_lost_edge(batch, layers):
    """With the nets of tests/test_critic_gpu.py (every bias ~ 0.01, contrast 20) some rectify units are inactive on every row
    of xg, xd and xp: the oracle's dL/dW_l has an exactly zero column there and dL/dW_{l+1} an exactly zero row -- in every
    weight tensor past the first -- so a kernel that loses exactly such a unit returns the oracle's answer.  The flat
    comparison of that file (atol 2e-5 of the largest element, which the contrast row of W_1 sets) also passes a zeroed row of
    a later tensor whenever the row is small against the contrast row.  The cases of critic_cases have no such unit."""
    params, xg, xd, xp, cond = _setup_of_test_critic_gpu(batch, 8, layers, seed=batch)
    ps = [p.clone().requires_grad_(True) for p in params]
    tg, td, tp, tc = (og.t64(a) for a in (xg, xd, xp, cond))
    grads = [g.numpy() for g in torch.autograd.grad(og.critic_loss(ps, tg, td, tp, tc, tc, tc, 10.0), ps)]
    zero_rows = [int((np.abs(grads[2 * l]).max(axis=1) == 0).sum()) for l in range(1, len(layers))]
    zero_rows.append(int((grads[-1][:, 0] == 0).sum()))
    print('%s, %d rows: exactly zero gradient rows of W_2 ... W_out: %s' % (layers, batch, zero_rows))
    assert all(n > 0 for n in zero_rows[:-1]), zero_rows
    for c in cc.CASES:
        assert all((np.abs(g).max(axis=0) > 0).all() and (np.abs(g).max(axis=1) > 0).all() for g in cc.oracle(c)['grads'] if g.ndim == 2)

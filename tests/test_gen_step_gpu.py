"""The small kernels around a generator step held to the fp64 restatements of oracle/gen_step_cases.py ONE BY ONE: build_w,
the stimulus forms, jds_grad, the penalty means with their probe gather, the gradient vector of a step and its update with
per-element bounds -- each entry point against the oracle and never against a forward's tolerance.  Cases, inputs, measures
and tolerances: oracle/gen_step_cases.py (checked without a GPU in tests/test_gen_step_cases.py); nothing here is fitted to
a kernel."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import gen_step_cases as gc

pytestmark = pytest.mark.gpu

INVALID = 1000 + 1                    # SSN_ERR_BASE + hipErrorInvalidValue
RAN = set()                           # the entry points whose test ran to the end
WORST = {}                            # entry -> (largest |got - want| / allowed, case)
_SCRATCH = {}
TD = {True: torch.float32, False: torch.float64}


def _id(c):
    return '-'.join(str(v) for v in c)


def _note(entry, ratio, case):
    ratio = float(ratio)
    print('%s %s: %.3f of the tolerance' % (entry, case, ratio))
    if ratio >= WORST.get(entry, (-1.0, ''))[0]:
        WORST[entry] = (ratio, case)
    return ratio


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype).contiguous()


def _host(t):
    return t.detach().cpu().numpy().astype('float64')


def _shifted(a, dtype, fill=None):
    """A device view of `a`'s shape that starts one element into its allocation (`a`'s values, or `fill`)."""
    a = np.asarray(a)
    flat = torch.full((a.size + 8,), float('nan'), device='cuda', dtype=dtype)
    v = flat[1:1 + a.size].view(*a.shape)
    if fill is None:
        v.copy_(_dev(a, dtype))
    assert v.data_ptr() % (4 * v.element_size()) == v.element_size() and v.is_contiguous()
    return v


def _c4(a, ct):
    return (ct * 4)(*np.asarray(a, dtype='float64').reshape(4))


def _scratch(name, doubles):
    """One zeroed scratch per kernel family for the whole module: the ticket's state belongs to the tests."""
    if name not in _SCRATCH:
        _SCRATCH[name] = torch.zeros(doubles, device='cuda', dtype=torch.float64)
    return _SCRATCH[name]


def _ratio(got, o):
    assert got.shape == o['want'].shape and np.isfinite(got).all()
    return float((np.abs(got - o['want']) / o['allowed']).max())


# ------------------------------------------------------------------ build_w
@pytest.mark.parametrize('c', gc.BUILD_W_CASES, ids=_id)
def test_build_w_elementwise(c):
    """Every element of W against fp64, the named edge elements (first, last, both sides of the sweep boundary) by name; a view
    one element into its allocation takes the scalar path and gives the aligned call's bits; devparams: the bits of
    ssn_build_w_f32 given the same twelve numbers."""
    from tc_gan_amd import clib, weight_gen
    lib = clib.libssnode
    x, o = gc.build_w_inputs(c), gc.build_w_oracle(c)
    fp32 = gc._is32(c.entry)
    td, ct = TD[fp32], (ctypes.c_float if fp32 else ctypes.c_double)
    M = 2 * c.N
    z = _shifted(x['z'], td) if c.shift else _dev(x['z'], td)
    W = _shifted(x['z'], td, fill=True) if c.shift else torch.full((c.B, M, M), float('nan'), device='cuda', dtype=td)
    if c.entry == 'ssn_build_w_devparams_f32':
        p12 = _dev(np.concatenate([x[k].reshape(4) for k in ('J', 'D', 'S')]))
        rc = lib.ssn_build_w_devparams_f32(z.data_ptr(), p12.data_ptr(), W.data_ptr(), c.B, c.N, clib.stream_ptr())
    else:
        rc = getattr(lib, c.entry)(z.data_ptr(), _c4(x['J'], ct), _c4(x['D'], ct), _c4(x['S'], ct), W.data_ptr(), c.B, c.N, clib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    got = _host(W)
    err = np.abs(got - o['want']) / o['allowed']
    for name, g in gc.build_w_named(c).items():
        assert err.reshape(-1)[g] <= 1.0, (name, g, err.reshape(-1)[g])
    r = _note(c.entry, _ratio(got, o), _id(c))
    assert r <= 1.0
    if c.entry == 'ssn_build_w_devparams_f32' or c.shift:       # the bits of the aligned ssn_build_w_f32 / _f64 call
        plain = weight_gen.generate_weight_batch(c.N, x['J'], x['D'], x['S'], _dev(x['z'], td), dtype='float32' if fp32 else 'float64')
        assert torch.equal(plain, W)
    RAN.add(c.entry)


# ------------------------------------------------------------------ stimulus
def _stimulus(c, x):
    from tc_gan_amd import clib, stimuli
    fp32 = gc._is32(c.entry)
    if 'hetero' in c.entry:
        return stimuli.stimulus_batch(x['bw'], x['con'], x['smooth'], c.N, zin=_dev(x['zin']), v=_dev(x['v']))
    if 'amp' in c.entry:
        return stimuli.stimulus_batch(x['bw'], x['con'], x['smooth'], c.N, dtype='float32' if fp32 else 'float64', amp=x['gain'])
    td, ct = TD[fp32], (ctypes.c_float if fp32 else ctypes.c_double)
    ext = torch.full((c.B, c.NB, 2 * c.N), float('nan'), device='cuda', dtype=td)
    bw, con = _dev(x['bw'], td), _dev(x['con'], td)
    rc = getattr(clib.libssnode, c.entry)(bw.data_ptr(), con.data_ptr(), ct(x['smooth']), ext.data_ptr(), c.B, c.NB, c.N, clib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    return ext


@pytest.mark.parametrize('c', gc.STIM_CASES, ids=_id)
def test_stimulus_elementwise(c):
    """Every element against fp64; a zero contrast gives exactly 0; the hetero form gives the bits of the amp form fed the
    float32 gain 1 + fl(v z) made on the host (two roundings)."""
    from tc_gan_amd import stimuli
    x, o = gc.stim_inputs(c), gc.stim_oracle(c)
    ext = _stimulus(c, x)
    got = _host(ext)
    assert (got[o['want'] == 0] == 0).all()
    err = np.abs(got - o['want']) / o['allowed']
    for name, g in gc.stim_named(c).items():
        assert err.reshape(-1)[g] <= 1.0, (name, g)
    r = _note(c.entry, _ratio(got, o), _id(c))
    assert r <= 1.0
    if 'hetero' in c.entry:
        amp = stimuli.stimulus_batch(x['bw'], x['con'], x['smooth'], c.N, amp=gc.hetero_gain(x['v'], x['zin'], c.N))
        assert torch.equal(amp, ext)
    RAN.add(c.entry)


def test_stimulus_hetero_refusals():
    """nv = 3 and a null zin: the invalid-argument status, and ext keeps its bits."""
    from tc_gan_amd import clib
    c = next(k for k in gc.STIM_CASES if 'hetero' in k.entry and k.N == 5)
    x = gc.stim_inputs(c)
    bw, con, zin, v = _dev(x['bw']), _dev(x['con']), _dev(x['zin']), _dev(np.full(3, 0.25))
    ext = torch.full((c.B, c.NB, 10), -7.5, device='cuda')
    fn = clib.libssnode.ssn_stimulus_hetero_f32
    rcs = [fn(bw.data_ptr(), con.data_ptr(), ctypes.c_float(x['smooth']), zin.data_ptr(), v.data_ptr(), 3, ext.data_ptr(), c.B, c.NB, 5, clib.stream_ptr()),
           fn(bw.data_ptr(), con.data_ptr(), ctypes.c_float(x['smooth']), None, v.data_ptr(), 2, ext.data_ptr(), c.B, c.NB, 5, clib.stream_ptr())]
    torch.cuda.synchronize()
    assert rcs == [INVALID, INVALID] and 'invalid argument' in clib.last_error() and bool((ext == -7.5).all())


# ------------------------------------------------------------------ jds_grad
@pytest.mark.parametrize('c', gc.JDS_CASES, ids=_id)
def test_jds_grad_elementwise(c):
    """out[b][pq][t] against fp64 in |delta| / sum |terms|; with gW zero but for one element every out not fed is exactly 0."""
    from tc_gan_amd import genops
    x, res = gc.jds_inputs(c), gc.jds_oracle(c)
    td = TD[gc._is32(c.entry)]
    z = _dev(x['z'], td)
    worst = 0.0
    for k, (gW, o) in enumerate(zip(x['gW'], res)):
        got = _host(genops.jds_grad_parts(_dev(gW, td), z, x['J'], x['D'], x['S']))
        assert got.shape == (c.B, 4, 3) and np.isfinite(got).all()
        assert (got[o['scale'] == 0] == 0).all(), k
        with np.errstate(divide='ignore', invalid='ignore'):
            r = np.where(o['allowed'] > 0, np.abs(got - o['want']) / o['allowed'], 0.0)
        worst = max(worst, float(r.max()))
    assert _note(c.entry, worst, _id(c)) <= 1.0
    RAN.add(c.entry)


# ------------------------------------------------------------------ penalty_means
def _penalty_call(fp32, dyn, rate, sd, sr, ws, probe=None):
    from tc_gan_amd import clib
    td, sfx = TD[fp32], ('f32' if fp32 else 'f64')
    n = len(dyn)
    d, r = (_dev(dyn, td), _dev(rate, td)) if n else (None, None)
    out = torch.full((2,), -7.5, device='cuda', dtype=torch.float64)
    tc = None
    if probe is None:
        rc = getattr(clib.libssnode, 'ssn_penalty_means_' + sfx)(d.data_ptr() if n else None, r.data_ptr() if n else None, n, sd, sr,
                                                                ws.data_ptr(), out.data_ptr(), clib.stream_ptr())
    else:
        ta, ids, probes, NB, M = probe
        t, i, p = _dev(ta, td), _dev(ids, torch.int64), _dev(probes, torch.int64)
        tc = torch.full((len(ids), NB), float('nan'), device='cuda', dtype=td)
        rc = getattr(clib.libssnode, 'ssn_penalty_means_probe_' + sfx)(
            d.data_ptr() if n else None, r.data_ptr() if n else None, n, sd, sr, ws.data_ptr(), out.data_ptr(), t.data_ptr(),
            i.data_ptr() if len(ids) else None, p.data_ptr() if len(ids) else None, tc.data_ptr() if len(ids) else None,
            len(ids), NB, M, clib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    return out.cpu().numpy(), tc


def _check_penalties(entry, fp32, n, call, ws, probe=None):
    dyn, rate, sd, sr = gc.penalty_inputs(n, call, fp32)
    out, tc = _penalty_call(fp32, dyn, rate, sd, sr, ws, probe)
    worst = 0.0
    parts = ws.cpu().numpy()
    for k, (x, s) in enumerate(((dyn, sd), (rate, sr))):
        want, wg = gc.penalty_means_in_order(x, s)
        assert out[k] == want, (n, call, k, out[k], want)                          # bit for bit: the stated order
        assert np.array_equal(parts[k:2 * len(wg):2], wg)                          # and so are the workgroup partials it left
        exact, bound = gc.penalty_bound(x, s)
        assert abs(out[k] - exact) <= bound
        worst = max(worst, abs(out[k] - exact) / bound if bound else 0.0)
    assert parts[2 * gc.PEN_BLOCKS:].view(np.int64)[0] == 0                        # the ticket is back at zero
    _note(entry, worst, 'n%d-call%d' % (n, call))
    return out, tc


@pytest.mark.parametrize('fp32', [True, False], ids=['f32', 'f64'])
@pytest.mark.parametrize('n', gc.PEN_N)
def test_penalty_means_in_order_three_calls_on_one_scratch(n, fp32):
    ws = _scratch('penalty', 2 * gc.PEN_BLOCKS + 1)
    entry = 'ssn_penalty_means_' + ('f32' if fp32 else 'f64')
    for call in range(3):
        _check_penalties(entry, fp32, n, call, ws)
    if n == 0:                       # the wrapper's scales for an empty dynamics row: NaN and 1 / n_rate
        out, _ = _penalty_call(fp32, np.zeros(0), np.zeros(0), float('nan'), 0.125, ws)
        assert math.isnan(out[0]) and out[1] == 0.0 and not math.copysign(1, out[1]) < 0
    RAN.add(entry)


@pytest.mark.parametrize('fp32', [True, False], ids=['f32', 'f64'])
@pytest.mark.parametrize('p', gc.PROBE_CASES, ids=_id)
def test_penalty_means_probe_gathers_and_keeps_the_penalties(p, fp32):
    """tc is bit-equal to the gather (ids and probes collide and are out of order; nsamp NB below 256, above the grid's threads,
    and 0) and the penalties are the bits of the call without a probe."""
    ws = _scratch('penalty', 2 * gc.PEN_BLOCKS + 1)
    entry = 'ssn_penalty_means_probe_' + ('f32' if fp32 else 'f64')
    ta, ids, probes = gc.probe_inputs(p, fp32)
    for call in range(3):
        out, tc = _check_penalties(entry, fp32, p.n, call, ws, probe=(ta, ids, probes, p.NB, p.M))
        assert np.array_equal(_host(tc), gc.probe_gather(ta, ids, probes))
        dyn, rate, sd, sr = gc.penalty_inputs(p.n, call, fp32)
        plain, _ = _penalty_call(fp32, dyn, rate, sd, sr, ws)
        assert np.array_equal(plain, out)
    RAN.add(entry)


# ------------------------------------------------------------------ gen_grads
def _gen_grads(x, ws, out=None, nv=None, M=None, null_ws=False):
    from tc_gan_amd import clib
    nv = x['nv'] if nv is None else nv
    t = dict(parts=_dev(x['parts'], torch.float64), dmean=_dev([x['dmean']]))
    out = torch.full((nv + 13,), float('nan'), device='cuda') if out is None else out
    a = clib.GenGrads(jds_part=t['parts'].data_ptr(), B=int(x['parts'].shape[0]), nv=int(nv), dmean=t['dmean'].data_ptr(),
                      dynamics_cost=x['dynamics_cost'], rate_cost=x['rate_cost'], ws=None if null_ws else ws.data_ptr(), out=out.data_ptr())
    if x['pens'] is not None:
        t['pens'] = _dev(x['pens'], torch.float64)
        a.pens64 = t['pens'].data_ptr()
    if x.get('g_ext') is not None:
        t.update({k: _dev(x[k]) for k in ('g_ext', 'ext_base', 'zin')})
        a.g_ext, a.ext_base, a.zin = (t[k].data_ptr() for k in ('g_ext', 'ext_base', 'zin'))
        a.NB, a.M = int(x['g_ext'].shape[1]), int(x['g_ext'].shape[2] if M is None else M)
    rc = clib.libssnode.ssn_gen_grads_f32(ctypes.byref(a), clib.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize('c', gc.GG_CASES, ids=_id)
def test_gen_grads_order_and_accuracy(c):
    """Three calls on one scratch with inputs whose products are exact: out is the float32 rounding of the fp64 restatement in
    kernel order, bit for bit, and the workgroup partials left in the scratch are its fp64 bits; then free inputs: every output
    within one float32 ulp (plus the fp64 accumulation) of the math.fsum value."""
    ws = _scratch('gen_grads', 2 * gc.GT_BLOCKS + 1)
    for call in range(3):
        x = gc.gen_grads_inputs(c, call, 'exact')
        rc, out = _gen_grads(x, ws)
        assert rc == 0
        want, wg = gc.gen_grads_in_order(x['parts'], x['dmean'], x['pens'], x['dynamics_cost'], x['rate_cost'], c.nv,
                                         x.get('g_ext'), x.get('ext_base'), x.get('zin'))
        assert np.array_equal(out.cpu().numpy(), want), (call, out.cpu().numpy(), want)
        parts = ws.cpu().numpy()
        if wg is not None:
            assert np.array_equal(parts[:2 * len(wg)].reshape(-1, 2), wg)
        assert parts[2 * gc.GT_BLOCKS:].view(np.int64)[0] == 0
    x = gc.gen_grads_inputs(c, 0, 'free')
    rc, out = _gen_grads(x, ws)
    assert rc == 0
    want, allowed = gc.gen_grads_exact(x)
    r = np.abs(_host(out) - want) / allowed
    assert _note('ssn_gen_grads_f32', r.max(), _id(c)) <= 1.0
    RAN.add('ssn_gen_grads_f32')


def test_gen_grads_layout_through_the_wrapper():
    """[dV (nv), dJ (4), dD (4), dS (4), loss]: parts non-zero in one (pq, t) at a time land in out[nv + 4 t + pq] alone; nv = 1 is
    the sum of the two populations' nv = 2 values (small integers: every sum is exact)."""
    from tc_gan_amd import genops
    rs = np.random.RandomState(9)
    g_ext, ext_base = _dev(rs.randint(-8, 9, (2, 3, 10))), _dev(rs.randint(1, 5, (2, 3, 10)))
    zin, dmean, pens = _dev(rs.choice([-1.0, 1.0], (2, 10))), _dev([0.5]), _dev([2.0, 4.0], torch.float64)
    t = _host(g_ext) * _host(ext_base) * _host(zin)[:, None, :]
    vE, vI = t[..., :5].sum(), t[..., 5:].sum()
    assert vE != vI and vE != 0 and vI != 0
    for nv in (0, 1, 2):
        for q in range(4):
            for tt in range(3):
                parts = np.zeros((2, 4, 3))
                parts[:, q, tt] = [1.5, 2.0]
                kw = dict(nv=nv, g_ext=g_ext, ext_base=ext_base, zin=zin) if nv else {}
                out = genops.gen_grads(_dev(parts, torch.float64), dmean, pens, 0.25, 0.5, **kw).cpu().numpy()
                want = np.zeros(nv + 13)
                want[:nv] = [vE + vI] if nv == 1 else [vE, vI][:nv]
                want[nv + 4 * tt + q] = 3.5
                want[nv + 12] = -0.5 + 0.25 * 2.0 + 0.5 * 4.0
                assert np.array_equal(out, want.astype('float32')), (nv, q, tt, out)


def test_gen_grads_refusals():
    """nv = 3, an odd M and a null scratch: the invalid-argument status, out keeps its bits and the ticket stays zero."""
    from tc_gan_amd import clib
    ws = _scratch('gen_grads', 2 * gc.GT_BLOCKS + 1)
    c = next(k for k in gc.GG_CASES if k.nv == 2 and k.B == 1)
    x = gc.gen_grads_inputs(c, 0, 'free')
    out = torch.full((16,), -7.5, device='cuda')
    rcs = [_gen_grads(x, ws, out=out, nv=3)[0], _gen_grads(x, ws, out=out, M=c.M - 1)[0], _gen_grads(x, ws, out=out, null_ws=True)[0]]
    assert rcs == [INVALID] * 3 and 'invalid argument' in clib.last_error()
    assert bool((out == -7.5).all()) and ws.cpu().numpy()[2 * gc.GT_BLOCKS:].view(np.int64)[0] == 0


# ------------------------------------------------------------------ gen_apply
def _opt(rule, step, reserved=0):
    from tc_gan_amd import clib
    h = gc.APPLY_HYPER
    return clib.OptParams(kind=gc.RULES.index(rule), step=step, clip=0, reserved=reserved, learning_rate=gc.APPLY_LR, beta1=h['beta1'],
                          beta2=h['beta2'], epsilon=h['epsilon_adam'] if rule == 'adam' else h['epsilon_rmsprop'], rho=h['rho'])


def _apply(t, n, opt, record=True, lo=True, hi=True, grads=None):
    from tc_gan_amd import clib
    rc = clib.libssnode.ssn_gen_apply_f32(t['p'].data_ptr(), (t['g'] if grads is None else grads).data_ptr(), t['s1'].data_ptr(), t['s2'].data_ptr(), n,
                                          ctypes.byref(opt), t['lo'].data_ptr() if lo else None, t['hi'].data_ptr() if hi else None,
                                          t['rec'].data_ptr() if record else None, clib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _apply_state(c, x, s1=None, s2=None):
    n = c.n
    return dict(p=_dev(x['p0']), g=_dev(x['g'][0]), s1=_dev(np.zeros(n) if s1 is None else s1), s2=_dev(np.zeros(n) if s2 is None else s2),
                lo=_dev(x['lo']), hi=_dev(x['hi']), rec=torch.full((n + 1,), -7.5, device='cuda'))


@pytest.mark.parametrize('c', gc.APPLY_CASES, ids=_id)
def test_gen_apply_two_steps_with_per_element_bounds(c):
    """Two consecutive steps against the fp64 update followed by the clip: a clipped element equals its bound exactly (lo == hi for
    element 2), the others and the moments lie within the optimizer test's tolerance; record[:n] holds the new parameters' bits
    and record[n] is grads[n]."""
    x, tr = gc.apply_inputs(c), gc.apply_trace(c, gc.apply_inputs(c))
    t = _apply_state(c, x)
    worst = 0.0
    for k, s in enumerate(tr['steps']):
        t['g'] = _dev(x['g'][k])
        assert _apply(t, c.n, _opt(c.rule, k + 1)) == 0
        got = _host(t['p'])
        clipped = s['where'] != 0
        assert np.array_equal(got[clipped], np.where(s['where'] < 0, x['lo'], x['hi'])[clipped]) and got[2] == 0.25
        assert (s['where'] == 0).any() and clipped.any()
        r = np.abs(got - s['p']) / gc.apply_tol(s['p'])
        worst = max(worst, float(r.max()))
        assert r.max() <= 1.0, (k, int(r.argmax()))
        for name, want in (('s1', s['m']), ('s2', s['v'])):
            if want is not None:
                assert (np.abs(_host(t[name]) - want) <= gc.apply_tol(want)).all(), (k, name)
        rec = t['rec'].cpu().numpy()
        assert np.array_equal(rec[:c.n], t['p'].cpu().numpy()) and rec[c.n] == np.float32(x['g'][k][c.n])
    _note('ssn_gen_apply_f32', worst, _id(c))
    RAN.add('ssn_gen_apply_f32')


@pytest.mark.parametrize('rule', gc.RULES)
@pytest.mark.parametrize('n', [13, 14, 15])
def test_gen_apply_non_finite_gate(n, rule):
    """`reserved` bit 0 with a NaN, then an Inf, in the first, a middle and the last gradient element: parameters and both moments
    keep their bits, record[:n] holds the old parameters and record[n] is NaN.  Gate off, the same gradient: that element
    becomes what the fp64 update gives -- NaN, never a bound, for a NaN gradient under every rule and for an Inf under adam and
    rmsprop (inf / inf); sgd sends an Inf to -inf, which the clip takes to lo -- and the others update.  (The gate is defined for
    vectors of at most 64 elements with a record, ssn_opt_params.reserved: it runs at the sizes of the real vectors.)"""
    c = gc.Apply(n, rule)
    x = gc.apply_inputs(c)
    rs = np.random.RandomState(n)
    s1, s2 = gc._f32(np.abs(rs.randn(n)) * 0.1 if rule == 'rmsprop' else rs.randn(n) * 0.1), gc._f32(rs.rand(n) * 0.1)
    for bad in (float('nan'), float('inf')):
        for pos in (0, n // 2, n - 1):
            g = x['g'][0].copy()
            g[pos] = bad
            t = _apply_state(c, x, s1, s2)
            t['g'] = _dev(g)
            old = {k: t[k].clone() for k in ('p', 's1', 's2')}
            assert _apply(t, n, _opt(rule, 3, reserved=1)) == 0
            assert all(torch.equal(t[k].view(torch.int32), old[k].view(torch.int32)) for k in old)
            rec = t['rec'].cpu().numpy()
            assert np.array_equal(rec[:n], old['p'].cpu().numpy()) and math.isnan(rec[n])
            # gate off
            t = _apply_state(c, x, s1, s2)
            t['g'] = _dev(g)
            assert _apply(t, n, _opt(rule, 3)) == 0
            state = dict(t=2, m=s1.copy(), v=s2.copy(), a=s1.copy())
            _, want = gc.apply_step(rule, x['p0'], g[:n], state, x['lo'], x['hi'])
            got = _host(t['p'])
            assert np.array_equal(np.isnan(got), np.isnan(want))
            assert math.isnan(want[pos]) == (math.isnan(bad) or rule != 'sgd') and (math.isnan(want[pos]) or got[pos] == x['lo'][pos])
            ok = ~np.isnan(want)
            assert (np.abs(got[ok] - want[ok]) <= gc.apply_tol(want[ok])).all() and ok.sum() >= n - 1
            assert np.array_equal(t['rec'].cpu().numpy()[:n], t['p'].cpu().numpy(), equal_nan=True)


def test_gen_apply_without_a_record_does_not_use_the_tail():
    """A null record: grads[n] is a NaN guard -- with `reserved` set as well -- and parameters and moments come out finite and
    bit-equal to a call that records a finite tail."""
    c = gc.Apply(13, 'adam')
    x = gc.apply_inputs(c)
    g = x['g'][0].copy()
    a, b = _apply_state(c, x), _apply_state(c, x)
    g[c.n] = float('nan')
    a['g'] = _dev(g)
    assert _apply(a, c.n, _opt('adam', 1, reserved=1), record=False) == 0
    assert _apply(b, c.n, _opt('adam', 1)) == 0
    assert all(torch.equal(a[k], b[k]) and bool(torch.isfinite(a[k]).all()) for k in ('p', 's1', 's2'))
    assert bool((a['rec'] == -7.5).all()) and math.isnan(float(a['g'][c.n]))


def test_gen_apply_refusals():
    """n = 0, and lo given without hi (or hi without lo): the invalid-argument status, nothing is written."""
    from tc_gan_amd import clib
    c = gc.Apply(13, 'sgd')
    x = gc.apply_inputs(c)
    t = _apply_state(c, x)
    old = t['p'].clone()
    rcs = [_apply(t, 0, _opt('sgd', 1)), _apply(t, c.n, _opt('sgd', 1), hi=False), _apply(t, c.n, _opt('sgd', 1), lo=False)]
    assert rcs == [INVALID] * 3 and 'invalid argument' in clib.last_error()
    assert torch.equal(t['p'], old) and bool((t['rec'] == -7.5).all())


def test_zz_every_entry_ran_to_the_end_and_the_largest_figures():
    """(Runs last in the module.)  Every entry point of the coverage list was called directly and its test ran to the end;
    prints, per entry, the largest error as a fraction of its tolerance.  Meaningful only after the tests above, in the same
    process; it launches nothing itself."""
    for entry in gc.ENTRIES:
        if entry in WORST:
            print('%-32s largest error %.2g of its tolerance (%s)' % ((entry,) + WORST[entry]))
    missing = [e for e in gc.ENTRIES if e not in RAN]
    assert not missing, 'never ran to the end: %r' % (missing,)

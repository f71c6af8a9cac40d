"""The six segmented kernels of an ensemble step (csrc/ssn_ensemble.hip) held to the fp64 restatements of
oracle/ens_step_cases.py ONE BY ONE, at every loop and member edge: the moment sums and loss gradient, the chain rule through
make_W, the gradient assembly (with its own L0 and with a given one), the optimizer and the heterogeneous-input stimulus --
each entry point against the oracle, and against its single-run counterpart where one exists.  Cases, inputs, measures and
tolerances: oracle/ens_step_cases.py (checked without a GPU in tests/test_ens_step_cases.py); nothing here is fitted to a
kernel."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import ens_step_cases as ec
from oracle import gen_step_cases as gc

pytestmark = pytest.mark.gpu

INVALID = 1000 + 1                    # SSN_ERR_BASE + hipErrorInvalidValue
GUARD = -7.5                          # what a word nobody may write holds
RAN = set()                           # the entry points whose test ran to the end
WORST = {}                            # entry -> (largest |got - want| / allowed, case)
F32, F64 = torch.float32, torch.float64


def _id(c):
    return '-'.join(str(v) for v in c)


def _note(entry, ratio, case):
    ratio = float(ratio)
    print('%s %s: %.3f of the tolerance' % (entry, case, ratio))
    if ratio >= WORST.get(entry, (-1.0, ''))[0]:
        WORST[entry] = (ratio, case)
    return ratio


def _dev(a, dtype=F32):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype).contiguous()


def _host(t):
    return t.detach().cpu().numpy().astype('float64')


def _ratio(got, want, allowed):
    assert got.shape == want.shape and np.isfinite(got).all()
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.where(allowed > 0, np.abs(got - want) / allowed, np.where(got == want, 0.0, np.inf)).max())


def _lib():
    from tc_gan_amd import clib
    return clib, clib.libssnode


# ------------------------------------------------------------------ moments
def _moments(c, x, xdev=None):
    clib, lib = _lib()
    K, B, D = c.K, c.B, c.D
    R = int(lib.ssn_ens_record_doubles(D, 12)) + 2
    t = dict(x=_dev(x['x']) if xdev is None else xdev, dm=_dev(x['dm'], F64), w=_dev(x['w'], F64),
             rec=torch.full((K, R), GUARD, device='cuda', dtype=F64), sums=torch.full((K, 2, D), GUARD, device='cuda', dtype=F64),
             gx=torch.full((K * B, D), GUARD, device='cuda'))
    rc = lib.ssn_ens_moments_f32(t['x'].data_ptr(), K, B, D, t['sums'].data_ptr(), t['dm'].data_ptr(), t['w'].data_ptr(),
                                 t['gx'].data_ptr(), t['rec'].data_ptr(), R, clib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    return t


@pytest.mark.parametrize('c', ec.MOM_CASES, ids=_id)
def test_moments_sums_in_order_and_loss_gradient_elementwise(c):
    """sums bit for bit the in-order restatement; m, s of the record and every gx against fp64 from exactly summed inputs; the
    record words outside [1, 1 + 2 D) of every row keep their bits."""
    x, o = ec.mom_inputs(c), ec.mom_oracle(c)
    t = _moments(c, x)
    D = c.D
    assert np.array_equal(t['sums'].cpu().numpy(), ec.moment_sums_in_order(x['x'], c.K, c.B, D))
    rec = t['rec'].cpu().numpy()
    assert (rec[:, 0] == GUARD).all() and (rec[:, 1 + 2 * D:] == GUARD).all()
    r = max(_ratio(rec[:, 1:1 + D], o['m'], o['allowed_m']), _ratio(rec[:, 1 + D:1 + 2 * D], o['s'], o['allowed_s']),
            _ratio(_host(t['gx']), o['gx'], o['allowed_gx']))
    assert _note(ec.ENTRIES[0], r, _id(c)) <= 1.0
    RAN.add(ec.ENTRIES[0])


def test_moments_nan_past_row_256_stays_in_its_member_and_channel():
    c = ec.Mom(3, 257, 7, 'free')
    x = ec.mom_inputs(c)
    clean = _moments(c, x)
    bad = x['x'].copy()
    bad[c.B + 256, 3] = float('nan')                      # member 1's last row: the second trip of the strided loops
    t = _moments(c, x, xdev=_dev(bad))
    hit = np.zeros((c.K, c.D), dtype=bool)
    hit[1, 3] = True
    for name, shape in (('sums', (c.K, 2, c.D)), ('gx', (c.K, c.B, c.D))):
        got, ref = t[name].cpu().numpy().reshape(shape), clean[name].cpu().numpy().reshape(shape)
        mask = np.broadcast_to(hit[:, None, :], shape)
        assert np.isnan(got[mask]).all() and np.array_equal(got[~mask], ref[~mask])
    rec, ref = t['rec'].cpu().numpy(), clean['rec'].cpu().numpy()
    assert np.isnan(rec[1, [1 + 3, 1 + c.D + 3]]).all() and np.isnan(rec).sum() == 2
    assert np.array_equal(rec[~np.isnan(rec)], ref[~np.isnan(rec)])


# ------------------------------------------------------------------ jds_grad
@pytest.mark.parametrize('c', ec.JDS_CASES, ids=_id)
def test_jds_grad_elementwise_with_the_members_parameters(c):
    """out[b][pq][t] against fp64 with the parameters of the draw's member, four distinct entries per member; bit-equal to the
    single-run kernel per member; with gW zero but for one element every out not fed is exactly 0."""
    from tc_gan_amd import genops
    from tc_gan_amd.networks.moment_matching_ensemble import _jds16
    clib, lib = _lib()
    x, res = ec.ens_jds_inputs(c), ec.ens_jds_oracle(c)
    nb = c.K * c.B
    p16 = np.stack([ec.jds16(*p) for p in x['jds']])
    assert np.array_equal(p16, np.stack([_jds16(*p) for p in x['jds']]))
    p16, z = _dev(p16), _dev(x['z'])
    worst = 0.0
    for k, (gW, o) in enumerate(zip(x['gW'], res)):
        g = _dev(gW)
        out = torch.full((nb, 4, 3), float('nan'), device='cuda', dtype=F64)
        rc = lib.ssn_ens_jds_grad_f32(g.data_ptr(), z.data_ptr(), p16.data_ptr(), out.data_ptr(), c.K, c.B, c.N, clib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        got = _host(out)
        assert (got[o['scale'] == 0] == 0).all(), k
        worst = max(worst, _ratio(got, o['want'], o['allowed']))
        if c.gw == 'free' or k % 3 == 2:
            for m, sl in enumerate(ec._rows(c.K, c.B)):
                solo = genops.jds_grad_parts(g[sl].contiguous(), z[sl].contiguous(), *x['jds'][m])
                assert torch.equal(solo, out[sl]), (k, m)
    assert _note(ec.ENTRIES[1], worst, _id(c)) <= 1.0
    RAN.add(ec.ENTRIES[1])


# ------------------------------------------------------------------ gen_grads
def _gen_grads(c, x, D=None, g_ext=None, with_l0=None):
    """(rc, grads (K, P), rec (K, stride) as numpy, the stride's first free word)."""
    clib, lib = _lib()
    K, B, nv = c.K, c.B, c.nv
    D = c.D if D is None else D
    P = nv + 12
    R = int(lib.ssn_ens_record_doubles(D, P))
    stride = R + 3
    t = dict(parts=_dev(x['parts'], F64), dyn=_dev(x['dyn']), rate=_dev(x['rate']), costs=_dev(x['costs'], F64),
             grads=torch.full((K, P), GUARD, device='cuda'), rec=torch.full((K, stride), GUARD, device='cuda', dtype=F64))
    a = clib.EnsGrads(K=K, B=B, nv=nv, NB=c.NB, M=c.M, D=D, part=t['parts'].data_ptr(), dyn_row=t['dyn'].data_ptr(),
                      rate_row=t['rate'].data_ptr(), scale_dyn=x['scale_dyn'], scale_rate=x['scale_rate'], costs=t['costs'].data_ptr(),
                      grads=t['grads'].data_ptr(), rec=t['rec'].data_ptr(), rstride=stride)
    if nv:
        t.update(g_ext=_dev(x['g_ext'] if g_ext is None else g_ext), ext_base=_dev(x['ext_base']), zin=_dev(x['zin']))
        a.g_ext, a.ext_base, a.zin = (t[k].data_ptr() for k in ('g_ext', 'ext_base', 'zin'))
    l0 = (c.entry == ec.ENTRIES[3]) if with_l0 is None else with_l0
    if 'dm' in x:
        t.update(dm=_dev(x['dm'], F64), w=_dev(x['w'], F64))
        if not l0:
            a.data_moments, a.weights = t['dm'].data_ptr(), t['w'].data_ptr()
        if D:
            t['rec'][:, 1:1 + 2 * D] = _dev(x['mom'], F64)
    if l0:
        t['l0'] = _dev(x['l0'], F64) if 'l0' in x else torch.zeros(K, device='cuda', dtype=F64)
        rc = lib.ssn_ens_gen_grads_l0_f32(ctypes.byref(a), t['l0'].data_ptr(), clib.stream_ptr())
    else:
        rc = lib.ssn_ens_gen_grads_f32(ctypes.byref(a), clib.stream_ptr())
    torch.cuda.synchronize()
    return rc, t['grads'].cpu().numpy(), t['rec'].cpu().numpy(), R


def _check_record_frame(c, x, rec, R):
    """rec[k][1 .. 2 D] is read and not written; the words from 4 + 2 D on (the optimizer's, and past the record) keep theirs."""
    D = c.D
    if D:
        assert np.array_equal(rec[:, 1:1 + 2 * D], x['mom'])
    assert (rec[:, 4 + 2 * D:] == GUARD).all() and R == 4 + 2 * D + 2 * (c.nv + 12)


@pytest.mark.parametrize('c', ec.GG_CASES, ids=_id)
def test_gen_grads_order_and_accuracy(c):
    """Lattice inputs (every product exact): grads, L0, both penalties and the loss bit for bit the fp64 restatement in kernel
    order.  Free inputs: the penalties still bit for bit (and the float32 roundings of the means), grads within one float32 ulp
    of the math.fsum value, L0 within its derived fp64 bound, the loss formed from the record's own ROUNDED penalties."""
    x = ec.gg_inputs(c, 'exact')
    rc, grads, rec, R = _gen_grads(c, x)
    assert rc == 0
    o = ec.gen_grads_in_order(c, x)
    D = c.D
    assert np.array_equal(grads, o['grads']), (grads, o['grads'])
    assert np.array_equal(rec[:, 0], o['L0']) and np.array_equal(rec[:, 1 + 2 * D], o['dyn']) and np.array_equal(rec[:, 2 + 2 * D], o['rate'])
    assert np.array_equal(rec[:, 3 + 2 * D], o['loss'])
    _check_record_frame(c, x, rec, R)
    x = ec.gg_inputs(c, 'free')
    rc, grads, rec, R = _gen_grads(c, x)
    assert rc == 0
    o, ex = ec.gen_grads_in_order(c, x), ec.gen_grads_exact(c, x)
    fd, fr = rec[:, 1 + 2 * D], rec[:, 2 + 2 * D]
    assert np.array_equal(fd, o['dyn']) and np.array_equal(fr, o['rate'])
    assert np.array_equal(fd, fd.astype('float32').astype('float64')) and np.array_equal(fr, fr.astype('float32').astype('float64'))
    for got, k in ((fd, 'dyn'), (fr, 'rate')):
        assert (np.abs(got - ex[k]) <= ec.U * np.abs(ex[k]) * (1 + 1e-6)).all()
    r = _ratio(grads.astype('float64'), ex['grads'], ex['grads_allowed'])
    if D:
        r = max(r, _ratio(rec[:, 0], ex['L0'], ex['L0_allowed']))
    else:
        assert np.array_equal(rec[:, 0], x['l0'])
    loss = rec[:, 0] + x['costs'][:, 0] * fd + x['costs'][:, 1] * fr
    r = max(r, _ratio(rec[:, 3 + 2 * D], loss, ec.loss_allowed(rec[:, 0], x['costs'], fd, fr)))
    _check_record_frame(c, x, rec, R)
    assert _note(c.entry, r, _id(c)) <= 1.0
    RAN.add(c.entry)


@pytest.mark.parametrize('entry', ec.ENTRIES[2:4])
def test_gen_grads_one_hot_on_each_side_of_the_population_split(entry):
    """nv = 2: g_ext zero but for one element of member 1 at m = N - 1, then at m = N: dV_E, then dV_I, of member 1 alone."""
    c = next(k for k in ec.GG_CASES if k.entry == entry and k.nv == 2 and k.K == 3 and k.M == 18)
    x = ec.gg_inputs(c, 'exact')
    N = c.M // 2
    b, s = c.B + 1, 3                                       # a draw of member 1; e = (1 NB + 3) M + m > 64: past one wavefront
    for m, slot in ((N - 1, 0), (N, 1)):
        g = np.zeros_like(x['g_ext'])
        g[b, s, m] = 0.75
        rc, grads, _, _ = _gen_grads(c, x, g_ext=g)
        assert rc == 0
        want = np.zeros((c.K, 2), dtype='float32')
        want[1, slot] = np.float32(0.75 * x['ext_base'][b, s, m] * x['zin'][b, m])
        assert want[1, slot] != 0 and np.array_equal(grads[:, :2], want), (m, grads[:, :2])


def test_gen_grads_refuses_a_record_without_moments_and_names_the_entry_that_takes_it():
    """D = 0 in ssn_ens_gen_grads_f32 (L0 = 0 / 0): the invalid-argument status with the l0 entry's name; nothing is written."""
    clib, _ = _lib()
    c = next(k for k in ec.GG_CASES if k.entry == ec.ENTRIES[2] and k.nv == 1 and k.B == 1)
    x = ec.gg_inputs(c, 'free')
    rc, grads, rec, _ = _gen_grads(c, x, D=0)
    assert rc == INVALID and 'ssn_ens_gen_grads_l0_f32' in clib.last_error()
    assert (grads == GUARD).all() and (rec == GUARD).all()
    rc, grads, rec, _ = _gen_grads(c, dict(x, l0=np.arange(3.0)), D=0, with_l0=True)          # ... which does take it
    assert rc == 0 and np.array_equal(rec[:, 0], np.arange(3.0)) and np.isfinite(rec[:, :4]).all()


# ------------------------------------------------------------------ apply
def _hyp(c, x, step):
    h = np.zeros((c.K, 8), dtype='float32')
    h[:, 0] = x['hyp'][:, 0]
    h[:, 1] = [np.float32(ec.adam_a_t(float(lr), step)) for lr in x['hyp'][:, 0]]
    h[:, 2:6] = x['hyp'][:, 1:]
    return h


def _apply_state(c, x, scalar_clip=False):
    n = c.K * c.P
    lo, hi = (np.full(n, x['lo'].min()), np.full(n, x['hi'].max())) if scalar_clip else (x['lo'], x['hi'])
    return dict(p=_dev(x['p0']), s1=torch.zeros(n, device='cuda'), s2=torch.zeros(n, device='cuda'), lo=_dev(lo), hi=_dev(hi),
                rec=torch.full((c.K, 4 + 2 * c.P + 1), GUARD, device='cuda', dtype=F64))


def _apply(c, x, t, g, step, kind=None, P=None, rstride=None, s2=True):
    clib, lib = _lib()
    h = ec.APPLY_HYPER
    t['hyp'], t['g'] = _dev(_hyp(c, x, step)), _dev(g)
    o = clib.EnsApply(K=c.K, P=c.P if P is None else P, kind=gc.RULES.index(c.rule) if kind is None else kind, beta1=h['beta1'],
                      beta2=h['beta2'], eps=h['epsilon_adam'] if c.rule == 'adam' else h['epsilon_rmsprop'], rho=h['rho'],
                      hyp=t['hyp'].data_ptr(), clip_lo=t['lo'].data_ptr(), clip_hi=t['hi'].data_ptr(), p=t['p'].data_ptr(),
                      s1=t['s1'].data_ptr(), s2=t['s2'].data_ptr() if s2 else None, g=t['g'].data_ptr(), rec=t['rec'].data_ptr(),
                      rstride=t['rec'].shape[1] if rstride is None else rstride, rec_off=4)
    rc = lib.ssn_ens_apply_f32(ctypes.byref(o), clib.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('c', ec.APPLY_CASES, ids=_id)
def test_apply_two_steps_with_regularisation_and_per_element_bounds(c):
    """Two consecutive steps (the moments carry) with the member's learning rate, a_t and four nonzero regularisation weights
    against the fp64 trace: a clipped element equals its bound exactly, the others and the moments lie within the optimizer
    test's tolerance; rec[i] holds the new parameter's bits and rec[P + i] the gradient AS HANDED IN."""
    x, tr = ec.apply_inputs(c), ec.apply_trace(c, ec.apply_inputs(c))
    t = _apply_state(c, x)
    P = c.P
    worst = 0.0
    for k, s in enumerate(tr['steps']):
        assert _apply(c, x, t, x['g'][k], k + 1) == 0
        got = _host(t['p'])
        clipped = s['where'] != 0
        assert np.array_equal(got[clipped], np.where(s['where'] < 0, x['lo'], x['hi'])[clipped]) and got[2] == 0.25
        worst = max(worst, _ratio(got, s['p'], ec.apply_tol(s['p'])))
        for name, want in (('s1', s['m']), ('s2', s['v'])):
            if want is not None:
                worst = max(worst, _ratio(_host(t[name]), want, ec.apply_tol(want)))
            else:
                assert bool((t[name] == 0).all())                  # sgd has no state, rmsprop one
        rec = t['rec'].cpu().numpy()
        assert np.array_equal(rec[:, 4:4 + P].reshape(-1), got)
        assert np.array_equal(rec[:, 4 + P:4 + 2 * P].reshape(-1), x['g'][k])
        assert (rec[:, :4] == GUARD).all() and (rec[:, 4 + 2 * P:] == GUARD).all()
    assert _note(ec.ENTRIES[4], worst, _id(c)) <= 1.0
    RAN.add(ec.ENTRIES[4])


@pytest.mark.parametrize('rule', gc.RULES)
def test_apply_with_scalar_bounds_is_the_single_run_optimizer_bit_for_bit(rule):
    """Per member the bits of ssn_optimizer_step with the same nonzero regularisation weights, over two steps, under every rule."""
    clib, lib = _lib()
    c = ec.EnsApply(3, 13, rule)
    x = ec.apply_inputs(c)
    tr = ec.apply_trace(c, x, scalar_clip=True)
    t = _apply_state(c, x, scalar_clip=True)
    h = ec.APPLY_HYPER
    solo = [dict(p=_dev(x['p0'][k * c.P:(k + 1) * c.P]), s1=torch.zeros(c.P, device='cuda'), s2=torch.zeros(c.P, device='cuda')) for k in range(c.K)]
    for step, s in enumerate(tr['steps'], 1):
        assert _apply(c, x, t, x['g'][step - 1], step) == 0
        assert _ratio(_host(t['p']), s['p'], ec.apply_tol(s['p'])) <= 1.0
        for k, q in enumerate(solo):
            lr, l2p, l1p, l2d, l1d = (float(v) for v in x['hyp'][k])
            op = clib.OptParams(kind=gc.RULES.index(rule), step=step, clip=1, reserved=0, learning_rate=lr, beta1=h['beta1'], beta2=h['beta2'],
                                epsilon=h['epsilon_adam'] if rule == 'adam' else h['epsilon_rmsprop'], rho=h['rho'], reg_l2_penalty=l2p,
                                reg_l1_penalty=l1p, reg_l2_decay=l2d, reg_l1_decay=l1d, clip_lo=float(x['lo'].min()), clip_hi=float(x['hi'].max()))
            gk = _dev(x['g'][step - 1][k * c.P:(k + 1) * c.P])
            clib.check(lib.ssn_optimizer_step(q['p'].data_ptr(), gk.data_ptr(), q['s1'].data_ptr(), q['s2'].data_ptr(), c.P, ctypes.byref(op),
                                              clib.stream_ptr()), 'ssn_optimizer_step')
            torch.cuda.synchronize()
            for name in ('p', 's1', 's2'):
                assert torch.equal(t[name][k * c.P:(k + 1) * c.P], q[name]), (step, k, name)


def test_apply_nan_gradient_element_poisons_that_element_alone():
    """After one clean step, a NaN in one gradient element of member 1: that parameter and its moments become NaN; every other
    element of every member has the bits of the clean second step."""
    c = ec.EnsApply(3, 13, 'adam')
    x = ec.apply_inputs(c)
    runs = []
    e = c.P + 5
    for poison in (False, True):
        t = _apply_state(c, x)
        assert _apply(c, x, t, x['g'][0], 1) == 0
        g = x['g'][1].copy()
        if poison:
            g[e] = float('nan')
        assert _apply(c, x, t, g, 2) == 0
        runs.append({k: t[k].cpu().numpy() for k in ('p', 's1', 's2', 'rec')})
    clean, bad = runs
    keep = np.arange(c.K * c.P) != e
    for name in ('p', 's1', 's2'):
        assert math.isnan(bad[name][e]) and np.array_equal(bad[name][keep], clean[name][keep]) and np.isfinite(clean[name]).all()
    rec = bad['rec']
    assert np.isnan(rec).sum() == 2 and math.isnan(rec[1, 4 + 5]) and math.isnan(rec[1, 4 + c.P + 5])


def test_apply_refusals():
    """kind 3, P = 0, a row stride one short of rec_off + 2 P, and Adam without its second moments: the invalid-argument status,
    nothing is written."""
    clib, _ = _lib()
    c = ec.EnsApply(3, 13, 'adam')
    x = ec.apply_inputs(c)
    t = _apply_state(c, x)
    rcs = [_apply(c, x, t, x['g'][0], 1, kind=3), _apply(c, x, t, x['g'][0], 1, P=0), _apply(c, x, t, x['g'][0], 1, rstride=4 + 2 * c.P - 1),
           _apply(c, x, t, x['g'][0], 1, s2=False)]
    assert rcs == [INVALID] * 4 and 'invalid argument' in clib.last_error()
    assert np.array_equal(t['p'].cpu().numpy(), x['p0'].astype('float32')) and bool((t['rec'] == GUARD).all())
    assert bool((t['s1'] == 0).all()) and bool((t['s2'] == 0).all())


# ------------------------------------------------------------------ stimulus
def _ens_stimulus(c, x, v=None):
    clib, lib = _lib()
    t = dict(bw=_dev(x['bw']), con=_dev(x['con']), zin=_dev(x['zin']), v=_dev(x['v'] if v is None else v))
    ext = torch.full((c.K * c.B, c.NB, 2 * c.N), float('nan'), device='cuda')
    rc = lib.ssn_ens_stimulus_hetero_f32(t['bw'].data_ptr(), t['con'].data_ptr(), ctypes.c_float(x['smooth']), t['zin'].data_ptr(),
                                         t['v'].data_ptr(), ext.data_ptr(), c.K, c.B, c.NB, c.N, clib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    return ext, t


@pytest.mark.parametrize('c', ec.STIM_CASES, ids=_id)
def test_stimulus_hetero_elementwise_with_the_members_v(c):
    """Generic zin in (-1, 1): every element against fp64 with the gain 1 + fl(v z) of the draw's member (both sides of the sweep
    boundary of the capped grid by name); per member the bits of ssn_stimulus_hetero_f32 and of the amp form fed the
    two-rounding gain made on the host -- a product contracted into the addition breaks both."""
    from tc_gan_amd import stimuli
    x, o = ec.ens_stim_inputs(c), ec.ens_stim_oracle(c)
    ext, t = _ens_stimulus(c, x)
    got = _host(ext)
    err = (np.abs(got - o['want']) / o['allowed']).reshape(-1)
    named = dict(first=0, last=err.size - 1)
    if err.size > ec.STIM_SWEEP:
        named.update({'sweep0-last': ec.STIM_SWEEP - 1, 'sweep1-first': ec.STIM_SWEEP})
    for name, g in named.items():
        assert err[g] <= 1.0, (name, g, err[g])
    assert _note(ec.ENTRIES[5], _ratio(got, o['want'], o['allowed']), _id(c)) <= 1.0
    for k, sl in enumerate(ec._rows(c.K, c.B)):
        solo = stimuli.stimulus_batch(x['bw'][sl], x['con'][sl], x['smooth'], c.N, zin=t['zin'][sl].contiguous(), v=t['v'][k].contiguous())
        assert torch.equal(solo, ext[sl]), k
    amp = stimuli.stimulus_batch(x['bw'], x['con'], x['smooth'], c.N, amp=x['gain'])
    assert torch.equal(amp, ext)
    RAN.add(ec.ENTRIES[5])


def test_stimulus_hetero_non_finite_v_stays_in_its_member():
    c = ec.STIM_CASES[1]
    x = ec.ens_stim_inputs(c)
    clean, _ = _ens_stimulus(c, x)
    v = x['v'].copy()
    v[1] = [float('inf'), float('nan')]
    ext, _ = _ens_stimulus(c, x, v=v)
    sl = ec._rows(c.K, c.B)[1]
    keep = np.ones(c.K * c.B, dtype=bool)
    keep[sl] = False
    got, ref = ext.cpu().numpy(), clean.cpu().numpy()
    assert not np.isfinite(got[sl]).any() and np.array_equal(got[keep], ref[keep]) and np.isfinite(ref).all()


def test_zz_every_entry_ran_to_the_end_and_the_largest_figures():
    """(Runs last in the module.)  Every entry point of the coverage list was called directly and its test ran to the end;
    prints, per entry, the largest error as a fraction of its tolerance.  Meaningful only after the tests above, in the same
    process; it launches nothing itself."""
    for entry in ec.ENTRIES:
        if entry in WORST:
            print('%-32s largest error %.2g of its tolerance (%s)' % ((entry,) + WORST[entry]))
    missing = [e for e in ec.ENTRIES if e not in RAN]
    assert not missing, 'never ran to the end: %r' % (missing,)

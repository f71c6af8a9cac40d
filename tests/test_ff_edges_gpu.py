"""The feed-forward kernels (tc_gan_amd/csrc/ssn_ff.hip) held to the fp64 oracle of oracle/ff_cases.py ELEMENT BY ELEMENT at
every grid and list edge: den, q, out of the dense and of the connection-list forward, dsig of the two second passes (through
the C ABI, on the oracle's q and den rounded to float32, one gq pattern per group of stimuli), each entry point against the
oracle and never against another.  Cases, inputs, measures and tolerances: oracle/ff_cases.py (checked without a GPU in
tests/test_ff_cases.py); nothing here is fitted to a kernel."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ff_cases as fc

pytestmark = pytest.mark.gpu

INVALID = 1000 + 1                    # SSN_ERR_BASE + hipErrorInvalidValue
RAN = set()                           # the cases that ran in this session
WORST = {}                            # (quantity, path) -> (largest error, largest share of a tolerance, case)


def _note(c, quantity, err, tol):
    RAN.add(c)
    err = float(np.max(err))
    used = err / tol if tol > 0 else 0.0
    print('%s %s: %.2e of %.2e (%.2f)' % (fc.case_id(c), quantity, err, tol, used))
    old = WORST.get((quantity, c.path), (0.0, 0.0, ''))
    WORST[(quantity, c.path)] = (max(old[0], err), max(old[1], used), fc.case_id(c) if used >= old[1] else old[2])
    return err


def _forward(c, x, keep=True):
    from tc_gan_amd import ff_model
    if c.entry in ('forward', 'backward'):
        return ff_model.ff_forward(x['params'], x['RF_w'], x['FF_con'], x['FF_str'], x['TH_sam'], x['stim'], c.box, keep=keep)
    return ff_model.ff_forward_sparse(x['params'], x['RF_w'], x['idx'], x['str'], x['TH_sam'], x['stim'], c.box, keep=keep)


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype).contiguous()


def _ff_params(c, x, **over):
    from tc_gan_amd import clib
    kw = dict(nsam=c.nsam, nhid=c.nhid, ni=c.ni, box=c.box, **x['val'])
    kw.update(over)
    return clib.FFParams(**kw)


def _second_pass(c, x, q, den, gq, fp=None):
    """`ssn_ff_backward_f32` / `ssn_ff_backward_sparse_f32` through the C ABI: (status, dsig (nsam, nhid, 2))."""
    from tc_gan_amd import clib
    lib = clib.libssnode
    fp = fp or _ff_params(c, x)
    t = dict(RF_w=_dev(x['RF_w']), stim=_dev(x['stim']), q=_dev(q), den=_dev(den), gq=_dev(gq))
    dsig = torch.full((c.nsam, c.nhid, 2), float('nan'), device='cuda', dtype=torch.float32)
    if c.entry == 'backward':
        t.update(con=_dev(x['FF_con']), strn=_dev(x['FF_str']))
        rc = lib.ssn_ff_backward_f32(t['RF_w'].data_ptr(), t['con'].data_ptr(), t['strn'].data_ptr(), t['stim'].data_ptr(), t['q'].data_ptr(),
                                     t['den'].data_ptr(), t['gq'].data_ptr(), dsig.data_ptr(), ctypes.byref(fp), clib.stream_ptr())
    else:
        t.update(idx=_dev(x['idx'], torch.int32), val=_dev(x['str']))
        rc = lib.ssn_ff_backward_sparse_f32(t['RF_w'].data_ptr(), t['idx'].data_ptr() if c.ncon else None, t['val'].data_ptr() if c.ncon else None,
                                            c.ncon, t['stim'].data_ptr(), t['q'].data_ptr(), t['den'].data_ptr(), t['gq'].data_ptr(),
                                            dsig.data_ptr(), ctypes.byref(fp), clib.stream_ptr())
    torch.cuda.synchronize()
    return rc, dsig.cpu().numpy().astype('float64')


@pytest.mark.parametrize('c', [c for c in fc.CASES if c.entry.startswith('forward')], ids=fc.case_id)
def test_forward_elementwise(c):
    """den, q and out of one forward entry point against the oracle, each element in its own measure; `out > 0` is the oracle's
    pattern exactly."""
    x, o = fc.inputs(c), fc.oracle(c)
    assert fc.predicted_path(c.entry, c.box, x['stim']) == c.path
    out, saved = _forward(c, x)
    got = dict(out=out.cpu().numpy().astype('float64'), q=saved['q'].cpu().numpy().astype('float64'),
               den=saved['den'].cpu().numpy().astype('float64'))
    assert all(np.isfinite(v).all() for v in got.values())
    err = {k: _note(c, k, v, o['tol'][k]) for k, v in fc.errors(o, got).items()}
    assert np.array_equal(got['out'] > 0, o['out'] > 0)
    for k in ('den', 'q', 'out'):
        assert err[k] <= o['tol'][k], (k, err[k], o['tol'][k])
    plain = _forward(c, x, keep=False)                    # q = den = NULL: the same outputs
    assert torch.equal(plain, out)


@pytest.mark.parametrize('c', [c for c in fc.CASES if c.entry.startswith('backward')], ids=fc.case_id)
def test_second_pass_elementwise(c):
    """dsig[s][h][0:2] of one second pass, fed the ORACLE's q and den (rounded to float32), for every gq pattern; then once
    through `ff_model.ff_backward` on the kernel's own q, den: the five parameter gradients, as a consequence."""
    from tc_gan_amd import ff_model
    x, o = fc.inputs(c), fc.oracle(c)
    got = []
    for r in range(x['gq'].shape[0]):
        rc, d = _second_pass(c, x, o['q32'], o['den32'], x['gq'][r])
        assert rc == 0
        got.append(d)
    got = np.stack(got)
    assert np.isfinite(got).all()
    err = _note(c, 'dsig', fc.errors(o, dict(dsig=got))['dsig'], o['tol']['dsig'])
    assert err <= o['tol']['dsig']
    out, saved = _forward(c, x)
    assert np.array_equal(out.cpu().numpy() > 0, o['out'] > 0)
    grads = ff_model.ff_backward(x['params'], saved, out, _dev(x['gq'][0]))
    want, atol = fc.param_grads(c, o)
    for name in ff_model.PARAM_NAMES:
        print('%s dL/d%s: %.3e, oracle %.3e, allowed %.1e' % (fc.case_id(c), name, grads[name], want[name], atol[name]))
        assert abs(grads[name] - want[name]) <= atol[name], name


@pytest.mark.parametrize('entry', fc.ENTRIES)
def test_a_sample_alone_gives_the_bits_it_gives_in_the_batch(entry):
    from tc_gan_amd import ff_model
    c = next(k for k in fc.CASES if k.entry == entry and k.nhid == 3 and k.box == 12 and (k.stim == 'lattice') == entry.startswith('forward'))
    x, o = fc.inputs(c), fc.oracle(c)
    for s in range(c.nsam):
        one = dict(x, RF_w=x['RF_w'][s:s + 1], FF_con=x['FF_con'][s:s + 1], FF_str=x['FF_str'][s:s + 1], idx=x['idx'][s:s + 1],
                   str=x['str'][s:s + 1], TH_sam=x['TH_sam'][s:s + 1])
        c1 = c._replace(nsam=1)
        if entry.startswith('forward'):
            out, saved = _forward(c, x)
            out1, saved1 = _forward(c1, one)
            assert torch.equal(out1[0], out[s]) and torch.equal(saved1['q'][0], saved['q'][s]) and torch.equal(saved1['den'][0], saved['den'][s])
        else:
            rc, d = _second_pass(c, x, o['q32'], o['den32'], x['gq'][0])
            rc1, d1 = _second_pass(c1, one, o['q32'][s:s + 1], o['den32'][s:s + 1], x['gq'][0][s:s + 1])
            assert rc == 0 and rc1 == 0 and np.array_equal(d1[0], d[s])


def test_invalid_arguments_are_refused_without_a_launch():
    """ni = 0, ni = 33 and ncon < 0: the invalid-argument status, and the output buffers keep their bits."""
    from tc_gan_amd import clib
    lib = clib.libssnode
    c = next(k for k in fc.CASES if k.box == 4 and k.stim == 'free' and k.entry == 'forward')
    x, o = fc.inputs(c), fc.oracle(c)
    t = dict(RF_w=_dev(x['RF_w']), con=_dev(x['FF_con']), strn=_dev(x['FF_str']), ths=_dev(x['TH_sam']), stim=_dev(np.zeros((40, 3))),
             idx=_dev(x['idx'], torch.int32), val=_dev(x['str']))
    sent = torch.full((c.nsam, 40, c.nhid), -7.5, device='cuda')
    outs = [sent.clone() for _ in range(3)]
    op = [v.data_ptr() for v in outs]
    st = clib.stream_ptr()
    calls = []
    for ni, ncon in ((0, c.ncon), (33, c.ncon), (c.ni, -1)):
        fp = _ff_params(c, x, ni=ni)
        if ncon >= 0:
            calls.append(lib.ssn_ff_forward_f32(t['RF_w'].data_ptr(), t['con'].data_ptr(), t['strn'].data_ptr(), t['ths'].data_ptr(), t['stim'].data_ptr(),
                                                op[0], op[1], op[2], ctypes.byref(fp), st))
            calls.append(lib.ssn_ff_backward_f32(t['RF_w'].data_ptr(), t['con'].data_ptr(), t['strn'].data_ptr(), t['stim'].data_ptr(), op[1], op[2],
                                                 op[1], op[0], ctypes.byref(fp), st))
        calls.append(lib.ssn_ff_forward_sparse_f32(t['RF_w'].data_ptr(), t['idx'].data_ptr(), t['val'].data_ptr(), ncon, t['ths'].data_ptr(),
                                                   t['stim'].data_ptr(), op[0], op[1], op[2], ctypes.byref(fp), st))
        calls.append(lib.ssn_ff_backward_sparse_f32(t['RF_w'].data_ptr(), t['idx'].data_ptr(), t['val'].data_ptr(), ncon, t['stim'].data_ptr(), op[1], op[2],
                                                    op[1], op[0], ctypes.byref(fp), st))
    torch.cuda.synchronize()
    assert len(calls) == 10 and all(rc == INVALID for rc in calls), calls
    assert 'invalid argument' in clib.last_error()
    assert all(torch.equal(v, sent) for v in outs)


def _shifted(a):
    """A float32 device view of `a` that starts 4 bytes past a 16-byte boundary."""
    flat = torch.empty(a.size + 5, device='cuda', dtype=torch.float32)
    assert flat.data_ptr() % 16 == 0
    v = flat[1:1 + a.size].view(*a.shape)
    v.copy_(_dev(a))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def test_misaligned_dense_streams_are_refused_and_ff_model_realigns():
    """The dense kernels load 16 bytes at a time when box^3 % 4 == 0: the C entry points refuse RF_w, FF_con or FF_str off a
    16-byte boundary (host check, nothing launched; with an odd box^3 they take them), and `ff_model` hands over aligned
    storage -- views that start 4 bytes past a boundary give the bits of the aligned call, dense and from the lists."""
    from tc_gan_amd import clib, ff_model
    lib = clib.libssnode
    for box in (4, 3):
        c = next(k for k in fc.CASES if k.box == box and k.stim == 'free' and k.entry == 'forward' and k.ncon > 1)
        x, o = fc.inputs(c), fc.oracle(c)
        names = ('RF_w', 'FF_con', 'FF_str')
        good = {k: _dev(x[k]) for k in names}
        bad = {k: _shifted(x[k]) for k in names}
        ths, stim, fp = _dev(x['TH_sam']), _dev(x['stim']), _ff_params(c, x)
        sent = torch.full((c.nsam, c.ni, c.nhid), -7.5, device='cuda')
        ref = sent.clone()
        assert lib.ssn_ff_forward_f32(good['RF_w'].data_ptr(), good['FF_con'].data_ptr(), good['FF_str'].data_ptr(), ths.data_ptr(), stim.data_ptr(),
                                      ref.data_ptr(), None, None, ctypes.byref(fp), clib.stream_ptr()) == 0
        q, den, gq = _dev(o['q32']), _dev(o['den32']), _dev(x['gq'][0])
        for k in names:
            t = dict(good, **{k: bad[k]})
            out, dsig = sent.clone(), torch.full((c.nsam, c.nhid, 2), -7.5, device='cuda')
            rc = lib.ssn_ff_forward_f32(t['RF_w'].data_ptr(), t['FF_con'].data_ptr(), t['FF_str'].data_ptr(), ths.data_ptr(), stim.data_ptr(),
                                        out.data_ptr(), None, None, ctypes.byref(fp), clib.stream_ptr())
            rb = lib.ssn_ff_backward_f32(t['RF_w'].data_ptr(), t['FF_con'].data_ptr(), t['FF_str'].data_ptr(), stim.data_ptr(), q.data_ptr(),
                                         den.data_ptr(), gq.data_ptr(), dsig.data_ptr(), ctypes.byref(fp), clib.stream_ptr())
            torch.cuda.synchronize()
            if box ** 3 % 4 == 0:
                assert rc == INVALID and rb == INVALID and '16-byte aligned' in clib.last_error()
                assert torch.equal(out, sent) and bool((dsig == -7.5).all())
            else:                                        # scalar loads: any 4-byte aligned pointer
                assert rc == 0 and rb == 0 and torch.equal(out, ref)
        # through ff_model: the bits of the aligned call
        want, ws = ff_model.ff_forward(x['params'], good['RF_w'], good['FF_con'], good['FF_str'], x['TH_sam'], x['stim'], box, keep=True)
        got, gs = ff_model.ff_forward(x['params'], bad['RF_w'], bad['FF_con'], bad['FF_str'], x['TH_sam'], x['stim'], box, keep=True)
        assert torch.equal(got, want) and torch.equal(gs['q'], ws['q']) and torch.equal(gs['den'], ws['den'])
        g_want = ff_model.ff_backward(x['params'], ws, want, gq)
        g_got = ff_model.ff_backward(x['params'], gs, got, gq)
        assert g_got == g_want
        lat = next(k for k in fc.CASES if k.box == box and k.stim == 'lattice' and k.entry == 'forward_sparse' and k.ncon > 1)
        y = fc.inputs(lat)
        sw = ff_model.ff_forward_sparse(y['params'], _dev(y['RF_w']), y['idx'], y['str'], y['TH_sam'], y['stim'], box)
        sg = ff_model.ff_forward_sparse(y['params'], _shifted(y['RF_w']), y['idx'], _shifted(y['str']), y['TH_sam'], y['stim'], box)
        assert torch.equal(sg, sw)


def test_zz_every_path_ran_and_the_largest_figures():
    """(Runs last in the module.)  Every kernel path was held in every quantity it produces; prints the largest error and the
    largest share of a tolerance per quantity and path."""
    for key in sorted(WORST):
        print('%-5s %-15s largest error %.2e, most of a tolerance used %.2f (%s)' % (key + WORST[key]))
    if len(RAN) == len(fc.CASES):                     # (a selection of the module's tests proves nothing about coverage)
        assert {p for q, p in WORST if q == 'den'} == {'generic', 'lattice', 'sparse-generic', 'sparse-lattice'}
        assert {p for q, p in WORST if q == 'dsig'} == {'generic', 'sparse-generic'}

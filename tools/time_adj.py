"""HIP-event timing of the adjoint sweep, alone and with dL/dW, at the C3 shape (1024 draws x 8 stimuli x 1200 steps, 2N = 200).
usage: tools/time_adj.py [kernel] [paper]     kernel: a code of clib.GEN_KERNELS, default 8 (2: the fp32 matrix-core sweep)"""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tc_gan_amd import genops
B, NB, M, T, skip = 1024, 8, 200, 1200, 1000
KERNEL, GEN = next((int(a) for a in sys.argv[1:] if a.isdigit()), 8), {}
if 'paper' in sys.argv[1:]:       # the paper's run: 128 draws, 2N = 202, 240 / 200 steps, tau_E = 2, the library's own choice
    B, NB, M, T, skip, KERNEL, GEN = 128, 8, 202, 240, 200, 0, dict(tau_E=2.0)
g = torch.Generator(device='cuda'); g.manual_seed(1)
W = (torch.rand((B, M, M), device='cuda', generator=g) - 0.6) * 0.02
ext = torch.rand((B, NB, M), device='cuda', generator=g) * 20
gp = genops.make_gen_params(seqlen=T, skip_steps=skip, kernel=KERNEL, **GEN)
out = genops.gen_forward(W, ext, gp, save=True)
gta = torch.rand((B, NB, M), device='cuda', generator=g)
traj, df = out['traj'], out['df']
def bwd(): return genops.gen_backward(W, traj, df, gta, 1.0, 0.01, gp)
bwd(); e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(3): bwd()
e1.record(); torch.cuda.synchronize()
print('kernel %d: adjoint (in place, repeated) %.3f ms' % (KERNEL, e0.elapsed_time(e1) / 3), flush=True)
if hasattr(genops.libssnode, 'ssn_debug_duo_stamps'):       # diagnostic build (-DSSN_DUO_STAMP=1): the steps after the window
    import ctypes
    buf = (ctypes.c_ulonglong * 64)()
    genops.libssnode.ssn_debug_duo_stamps(buf)
    for w in (0, 3):                                        # draw 0: the lightest and the four-tile wave
        n = max(int(buf[8 * w + 7]), 1)
        print('  draw 0 wave %d: serial %.0f  barrier %.0f  chain %.0f  barrier %.0f cycles per step (%d steps)'
              % ((w,) + tuple(buf[8 * w + i] / n for i in range(4)) + (n,)))
xmax = genops.rate_bound(gp)
out = genops.gen_forward(W, ext, gp, save=True)      # (the loop above ran the in-place sweep over its own output)
traj, df = out['traj'], out['df']
dmax = torch.empty((B,), device='cuda')
def two():
    d, dm = genops.gen_backward(W, traj, df.clone(), gta, 1.0 / out['n_dyn'], 0.01 / out['n_rate'], gp, want_dmax=True)
    return genops.weight_grad(d, traj, dmax=dm, xmax=xmax)
def fused(): return genops.gen_backward_fused(W, traj, df, gta, 1.0 / out['n_dyn'], 0.01 / out['n_rate'], gp, xmax)
def clone(): return df.clone()
for name, fn in (('df.clone()', clone), ('two launches (adjoint + dL/dW, incl. the clone)', two), ('fused adjoint + dL/dW', fused)):
    fn(); torch.cuda.synchronize()
    e0.record()
    for _ in range(10): r = fn()
    e1.record(); torch.cuda.synchronize()
    print('%s %.3f ms' % (name, e0.elapsed_time(e1) / 10))
a = two(); b = fused()[0]
print('max |fused - two| / max |two| per draw: %.2e' % float(((a - b).abs().reshape(B, -1).max(dim=1).values / a.abs().reshape(B, -1).max(dim=1).values).max()))
if hasattr(genops.libssnode, 'ssn_debug_fuse_stamps'):
    import ctypes
    buf = (ctypes.c_ulonglong * 32)()
    genops.libssnode.ssn_debug_fuse_stamps(buf)
    for w in range(4):
        n = max(int(buf[8 * w + 7]), 1)
        print('  wave %d: update+serial %.0f  barrier %.0f  chain %.0f  barrier %.0f cycles per step' % ((w,) + tuple(buf[8 * w + i] / n for i in range(4))))

"""The refusals of the C surface (csrc/ssn_capi.hip), pinned: return code and `ssn_last_error()` string of every entry point
that checks its arguments, byte for byte.  Refusals are host arithmetic that runs before any HIP call, so no device is needed;
the table holds only calls that the library refuses (or answers with an early 0 / 1) without touching the runtime.  `X` stands
for "some non-null pointer": no row lets it reach a launcher.

`ssn_last_error()` is sticky across successful calls: every row is preceded by one fixed refused call with another message
(`_SENTINEL`), so a row's message is its own, and a row that returns early leaves the sentinel's message standing.

Left out on purpose: the entry points that dereference a null argument on the host (`ssn_io_eval_*` with p == NULL, the
callers of pack_jds with a null J: `ssn_build_w_*`, `ssn_build_w_philox_*`, `ssn_jds_grad_*`, `ssn_build_dw_*` with B == 0),
the ones without any check (`ssn_stimulus_*`, `ssn_stimulus_amp_*`), and the three messages that only a failure inside the
runtime or the library can produce ("solve_dynamics: batched launch failed", jump_poly's "did not come out with degree 19937",
the late `seg_bounds` refusal of `ssn_critic_step_run`, which comes after its launches)."""
import ctypes
from ctypes import Structure, byref, c_double, c_float, c_int

import numpy as np
import pytest

from tc_gan_amd import clib

lib = clib.libssnode
INV = clib.SSN_ERR_BASE + 1                       # SSN_ERR_BASE + hipErrorInvalidValue

_buf = np.zeros(64, dtype=np.float64)
X = _buf.ctypes.data + (-_buf.ctypes.data) % 16   # a 16-byte aligned non-null pointer that no row lets the library follow
F4 = (c_float * 4)(1, 1, 1, 1)                    # J / D / S of the entries that take them as float[4]
D4 = (c_double * 4)()                             # W / ext / r0 / r1 of the drop-in solver at N = 1
TICKET, POS = c_int(7), c_int(0)


def ints(*v):
    return (c_int * len(v))(*v)


def at(a):                                        # a ctypes array for a `void *` parameter
    return ctypes.addressof(a)


DIMS = ints(11, 32, 32)
FLAGS_02, FLAGS_40 = ints(0, 2), ints(4, 0)          # kept alive here: the _act entries take them as `void *`


def sp(**kw):
    d = dict(io_type=2, max_iter=10, k=0.01, n=2.2, tau_E=0.01, tau_I=0.002, dt=8e-4, atol=1e-5, rate_soft_bound=200.,
             rate_hard_bound=1000.)
    d.update(kw)
    return clib.SolverParams(**d)


def gp(**kw):
    d = dict(io_type=2, seqlen=10, skip_steps=5, kernel=0, k=0.01, n=2.2, tau_E=10., tau_I=1., dt=0.1, rate_soft_bound=200.,
             rate_hard_bound=1000., rate_penalty_threshold=1.)
    d.update(kw)
    return clib.GenParams(**d)


def op(**kw):
    d = dict(kind=1, step=1, learning_rate=1e-3, beta1=0.5, beta2=0.9, epsilon=1e-8, rho=0.9)
    d.update(kw)
    return clib.OptParams(**d)


def fp(**kw):
    d = dict(nsam=2, nhid=3, ni=4, box=2, RF_l=1., RF_d=1., TH=1., TH_d=1., J=1., a=1.)
    d.update(kw)
    return clib.FFParams(**d)


def gg(**kw):
    d = dict(jds_part=X, B=1, nv=0, g_ext=X, ext_base=X, zin=X, NB=1, M=2, dmean=X, pens64=X, ws=X, out=X)
    d.update(kw)
    return clib.GenGrads(**d)


def eg(**kw):
    d = dict(K=1, B=1, nv=0, NB=1, M=2, D=1, part=X, g_ext=X, ext_base=X, zin=X, dyn_row=X, rate_row=X, scale_dyn=1.,
             scale_rate=1., data_moments=X, weights=X, costs=X, grads=X, rec=X, rstride=100)
    d.update(kw)
    return clib.EnsGrads(**d)


def eg0(**kw):                                    # what ssn_ens_gen_grads_l0_f32 takes
    return eg(**dict(dict(D=0, data_moments=None, weights=None), **kw))


def ea(**kw):
    d = dict(K=1, P=2, kind=0, hyp=X, clip_lo=X, clip_hi=X, p=X, s1=X, s2=X, g=X, rec=X, rstride=10, rec_off=0)
    d.update(kw)
    return clib.EnsApply(**d)


def gi(**kw):
    d = dict(J=F4, D=F4, S=F4, bw=X, con=X, smoothness=1., v=None, W=X, z=X, zin=X, amp=X, ext=X, B=1, NB=1, N=2)
    d.update(kw)
    for k in 'JDS':
        if d[k] is not None:
            d[k] = ctypes.cast(d[k], ctypes.POINTER(c_float))
    return clib.GenInputs(**d)


_OPT = op()


def cs(**kw):
    d = dict(params=X, dims=DIMS, layer_norm=None, nlayers=2, leak=0., xg=X, xd=X, cond=X, eps=X, n=4, precision=1, lmd=10.,
             xp=X, grads=X, stats=X, dvals=X, workspace=X, opt_s1=X, opt_s2=X, opt=ctypes.pointer(_OPT), seg_bounds=X, nseg=0,
             seg_ws=X, pens64=X, acc_dvals=X, tail=X)
    d.update(kw)
    for k in ('dims', 'layer_norm'):
        if d[k] is not None:
            d[k] = ctypes.cast(d[k], ctypes.POINTER(c_int))
    return clib.CriticStep(**d)


_SENTINEL = ('ssn_mt19937_jump_poly', (0, None), 'ssn_mt19937_jump_poly: null output')
_SENTINEL2 = ('ssn_interpolate_f32', (None, None, None, None, -1, 3, None), 'ssn_interpolate: invalid argument')
SAME = None                                       # expected message of a row that returns early: the sentinel's, left standing

M_LAYOUT = 'invalid layer flags / activation / slope, or more than 8 layers'
M_FLAGS01 = 'layer_norm flags are 0 / 1 (scaled layers: the _act entry points)'
M_LEAKNORM = 'leak with layer-normalised layers (that critic: the _act entry points)'
M_ACT = 'invalid layer flags / activation'
M_GEN = ('invalid argument, unsupported size or kernel not one of 0 (automatic), 1 (tile), 2 / 3 (fp32 MFMA), '
         '4 / 5 / 6 (fp16-split), 8 (two-draw)')
M_MFMA = 'the MFMA kernels need fp32, NB >= 4, 2N <= 208 and NB T 2N < 2^29'
M_SPLIT = 'the fp16-split MFMA kernels need asym_tanh, rate_hard_bound < 3e4 and dt <= tau'
M_FUSED = ('ssn_gen_backward_fused: invalid argument or unsupported size (fp32, NB <= 8, even 2N <= 208, '
           'NB T 2N < 2^29, 0 < xmax < inf)')
M_WGS = 'ssn_weight_grad_scaled: invalid argument (fp32, M <= 224, K M < 2^29, dmax on the device, 0 < xmax < inf)'
M_ALIGN = 'RF_w, FF_con, FF_str must be 16-byte aligned when box^3 % 4 == 0'
M_DIRS = 'more than 4096 directions'
M_ROWS = 'more than 4096 rows (keys and values are sorted in 48 KiB of LDS)'
M_ENS_ROWS = 'more than 4096 rows per member (keys and values are sorted in 48 KiB of LDS)'
M_KS = 'more than 16384 values per column (the sort runs in 64 KiB of LDS)'
M_FPSEL = 'more than 8192 candidates in one round (the accepted indices of a round are kept in LDS)'
M_VARIANT = 'ssn_solve_batch: requested kernel variant has no instantiation for this size'
M_GATED = 'ssn_critic_step_gated_run: needs pens64 and a positive bound'
M_ENS_D = ('ssn_ens_gen_grads: D must be at least 1 (a loss that is not a function of moments takes '
           'ssn_ens_gen_grads_l0_f32)')
M_ENS_L0 = 'ssn_ens_gen_grads_l0: invalid argument (D must be 0, data_moments and weights null)'
M_TAILKIND = 'ssn_mt19937_random_sample_tail_begin: tail_kind must be 1 (choice(2, n) * 2 - 1) or 2 (rand(n) * 2 - 1)'
NAN, INF = float('nan'), float('inf')

F32_F64 = ('_f32', '_f64')


def pair(stem, tail=''):
    return tuple(stem + s + tail for s in F32_F64)


SOLVE = pair('ssn_solve_batch')
SOLVE_V = pair('ssn_solve_batch', '_variant')
SOLVE_H = pair('ssn_solve_batch_host')
LEGACY = ('solve_dynamics_asym_power_euler', 'solve_dynamics_asym_linear_euler', 'solve_dynamics_asym_tanh_euler')
GEN_F, GEN_B, GEN_BE = pair('ssn_gen_forward'), pair('ssn_gen_backward'), pair('ssn_gen_backward_ext')
PM, PMP = pair('ssn_penalty_means'), pair('ssn_penalty_means_probe')
FPS = 'ssn_fp_select'

# (entry point or entry points, arguments, expected return code, expected ssn_last_error()).  A tuple of names: the same
# row for each of them (the f32 / f64 members of a pair, the three drop-in solvers).
TABLE = [
    # ---- errors / version / device: nothing to refuse
    # ---- solver: device buffers.  W, ext, ext_per_draw, r, r_prev, codes, steps, B, NB, M, p, stream
    (SOLVE, (None, None, 0, None, None, None, None, 0, 3, 8, None, None), 0, SAME),
    (SOLVE, (None, None, 0, None, None, None, None, 3, 0, 8, None, None), 0, SAME),
    (SOLVE, (X, X, 0, X, None, X, None, -1, 1, 8, sp(), None), INV, 'ssn_solve_batch: invalid argument'),
    (SOLVE, (X, X, 0, X, None, X, None, 1, -1, 8, sp(), None), INV, 'ssn_solve_batch: invalid argument'),
    (SOLVE, (X, X, 0, X, None, X, None, 1, 1, 0, sp(), None), INV, 'ssn_solve_batch: invalid argument'),
    (SOLVE, (X, X, 0, X, None, X, None, 1, 1, -2, sp(), None), INV, 'ssn_solve_batch: invalid argument'),
    (SOLVE, (X, X, 0, X, None, X, None, 1, 1, 7, sp(), None), INV, 'ssn_solve_batch: invalid argument'),
    (SOLVE, (None, X, 0, X, None, X, None, 1, 1, 8, sp(), None), INV, 'ssn_solve_batch: invalid argument'),
    (SOLVE, (X, None, 0, X, None, X, None, 1, 1, 8, sp(), None), INV, 'ssn_solve_batch: invalid argument'),
    (SOLVE, (X, X, 0, None, None, X, None, 1, 1, 8, sp(), None), INV, 'ssn_solve_batch: invalid argument'),
    (SOLVE, (X, X, 0, X, None, None, None, 1, 1, 8, sp(), None), INV, 'ssn_solve_batch: invalid argument'),
    (SOLVE, (X, X, 0, X, None, X, None, 1, 1, 8, None, None), INV, 'ssn_solve_batch: invalid argument'),
    (SOLVE, (X, X, 0, X, None, X, None, 1, 1, 8, sp(io_type=3), None), INV, 'ssn_solve_batch: invalid argument'),
    (SOLVE, (X, X, 0, X, None, X, None, 1, 1, 8, sp(io_type=-1), None), INV, 'ssn_solve_batch: invalid argument'),
    (SOLVE, (X, X, 0, X, None, X, None, 1, 1, 8, sp(max_iter=-1), None), INV, 'ssn_solve_batch: invalid argument'),
    # variant, then the same
    (SOLVE_V, (-1, None, None, 0, None, None, None, None, 0, 3, 8, None, None), 0, SAME),
    (SOLVE_V, (9, None, None, 0, None, None, None, None, 3, 0, 8, None, None), 0, SAME),
    (SOLVE_V, (-1, X, X, 0, X, None, X, None, -1, 1, 8, sp(), None), INV, 'ssn_solve_batch: invalid argument'),
    (SOLVE_V, (2, X, X, 0, X, None, X, None, 1, 1, 7, sp(), None), INV, 'ssn_solve_batch: invalid argument'),
    (SOLVE_V, (0, None, X, 0, X, None, X, None, 1, 1, 8, sp(), None), INV, 'ssn_solve_batch: invalid argument'),
    (SOLVE_V, (0, X, X, 0, X, None, X, None, 1, 1, 8, None, None), INV, 'ssn_solve_batch: invalid argument'),
    (SOLVE_V, (0, X, X, 0, X, None, X, None, 1, 1, 8, sp(io_type=3), None), INV, 'ssn_solve_batch: invalid argument'),
    (SOLVE_V, (0, X, X, 0, X, None, X, None, 1, 1, 8, sp(max_iter=-1), None), INV, 'ssn_solve_batch: invalid argument'),
    (SOLVE_V, (9, X, X, 0, X, None, X, None, 1, 1, 8, sp(), None), INV, M_VARIANT),
    (SOLVE_V, (100, X, X, 0, X, None, X, None, 2, 8, 200, sp(), None), INV, M_VARIANT),
    (SOLVE_V, (5, X, X, 0, X, None, X, None, 1, 1, 8, sp(), None), INV, M_VARIANT),          # MFMA: NB >= 4, fp32
    (SOLVE_V, (6, X, X, 0, X, None, X, None, 1, 1, 8, sp(), None), INV, M_VARIANT),
    (SOLVE_V, (8, X, X, 0, X, None, X, None, 1, 1, 8, sp(), None), INV, M_VARIANT),
    (SOLVE_V, (2, X, X, 0, X, None, X, None, 1, 1, 4000, sp(), None), INV, M_VARIANT),       # no tile kernel that large
    (SOLVE_V, (1, X, X, 0, X, None, X, None, 1, 1, 4000, sp(), None), INV, M_VARIANT),
    ('ssn_solve_batch_f32_variant', (6, X, X, 0, X, None, X, None, 64, 8, 200, sp(io_type=0), None), INV, M_VARIANT),
    ('ssn_solve_batch_f64_variant', (5, X, X, 0, X, None, X, None, 64, 8, 200, sp(), None), INV, M_VARIANT),
    ('ssn_solve_batch_variant_for', (1, 1, 7, 4, None), -1, 'ssn_solve_batch: invalid argument'),
    ('ssn_solve_batch_variant_for', (1, 1, 8, 8, sp(io_type=3)), -1, 'ssn_solve_batch: invalid argument'),
    ('ssn_solve_batch_variant_for', (0, 1, 8, 8, sp()), -1, SAME),
    # ---- solver: host buffers.  W, ext, ext_per_draw, r, r_prev, codes, steps, B, NB, M, p
    (SOLVE_H, (None, None, 0, None, None, None, None, 0, 3, 8, None), 0, SAME),
    (SOLVE_H, (None, None, 0, None, None, None, None, 3, 0, 8, None), 0, SAME),
    (SOLVE_H, (X, X, 0, X, None, X, None, -1, 1, 8, sp()), INV, 'ssn_solve_batch_host: invalid argument'),
    (SOLVE_H, (X, X, 0, X, None, X, None, 1, -1, 8, sp()), INV, 'ssn_solve_batch_host: invalid argument'),
    (SOLVE_H, (X, X, 0, X, None, X, None, 1, 1, 0, sp()), INV, 'ssn_solve_batch_host: invalid argument'),
    (SOLVE_H, (X, X, 0, X, None, X, None, 1, 1, 7, sp()), INV, 'ssn_solve_batch_host: invalid argument'),
    (SOLVE_H, (None, X, 0, X, None, X, None, 1, 1, 8, sp()), INV, 'ssn_solve_batch_host: invalid argument'),
    (SOLVE_H, (X, None, 0, X, None, X, None, 1, 1, 8, sp()), INV, 'ssn_solve_batch_host: invalid argument'),
    (SOLVE_H, (X, X, 0, None, None, X, None, 1, 1, 8, sp()), INV, 'ssn_solve_batch_host: invalid argument'),
    (SOLVE_H, (X, X, 0, X, None, None, None, 1, 1, 8, sp()), INV, 'ssn_solve_batch_host: invalid argument'),
    (SOLVE_H, (X, X, 0, X, None, X, None, 1, 1, 8, None), INV, 'ssn_solve_batch_host: invalid argument'),
    # ---- solver: drop-in.  N, W, ext, k, n, r0, r1, tau_E, tau_I, dt, max_iter, atol, soft, hard
    (LEGACY, (0, D4, D4, .01, 2.2, D4, D4, .01, .002, 8e-4, 10, 1e-5, 200., 1000.), INV, 'solve_dynamics: invalid argument'),
    (LEGACY, (-1, D4, D4, .01, 2.2, D4, D4, .01, .002, 8e-4, 10, 1e-5, 200., 1000.), INV, 'solve_dynamics: invalid argument'),
    (LEGACY, (1, None, D4, .01, 2.2, D4, D4, .01, .002, 8e-4, 10, 1e-5, 200., 1000.), INV, 'solve_dynamics: invalid argument'),
    (LEGACY, (1, D4, None, .01, 2.2, D4, D4, .01, .002, 8e-4, 10, 1e-5, 200., 1000.), INV, 'solve_dynamics: invalid argument'),
    (LEGACY, (1, D4, D4, .01, 2.2, None, D4, .01, .002, 8e-4, 10, 1e-5, 200., 1000.), INV, 'solve_dynamics: invalid argument'),
    (LEGACY, (1, D4, D4, .01, 2.2, D4, None, .01, .002, 8e-4, 10, 1e-5, 200., 1000.), INV, 'solve_dynamics: invalid argument'),
    (LEGACY, (1, D4, D4, .01, 2.2, D4, D4, .01, .002, 8e-4, 0, 1e-5, 200., 1000.), 1, SAME),     # no step: code 1, untouched
    (LEGACY, (1, D4, D4, .01, 2.2, D4, D4, .01, .002, 8e-4, -3, 1e-5, 200., 1000.), 1, SAME),

    # ---- weights and stimuli
    # z, jds_dev, W, B, N, stream
    ('ssn_build_w_devparams_f32', (X, None, X, 1, 2, None), INV, 'ssn_build_w_devparams_f32: invalid argument'),
    ('ssn_build_w_devparams_f32', (None, X, X, 1, 2, None), INV, 'ssn_build_w_devparams_f32: invalid argument'),
    ('ssn_build_w_devparams_f32', (X, X, None, 1, 2, None), INV, 'ssn_build_w_devparams_f32: invalid argument'),
    ('ssn_build_w_devparams_f32', (X, X, X, 1, 0, None), INV, 'ssn_build_w_devparams_f32: invalid argument'),
    ('ssn_build_w_devparams_f32', (X, X, X, -1, 2, None), INV, 'ssn_build_w_devparams_f32: invalid argument'),
    # z, jds_table, W, S, B, N, stream
    ('ssn_build_w_table_f32', (X, X, X, -1, 1, 2, None), INV, 'ssn_build_w_table_f32: invalid argument'),
    ('ssn_build_w_table_f32', (X, X, X, 1, -1, 2, None), INV, 'ssn_build_w_table_f32: invalid argument'),
    ('ssn_build_w_table_f32', (X, X, X, 1, 1, 0, None), INV, 'ssn_build_w_table_f32: invalid argument'),
    ('ssn_build_w_table_f32', (None, X, X, 1, 1, 2, None), INV, 'ssn_build_w_table_f32: invalid argument'),
    ('ssn_build_w_table_f32', (X, None, X, 1, 1, 2, None), INV, 'ssn_build_w_table_f32: invalid argument'),
    ('ssn_build_w_table_f32', (X, X, None, 1, 1, 2, None), INV, 'ssn_build_w_table_f32: invalid argument'),
    ('ssn_build_w_table_f64', (X, X, X, -1, 1, 2, None), INV, 'ssn_build_w_table_f64: invalid argument'),
    ('ssn_build_w_table_f64', (X, X, X, 1, -1, 2, None), INV, 'ssn_build_w_table_f64: invalid argument'),
    ('ssn_build_w_table_f64', (X, X, X, 1, 1, 0, None), INV, 'ssn_build_w_table_f64: invalid argument'),
    ('ssn_build_w_table_f64', (None, X, X, 1, 1, 2, None), INV, 'ssn_build_w_table_f64: invalid argument'),
    ('ssn_build_w_table_f64', (X, None, X, 1, 1, 2, None), INV, 'ssn_build_w_table_f64: invalid argument'),
    ('ssn_build_w_table_f64', (X, X, None, 1, 1, 2, None), INV, 'ssn_build_w_table_f64: invalid argument'),
    # bw, con, smoothness, zin, v, nv, ext, B, NB, N, stream
    ('ssn_stimulus_hetero_f32', (X, X, 1., None, X, 1, X, 1, 1, 4, None), INV, 'ssn_stimulus_hetero: invalid argument'),
    ('ssn_stimulus_hetero_f32', (X, X, 1., X, None, 1, X, 1, 1, 4, None), INV, 'ssn_stimulus_hetero: invalid argument'),
    ('ssn_stimulus_hetero_f32', (X, X, 1., X, X, 0, X, 1, 1, 4, None), INV, 'ssn_stimulus_hetero: invalid argument'),
    ('ssn_stimulus_hetero_f32', (X, X, 1., X, X, 3, X, 1, 1, 4, None), INV, 'ssn_stimulus_hetero: invalid argument'),
    ('ssn_stimulus_hetero_f32', (X, X, 1., X, X, 1, X, -1, 1, 4, None), INV, 'ssn_stimulus_hetero: invalid argument'),
    ('ssn_stimulus_hetero_f32', (X, X, 1., X, X, 1, X, 1, -1, 4, None), INV, 'ssn_stimulus_hetero: invalid argument'),
    ('ssn_stimulus_hetero_f32', (X, X, 1., X, X, 1, X, 1, 1, 0, None), INV, 'ssn_stimulus_hetero: invalid argument'),
    # a, stream
    ('ssn_gen_inputs_philox_f32', (None, None), INV, 'ssn_gen_inputs_philox: invalid argument'),
    ('ssn_gen_inputs_philox_f32', (gi(J=None), None), INV, 'ssn_gen_inputs_philox: invalid argument'),
    ('ssn_gen_inputs_philox_f32', (gi(D=None), None), INV, 'ssn_gen_inputs_philox: invalid argument'),
    ('ssn_gen_inputs_philox_f32', (gi(S=None), None), INV, 'ssn_gen_inputs_philox: invalid argument'),
    ('ssn_gen_inputs_philox_f32', (gi(bw=None), None), INV, 'ssn_gen_inputs_philox: invalid argument'),
    ('ssn_gen_inputs_philox_f32', (gi(con=None), None), INV, 'ssn_gen_inputs_philox: invalid argument'),
    ('ssn_gen_inputs_philox_f32', (gi(W=None), None), INV, 'ssn_gen_inputs_philox: invalid argument'),
    ('ssn_gen_inputs_philox_f32', (gi(ext=None), None), INV, 'ssn_gen_inputs_philox: invalid argument'),
    ('ssn_gen_inputs_philox_f32', (gi(B=-1), None), INV, 'ssn_gen_inputs_philox: invalid argument'),
    ('ssn_gen_inputs_philox_f32', (gi(NB=-1), None), INV, 'ssn_gen_inputs_philox: invalid argument'),
    ('ssn_gen_inputs_philox_f32', (gi(N=0), None), INV, 'ssn_gen_inputs_philox: invalid argument'),
    ('ssn_gen_inputs_philox_f32', (gi(v=X, zin=None), None), INV, 'ssn_gen_inputs_philox: invalid argument'),
    ('ssn_gen_inputs_philox_f32', (gi(v=X, amp=None), None), INV, 'ssn_gen_inputs_philox: invalid argument'),

    # ---- generator.  W, ext, time_avg, dyn_row, rate_row, traj, df, B, NB, M, g, stream
    (GEN_F, (None, None, None, None, None, None, None, 0, 3, 8, None, None), 0, SAME),
    (GEN_F, (None, None, None, None, None, None, None, 3, 0, 8, None, None), 0, SAME),
    (GEN_F, (None, X, X, X, X, None, None, 1, 1, 8, gp(), None), INV, 'ssn_gen_forward: ' + M_GEN),
    (GEN_F, (X, None, X, X, X, None, None, 1, 1, 8, gp(), None), INV, 'ssn_gen_forward: ' + M_GEN),
    (GEN_F, (X, X, None, X, X, None, None, 1, 1, 8, gp(), None), INV, 'ssn_gen_forward: ' + M_GEN),
    (GEN_F, (X, X, X, None, X, None, None, 1, 1, 8, gp(), None), INV, 'ssn_gen_forward: ' + M_GEN),
    (GEN_F, (X, X, X, X, None, None, None, 1, 1, 8, gp(), None), INV, 'ssn_gen_forward: ' + M_GEN),
    (GEN_F, (X, X, X, X, X, X, None, 1, 1, 8, gp(), None), INV, 'ssn_gen_forward: ' + M_GEN),
    (GEN_F, (X, X, X, X, X, None, X, 1, 1, 8, gp(), None), INV, 'ssn_gen_forward: ' + M_GEN),
    (GEN_F, (X, X, X, X, X, None, None, 1, 1, 8, None, None), INV, 'ssn_gen_forward: ' + M_GEN),
    (GEN_F, (X, X, X, X, X, None, None, 1, 1, 7, gp(), None), INV, 'ssn_gen_forward: ' + M_GEN),
    (GEN_F, (X, X, X, X, X, None, None, 1, 1, 0, gp(), None), INV, 'ssn_gen_forward: ' + M_GEN),
    (GEN_F, (X, X, X, X, X, None, None, 1, 1, 4000, gp(), None), INV, 'ssn_gen_forward: ' + M_GEN),
    (GEN_F, (X, X, X, X, X, None, None, 1, 1, 8, gp(seqlen=0, skip_steps=0), None), INV, 'ssn_gen_forward: ' + M_GEN),
    (GEN_F, (X, X, X, X, X, None, None, 1, 1, 8, gp(skip_steps=-1), None), INV, 'ssn_gen_forward: ' + M_GEN),
    (GEN_F, (X, X, X, X, X, None, None, 1, 1, 8, gp(skip_steps=10), None), INV, 'ssn_gen_forward: ' + M_GEN),
    (GEN_F, (X, X, X, X, X, None, None, 1, 1, 8, gp(kernel=-1), None), INV, 'ssn_gen_forward: ' + M_GEN),
    (GEN_F, (X, X, X, X, X, None, None, 1, 1, 8, gp(kernel=7), None), INV, 'ssn_gen_forward: ' + M_GEN),
    (GEN_F, (X, X, X, X, X, None, None, 1, 1, 8, gp(kernel=9), None), INV, 'ssn_gen_forward: ' + M_GEN),
    (GEN_F, (X, X, X, X, X, None, None, 1, 1, 8, gp(io_type=3), None), INV, 'ssn_gen_forward: ' + M_GEN),
    (GEN_F, (X, X, X, X, X, None, None, 1, 1, 8, gp(io_type=-1), None), INV, 'ssn_gen_forward: ' + M_GEN),
    ('ssn_gen_forward_f32', (X, X, X, X, X, None, None, 1, 1, 8, gp(kernel=2), None), INV, 'ssn_gen_forward: ' + M_MFMA),
    ('ssn_gen_forward_f32', (X, X, X, X, X, None, None, 1, 3, 8, gp(kernel=8), None), INV, 'ssn_gen_forward: ' + M_MFMA),
    ('ssn_gen_forward_f32', (X, X, X, X, X, None, None, 1, 4, 210, gp(kernel=3), None), INV, 'ssn_gen_forward: ' + M_MFMA),
    ('ssn_gen_forward_f32', (X, X, X, X, X, X, X, 1, 8, 200, gp(kernel=2, seqlen=400000, skip_steps=0), None), INV,
     'ssn_gen_forward: ' + M_MFMA),
    ('ssn_gen_forward_f32', (X, X, X, X, X, None, None, 1, 4, 8, gp(kernel=4, io_type=0), None), INV,
     'ssn_gen_forward: ' + M_SPLIT),
    ('ssn_gen_forward_f32', (X, X, X, X, X, None, None, 1, 4, 8, gp(kernel=8, io_type=1), None), INV,
     'ssn_gen_forward: ' + M_SPLIT),
    ('ssn_gen_forward_f32', (X, X, X, X, X, None, None, 1, 4, 8, gp(kernel=5, rate_hard_bound=5e4), None), INV,
     'ssn_gen_forward: ' + M_SPLIT),
    ('ssn_gen_forward_f32', (X, X, X, X, X, None, None, 1, 4, 8, gp(kernel=6, dt=2.), None), INV,
     'ssn_gen_forward: ' + M_SPLIT),
    ('ssn_gen_forward_variant', (1, 1, 7, 10, 0, byref(gp())), -1, 'ssn_gen_forward: ' + M_GEN),
    ('ssn_gen_forward_variant', (1, 1, 8, 10, 0, byref(gp(kernel=2))), -1, 'ssn_gen_forward: ' + M_MFMA),
    ('ssn_gen_forward_variant', (1, 1, 8, 10, 0, None), -1, SAME),
    ('ssn_gen_forward_variant', (0, 1, 8, 10, 0, byref(gp())), -1, SAME),
    # W, traj, df_delta, g_time_avg, c_dyn, c_rate, B, NB, M, g, stream
    (GEN_B, (None, None, None, None, 1., 1., 0, 3, 8, None, None), 0, SAME),
    (GEN_B, (None, None, None, None, 1., 1., 3, 0, 8, None, None), 0, SAME),
    (GEN_B, (None, X, X, X, 1., 1., 1, 1, 8, gp(), None), INV, 'ssn_gen_backward: ' + M_GEN),
    (GEN_B, (X, None, X, X, 1., 1., 1, 1, 8, gp(), None), INV, 'ssn_gen_backward: ' + M_GEN),
    (GEN_B, (X, X, None, X, 1., 1., 1, 1, 8, gp(), None), INV, 'ssn_gen_backward: ' + M_GEN),
    (GEN_B, (X, X, X, None, 1., 1., 1, 1, 8, gp(), None), INV, 'ssn_gen_backward: ' + M_GEN),
    (GEN_B, (X, X, X, X, 1., 1., 1, 1, 8, None, None), INV, 'ssn_gen_backward: ' + M_GEN),
    (GEN_B, (X, X, X, X, 1., 1., 1, 1, 7, gp(), None), INV, 'ssn_gen_backward: ' + M_GEN),
    (GEN_B, (X, X, X, X, 1., 1., 1, 1, 0, gp(), None), INV, 'ssn_gen_backward: ' + M_GEN),
    (GEN_B, (X, X, X, X, 1., 1., 1, 1, 8, gp(seqlen=0, skip_steps=0), None), INV, 'ssn_gen_backward: ' + M_GEN),
    (GEN_B, (X, X, X, X, 1., 1., 1, 1, 8, gp(skip_steps=10), None), INV, 'ssn_gen_backward: ' + M_GEN),
    (GEN_B, (X, X, X, X, 1., 1., 1, 1, 8, gp(kernel=7), None), INV, 'ssn_gen_backward: ' + M_GEN),
    (GEN_B, (X, X, X, X, 1., 1., 1, 1, 8, gp(kernel=9), None), INV, 'ssn_gen_backward: ' + M_GEN),
    ('ssn_gen_backward_f32', (X, X, X, X, 1., 1., 1, 1, 8, gp(kernel=2), None), INV, 'ssn_gen_backward: ' + M_MFMA),
    ('ssn_gen_backward_f32', (X, X, X, X, 1., 1., 1, 4, 210, gp(kernel=4), None), INV, 'ssn_gen_backward: ' + M_MFMA),
    # W, traj, df_delta, g_time_avg, g_ext, c_dyn, c_rate, B, NB, M, g, stream
    (GEN_BE, (None, None, None, None, None, 1., 1., 0, 3, 8, None, None), 0, SAME),
    (GEN_BE, (None, X, X, X, X, 1., 1., 1, 1, 8, gp(), None), INV, 'ssn_gen_backward: ' + M_GEN),
    (GEN_BE, (X, X, X, None, None, 1., 1., 1, 1, 8, gp(), None), INV, 'ssn_gen_backward: ' + M_GEN),
    (GEN_BE, (X, X, X, X, X, 1., 1., 1, 1, 7, gp(), None), INV, 'ssn_gen_backward: ' + M_GEN),
    (GEN_BE, (X, X, X, X, X, 1., 1., 1, 1, 8, gp(kernel=7), None), INV, 'ssn_gen_backward: ' + M_GEN),
    ('ssn_gen_backward_ext_f32', (X, X, X, X, X, 1., 1., 1, 1, 8, gp(kernel=8), None), INV, 'ssn_gen_backward: ' + M_MFMA),
    # W, traj, df_delta, g_time_avg, g_ext, dmax, tracked, c_dyn, c_rate, B, NB, M, g, stream
    ('ssn_gen_backward_max_f32', (None, None, None, None, None, None, None, 1., 1., 0, 3, 8, None, None), 0, SAME),
    ('ssn_gen_backward_max_f32', (None, X, X, X, X, X, None, 1., 1., 1, 1, 8, gp(), None), INV, 'ssn_gen_backward: ' + M_GEN),
    ('ssn_gen_backward_max_f32', (X, X, X, X, X, X, byref(TICKET), 1., 1., 1, 1, 7, gp(), None), INV,
     'ssn_gen_backward: ' + M_GEN),
    ('ssn_gen_backward_max_f32', (X, X, X, X, X, X, None, 1., 1., 1, 1, 8, gp(kernel=9), None), INV,
     'ssn_gen_backward: ' + M_GEN),
    ('ssn_gen_backward_max_f32', (X, X, X, X, X, X, None, 1., 1., 1, 1, 8, gp(kernel=2), None), INV,
     'ssn_gen_backward: ' + M_MFMA),
    # W, traj, df, g_time_avg, g_ext, gW, dmax, xmax, c_dyn, c_rate, B, NB, M, p, stream
    ('ssn_gen_backward_fused_f32', (None, None, None, None, None, None, None, 1., 1., 1., 0, 3, 8, None, None), 0, SAME),
    ('ssn_gen_backward_fused_f32', (None, None, None, None, None, None, None, 1., 1., 1., 3, 0, 8, None, None), 0, SAME),
    ('ssn_gen_backward_fused_f32', (X, X, X, X, X, X, None, 1., 1., 1., 1, 1, 8, None, None), INV, M_FUSED),
    ('ssn_gen_backward_fused_f32', (None, X, X, X, X, X, None, 1., 1., 1., 1, 1, 8, gp(), None), INV, M_FUSED),
    ('ssn_gen_backward_fused_f32', (X, None, X, X, X, X, None, 1., 1., 1., 1, 1, 8, gp(), None), INV, M_FUSED),
    ('ssn_gen_backward_fused_f32', (X, X, None, X, X, X, None, 1., 1., 1., 1, 1, 8, gp(), None), INV, M_FUSED),
    ('ssn_gen_backward_fused_f32', (X, X, X, None, X, X, None, 1., 1., 1., 1, 1, 8, gp(), None), INV, M_FUSED),
    ('ssn_gen_backward_fused_f32', (X, X, X, X, X, None, None, 1., 1., 1., 1, 1, 8, gp(), None), INV, M_FUSED),
    ('ssn_gen_backward_fused_f32', (X, X, X, X, X, X, None, 1., 1., 1., -1, 1, 8, gp(), None), INV, M_FUSED),
    ('ssn_gen_backward_fused_f32', (X, X, X, X, X, X, None, 1., 1., 1., 1, 9, 8, gp(), None), INV, M_FUSED),
    ('ssn_gen_backward_fused_f32', (X, X, X, X, X, X, None, 1., 1., 1., 1, 1, 7, gp(), None), INV, M_FUSED),
    ('ssn_gen_backward_fused_f32', (X, X, X, X, X, X, None, 1., 1., 1., 1, 1, 210, gp(), None), INV, M_FUSED),
    ('ssn_gen_backward_fused_f32', (X, X, X, X, X, X, None, 0., 1., 1., 1, 1, 8, gp(), None), INV, M_FUSED),
    ('ssn_gen_backward_fused_f32', (X, X, X, X, X, X, None, INF, 1., 1., 1, 1, 8, gp(), None), INV, M_FUSED),
    ('ssn_gen_backward_fused_f32', (X, X, X, X, X, X, None, 1., 1., 1., 1, 1, 8, gp(skip_steps=10), None), INV, M_FUSED),
    ('ssn_gen_backward_fused_f32', (X, X, X, X, X, X, None, 1., 1., 1., 1, 1, 8, gp(skip_steps=-1), None), INV, M_FUSED),
    # a, stream
    ('ssn_gen_grads_f32', (None, None), INV, 'ssn_gen_grads: invalid argument'),
    ('ssn_gen_grads_f32', (gg(jds_part=None), None), INV, 'ssn_gen_grads: invalid argument'),
    ('ssn_gen_grads_f32', (gg(B=-1), None), INV, 'ssn_gen_grads: invalid argument'),
    ('ssn_gen_grads_f32', (gg(nv=-1), None), INV, 'ssn_gen_grads: invalid argument'),
    ('ssn_gen_grads_f32', (gg(nv=3), None), INV, 'ssn_gen_grads: invalid argument'),
    ('ssn_gen_grads_f32', (gg(dmean=None), None), INV, 'ssn_gen_grads: invalid argument'),
    ('ssn_gen_grads_f32', (gg(ws=None), None), INV, 'ssn_gen_grads: invalid argument'),
    ('ssn_gen_grads_f32', (gg(out=None), None), INV, 'ssn_gen_grads: invalid argument'),
    ('ssn_gen_grads_f32', (gg(nv=1, g_ext=None), None), INV, 'ssn_gen_grads: invalid argument'),
    ('ssn_gen_grads_f32', (gg(nv=2, zin=None), None), INV, 'ssn_gen_grads: invalid argument'),
    ('ssn_gen_grads_f32', (gg(nv=1, NB=0), None), INV, 'ssn_gen_grads: invalid argument'),
    ('ssn_gen_grads_f32', (gg(nv=1, M=3), None), INV, 'ssn_gen_grads: invalid argument'),
    # params, grads, s1, s2, n, opt, clip_lo, clip_hi, record, stream
    ('ssn_gen_apply_f32', (None, X, X, X, 4, op(), None, None, None, None), INV, 'ssn_gen_apply: invalid argument'),
    ('ssn_gen_apply_f32', (X, None, X, X, 4, op(), None, None, None, None), INV, 'ssn_gen_apply: invalid argument'),
    ('ssn_gen_apply_f32', (X, X, X, X, 0, op(), None, None, None, None), INV, 'ssn_gen_apply: invalid argument'),
    ('ssn_gen_apply_f32', (X, X, X, X, -1, op(), None, None, None, None), INV, 'ssn_gen_apply: invalid argument'),
    ('ssn_gen_apply_f32', (X, X, X, X, 4, op(), X, None, None, None), INV, 'ssn_gen_apply: invalid argument'),
    ('ssn_gen_apply_f32', (X, X, X, X, 4, op(), None, X, None, None), INV, 'ssn_gen_apply: invalid argument'),
    ('ssn_gen_apply_f32', (X, X, X, X, 4, None, X, X, X, None), INV, 'ssn_optimizer_step: invalid argument'),
    ('ssn_gen_apply_f32', (X, X, X, X, 4, op(kind=3), X, X, X, None), INV, 'ssn_optimizer_step: invalid argument'),

    # ---- weight and parameter gradients.  delta, traj, gW, B, K, M, kernel, stream
    (pair('ssn_weight_grad'), (X, X, X, -1, 1, 2, 0, None), INV, 'ssn_weight_grad: invalid argument'),
    (pair('ssn_weight_grad'), (X, X, X, 1, -1, 2, 0, None), INV, 'ssn_weight_grad: invalid argument'),
    (pair('ssn_weight_grad'), (X, X, X, 1, 1, -1, 0, None), INV, 'ssn_weight_grad: invalid argument'),
    (pair('ssn_weight_grad'), (X, X, None, 1, 0, 2, 0, None), INV, 'ssn_weight_grad: invalid argument'),
    (pair('ssn_weight_grad'), (None, X, X, 1, 1, 2, 0, None), INV, 'ssn_weight_grad: invalid argument'),
    (pair('ssn_weight_grad'), (X, None, X, 1, 1, 2, 0, None), INV, 'ssn_weight_grad: invalid argument'),
    # delta, traj, gW, B, K, M, dmax, xmax, stream
    ('ssn_weight_grad_scaled_f32', (None, X, X, 1, 1, 2, X, 1., None), INV, M_WGS),
    ('ssn_weight_grad_scaled_f32', (X, None, X, 1, 1, 2, X, 1., None), INV, M_WGS),
    ('ssn_weight_grad_scaled_f32', (X, X, None, 1, 1, 2, X, 1., None), INV, M_WGS),
    ('ssn_weight_grad_scaled_f32', (X, X, X, 1, 1, 2, None, 1., None), INV, M_WGS),
    ('ssn_weight_grad_scaled_f32', (X, X, X, -1, 1, 2, X, 1., None), INV, M_WGS),
    ('ssn_weight_grad_scaled_f32', (X, X, X, 1, -1, 2, X, 1., None), INV, M_WGS),
    ('ssn_weight_grad_scaled_f32', (X, X, X, 1, 1, 0, X, 1., None), INV, M_WGS),
    ('ssn_weight_grad_scaled_f32', (X, X, X, 1, 1, 226, X, 1., None), INV, M_WGS),
    ('ssn_weight_grad_scaled_f32', (X, X, X, 1, 1, 2, X, 0., None), INV, M_WGS),
    ('ssn_weight_grad_scaled_f32', (X, X, X, 1, 1, 2, X, INF, None), INV, M_WGS),
    ('ssn_weight_grad_scaled_f32', (X, X, X, 1, 1, 2, X, NAN, None), INV, M_WGS),
    ('ssn_weight_grad_scaled_f32', (X, X, X, 1, 1 << 27, 4, X, 1., None), INV, M_WGS),
    # n, x, bounds, out [, ws]
    ('ssn_segment_sqnorms2_f32', (X, X, -1, X, X, None), INV, 'ssn_segment_sqnorms2: invalid argument'),
    ('ssn_segment_sqnorms2_f32', (None, X, 1, X, X, None), INV, 'ssn_segment_sqnorms2: invalid argument'),
    ('ssn_segment_sqnorms2_f32', (X, None, 1, X, X, None), INV, 'ssn_segment_sqnorms2: invalid argument'),
    ('ssn_segment_sqnorms2_f32', (X, X, 1, None, X, None), INV, 'ssn_segment_sqnorms2: invalid argument'),
    ('ssn_segment_sqnorms2_f32', (X, X, 1, X, None, None), INV, 'ssn_segment_sqnorms2: invalid argument'),
    ('ssn_segment_sqnorms_f32', (X, X, -1, X, None), INV, 'ssn_segment_sqnorms: invalid argument'),
    ('ssn_segment_sqnorms_f32', (None, X, 1, X, None), INV, 'ssn_segment_sqnorms: invalid argument'),
    ('ssn_segment_sqnorms_f32', (X, None, 1, X, None), INV, 'ssn_segment_sqnorms: invalid argument'),
    ('ssn_segment_sqnorms_f32', (X, X, 1, None, None), INV, 'ssn_segment_sqnorms: invalid argument'),
    ('ssn_segment_sqnorms_f32', (None, None, 0, None, None), 0, SAME),
    # g, ids, probes, g_ta, n, B, NB, M, stream
    (pair('ssn_probe_scatter'), (X, X, X, X, -1, 1, 1, 1, None), INV, 'ssn_probe_scatter: invalid argument'),
    (pair('ssn_probe_scatter'), (X, X, X, X, 1, -1, 1, 1, None), INV, 'ssn_probe_scatter: invalid argument'),
    (pair('ssn_probe_scatter'), (X, X, X, X, 1, 1, -1, 1, None), INV, 'ssn_probe_scatter: invalid argument'),
    (pair('ssn_probe_scatter'), (X, X, X, X, 1, 1, 1, -1, None), INV, 'ssn_probe_scatter: invalid argument'),
    (pair('ssn_probe_scatter'), (X, X, X, None, 0, 1, 1, 1, None), INV, 'ssn_probe_scatter: invalid argument'),
    (pair('ssn_probe_scatter'), (None, X, X, X, 1, 0, 1, 1, None), INV, 'ssn_probe_scatter: invalid argument'),
    (pair('ssn_probe_scatter'), (X, None, X, X, 1, 0, 1, 1, None), INV, 'ssn_probe_scatter: invalid argument'),
    (pair('ssn_probe_scatter'), (X, X, None, X, 1, 0, 1, 1, None), INV, 'ssn_probe_scatter: invalid argument'),
    # dyn, rate, n, scale_dyn, scale_rate, ws, out, stream
    (PM, (X, X, -1, 1., 1., X, X, None), INV, 'ssn_penalty_means: invalid argument'),
    (PM, (X, X, 1, 1., 1., None, X, None), INV, 'ssn_penalty_means: invalid argument'),
    (PM, (X, X, 1, 1., 1., X, None, None), INV, 'ssn_penalty_means: invalid argument'),
    (PM, (None, X, 1, 1., 1., X, X, None), INV, 'ssn_penalty_means: invalid argument'),
    (PM, (X, None, 1, 1., 1., X, X, None), INV, 'ssn_penalty_means: invalid argument'),
    # ... time_avg, ids, probes, tc, nsamp, NB, M, stream
    (PMP, (X, X, -1, 1., 1., X, X, X, X, X, X, 1, 1, 1, None), INV, 'ssn_penalty_means_probe: invalid argument'),
    (PMP, (X, X, 1, 1., 1., None, X, X, X, X, X, 1, 1, 1, None), INV, 'ssn_penalty_means_probe: invalid argument'),
    (PMP, (X, X, 1, 1., 1., X, None, X, X, X, X, 1, 1, 1, None), INV, 'ssn_penalty_means_probe: invalid argument'),
    (PMP, (None, X, 1, 1., 1., X, X, X, X, X, X, 1, 1, 1, None), INV, 'ssn_penalty_means_probe: invalid argument'),
    (PMP, (X, None, 1, 1., 1., X, X, X, X, X, X, 1, 1, 1, None), INV, 'ssn_penalty_means_probe: invalid argument'),
    (PMP, (X, X, 1, 1., 1., X, X, X, X, X, X, -1, 1, 1, None), INV, 'ssn_penalty_means_probe: invalid argument'),
    (PMP, (X, X, 1, 1., 1., X, X, X, X, X, X, 1, -1, 1, None), INV, 'ssn_penalty_means_probe: invalid argument'),
    (PMP, (X, X, 1, 1., 1., X, X, X, X, X, X, 1, 1, -1, None), INV, 'ssn_penalty_means_probe: invalid argument'),
    (PMP, (X, X, 1, 1., 1., X, X, None, X, X, X, 1, 1, 1, None), INV, 'ssn_penalty_means_probe: invalid argument'),
    (PMP, (X, X, 1, 1., 1., X, X, X, None, X, X, 1, 1, 1, None), INV, 'ssn_penalty_means_probe: invalid argument'),
    (PMP, (X, X, 1, 1., 1., X, X, X, X, None, X, 1, 1, 1, None), INV, 'ssn_penalty_means_probe: invalid argument'),
    (PMP, (X, X, 1, 1., 1., X, X, X, X, X, None, 1, 1, 1, None), INV, 'ssn_penalty_means_probe: invalid argument'),

    # ---- critic: every family names the entry that was called; an empty batch returns first in the plain and leaky passes
    # params, dims, nlayers, x, cond, batch, hide_cell_type, out, workspace, precision, stream
    ('ssn_critic_forward', (None, None, 9, None, None, 0, 0, None, None, 1, None), 0, SAME),
    ('ssn_critic_forward', (None, None, 9, None, None, 4, 0, None, None, 1, None), INV, 'ssn_critic_forward: ' + M_LAYOUT),
    ('ssn_critic_forward', (None, None, -1, None, None, 4, 0, None, None, 1, None), INV, 'ssn_critic_forward: ' + M_LAYOUT),
    ('ssn_critic_loss_grad', (None, None, 9) + (None,) * 6 + (4, 4, 4, 10., 0, None, None, None, None, 1, None), INV,
     'ssn_critic_loss_grad: ' + M_LAYOUT),
    ('ssn_critic_loss_grad', (None, None, -1) + (None,) * 6 + (4, 4, 4, 10., 0, None, None, None, None, 1, None), INV,
     'ssn_critic_loss_grad: ' + M_LAYOUT),
    ('ssn_critic_input_grad', (None, None, 9, None, None, 0, 0, 1., None, None, None, 1, None), 0, SAME),
    ('ssn_critic_input_grad', (None, None, 9, None, None, 4, 0, 1., None, None, None, 1, None), INV,
     'ssn_critic_input_grad: ' + M_LAYOUT),
    # ... hide_cell_type, leak, ...
    ('ssn_critic_forward_leaky', (None, None, 9, None, None, 0, 0, .5, None, None, 1, None), 0, SAME),
    ('ssn_critic_forward_leaky', (None, None, 9, None, None, 4, 0, .5, None, None, 1, None), INV,
     'ssn_critic_forward_leaky: ' + M_LAYOUT),
    ('ssn_critic_forward_leaky', (None, DIMS, 2, None, None, 4, 0, 2., None, None, 1, None), INV,
     'ssn_critic_forward_leaky: ' + M_LAYOUT),
    ('ssn_critic_forward_leaky', (None, DIMS, 2, None, None, 4, 0, -.1, None, None, 1, None), INV,
     'ssn_critic_forward_leaky: ' + M_LAYOUT),
    ('ssn_critic_forward_leaky', (None, DIMS, 2, None, None, 4, 0, NAN, None, None, 1, None), INV,
     'ssn_critic_forward_leaky: ' + M_LAYOUT),
    ('ssn_critic_loss_grad_leaky', (None, None, 9) + (None,) * 6 + (4, 4, 4, 10., 0, .5, None, None, None, None, 1, None), INV,
     'ssn_critic_loss_grad_leaky: ' + M_LAYOUT),
    ('ssn_critic_loss_grad_leaky', (None, DIMS, 2) + (None,) * 6 + (4, 4, 4, 10., 0, 2., None, None, None, None, 1, None), INV,
     'ssn_critic_loss_grad_leaky: ' + M_LAYOUT),
    ('ssn_critic_input_grad_leaky', (None, None, 9, None, None, 0, 0, .5, 1., None, None, None, 1, None), 0, SAME),
    ('ssn_critic_input_grad_leaky', (None, None, 9, None, None, 4, 0, .5, 1., None, None, None, 1, None), INV,
     'ssn_critic_input_grad_leaky: ' + M_LAYOUT),
    ('ssn_critic_input_grad_leaky', (None, DIMS, 2, None, None, 4, 0, 2., 1., None, None, None, 1, None), INV,
     'ssn_critic_input_grad_leaky: ' + M_LAYOUT),
    # params, dims, layer_norm, nlayers, ...
    ('ssn_critic_forward_norm', (None, None, None, 9, None, None, 4, 0, None, None, 1, None), INV,
     'ssn_critic_forward_norm: ' + M_LAYOUT),
    ('ssn_critic_forward_norm', (None, DIMS, ints(0, 3), 2, None, None, 4, 0, None, None, 1, None), INV,
     'ssn_critic_forward_norm: ' + M_FLAGS01),
    ('ssn_critic_forward_norm', (None, DIMS, ints(-1, 0), 2, None, None, 4, 0, None, None, 1, None), INV,
     'ssn_critic_forward_norm: ' + M_FLAGS01),
    ('ssn_critic_loss_grad_norm', (None, None, None, 9) + (None,) * 6 + (4, 4, 4, 10., 0, None, None, None, None, 1, None), INV,
     'ssn_critic_loss_grad_norm: ' + M_LAYOUT),
    ('ssn_critic_loss_grad_norm', (None, DIMS, ints(2, 0), 2) + (None,) * 6 + (4, 4, 4, 10., 0, None, None, None, None, 1, None),
     INV, 'ssn_critic_loss_grad_norm: ' + M_FLAGS01),
    ('ssn_critic_input_grad_norm', (None, None, None, 9, None, None, 4, 0, 1., None, None, None, 1, None), INV,
     'ssn_critic_input_grad_norm: ' + M_LAYOUT),
    ('ssn_critic_input_grad_norm', (None, DIMS, ints(0, 2), 2, None, None, 4, 0, 1., None, None, None, 1, None), INV,
     'ssn_critic_input_grad_norm: ' + M_FLAGS01),
    # params, dims, layer_norm, nlayers, leak, xg, cg, xd, cd, ng, nd, hide_cell_type, acc, dvals, workspace, precision, stream
    ('ssn_critic_accuracy', (None, None, None, 9, 0.) + (None,) * 4 + (4, 4, 0, None, None, None, 1, None), INV,
     'ssn_critic_accuracy: ' + M_LAYOUT),
    ('ssn_critic_accuracy', (None, DIMS, None, 2, 1.5) + (None,) * 4 + (4, 4, 0, None, None, None, 1, None), INV,
     'ssn_critic_accuracy: ' + M_LAYOUT),
    ('ssn_critic_accuracy', (None, DIMS, ints(3, 0), 2, 0.) + (None,) * 4 + (4, 4, 0, None, None, None, 1, None), INV,
     'ssn_critic_accuracy: ' + M_FLAGS01),
    ('ssn_critic_accuracy', (None, DIMS, ints(1, 0), 2, .5) + (None,) * 4 + (4, 4, 0, None, None, None, 1, None), INV,
     'ssn_critic_accuracy: ' + M_LEAKNORM),
    # params, dims, layer_flags, nlayers, act, ...
    ('ssn_critic_forward_act', (None, at(DIMS), None, 2, 8, None, None, 4, 0, None, None, 1, None), INV,
     'ssn_critic_forward_act: ' + M_ACT),
    ('ssn_critic_forward_act', (None, at(DIMS), None, 2, -1, None, None, 4, 0, None, None, 1, None), INV,
     'ssn_critic_forward_act: ' + M_ACT),
    ('ssn_critic_forward_act', (None, None, None, 9, 0, None, None, 4, 0, None, None, 1, None), INV,
     'ssn_critic_forward_act: ' + M_LAYOUT),
    ('ssn_critic_forward_act', (None, at(DIMS), at(FLAGS_02), 2, 0, None, None, 4, 0, None, None, 1, None), INV,
     'ssn_critic_forward_act: ' + M_LAYOUT),
    ('ssn_critic_forward_act', (None, at(DIMS), at(FLAGS_40), 2, 4, None, None, 4, 0, None, None, 1, None), INV,
     'ssn_critic_forward_act: ' + M_LAYOUT),
    ('ssn_critic_loss_grad_act', (None, at(DIMS), None, 2, 8) + (None,) * 6 + (4, 4, 4, 10., 0, None, None, None, None, 1, None),
     INV, 'ssn_critic_loss_grad_act: ' + M_ACT),
    ('ssn_critic_loss_grad_act', (None, None, None, 9, 0) + (None,) * 6 + (4, 4, 4, 10., 0, None, None, None, None, 1, None),
     INV, 'ssn_critic_loss_grad_act: ' + M_LAYOUT),
    ('ssn_critic_input_grad_act', (None, at(DIMS), None, 2, 8, None, None, 4, 0, 1., None, None, None, 1, None), INV,
     'ssn_critic_input_grad_act: ' + M_ACT),
    ('ssn_critic_input_grad_act', (None, None, None, 9, 0, None, None, 4, 0, 1., None, None, None, 1, None), INV,
     'ssn_critic_input_grad_act: ' + M_LAYOUT),
    ('ssn_critic_accuracy_act', (None, at(DIMS), None, 2, 8) + (None,) * 4 + (4, 4, 0, None, None, None, 1, None), INV,
     'ssn_critic_accuracy_act: ' + M_ACT),
    ('ssn_critic_accuracy_act', (None, None, None, 9, 0) + (None,) * 4 + (4, 4, 0, None, None, None, 1, None), INV,
     'ssn_critic_accuracy_act: ' + M_LAYOUT),
    # p, g, s1, s2, n, o, stream
    ('ssn_optimizer_step', (X, X, X, X, 4, None, None), INV, 'ssn_optimizer_step: invalid argument'),
    ('ssn_optimizer_step', (X, X, X, X, -1, op(), None), INV, 'ssn_optimizer_step: invalid argument'),
    ('ssn_optimizer_step', (X, X, X, X, 4, op(kind=3), None), INV, 'ssn_optimizer_step: invalid argument'),
    ('ssn_optimizer_step', (X, X, X, X, 4, op(kind=-1), None), INV, 'ssn_optimizer_step: invalid argument'),
    # a, stream
    ('ssn_critic_step_run', (None, None), INV, 'ssn_critic_step_run: invalid argument'),
    ('ssn_critic_step_run', (cs(n=0), None), INV, 'ssn_critic_step_run: invalid argument'),
    ('ssn_critic_step_run', (cs(n=-4), None), INV, 'ssn_critic_step_run: invalid argument'),
    ('ssn_critic_step_run', (cs(nseg=-1), None), INV, 'ssn_critic_step_run: invalid argument'),
    ('ssn_critic_step_run', (cs(params=None), None), INV, 'ssn_critic_step_run: invalid argument'),
    ('ssn_critic_step_run', (cs(dims=None), None), INV, 'ssn_critic_step_run: invalid argument'),
    ('ssn_critic_step_run', (cs(xg=None), None), INV, 'ssn_critic_step_run: invalid argument'),
    ('ssn_critic_step_run', (cs(xd=None), None), INV, 'ssn_critic_step_run: invalid argument'),
    ('ssn_critic_step_run', (cs(eps=None), None), INV, 'ssn_critic_step_run: invalid argument'),
    ('ssn_critic_step_run', (cs(xp=None), None), INV, 'ssn_critic_step_run: invalid argument'),
    ('ssn_critic_step_run', (cs(grads=None), None), INV, 'ssn_critic_step_run: invalid argument'),
    ('ssn_critic_step_run', (cs(stats=None), None), INV, 'ssn_critic_step_run: invalid argument'),
    ('ssn_critic_step_run', (cs(dvals=None), None), INV, 'ssn_critic_step_run: invalid argument'),
    ('ssn_critic_step_run', (cs(workspace=None), None), INV, 'ssn_critic_step_run: invalid argument'),
    ('ssn_critic_step_run', (cs(opt=None), None), INV, 'ssn_critic_step_run: invalid argument'),
    ('ssn_critic_step_run', (cs(acc_dvals=None), None), INV, 'ssn_critic_step_run: invalid argument'),
    ('ssn_critic_step_run', (cs(tail=None), None), INV, 'ssn_critic_step_run: invalid argument'),
    ('ssn_critic_step_run', (cs(nlayers=9), None), INV, 'ssn_critic_step_run: ' + M_LAYOUT),
    ('ssn_critic_step_run', (cs(leak=2.), None), INV, 'ssn_critic_step_run: ' + M_LAYOUT),
    ('ssn_critic_step_run', (cs(layer_norm=ints(0, 3)), None), INV, 'ssn_critic_step_run: ' + M_FLAGS01),
    ('ssn_critic_step_run', (cs(layer_norm=ints(1, 0), leak=.5), None), INV, 'ssn_critic_step_run: ' + M_LEAKNORM),
    # a, rate_penalty_bound, stream
    ('ssn_critic_step_gated_run', (None, 1., None), INV, M_GATED),
    ('ssn_critic_step_gated_run', (cs(pens64=None), 1., None), INV, M_GATED),
    ('ssn_critic_step_gated_run', (cs(), 0., None), INV, M_GATED),
    ('ssn_critic_step_gated_run', (cs(), -1., None), INV, M_GATED),
    ('ssn_critic_step_gated_run', (cs(), NAN, None), INV, M_GATED),
    ('ssn_critic_step_gated_run', (cs(n=0), 1., None), INV, 'ssn_critic_step_run: invalid argument'),
    ('ssn_critic_step_gated_run', (cs(nlayers=9), 1., None), INV, 'ssn_critic_step_run: ' + M_LAYOUT),
    # eps, xd, xg, xp, rows, cols, stream
    ('ssn_interpolate_f32', (X, X, X, X, -1, 3, None), INV, 'ssn_interpolate: invalid argument'),
    ('ssn_interpolate_f32', (X, X, X, X, 3, -1, None), INV, 'ssn_interpolate: invalid argument'),
    ('ssn_interpolate_f32', (None, X, X, X, 1, 1, None), INV, 'ssn_interpolate: invalid argument'),
    ('ssn_interpolate_f32', (X, None, X, X, 1, 1, None), INV, 'ssn_interpolate: invalid argument'),
    ('ssn_interpolate_f32', (X, X, None, X, 1, 1, None), INV, 'ssn_interpolate: invalid argument'),
    ('ssn_interpolate_f32', (X, X, X, None, 1, 1, None), INV, 'ssn_interpolate: invalid argument'),

    # ---- feed-forward model
    # RF_w, conn_idx, conn_str, ncon, TH_sam, stim, out, q, den, p, stream
    ('ssn_ff_forward_sparse_f32', (X, X, X, 1, X, X, X, X, X, None, None), INV, 'ssn_ff_forward_sparse: invalid argument'),
    ('ssn_ff_forward_sparse_f32', (X, X, X, 1, X, X, X, X, X, fp(nsam=-1), None), INV, 'ssn_ff_forward_sparse: invalid argument'),
    ('ssn_ff_forward_sparse_f32', (X, X, X, 1, X, X, X, X, X, fp(nhid=0), None), INV, 'ssn_ff_forward_sparse: invalid argument'),
    ('ssn_ff_forward_sparse_f32', (X, X, X, 1, X, X, X, X, X, fp(ni=0), None), INV, 'ssn_ff_forward_sparse: invalid argument'),
    ('ssn_ff_forward_sparse_f32', (X, X, X, 1, X, X, X, X, X, fp(ni=33), None), INV, 'ssn_ff_forward_sparse: invalid argument'),
    ('ssn_ff_forward_sparse_f32', (X, X, X, 1, X, X, X, X, X, fp(box=0), None), INV, 'ssn_ff_forward_sparse: invalid argument'),
    ('ssn_ff_forward_sparse_f32', (X, X, X, -1, X, X, X, X, X, fp(), None), INV, 'ssn_ff_forward_sparse: invalid argument'),
    ('ssn_ff_forward_sparse_f32', (X, X, X, 1, X, X, X, X, None, fp(), None), INV, 'ssn_ff_forward_sparse: invalid argument'),
    ('ssn_ff_forward_sparse_f32', (X, X, X, 1, X, X, X, None, X, fp(), None), INV, 'ssn_ff_forward_sparse: invalid argument'),
    ('ssn_ff_forward_sparse_f32', (None, X, X, 1, X, X, X, X, X, fp(), None), INV, 'ssn_ff_forward_sparse: invalid argument'),
    ('ssn_ff_forward_sparse_f32', (X, None, X, 1, X, X, X, X, X, fp(), None), INV, 'ssn_ff_forward_sparse: invalid argument'),
    ('ssn_ff_forward_sparse_f32', (X, X, None, 1, X, X, X, X, X, fp(), None), INV, 'ssn_ff_forward_sparse: invalid argument'),
    ('ssn_ff_forward_sparse_f32', (X, X, X, 1, None, X, X, X, X, fp(), None), INV, 'ssn_ff_forward_sparse: invalid argument'),
    ('ssn_ff_forward_sparse_f32', (X, X, X, 1, X, None, X, X, X, fp(), None), INV, 'ssn_ff_forward_sparse: invalid argument'),
    ('ssn_ff_forward_sparse_f32', (X, X, X, 1, X, X, None, X, X, fp(), None), INV, 'ssn_ff_forward_sparse: invalid argument'),
    # RF_w, conn_idx, conn_str, ncon, stim, q, den, gq, dsig, p, stream
    ('ssn_ff_backward_sparse_f32', (X, X, X, 1, X, X, X, X, X, None, None), INV, 'ssn_ff_backward_sparse: invalid argument'),
    ('ssn_ff_backward_sparse_f32', (X, X, X, 1, X, X, X, X, X, fp(nsam=-1), None), INV, 'ssn_ff_backward_sparse: invalid argument'),
    ('ssn_ff_backward_sparse_f32', (X, X, X, 1, X, X, X, X, X, fp(nhid=0), None), INV, 'ssn_ff_backward_sparse: invalid argument'),
    ('ssn_ff_backward_sparse_f32', (X, X, X, 1, X, X, X, X, X, fp(ni=0), None), INV, 'ssn_ff_backward_sparse: invalid argument'),
    ('ssn_ff_backward_sparse_f32', (X, X, X, 1, X, X, X, X, X, fp(ni=33), None), INV, 'ssn_ff_backward_sparse: invalid argument'),
    ('ssn_ff_backward_sparse_f32', (X, X, X, 1, X, X, X, X, X, fp(box=0), None), INV, 'ssn_ff_backward_sparse: invalid argument'),
    ('ssn_ff_backward_sparse_f32', (X, X, X, -1, X, X, X, X, X, fp(), None), INV, 'ssn_ff_backward_sparse: invalid argument'),
    ('ssn_ff_backward_sparse_f32', (X, X, X, 1, X, None, X, X, X, fp(), None), INV, 'ssn_ff_backward_sparse: invalid argument'),
    ('ssn_ff_backward_sparse_f32', (X, X, X, 1, X, X, None, X, X, fp(), None), INV, 'ssn_ff_backward_sparse: invalid argument'),
    ('ssn_ff_backward_sparse_f32', (X, X, X, 1, X, X, X, None, X, fp(), None), INV, 'ssn_ff_backward_sparse: invalid argument'),
    ('ssn_ff_backward_sparse_f32', (X, X, X, 1, X, X, X, X, None, fp(), None), INV, 'ssn_ff_backward_sparse: invalid argument'),
    ('ssn_ff_backward_sparse_f32', (None, X, X, 1, X, X, X, X, X, fp(), None), INV, 'ssn_ff_backward_sparse: invalid argument'),
    ('ssn_ff_backward_sparse_f32', (X, None, X, 1, X, X, X, X, X, fp(), None), INV, 'ssn_ff_backward_sparse: invalid argument'),
    ('ssn_ff_backward_sparse_f32', (X, X, None, 1, X, X, X, X, X, fp(), None), INV, 'ssn_ff_backward_sparse: invalid argument'),
    ('ssn_ff_backward_sparse_f32', (X, X, X, 1, None, X, X, X, X, fp(), None), INV, 'ssn_ff_backward_sparse: invalid argument'),
    # RF_w, FF_con, FF_str, TH_sam, stim, out, q, den, p, stream
    ('ssn_ff_forward_f32', (X, X, X, X, X, X, X, X, None, None), INV, 'ssn_ff_forward: invalid argument'),
    ('ssn_ff_forward_f32', (X, X, X, X, X, X, X, X, fp(nsam=-1), None), INV, 'ssn_ff_forward: invalid argument'),
    ('ssn_ff_forward_f32', (X, X, X, X, X, X, X, X, fp(nhid=0), None), INV, 'ssn_ff_forward: invalid argument'),
    ('ssn_ff_forward_f32', (X, X, X, X, X, X, X, X, fp(ni=0), None), INV, 'ssn_ff_forward: invalid argument'),
    ('ssn_ff_forward_f32', (X, X, X, X, X, X, X, X, fp(ni=33), None), INV, 'ssn_ff_forward: invalid argument'),
    ('ssn_ff_forward_f32', (X, X, X, X, X, X, X, X, fp(box=0), None), INV, 'ssn_ff_forward: invalid argument'),
    ('ssn_ff_forward_f32', (X, X, X, X, X, X, X, None, fp(), None), INV, 'ssn_ff_forward: invalid argument'),
    ('ssn_ff_forward_f32', (X, X, X, X, X, X, None, X, fp(), None), INV, 'ssn_ff_forward: invalid argument'),
    ('ssn_ff_forward_f32', (X + 4, X, X, X, X, X, X, X, fp(), None), INV, 'ssn_ff_forward: ' + M_ALIGN),
    ('ssn_ff_forward_f32', (X, X + 8, X, X, X, X, X, X, fp(), None), INV, 'ssn_ff_forward: ' + M_ALIGN),
    ('ssn_ff_forward_f32', (X, X, X + 12, X, X, X, None, None, fp(box=4), None), INV, 'ssn_ff_forward: ' + M_ALIGN),
    # RF_w, FF_con, FF_str, stim, q, den, gq, dsig, p, stream
    ('ssn_ff_backward_f32', (X, X, X, X, X, X, X, X, None, None), INV, 'ssn_ff_backward: invalid argument'),
    ('ssn_ff_backward_f32', (X, X, X, X, X, X, X, X, fp(nsam=-1), None), INV, 'ssn_ff_backward: invalid argument'),
    ('ssn_ff_backward_f32', (X, X, X, X, X, X, X, X, fp(nhid=0), None), INV, 'ssn_ff_backward: invalid argument'),
    ('ssn_ff_backward_f32', (X, X, X, X, X, X, X, X, fp(ni=0), None), INV, 'ssn_ff_backward: invalid argument'),
    ('ssn_ff_backward_f32', (X, X, X, X, X, X, X, X, fp(ni=33), None), INV, 'ssn_ff_backward: invalid argument'),
    ('ssn_ff_backward_f32', (X, X, X, X, X, X, X, X, fp(box=0), None), INV, 'ssn_ff_backward: invalid argument'),
    ('ssn_ff_backward_f32', (X, X, X, X, None, X, X, X, fp(), None), INV, 'ssn_ff_backward: invalid argument'),
    ('ssn_ff_backward_f32', (X, X, X, X, X, None, X, X, fp(), None), INV, 'ssn_ff_backward: invalid argument'),
    ('ssn_ff_backward_f32', (X, X, X, X, X, X, None, X, fp(), None), INV, 'ssn_ff_backward: invalid argument'),
    ('ssn_ff_backward_f32', (X, X, X, X, X, X, X, None, fp(), None), INV, 'ssn_ff_backward: invalid argument'),
    ('ssn_ff_backward_f32', (X + 4, X, X, X, X, X, X, X, fp(), None), INV, 'ssn_ff_backward: ' + M_ALIGN),
    ('ssn_ff_backward_f32', (X, X + 8, X, X, X, X, X, X, fp(), None), INV, 'ssn_ff_backward: ' + M_ALIGN),
    ('ssn_ff_backward_f32', (X, X, X + 12, X, X, X, X, X, fp(box=4), None), INV, 'ssn_ff_backward: ' + M_ALIGN),
    # x, B, D, sums, stream
    ('ssn_moment_sums_f32', (X, -1, 1, X, None), INV, 'ssn_moment_sums: invalid argument'),
    ('ssn_moment_sums_f32', (X, 1, -1, X, None), INV, 'ssn_moment_sums: invalid argument'),
    ('ssn_moment_sums_f32', (None, 1, 1, X, None), INV, 'ssn_moment_sums: invalid argument'),
    ('ssn_moment_sums_f32', (X, 1, 1, None, None), INV, 'ssn_moment_sums: invalid argument'),
    # x, sums, global_batch, data_moments, weights, B, D, gx, out, stream
    ('ssn_moment_loss_grad_f32', (X, X, 1., X, X, -1, 1, X, X, None), INV, 'ssn_moment_loss_grad: invalid argument'),
    ('ssn_moment_loss_grad_f32', (X, X, 1., X, X, 1, -1, X, X, None), INV, 'ssn_moment_loss_grad: invalid argument'),
    ('ssn_moment_loss_grad_f32', (X, X, 0., X, X, 1, 1, X, X, None), INV, 'ssn_moment_loss_grad: invalid argument'),
    ('ssn_moment_loss_grad_f32', (X, X, NAN, X, X, 1, 1, X, X, None), INV, 'ssn_moment_loss_grad: invalid argument'),
    ('ssn_moment_loss_grad_f32', (X, X, 1., X, X, 1, 1, X, None, None), INV, 'ssn_moment_loss_grad: invalid argument'),
    ('ssn_moment_loss_grad_f32', (None, X, 1., X, X, 1, 1, X, X, None), INV, 'ssn_moment_loss_grad: invalid argument'),
    ('ssn_moment_loss_grad_f32', (X, None, 1., X, X, 1, 1, X, X, None), INV, 'ssn_moment_loss_grad: invalid argument'),
    ('ssn_moment_loss_grad_f32', (X, X, 1., None, X, 1, 1, X, X, None), INV, 'ssn_moment_loss_grad: invalid argument'),
    ('ssn_moment_loss_grad_f32', (X, X, 1., X, None, 1, 1, X, X, None), INV, 'ssn_moment_loss_grad: invalid argument'),
    ('ssn_moment_loss_grad_f32', (X, X, 1., X, X, 1, 1, None, X, None), INV, 'ssn_moment_loss_grad: invalid argument'),

    # ---- steady-state gradient.  z, J, D, S, which, dW, B, N, stream
    (pair('ssn_build_dw'), (X, None, None, None, 0, X, -1, 2, None), INV, 'ssn_build_dw: invalid argument'),
    (pair('ssn_build_dw'), (X, None, None, None, 0, X, 1, 0, None), INV, 'ssn_build_dw: invalid argument'),
    (pair('ssn_build_dw'), (X, None, None, None, 3, X, 1, 2, None), INV, 'ssn_build_dw: invalid argument'),
    (pair('ssn_build_dw'), (X, None, None, None, -1, X, 1, 2, None), INV, 'ssn_build_dw: invalid argument'),
    (pair('ssn_build_dw'), (X, None, None, None, 0, X, 1, 2, None), INV, 'ssn_build_dw: invalid argument'),    # null J, D, S
    # R, W, dW, dw_per_draw, I, i_per_draw, nz, nb, M, p, A, rhs, stream
    (pair('ssn_ss_grad_system'), (None, None, None, 0, None, 0, 0, 3, 8, None, None, None, None), 0, SAME),
    (pair('ssn_ss_grad_system'), (None, None, None, 0, None, 0, 3, 0, 8, None, None, None, None), 0, SAME),
    (pair('ssn_ss_grad_system'), (X, X, X, 0, X, 0, -1, 1, 8, sp(), X, X, None), INV, 'ssn_ss_grad_system: invalid argument'),
    (pair('ssn_ss_grad_system'), (X, X, X, 0, X, 0, 1, -1, 8, sp(), X, X, None), INV, 'ssn_ss_grad_system: invalid argument'),
    (pair('ssn_ss_grad_system'), (X, X, X, 0, X, 0, 1, 1, 0, sp(), X, X, None), INV, 'ssn_ss_grad_system: invalid argument'),
    (pair('ssn_ss_grad_system'), (X, X, X, 0, X, 0, 1, 1, 7, sp(), X, X, None), INV, 'ssn_ss_grad_system: invalid argument'),
    (pair('ssn_ss_grad_system'), (X, X, X, 0, X, 0, 1, 1, 8, None, X, X, None), INV, 'ssn_ss_grad_system: invalid argument'),
    (pair('ssn_ss_grad_system'), (X, X, X, 0, X, 0, 1, 1, 8, sp(io_type=3), X, X, None), INV,
     'ssn_ss_grad_system: invalid argument'),
    (pair('ssn_ss_grad_system'), (X, X, X, 0, X, 0, 1, 1, 8, sp(io_type=-1), X, X, None), INV,
     'ssn_ss_grad_system: invalid argument'),
    (pair('ssn_ss_grad_system'), (None, X, X, 0, X, 0, 1, 1, 8, sp(), X, X, None), INV, 'ssn_ss_grad_system: invalid argument'),
    (pair('ssn_ss_grad_system'), (X, None, X, 0, X, 0, 1, 1, 8, sp(), X, X, None), INV, 'ssn_ss_grad_system: invalid argument'),
    (pair('ssn_ss_grad_system'), (X, X, None, 0, X, 0, 1, 1, 8, sp(), X, X, None), INV, 'ssn_ss_grad_system: invalid argument'),
    (pair('ssn_ss_grad_system'), (X, X, X, 0, None, 0, 1, 1, 8, sp(), X, X, None), INV, 'ssn_ss_grad_system: invalid argument'),
    (pair('ssn_ss_grad_system'), (X, X, X, 0, X, 0, 1, 1, 8, sp(), None, X, None), INV, 'ssn_ss_grad_system: invalid argument'),
    (pair('ssn_ss_grad_system'), (X, X, X, 0, X, 0, 1, 1, 8, sp(), X, None, None), INV, 'ssn_ss_grad_system: invalid argument'),
    # A, rhs, info, nsys, M, nrhs, stream
    (pair('ssn_lu_solve'), (X, X, X, -1, 2, 1, None), INV, 'ssn_lu_solve: invalid argument'),
    (pair('ssn_lu_solve'), (X, X, X, 1, -1, 1, None), INV, 'ssn_lu_solve: invalid argument'),
    (pair('ssn_lu_solve'), (None, X, X, 1, 2, 1, None), INV, 'ssn_lu_solve: invalid argument'),
    (pair('ssn_lu_solve'), (X, None, X, 1, 2, 1, None), INV, 'ssn_lu_solve: invalid argument'),

    # ---- ensembles.  x, K, B, D, sums, data_moments, weights, gx, rec, rstride, stream
    ('ssn_ens_moments_f32', (X, -1, 1, 2, X, X, X, X, X, 8, None), INV, 'ssn_ens_moments: invalid argument'),
    ('ssn_ens_moments_f32', (X, 1, 0, 2, X, X, X, X, X, 8, None), INV, 'ssn_ens_moments: invalid argument'),
    ('ssn_ens_moments_f32', (X, 1, 1, -1, X, X, X, X, X, 8, None), INV, 'ssn_ens_moments: invalid argument'),
    ('ssn_ens_moments_f32', (X, 1, 1, 2, X, X, X, X, X, 7, None), INV, 'ssn_ens_moments: invalid argument'),
    ('ssn_ens_moments_f32', (None, 1, 1, 2, X, X, X, X, X, 8, None), INV, 'ssn_ens_moments: invalid argument'),
    ('ssn_ens_moments_f32', (X, 1, 1, 2, None, X, X, X, X, 8, None), INV, 'ssn_ens_moments: invalid argument'),
    ('ssn_ens_moments_f32', (X, 1, 1, 2, X, None, X, X, X, 8, None), INV, 'ssn_ens_moments: invalid argument'),
    ('ssn_ens_moments_f32', (X, 1, 1, 2, X, X, None, X, X, 8, None), INV, 'ssn_ens_moments: invalid argument'),
    ('ssn_ens_moments_f32', (X, 1, 1, 2, X, X, X, None, X, 8, None), INV, 'ssn_ens_moments: invalid argument'),
    ('ssn_ens_moments_f32', (X, 1, 1, 2, X, X, X, X, None, 8, None), INV, 'ssn_ens_moments: invalid argument'),
    # gW, z, p16, out, K, B, N, stream
    ('ssn_ens_jds_grad_f32', (X, X, X, X, -1, 1, 2, None), INV, 'ssn_ens_jds_grad: invalid argument'),
    ('ssn_ens_jds_grad_f32', (X, X, X, X, 1, -1, 2, None), INV, 'ssn_ens_jds_grad: invalid argument'),
    ('ssn_ens_jds_grad_f32', (X, X, X, X, 1, 1, 0, None), INV, 'ssn_ens_jds_grad: invalid argument'),
    ('ssn_ens_jds_grad_f32', (None, X, X, X, 1, 1, 2, None), INV, 'ssn_ens_jds_grad: invalid argument'),
    ('ssn_ens_jds_grad_f32', (X, None, X, X, 1, 1, 2, None), INV, 'ssn_ens_jds_grad: invalid argument'),
    ('ssn_ens_jds_grad_f32', (X, X, None, X, 1, 1, 2, None), INV, 'ssn_ens_jds_grad: invalid argument'),
    ('ssn_ens_jds_grad_f32', (X, X, X, None, 1, 1, 2, None), INV, 'ssn_ens_jds_grad: invalid argument'),
    # a, stream
    ('ssn_ens_gen_grads_f32', (None, None), INV, 'ssn_ens_gen_grads: invalid argument'),
    ('ssn_ens_gen_grads_f32', (eg(D=0), None), INV, M_ENS_D),
    ('ssn_ens_gen_grads_f32', (eg(D=-1), None), INV, 'ssn_ens_gen_grads: invalid argument'),
    ('ssn_ens_gen_grads_f32', (eg(K=-1), None), INV, 'ssn_ens_gen_grads: invalid argument'),
    ('ssn_ens_gen_grads_f32', (eg(B=0), None), INV, 'ssn_ens_gen_grads: invalid argument'),
    ('ssn_ens_gen_grads_f32', (eg(nv=-1), None), INV, 'ssn_ens_gen_grads: invalid argument'),
    ('ssn_ens_gen_grads_f32', (eg(nv=3), None), INV, 'ssn_ens_gen_grads: invalid argument'),
    ('ssn_ens_gen_grads_f32', (eg(NB=0), None), INV, 'ssn_ens_gen_grads: invalid argument'),
    ('ssn_ens_gen_grads_f32', (eg(M=0), None), INV, 'ssn_ens_gen_grads: invalid argument'),
    ('ssn_ens_gen_grads_f32', (eg(M=3), None), INV, 'ssn_ens_gen_grads: invalid argument'),
    ('ssn_ens_gen_grads_f32', (eg(rstride=29), None), INV, 'ssn_ens_gen_grads: invalid argument'),     # 4 + 2 D + 2 (nv + 12)
    ('ssn_ens_gen_grads_f32', (eg(part=None), None), INV, 'ssn_ens_gen_grads: invalid argument'),
    ('ssn_ens_gen_grads_f32', (eg(dyn_row=None), None), INV, 'ssn_ens_gen_grads: invalid argument'),
    ('ssn_ens_gen_grads_f32', (eg(rate_row=None), None), INV, 'ssn_ens_gen_grads: invalid argument'),
    ('ssn_ens_gen_grads_f32', (eg(data_moments=None), None), INV, 'ssn_ens_gen_grads: invalid argument'),
    ('ssn_ens_gen_grads_f32', (eg(weights=None), None), INV, 'ssn_ens_gen_grads: invalid argument'),
    ('ssn_ens_gen_grads_f32', (eg(costs=None), None), INV, 'ssn_ens_gen_grads: invalid argument'),
    ('ssn_ens_gen_grads_f32', (eg(grads=None), None), INV, 'ssn_ens_gen_grads: invalid argument'),
    ('ssn_ens_gen_grads_f32', (eg(rec=None), None), INV, 'ssn_ens_gen_grads: invalid argument'),
    ('ssn_ens_gen_grads_f32', (eg(nv=1, g_ext=None), None), INV, 'ssn_ens_gen_grads: invalid argument'),
    ('ssn_ens_gen_grads_f32', (eg(nv=2, ext_base=None), None), INV, 'ssn_ens_gen_grads: invalid argument'),
    ('ssn_ens_gen_grads_f32', (eg(nv=2, zin=None), None), INV, 'ssn_ens_gen_grads: invalid argument'),
    # a, l0, stream
    ('ssn_ens_gen_grads_l0_f32', (None, X, None), INV, M_ENS_L0),
    ('ssn_ens_gen_grads_l0_f32', (eg0(D=1), X, None), INV, M_ENS_L0),
    ('ssn_ens_gen_grads_l0_f32', (eg0(data_moments=X), X, None), INV, M_ENS_L0),
    ('ssn_ens_gen_grads_l0_f32', (eg0(weights=X), X, None), INV, M_ENS_L0),
    ('ssn_ens_gen_grads_l0_f32', (eg0(), None, None), INV, M_ENS_L0),
    ('ssn_ens_gen_grads_l0_f32', (eg0(K=-1), X, None), INV, M_ENS_L0),
    ('ssn_ens_gen_grads_l0_f32', (eg0(B=0), X, None), INV, M_ENS_L0),
    ('ssn_ens_gen_grads_l0_f32', (eg0(nv=3), X, None), INV, M_ENS_L0),
    ('ssn_ens_gen_grads_l0_f32', (eg0(nv=-1), X, None), INV, M_ENS_L0),
    ('ssn_ens_gen_grads_l0_f32', (eg0(NB=0), X, None), INV, M_ENS_L0),
    ('ssn_ens_gen_grads_l0_f32', (eg0(M=3), X, None), INV, M_ENS_L0),
    ('ssn_ens_gen_grads_l0_f32', (eg0(rstride=27), X, None), INV, M_ENS_L0),
    ('ssn_ens_gen_grads_l0_f32', (eg0(part=None), X, None), INV, M_ENS_L0),
    ('ssn_ens_gen_grads_l0_f32', (eg0(costs=None), X, None), INV, M_ENS_L0),
    ('ssn_ens_gen_grads_l0_f32', (eg0(grads=None), X, None), INV, M_ENS_L0),
    ('ssn_ens_gen_grads_l0_f32', (eg0(rec=None), X, None), INV, M_ENS_L0),
    ('ssn_ens_gen_grads_l0_f32', (eg0(nv=1, g_ext=None), X, None), INV, M_ENS_L0),
    # a, stream
    ('ssn_ens_apply_f32', (None, None), INV, 'ssn_ens_apply: invalid argument'),
    ('ssn_ens_apply_f32', (ea(K=-1), None), INV, 'ssn_ens_apply: invalid argument'),
    ('ssn_ens_apply_f32', (ea(P=0), None), INV, 'ssn_ens_apply: invalid argument'),
    ('ssn_ens_apply_f32', (ea(kind=-1), None), INV, 'ssn_ens_apply: invalid argument'),
    ('ssn_ens_apply_f32', (ea(kind=3), None), INV, 'ssn_ens_apply: invalid argument'),
    ('ssn_ens_apply_f32', (ea(rec_off=-1), None), INV, 'ssn_ens_apply: invalid argument'),
    ('ssn_ens_apply_f32', (ea(rstride=3), None), INV, 'ssn_ens_apply: invalid argument'),
    ('ssn_ens_apply_f32', (ea(hyp=None), None), INV, 'ssn_ens_apply: invalid argument'),
    ('ssn_ens_apply_f32', (ea(clip_lo=None), None), INV, 'ssn_ens_apply: invalid argument'),
    ('ssn_ens_apply_f32', (ea(clip_hi=None), None), INV, 'ssn_ens_apply: invalid argument'),
    ('ssn_ens_apply_f32', (ea(p=None), None), INV, 'ssn_ens_apply: invalid argument'),
    ('ssn_ens_apply_f32', (ea(g=None), None), INV, 'ssn_ens_apply: invalid argument'),
    ('ssn_ens_apply_f32', (ea(rec=None), None), INV, 'ssn_ens_apply: invalid argument'),
    ('ssn_ens_apply_f32', (ea(kind=2, s1=None), None), INV, 'ssn_ens_apply: invalid argument'),
    ('ssn_ens_apply_f32', (ea(kind=1, s2=None), None), INV, 'ssn_ens_apply: invalid argument'),
    # bw, con, smoothness, zin, v, ext, K, B, NB, N, stream
    ('ssn_ens_stimulus_hetero_f32', (X, X, 1., X, X, X, -1, 1, 1, 2, None), INV, 'ssn_ens_stimulus_hetero: invalid argument'),
    ('ssn_ens_stimulus_hetero_f32', (X, X, 1., X, X, X, 1, -1, 1, 2, None), INV, 'ssn_ens_stimulus_hetero: invalid argument'),
    ('ssn_ens_stimulus_hetero_f32', (X, X, 1., X, X, X, 1, 1, -1, 2, None), INV, 'ssn_ens_stimulus_hetero: invalid argument'),
    ('ssn_ens_stimulus_hetero_f32', (X, X, 1., X, X, X, 1, 1, 1, 0, None), INV, 'ssn_ens_stimulus_hetero: invalid argument'),
    ('ssn_ens_stimulus_hetero_f32', (X, X, 0., X, X, X, 1, 1, 1, 2, None), INV, 'ssn_ens_stimulus_hetero: invalid argument'),
    ('ssn_ens_stimulus_hetero_f32', (X, X, NAN, X, X, X, 1, 1, 1, 2, None), INV, 'ssn_ens_stimulus_hetero: invalid argument'),
    ('ssn_ens_stimulus_hetero_f32', (None, X, 1., X, X, X, 1, 1, 1, 2, None), INV, 'ssn_ens_stimulus_hetero: invalid argument'),
    ('ssn_ens_stimulus_hetero_f32', (X, None, 1., X, X, X, 1, 1, 1, 2, None), INV, 'ssn_ens_stimulus_hetero: invalid argument'),
    ('ssn_ens_stimulus_hetero_f32', (X, X, 1., None, X, X, 1, 1, 1, 2, None), INV, 'ssn_ens_stimulus_hetero: invalid argument'),
    ('ssn_ens_stimulus_hetero_f32', (X, X, 1., X, None, X, 1, 1, 1, 2, None), INV, 'ssn_ens_stimulus_hetero: invalid argument'),
    ('ssn_ens_stimulus_hetero_f32', (X, X, 1., X, X, None, 1, 1, 1, 2, None), INV, 'ssn_ens_stimulus_hetero: invalid argument'),

    # ---- scorer and sliced Wasserstein.  tc, feat, rows, NC, NB, Q, stream
    ('ssn_tc_features_f32', (X, X, -1, 1, 1, 1, None), INV, 'ssn_tc_features_f32: invalid argument'),
    ('ssn_tc_features_f32', (X, X, 1, -1, 1, 1, None), INV, 'ssn_tc_features_f32: invalid argument'),
    ('ssn_tc_features_f32', (X, X, 1, 1, 0, 1, None), INV, 'ssn_tc_features_f32: invalid argument'),
    ('ssn_tc_features_f32', (X, X, 1, 1, 1, -1, None), INV, 'ssn_tc_features_f32: invalid argument'),
    ('ssn_tc_features_f32', (None, X, 1, 1, 1, 1, None), INV, 'ssn_tc_features_f32: invalid argument'),
    ('ssn_tc_features_f32', (X, None, 1, 1, 1, 1, None), INV, 'ssn_tc_features_f32: invalid argument'),
    # x, truth_sorted, m, S, B, C, T, n, num [, wnum], stream
    ('ssn_ks_columns_f32', (X, X, X, 1, 16385, 1, 1, X, X, None), INV, 'ssn_ks_columns_f32: ' + M_KS),
    ('ssn_ks_columns_f32', (X, X, X, -1, 4, 1, 1, X, X, None), INV, 'ssn_ks_columns_f32: invalid argument'),
    ('ssn_ks_columns_f32', (X, X, X, 1, 0, 1, 1, X, X, None), INV, 'ssn_ks_columns_f32: invalid argument'),
    ('ssn_ks_columns_f32', (X, X, X, 1, 4, -1, 1, X, X, None), INV, 'ssn_ks_columns_f32: invalid argument'),
    ('ssn_ks_columns_f32', (X, X, X, 1, 4, 1, -1, X, X, None), INV, 'ssn_ks_columns_f32: invalid argument'),
    ('ssn_ks_columns_f32', (None, X, X, 1, 4, 1, 1, X, X, None), INV, 'ssn_ks_columns_f32: invalid argument'),
    ('ssn_ks_columns_f32', (X, None, X, 1, 4, 1, 1, X, X, None), INV, 'ssn_ks_columns_f32: invalid argument'),
    ('ssn_ks_columns_f32', (X, X, None, 1, 4, 1, 1, X, X, None), INV, 'ssn_ks_columns_f32: invalid argument'),
    ('ssn_ks_columns_f32', (X, X, X, 1, 4, 1, 1, None, X, None), INV, 'ssn_ks_columns_f32: invalid argument'),
    ('ssn_ks_columns_f32', (X, X, X, 1, 4, 1, 1, X, None, None), INV, 'ssn_ks_columns_f32: invalid argument'),
    ('ssn_ks_w1_columns_f32', (X, X, X, 1, 16385, 1, 1, X, X, X, None), INV, 'ssn_ks_w1_columns_f32: ' + M_KS),
    ('ssn_ks_w1_columns_f32', (X, X, X, -1, 4, 1, 1, X, X, X, None), INV, 'ssn_ks_w1_columns_f32: invalid argument'),
    ('ssn_ks_w1_columns_f32', (X, X, X, 1, 0, 1, 1, X, X, X, None), INV, 'ssn_ks_w1_columns_f32: invalid argument'),
    ('ssn_ks_w1_columns_f32', (X, X, X, 1, 4, -1, 1, X, X, X, None), INV, 'ssn_ks_w1_columns_f32: invalid argument'),
    ('ssn_ks_w1_columns_f32', (X, X, X, 1, 4, 1, -1, X, X, X, None), INV, 'ssn_ks_w1_columns_f32: invalid argument'),
    ('ssn_ks_w1_columns_f32', (None, X, X, 1, 4, 1, 1, X, X, X, None), INV, 'ssn_ks_w1_columns_f32: invalid argument'),
    ('ssn_ks_w1_columns_f32', (X, None, X, 1, 4, 1, 1, X, X, X, None), INV, 'ssn_ks_w1_columns_f32: invalid argument'),
    ('ssn_ks_w1_columns_f32', (X, X, X, 1, 4, 1, 1, X, X, None, None), INV, 'ssn_ks_w1_columns_f32: invalid argument'),
    # x, rows, ldx, C, theta, L, out, stream
    ('ssn_project_rows_f32', (X, 1, 2, 2, X, 4097, X, None), INV, 'ssn_project_rows_f32: ' + M_DIRS),
    ('ssn_project_rows_f32', (X, -1, 2, 2, X, 1, X, None), INV, 'ssn_project_rows_f32: invalid argument'),
    ('ssn_project_rows_f32', (X, 1, 2, -1, X, 1, X, None), INV, 'ssn_project_rows_f32: invalid argument'),
    ('ssn_project_rows_f32', (X, 1, 2, 2, X, -1, X, None), INV, 'ssn_project_rows_f32: invalid argument'),
    ('ssn_project_rows_f32', (X, 1, 1, 2, X, 1, X, None), INV, 'ssn_project_rows_f32: invalid argument'),
    ('ssn_project_rows_f32', (X, 1, 2, 2, X, 1, None, None), INV, 'ssn_project_rows_f32: invalid argument'),
    ('ssn_project_rows_f32', (None, 1, 2, 2, X, 1, X, None), INV, 'ssn_project_rows_f32: invalid argument'),
    ('ssn_project_rows_f32', (X, 1, 2, 2, None, 1, X, None), INV, 'ssn_project_rows_f32: invalid argument'),
    # px, py, B, L, power, coef, loss_l, stream
    ('ssn_swd_match_f32', (X, X, 5000, 1, 2, X, X, None), INV, 'ssn_swd_match_f32: ' + M_ROWS),
    ('ssn_swd_match_f32', (X, X, 4, 4097, 2, X, X, None), INV, 'ssn_swd_match_f32: ' + M_DIRS),
    ('ssn_swd_match_f32', (X, X, -1, 1, 2, X, X, None), INV, 'ssn_swd_match_f32: invalid argument'),
    ('ssn_swd_match_f32', (X, X, 4, -1, 2, X, X, None), INV, 'ssn_swd_match_f32: invalid argument'),
    ('ssn_swd_match_f32', (X, X, 4, 1, 0, X, X, None), INV, 'ssn_swd_match_f32: invalid argument'),
    ('ssn_swd_match_f32', (X, X, 4, 1, 3, X, X, None), INV, 'ssn_swd_match_f32: invalid argument'),
    ('ssn_swd_match_f32', (None, X, 4, 1, 2, X, X, None), INV, 'ssn_swd_match_f32: invalid argument'),
    ('ssn_swd_match_f32', (X, None, 4, 1, 2, X, X, None), INV, 'ssn_swd_match_f32: invalid argument'),
    ('ssn_swd_match_f32', (X, X, 4, 1, 2, None, X, None), INV, 'ssn_swd_match_f32: invalid argument'),
    ('ssn_swd_match_f32', (X, X, 4, 1, 2, X, None, None), INV, 'ssn_swd_match_f32: invalid argument'),
    # coef, theta, B, L, D, gx, stream
    ('ssn_swd_backproject_f32', (X, X, 4, 4097, 2, X, None), INV, 'ssn_swd_backproject_f32: ' + M_DIRS),
    ('ssn_swd_backproject_f32', (X, X, -1, 1, 2, X, None), INV, 'ssn_swd_backproject_f32: invalid argument'),
    ('ssn_swd_backproject_f32', (X, X, 4, -1, 2, X, None), INV, 'ssn_swd_backproject_f32: invalid argument'),
    ('ssn_swd_backproject_f32', (X, X, 4, 1, -1, X, None), INV, 'ssn_swd_backproject_f32: invalid argument'),
    ('ssn_swd_backproject_f32', (X, X, 4, 1, 2, None, None), INV, 'ssn_swd_backproject_f32: invalid argument'),
    ('ssn_swd_backproject_f32', (None, X, 4, 1, 2, X, None), INV, 'ssn_swd_backproject_f32: invalid argument'),
    ('ssn_swd_backproject_f32', (X, None, 4, 1, 2, X, None), INV, 'ssn_swd_backproject_f32: invalid argument'),
    # x, y, theta, K, B, L, D, px, py, stream
    ('ssn_ens_swd_project_f32', (X, X, X, 2049, 4, 1, 2, X, X, None), INV, 'ssn_ens_swd_project_f32: more than 2048 members'),
    ('ssn_ens_swd_project_f32', (X, X, X, 1, 4097, 1, 2, X, X, None), INV, 'ssn_ens_swd_project_f32: ' + M_ENS_ROWS),
    ('ssn_ens_swd_project_f32', (X, X, X, 1, 4, 4097, 2, X, X, None), INV, 'ssn_ens_swd_project_f32: ' + M_DIRS),
    ('ssn_ens_swd_project_f32', (X, X, X, -1, 4, 1, 2, X, X, None), INV, 'ssn_ens_swd_project_f32: invalid argument'),
    ('ssn_ens_swd_project_f32', (X, X, X, 1, -1, 1, 2, X, X, None), INV, 'ssn_ens_swd_project_f32: invalid argument'),
    ('ssn_ens_swd_project_f32', (X, X, X, 1, 4, -1, 2, X, X, None), INV, 'ssn_ens_swd_project_f32: invalid argument'),
    ('ssn_ens_swd_project_f32', (X, X, X, 1, 4, 1, -1, X, X, None), INV, 'ssn_ens_swd_project_f32: invalid argument'),
    ('ssn_ens_swd_project_f32', (X, X, X, 1, 4, 1, 2, None, X, None), INV, 'ssn_ens_swd_project_f32: invalid argument'),
    ('ssn_ens_swd_project_f32', (X, X, X, 1, 4, 1, 2, X, None, None), INV, 'ssn_ens_swd_project_f32: invalid argument'),
    ('ssn_ens_swd_project_f32', (None, X, X, 1, 4, 1, 2, X, X, None), INV, 'ssn_ens_swd_project_f32: invalid argument'),
    ('ssn_ens_swd_project_f32', (X, None, X, 1, 4, 1, 2, X, X, None), INV, 'ssn_ens_swd_project_f32: invalid argument'),
    ('ssn_ens_swd_project_f32', (X, X, None, 1, 4, 1, 2, X, X, None), INV, 'ssn_ens_swd_project_f32: invalid argument'),
    # px, py, power (host), K, B, L, form, coef, loss_l, l0, stream
    ('ssn_ens_swd_match_f32', (X, X, ints(2), 2049, 4, 1, 0, X, X, X, None), INV, 'ssn_ens_swd_match_f32: more than 2048 members'),
    ('ssn_ens_swd_match_f32', (X, X, ints(2), 1, 4097, 1, 0, X, X, X, None), INV, 'ssn_ens_swd_match_f32: ' + M_ENS_ROWS),
    ('ssn_ens_swd_match_f32', (X, X, ints(2), 1, 4, 4097, 0, X, X, X, None), INV, 'ssn_ens_swd_match_f32: ' + M_DIRS),
    ('ssn_ens_swd_match_f32', (X, X, ints(2), -1, 4, 1, 0, X, X, X, None), INV, 'ssn_ens_swd_match_f32: invalid argument'),
    ('ssn_ens_swd_match_f32', (X, X, ints(2), 1, -1, 1, 0, X, X, X, None), INV, 'ssn_ens_swd_match_f32: invalid argument'),
    ('ssn_ens_swd_match_f32', (X, X, ints(2), 1, 4, -1, 0, X, X, X, None), INV, 'ssn_ens_swd_match_f32: invalid argument'),
    ('ssn_ens_swd_match_f32', (X, X, None, 1, 4, 1, 0, X, X, X, None), INV, 'ssn_ens_swd_match_f32: invalid argument'),
    ('ssn_ens_swd_match_f32', (X, X, ints(3), 1, 4, 1, 0, X, X, X, None), INV, 'ssn_ens_swd_match_f32: a power other than 1 or 2'),
    ('ssn_ens_swd_match_f32', (X, X, ints(1, 0), 2, 4, 1, 0, X, X, X, None), INV,
     'ssn_ens_swd_match_f32: a power other than 1 or 2'),
    ('ssn_ens_swd_match_f32', (X, X, ints(2), 1, 4, 1, 3, X, X, X, None), INV, 'ssn_ens_swd_match_f32: unknown form'),
    ('ssn_ens_swd_match_f32', (X, X, ints(2), 1, 4, 1, -1, X, X, X, None), INV, 'ssn_ens_swd_match_f32: unknown form'),
    ('ssn_ens_swd_match_f32', (X, X, ints(2), 1, 65, 1, 2, X, X, X, None), INV,
     'ssn_ens_swd_match_f32: the wave form takes at most 64 rows per member'),
    ('ssn_ens_swd_match_f32', (None, X, ints(2), 1, 4, 1, 0, X, X, X, None), INV,
     'ssn_ens_swd_match_f32: invalid argument (null pointer)'),
    ('ssn_ens_swd_match_f32', (X, None, ints(1), 1, 4, 1, 1, X, X, X, None), INV,
     'ssn_ens_swd_match_f32: invalid argument (null pointer)'),
    ('ssn_ens_swd_match_f32', (X, X, ints(1), 1, 4, 1, 2, None, X, X, None), INV,
     'ssn_ens_swd_match_f32: invalid argument (null pointer)'),
    ('ssn_ens_swd_match_f32', (X, X, ints(2), 1, 4, 1, 0, X, None, X, None), INV,
     'ssn_ens_swd_match_f32: invalid argument (null pointer)'),
    ('ssn_ens_swd_match_f32', (X, X, ints(2), 1, 4, 1, 0, X, X, None, None), INV,
     'ssn_ens_swd_match_f32: invalid argument (null pointer)'),
    # coef, theta, K, B, L, D, gx, stream
    ('ssn_ens_swd_backproject_f32', (X, X, 2049, 4, 1, 2, X, None), INV, 'ssn_ens_swd_backproject_f32: more than 2048 members'),
    ('ssn_ens_swd_backproject_f32', (X, X, 1, 4097, 1, 2, X, None), INV, 'ssn_ens_swd_backproject_f32: ' + M_ENS_ROWS),
    ('ssn_ens_swd_backproject_f32', (X, X, 1, 4, 4097, 2, X, None), INV, 'ssn_ens_swd_backproject_f32: ' + M_DIRS),
    ('ssn_ens_swd_backproject_f32', (X, X, -1, 4, 1, 2, X, None), INV, 'ssn_ens_swd_backproject_f32: invalid argument'),
    ('ssn_ens_swd_backproject_f32', (X, X, 1, -1, 1, 2, X, None), INV, 'ssn_ens_swd_backproject_f32: invalid argument'),
    ('ssn_ens_swd_backproject_f32', (X, X, 1, 4, -1, 2, X, None), INV, 'ssn_ens_swd_backproject_f32: invalid argument'),
    ('ssn_ens_swd_backproject_f32', (X, X, 1, 4, 1, -1, X, None), INV, 'ssn_ens_swd_backproject_f32: invalid argument'),
    ('ssn_ens_swd_backproject_f32', (X, X, 1, 4, 1, 2, None, None), INV, 'ssn_ens_swd_backproject_f32: invalid argument'),
    ('ssn_ens_swd_backproject_f32', (None, X, 1, 4, 1, 2, X, None), INV, 'ssn_ens_swd_backproject_f32: invalid argument'),
    ('ssn_ens_swd_backproject_f32', (X, None, 1, 4, 1, 2, X, None), INV, 'ssn_ens_swd_backproject_f32: invalid argument'),
    # codes, x, A, R, NB, M, probes, nprobe, set_of, cand0, NZ, verdict, out, accepted, used, rejections, draw_index, stream
    (FPS + '_f64', (X, X, 1, 8193, 1, 8, X, 1, X, 0, 1, X, X, X, X, X, X, None), INV, 'ssn_fp_select_f64: ' + M_FPSEL),
    (FPS + '_f32', (X, X, 1, 8193, 1, 8, X, 1, X, 0, 1, X, X, X, X, X, X, None), INV, 'ssn_fp_select_f32: ' + M_FPSEL),
] + [
    (FPS + s, args, INV, FPS + s + ': invalid argument') for s in ('_f64', '_f32') for args in (
        (X, X, -1, 1, 1, 8, X, 1, X, 0, 1, X, X, X, X, X, X, None),
        (X, X, 1, -1, 1, 8, X, 1, X, 0, 1, X, X, X, X, X, X, None),
        (X, X, 1, 1, 0, 8, X, 1, X, 0, 1, X, X, X, X, X, X, None),
        (X, X, 1, 1, 1, 0, X, 1, X, 0, 1, X, X, X, X, X, X, None),
        (X, X, 1, 1, 1, 7, X, 1, X, 0, 1, X, X, X, X, X, X, None),
        (X, X, 1, 1, 1, 8, X, -1, X, 0, 1, X, X, X, X, X, X, None),
        (X, X, 1, 1, 1, 8, X, 1, X, -1, 1, X, X, X, X, X, X, None),
        (X, X, 1, 1, 1, 8, X, 1, X, 0, 0, X, X, X, X, X, X, None),
        (X, X, 1, 1, 1 << 16, 1 << 16, X, 1, X, 0, 1, X, X, X, X, X, X, None),
        (X, X, 1, 1, 1, 8, X, 1, X, (1 << 31) - 1, 1, X, X, X, X, X, X, None),
        (None, X, 1, 1, 1, 8, X, 1, X, 0, 1, X, X, X, X, X, X, None),
        (X, None, 1, 1, 1, 8, X, 1, X, 0, 1, X, X, X, X, X, X, None),
        (X, X, 1, 1, 1, 8, None, 1, X, 0, 1, X, X, X, X, X, X, None),
        (X, X, 1, 1, 1, 8, X, 1, None, 0, 1, X, X, X, X, X, X, None),
        (X, X, 1, 1, 1, 8, X, 1, X, 0, 1, None, X, X, X, X, X, None),
        (X, X, 1, 1, 1, 8, X, 1, X, 0, 1, X, None, X, X, X, X, None),
        (X, X, 1, 1, 1, 8, X, 1, X, 0, 1, X, X, None, X, X, X, None),
        (X, X, 1, 1, 1, 8, X, 1, X, 0, 1, X, X, X, None, X, X, None),
        (X, X, 1, 1, 1, 8, X, 1, X, 0, 1, X, X, X, X, None, X, None),
        (X, X, 1, 1, 1, 8, X, 1, X, 0, 1, X, X, X, X, X, None, None),
    )
] + [
    # ---- MT19937 / Philox.  nblocks, bits
    ('ssn_mt19937_jump_poly', (0, None), INV, 'ssn_mt19937_jump_poly: null output'),
    ('ssn_mt19937_jump_poly', (5, None), INV, 'ssn_mt19937_jump_poly: null output'),
    # key, pos, total, skip, count, out, stream
    (pair('ssn_mt19937_random_sample'), (None, byref(POS), 8, 0, 8, X, None), INV, 'ssn_mt19937_random_sample: null state'),
    (pair('ssn_mt19937_random_sample'), (X, None, 8, 0, 8, X, None), INV, 'ssn_mt19937_random_sample: null state'),
    # key, pos, total, skip, count, out, stream, ticket
    (pair('ssn_mt19937_random_sample_begin'), (None, 0, 8, 0, 8, X, None, byref(TICKET)), INV,
     'ssn_mt19937_random_sample_begin: null state / ticket'),
    (pair('ssn_mt19937_random_sample_begin'), (X, 0, 8, 0, 8, X, None, None), INV,
     'ssn_mt19937_random_sample_begin: null state / ticket'),
    # key, pos, total, skip, count, out, tail_kind, tail_total, tail_skip, tail_count, tail_out, stream, ticket
    ('ssn_mt19937_random_sample_tail_begin_f32', (None, 0, 8, 0, 8, X, 1, 8, 0, 8, X, None, byref(TICKET)), INV,
     'ssn_mt19937_random_sample_tail_begin: null state / ticket'),
    ('ssn_mt19937_random_sample_tail_begin_f32', (X, 0, 8, 0, 8, X, 1, 8, 0, 8, X, None, None), INV,
     'ssn_mt19937_random_sample_tail_begin: null state / ticket'),
    ('ssn_mt19937_random_sample_tail_begin_f32', (X, 0, 8, 0, 8, X, 0, 8, 0, 8, X, None, byref(TICKET)), INV, M_TAILKIND),
    ('ssn_mt19937_random_sample_tail_begin_f32', (X, 0, 8, 0, 8, X, 3, 8, 0, 8, X, None, byref(TICKET)), INV, M_TAILKIND),
    # key, pos, B_total, b0, nb, J, D, S, W, z, N, stream, ticket
    ('ssn_build_w_mt19937_begin_f32', (None, 0, 2, 0, 1, F4, F4, F4, X, X, 2, None, byref(TICKET)), INV,
     'ssn_build_w_mt19937_begin: invalid argument'),
    ('ssn_build_w_mt19937_begin_f32', (X, 0, 2, 0, 1, F4, F4, F4, X, X, 2, None, None), INV,
     'ssn_build_w_mt19937_begin: invalid argument'),
    ('ssn_build_w_mt19937_begin_f32', (X, 0, 2, 0, 1, None, F4, F4, X, X, 2, None, byref(TICKET)), INV,
     'ssn_build_w_mt19937_begin: invalid argument'),
    ('ssn_build_w_mt19937_begin_f32', (X, 0, 2, 0, 1, F4, None, F4, X, X, 2, None, byref(TICKET)), INV,
     'ssn_build_w_mt19937_begin: invalid argument'),
    ('ssn_build_w_mt19937_begin_f32', (X, 0, 2, 0, 1, F4, F4, None, X, X, 2, None, byref(TICKET)), INV,
     'ssn_build_w_mt19937_begin: invalid argument'),
    ('ssn_build_w_mt19937_begin_f32', (X, 0, 2, 0, 1, F4, F4, F4, None, X, 2, None, byref(TICKET)), INV,
     'ssn_build_w_mt19937_begin: invalid argument'),
    ('ssn_build_w_mt19937_begin_f32', (X, 0, 2, 0, 1, F4, F4, F4, X, X, 0, None, byref(TICKET)), INV,
     'ssn_build_w_mt19937_begin: invalid argument'),
    ('ssn_build_w_mt19937_begin_f32', (X, 0, -1, 0, 0, F4, F4, F4, X, X, 2, None, byref(TICKET)), INV,
     'ssn_build_w_mt19937_begin: invalid argument'),
    ('ssn_build_w_mt19937_begin_f32', (X, 0, 2, -1, 1, F4, F4, F4, X, X, 2, None, byref(TICKET)), INV,
     'ssn_build_w_mt19937_begin: invalid argument'),
    ('ssn_build_w_mt19937_begin_f32', (X, 0, 2, 0, -1, F4, F4, F4, X, X, 2, None, byref(TICKET)), INV,
     'ssn_build_w_mt19937_begin: invalid argument'),
    ('ssn_build_w_mt19937_begin_f32', (X, 0, 2, 1, 2, F4, F4, F4, X, X, 2, None, byref(TICKET)), INV,
     'ssn_build_w_mt19937_begin: invalid argument'),
    # key, pos, B_total, b0, nb, J, D, S, W, z, N, tail_kind, zin, stream, ticket
    ('ssn_build_w_mt19937_tail_begin_f32', (None, 0, 2, 0, 1, F4, F4, F4, X, X, 2, 1, X, None, byref(TICKET)), INV,
     'ssn_build_w_mt19937_tail_begin: invalid argument'),
    ('ssn_build_w_mt19937_tail_begin_f32', (X, 0, 2, 0, 1, F4, F4, F4, X, X, 2, 1, X, None, None), INV,
     'ssn_build_w_mt19937_tail_begin: invalid argument'),
    ('ssn_build_w_mt19937_tail_begin_f32', (X, 0, 2, 0, 1, None, F4, F4, X, X, 2, 1, X, None, byref(TICKET)), INV,
     'ssn_build_w_mt19937_tail_begin: invalid argument'),
    ('ssn_build_w_mt19937_tail_begin_f32', (X, 0, 2, 0, 1, F4, F4, F4, None, X, 2, 1, X, None, byref(TICKET)), INV,
     'ssn_build_w_mt19937_tail_begin: invalid argument'),
    ('ssn_build_w_mt19937_tail_begin_f32', (X, 0, 2, 0, 1, F4, F4, F4, X, X, 2, 1, None, None, byref(TICKET)), INV,
     'ssn_build_w_mt19937_tail_begin: invalid argument'),
    ('ssn_build_w_mt19937_tail_begin_f32', (X, 0, 2, 0, 1, F4, F4, F4, X, X, 0, 1, X, None, byref(TICKET)), INV,
     'ssn_build_w_mt19937_tail_begin: invalid argument'),
    ('ssn_build_w_mt19937_tail_begin_f32', (X, 0, -1, 0, 0, F4, F4, F4, X, X, 2, 1, X, None, byref(TICKET)), INV,
     'ssn_build_w_mt19937_tail_begin: invalid argument'),
    ('ssn_build_w_mt19937_tail_begin_f32', (X, 0, 2, -1, 1, F4, F4, F4, X, X, 2, 1, X, None, byref(TICKET)), INV,
     'ssn_build_w_mt19937_tail_begin: invalid argument'),
    ('ssn_build_w_mt19937_tail_begin_f32', (X, 0, 2, 0, -1, F4, F4, F4, X, X, 2, 1, X, None, byref(TICKET)), INV,
     'ssn_build_w_mt19937_tail_begin: invalid argument'),
    ('ssn_build_w_mt19937_tail_begin_f32', (X, 0, 2, 1, 2, F4, F4, F4, X, X, 2, 1, X, None, byref(TICKET)), INV,
     'ssn_build_w_mt19937_tail_begin: invalid argument'),
    ('ssn_build_w_mt19937_tail_begin_f32', (X, 0, 2, 0, 1, F4, F4, F4, X, X, 2, 0, X, None, byref(TICKET)), INV,
     'ssn_build_w_mt19937_tail_begin: invalid argument'),
    ('ssn_build_w_mt19937_tail_begin_f32', (X, 0, 2, 0, 1, F4, F4, F4, X, X, 2, 3, X, None, byref(TICKET)), INV,
     'ssn_build_w_mt19937_tail_begin: invalid argument'),
    # pos, total, skip, count [, tail_kind, tail_total, tail_skip, tail_count], out
    ('ssn_mt19937_plan', (0, 8, 0, 8, None), INV, 'ssn_mt19937_plan: invalid argument'),
    ('ssn_mt19937_plan_tail', (0, 8, 0, 8, 1, 8, 0, 8, None), INV, 'ssn_mt19937_plan_tail: invalid argument'),
    # ticket, key, pos
    ('ssn_mt19937_random_sample_finish', (0, None, byref(POS)), INV, 'ssn_mt19937_random_sample_finish: null state'),
    ('ssn_mt19937_random_sample_finish', (0, X, None), INV, 'ssn_mt19937_random_sample_finish: null state'),
    # seed, offset, v, zin, amp, n, M, bernoulli, stream
    (pair('ssn_philox_amp'), (1, 0, None, X, X, 1, 2, 0, None), INV, 'ssn_philox_amp: invalid argument'),
    (pair('ssn_philox_amp'), (1, 0, X, None, X, 1, 2, 0, None), INV, 'ssn_philox_amp: invalid argument'),
    (pair('ssn_philox_amp'), (1, 0, X, X, None, 1, 2, 0, None), INV, 'ssn_philox_amp: invalid argument'),
    (pair('ssn_philox_amp'), (1, 0, X, X, X, 1, 0, 0, None), INV, 'ssn_philox_amp: invalid argument'),
    (pair('ssn_philox_amp'), (1, 0, X, X, X, 1, -2, 1, None), INV, 'ssn_philox_amp: invalid argument'),
    # seed, offset, out, n, stream
    (pair('ssn_philox_uniform'), (1, 0, None, 1, None), INV, 'ssn_philox_uniform: null output'),
    (pair('ssn_philox_uniform'), (1, 0, None, 1 << 40, None), INV, 'ssn_philox_uniform: null output'),
]


def _rows():
    for i, (names, args, code, msg) in enumerate(TABLE):
        for name in ((names,) if isinstance(names, str) else names):
            yield pytest.param(name, args, code, msg, id='%03d-%s' % (i, name))


def _call(name, args):
    return getattr(lib, name)(*[byref(a) if isinstance(a, Structure) else a for a in args])


@pytest.mark.parametrize('name, args, code, msg', list(_rows()))
def test_refusal(name, args, code, msg):
    sentinel = _SENTINEL2 if name == _SENTINEL[0] else _SENTINEL
    assert _call(sentinel[0], sentinel[1]) == INV and clib.last_error() == sentinel[2]
    if msg is SAME:
        msg = sentinel[2]
    rc = _call(name, args)
    print(name, rc, clib.last_error())
    assert rc == code
    assert clib.last_error() == msg


def test_table_names_every_checked_entry_point_and_both_members_of_a_pair():
    named = {n for names, _, _, _ in TABLE for n in ((names,) if isinstance(names, str) else names)}
    unchecked = {           # see the module docstring; the queries and the drop-in scalars refuse nothing
        'ssn_build_w_f32', 'ssn_build_w_f64', 'ssn_build_w_philox_f32', 'ssn_build_w_philox_f64', 'ssn_jds_grad_f32',
        'ssn_jds_grad_f64', 'ssn_io_eval_f32', 'ssn_io_eval_f64', 'ssn_stimulus_f32', 'ssn_stimulus_f64', 'ssn_stimulus_amp_f32',
        'ssn_stimulus_amp_f64', 'io_pow', 'io_alin', 'io_atanh', 'rate_to_volt', 'dot', 'ssn_abi_version', 'ssn_device_count',
        'ssn_last_error', 'ssn_solver_fast_path', 'ssn_gen_supported', 'ssn_critic_num_params', 'ssn_critic_num_params_act',
        'ssn_critic_workspace_floats', 'ssn_critic_norm_workspace_floats', 'ssn_set_operand_precision',
        'ssn_get_operand_precision', 'ssn_segment_sqnorms_ws_doubles', 'ssn_gen_backward_fused_supported',
        'ssn_gen_grads_ws_doubles', 'ssn_ens_record_doubles', 'ssn_fp_select_max_candidates',
    }
    assert named | unchecked == set(clib.DECLARED_SYMBOLS) and not named & unchecked
    for n in named:
        if n.endswith('_f32') and n[:-4] + '_f64' in clib.DECLARED_SYMBOLS:
            assert n[:-4] + '_f64' in named, n
